"""main.py's post-training eval loop steps the env that training ran on: with
ENV_DYNAMICS='physics' the printed episode rewards are the real game's.
CartPole pays exactly 1 per step and ends within its 200-step limit, so every
eval reward is a whole number in [1, 200]; the synthetic env's rewards
(1 - mean(x^2) per step) are not whole."""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_main(tmp_path, extra, cfg):
    cfg_path = tmp_path / "cfg.json"
    cfg_path.write_text(json.dumps(cfg))
    cmd = [sys.executable, os.path.join(REPO, "main.py"),
           "--config", str(cfg_path)] + extra
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", PYTHONPATH=REPO)
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                          text=True, timeout=300)


@pytest.mark.timeout(600)
def test_cartpole_physics_eval_rewards_are_whole_step_counts(tmp_path):
    cfg = {"GAME": "CartPole-v0", "ENV_DYNAMICS": "physics", "NUM_ENVS": 4,
           "MAX_EPOCH_STEPS": 64, "HIDDEN_SIZES": [16], "EPOCH_MAX": 8,
           "SEED": 7, "USE_GRAPHS": False, "MINIBATCH_SIZE": 0,
           "LOG_FILE_PATH": str(tmp_path / "logs")}
    r = _run_main(tmp_path, ["--rounds", "2", "--eval-episodes", "2"], cfg)
    assert r.returncode == 0, r.stderr[-2000:]
    rewards = [float(v) for v in
               re.findall(r"eval episode reward: (\S+)", r.stdout)]
    assert len(rewards) == 2, r.stdout[-2000:]
    for v in rewards:
        assert v == round(v) and 1.0 <= v <= 200.0, rewards
