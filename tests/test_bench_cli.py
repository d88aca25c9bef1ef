"""bench.py command line: the result line's contract, --dump-outputs and
--full, on a tiny CPU configuration (run in-process)."""

import json
import sys

import numpy as np
import pytest

import bench

TINY = ["--gpus", "1", "--warmup", "1", "--preset", "halfcheetah",
        "--num-envs", "4", "--rollout", "8", "--device", "cpu"]


def _run(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", *TINY, *extra])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_result_line_and_steps(monkeypatch, capsys):
    calls = []
    real = bench.DPPOEngine.train_round

    def counted(self):
        calls.append(1)
        return real(self)

    monkeypatch.setattr(bench.DPPOEngine, "train_round", counted)
    res = _run(monkeypatch, capsys, "--steps", "3")
    assert len(calls) == 1 + 3  # warmup + timed steps
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["unit"] == "env-steps/s" and res["higher_is_better"] is True
    assert res["dtype"] == "fp32"
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    env_steps_per_step = 4 * 8
    assert res["value"] == pytest.approx(
        env_steps_per_step / (res["ms_per_step"] / 1000.0), rel=1e-9)


def test_dump_outputs_repeatable(monkeypatch, capsys, tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        _run(monkeypatch, capsys, "--steps", "2", "--dump-outputs", str(d))
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == ["obs.npy", "params.npy", "stats.npy"]
    total = 0
    for name in names:
        a, b = np.load(dirs[0] / name), np.load(dirs[1] / name)
        assert a.dtype in (np.float32, np.float64)
        assert a.size > 0
        np.testing.assert_array_equal(a, b)  # seeded inputs, CPU: bitwise
        total += a.nbytes
    assert total <= 64 * 1024 * 1024
    stats = np.load(dirs[0] / "stats.npy")
    assert stats.shape == (len(bench.STATS_KEYS) + 1,)
    assert np.load(dirs[0] / "obs.npy").shape == (4 * 17,)
    # a different number of timed steps ends on a different round
    _run(monkeypatch, capsys, "--steps", "3", "--dump-outputs",
         str(tmp_path / "c"))
    assert not np.array_equal(np.load(tmp_path / "c" / "params.npy"),
                              np.load(dirs[0] / "params.npy"))


def test_dump_sample_is_fixed_and_capped(monkeypatch):
    import torch

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    t = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    a, b = bench._dump_array(t), bench._dump_array(t.clone())
    assert a.dtype == np.float32 and a.shape == (64,)
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) >= 0)  # sorted indices into an arange
    small = bench._dump_array(torch.ones(3, 5))
    assert small.shape == (15,)


def test_full_flag_accepted(monkeypatch, capsys):
    res = _run(monkeypatch, capsys, "--steps", "1", "--full")
    assert res["steps"] == 1 and res["ms_per_step"] > 0


def test_zero_steps_rejected(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", *TINY, "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.main()
