"""dw_mfma at a batch size where ceil(B / splits) * splits overshoots B.

The LDS-staged dW kernel returns early on a split that starts past the
last row and leaves that split's slab unwritten; the host therefore must
not launch such splits.  B = 4099 asks for 256 splits of 17 rows, of which
only 242 have rows.  A first call at B = 8192 fills every slab of the
persistent scratch with non-zero partials, so a stale slab read back by
the reduce shows as an error of the order of the gradient itself."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.ops import hip_ext


@pytest.mark.parametrize("in_dim", [376, 64])  # wide and narrow glds tiles
def test_dw_mfma_no_stale_trailing_splits(in_dim):
    ext = hip_ext()
    out_dim = 64
    g = torch.Generator(device="cuda").manual_seed(5)

    def run(B):
        delta = torch.randn(B, out_dim, device="cuda", generator=g)
        acts = torch.randn(B, in_dim, device="cuda", generator=g)
        grad = torch.zeros(out_dim * in_dim + out_dim, device="cuda")
        ext.dw_mfma(delta, acts, grad, 0, out_dim * in_dim, -1, -1, -1, 0)
        return delta, acts, grad

    run(8192)
    delta, acts, grad = run(4099)
    ref_w = (delta.double().t() @ acts.double()).float().flatten()
    ref_b = delta.double().sum(0).float()
    scale = float(ref_w.abs().max())
    # fp32 accumulation over 4099 unit-variance products: the project's
    # bound for the fused backward (test_gpu_mlp)
    torch.testing.assert_close(grad[:out_dim * in_dim], ref_w,
                               atol=scale * 2e-4, rtol=2e-3)
    torch.testing.assert_close(grad[out_dim * in_dim:], ref_b,
                               atol=scale * 2e-4, rtol=2e-3)
