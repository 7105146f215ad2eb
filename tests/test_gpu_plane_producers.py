"""GPU: the shared kernels of csrc/producers.h, every op of halo_producer_kernel and both normalisations of input_halo_kernel through
one body each, at the smallest shapes where the shared index arithmetic can go wrong: one slice (C = 32: the slice index is always 0)
and three (C = 96: not a power of two), one image and three, the smallest extent an op accepts and an odd one above it.  The
references are those of the per-file tests (torch's CPU fp32; equality for ReLU, the max-pools and the input layers, POOL_TOL relative
for the L2 pool, whose bound test_gpu_dists_kernels derives); the halo ring holds +0 in every plane, also on the second use of the
cached buffer."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dists_ref  # noqa: E402
import lpips_ref  # noqa: E402
from test_gpu_dists_kernels import POOL_TOL  # noqa: E402
from test_gpu_lpips_kernels import _border_is_zero, _planes, _value  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nchw(f, x):
    return f(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


# op -> (the ops call, the reference on (B, H, W, C) fp32, the output extent of n, the relative bound (0: equality), its two extents)
OPS = {
    "relu": (lambda ops, x, B, H, W, C: ops.relu_pool_halo(x, B, H, W, C, pool=False), F.relu, lambda n: n, 0.0, ((1, 1), (5, 7))),
    "max2x2": (lambda ops, x, B, H, W, C: ops.relu_pool_halo(x, B, H, W, C, pool=True),
               lambda x: _nchw(lambda t: F.max_pool2d(t, 2, 2), F.relu(x)), lambda n: n // 2, 0.0, ((2, 2), (5, 7))),
    "max3x3s2": (lambda ops, x, B, H, W, C: ops.relu_maxpool3_halo(x, B, H, W, C),
                 lambda x: _nchw(lambda t: F.max_pool2d(t, 3, 2), F.relu(x)), lambda n: (n - 3) // 2 + 1, 0.0, ((3, 3), (7, 8))),
    "l2": (lambda ops, x, B, H, W, C: ops.relu_l2pool_halo(x, B, H, W, C),
           lambda x: _nchw(dists_ref.l2pool, torch.relu(x.double())), lambda n: (n + 1) // 2, POOL_TOL, ((1, 1), (5, 7))),
}
HALO_CASES = [(op, H, W) for op, spec in OPS.items() for H, W in spec[4]]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("op,H,W", HALO_CASES)
def test_halo_producer(op, H, W, C, B):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    run, ref, extent, tol, _ = OPS[op]
    g = torch.Generator().manual_seed(1000 * B + 10 * C + H)
    for use in range(2):                       # the second use of the cached buffer: the interior is replaced, the border still zero
        x = torch.randn(B, H, W, C, generator=g)
        x[0, 0, 0, 0], x[-1, -1, -1, -1] = -1.0, 1.0                # both signs whatever the draw, in the first and the last lane
        hp = run(ops, x.to(DEV).reshape(B * H * W, C), B, H, W, C)
        want = ref(x)
        assert (hp.B, hp.H, hp.W, hp.C) == (B, extent(H), extent(W), C) == tuple(want.shape), (op, use)
        p = _planes(hp)
        got = _value(p)[:, 1:-1, 1:-1]
        if tol:
            err = float(((got.double() - want).abs() / want).max())
            print(f"{op} {(B, H, W, C)} use {use}: relative error {err:.3e} (bound {tol})")
            assert float(want.min()) > 0.999e-6 and err <= tol, (op, use)
        else:
            assert torch.equal(got, want), (op, use)
        assert _border_is_zero(p), (op, use)
    assert ops.halo_planes_buffer(torch.device(DEV), hp.B, hp.H, hp.W, C) is hp


INPUTS = {"lpips": ("lpips_input", lambda u8: lpips_ref.input_layer(u8, torch.float32)),
          "dists": ("dists_input", lambda u8: dists_ref.input_layer(u8, torch.float32)[1])}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7)])
@pytest.mark.parametrize("metric", sorted(INPUTS))
def test_input_layer(metric, H, W, B):
    """images 1 .. B of B + 2 slots: the slots in front and behind stay untouched"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    name, ref = INPUTS[metric]
    rng = np.random.default_rng(100 * B + H)
    hp = ops.HaloPlanes(torch.zeros(3 * (B + 2) * (H + 2) * (W + 2) * 32, dtype=torch.int16, device=DEV), B + 2, H, W, 32)
    for use in range(2):
        u8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        u8[0, 0, 0], u8[-1, -1, -1] = (0, 255, 0), (255, 0, 255)    # the extremes of the u8 range, in the first and the last pixel
        getattr(ops, name)(torch.from_numpy(u8).to(DEV), hp, 1)
        p = _planes(hp)
        want = ref(u8).permute(0, 2, 3, 1)                           # (B, H, W, 3)
        assert torch.equal(_value(p)[1:-1, 1:-1, 1:-1, :3], want), use
        assert not bool(p[..., 3:].view(torch.int32).any()) and _border_is_zero(p), use
        assert not bool(p[:, 0].view(torch.int32).any()) and not bool(p[:, -1].view(torch.int32).any()), use
        assert float(want.min()) < -1.7 and float(want.max()) > 2.2
