"""GPU: the three kernels of csrc/lpips.hip one by one.  The input layer and ReLU / max-pool are compared for equality (torch's CPU
fp32 does the same single operations, and the three bf16 planes of a normal fp32 value sum to it exactly); the head against numpy
fp64 within 1e-12 relative: it accumulates nonnegative fp64 terms (at most 512 per pixel, then the pixels), each with a few roundings
of 2^-53, in another order than numpy, and multiplies by 1 / (n + 1e-10) where the definition divides."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEAD_TOL = 1e-12


def _planes(hp):
    """HaloPlanes -> the three planes as fp32 (3, B, H+2, W+2, C)"""
    p = hp.t[:3 * hp.B * (hp.H + 2) * (hp.W + 2) * hp.C].view(3, hp.C // 32, hp.B, hp.H + 2, hp.W + 2, 32)
    p = p.permute(0, 2, 3, 4, 1, 5).reshape(3, hp.B, hp.H + 2, hp.W + 2, hp.C)
    return (p.to(torch.int32) << 16).view(torch.float32).cpu()


def _value(p):
    return (p[0] + p[1]) + p[2]


def _border_is_zero(p):
    """bitwise: every plane's halo ring holds +0"""
    bits = p.view(torch.int32)
    return not (bool(bits[:, :, 0].any()) or bool(bits[:, :, -1].any()) or bool(bits[:, :, :, 0].any()) or bool(bits[:, :, :, -1].any()))


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 16, 16)])
def test_input_layer(B, H, W):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    a[0, 0, 0], a[0, 0, 1] = (0, 0, 0), (255, 255, 255)
    hp = ops.HaloPlanes(torch.zeros(3 * 2 * B * (H + 2) * (W + 2) * 32, dtype=torch.int16, device=DEV), 2 * B, H, W, 32)
    ops.lpips_input(torch.from_numpy(b).to(DEV), hp, B)            # the second half alone: the first stays untouched
    p = _planes(hp)
    assert not bool(p[:, :B].view(torch.int32).any())
    ops.lpips_input(torch.from_numpy(a).to(DEV), hp, 0)
    p = _planes(hp)
    want = ref.input_layer(np.concatenate([a, b]), torch.float32).permute(0, 2, 3, 1)        # (2B, H, W, 3)
    got = _value(p)[:, 1:-1, 1:-1]
    assert torch.equal(got[..., :3], want)
    assert not bool(p[..., 3:].view(torch.int32).any()) and _border_is_zero(p)
    assert float(want.min()) < -2.0 and float(want.max()) > 2.5       # the extremes of the u8 range went through


@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 16, 16)])
def test_relu_pool_halo(B, H, W, C, pool):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + C + int(pool))
    for use in range(2):                       # the second use of the cached buffer: the interior is replaced, the border still zero
        x = torch.randn(B, H, W, C, generator=g)
        assert float(x.min()) < 0.0
        hp = ops.relu_pool_halo(x.to(DEV).reshape(B * H * W, C), B, H, W, C, pool=pool)
        want = F.relu(x)
        if pool:
            want = F.max_pool2d(want.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert (hp.B, hp.H, hp.W, hp.C) == (B,) + tuple(want.shape[1:3]) + (C,)
        if pool and (H, W) == (5, 7):
            assert (hp.H, hp.W) == (2, 3)
        p = _planes(hp)
        assert torch.equal(_value(p)[:, 1:-1, 1:-1], want), use
        assert _border_is_zero(p), use
    assert ops.halo_planes_buffer(torch.device(DEV), hp.B, hp.H, hp.W, C) is hp


def _head_ref(feat, w, B):
    f = np.maximum(feat.astype(np.float64), 0.0)
    u = f / (np.sqrt((f * f).sum(axis=2, keepdims=True)) + 1e-10)
    return (w.astype(np.float64) * (u[:B] - u[B:]) ** 2).sum(axis=2).mean(axis=1)


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (40, 72)])
def test_head(H, W, C):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    B, HW = 2, H * W
    rng = np.random.default_rng(HW + C)
    feat = rng.standard_normal((2 * B, HW, C)).astype(np.float32)
    feat[1, HW // 2] = -np.abs(feat[1, HW // 2])                     # pixels with no positive value: on one side ...
    if HW > 1:                                                       # ... and on both (a single pixel would leave the distance 0)
        feat[0, 0], feat[B, 0] = -np.abs(feat[0, 0]), -1.0
    w = rng.uniform(0.0, 2.0 / C, C).astype(np.float32)
    want = _head_ref(feat, w, B)
    d_feat, d_w = torch.from_numpy(feat).to(DEV).reshape(2 * B * HW, C), torch.from_numpy(w).to(DEV)
    got = ops.lpips_head(d_feat, d_w, B, H, W)
    again = ops.lpips_head(d_feat, d_w, B, H, W)
    assert got.dtype == torch.float64 and got.shape == (B,)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                 # the same bits twice
    got = got.cpu().numpy()
    err = float((np.abs(got - want) / want).max())
    print(f"head {H}x{W} C={C}: {got.tolist()} relative error {err:.3e}")
    assert np.all(np.isfinite(got)) and np.all(want > 0.0) and err <= HEAD_TOL
    same = ops.lpips_head(torch.cat([d_feat[:B * HW], d_feat[:B * HW]]), d_w, B, H, W).cpu().numpy()
    assert np.all(same == 0.0)


def test_refusals_come_before_any_launch():
    """every refused call is stopped by the host-side checks: the outputs keep their fill"""
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib
    size, B, H, W, C = ctypes.c_size_t, 1, 4, 6, 64
    FILL = 0x1234
    planes = torch.full((8 + 3 * 2 * (H + 2) * (W + 2) * C,), FILL, dtype=torch.int16, device=DEV)
    img = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    x = torch.zeros(8 + 2 * B * H * W * C, dtype=torch.float32, device=DEV)
    w = torch.zeros(4 + C, dtype=torch.float32, device=DEV)
    d = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    nbytes = size(0)
    _lib.call("sgic_lpips_head_work_bytes", B, H, W, ctypes.byref(nbytes))
    assert nbytes.value >= 8
    work = torch.zeros(16 + nbytes.value, dtype=torch.uint8, device=DEV)
    nb = size(nbytes.value)
    bad = {
        "sgic_lpips_input_split3": [(None, B, H, W, 2, 0, planes), (img, B, H, W, 2, 0, None), (img, 0, H, W, 2, 0, planes),
                                    (img, B, 0, W, 2, 0, planes), (img, B, H, 0, 2, 0, planes),
                                    (img, B, H, W, 2, 2, planes), (img, B, H, W, 2, -1, planes),        # a slot outside the buffer
                                    (img, B, H, W, 2, 0, planes[1:])],                                  # 2 bytes off
        "sgic_relu_pool_halo_split3": [(None, B, H, W, C, 1, planes), (x, B, H, W, C, 1, None), (x, 0, H, W, C, 0, planes),
                                       (x, B, 0, W, C, 0, planes), (x, B, H, 0, C, 0, planes), (x, B, H, W, 48, 0, planes),
                                       (x, B, H, W, 0, 0, planes), (x[1:], B, H, W, C, 0, planes), (x, B, H, W, C, 0, planes[4:]),
                                       (x, B, 1, W, C, 1, planes), (x, B, H, 1, C, 1, planes)],          # the pool leaves nothing
        "sgic_lpips_head": [(None, w, B, H, W, C, work, nb, d), (x, None, B, H, W, C, work, nb, d), (x, w, B, H, W, C, None, nb, d),
                            (x, w, B, H, W, C, work, nb, None), (x, w, 0, H, W, C, work, nb, d), (x, w, B, 0, W, C, work, nb, d),
                            (x, w, B, H, 0, C, work, nb, d), (x, w, B, H, W, 48, work, nb, d), (x[1:], w, B, H, W, C, work, nb, d),
                            (x, w[1:], B, H, W, C, work, nb, d), (x, w, B, H, W, C, work[8:], nb, d),
                            (x, w, B, H, W, C, work, size(nbytes.value - 1), d)],                        # a workspace one byte short
    }
    for name, calls in bad.items():
        for args in calls:
            with pytest.raises(_lib.SgicError, match="rc=-1"):
                _lib.call(name, *args)
    for args in ((0, H, W), (B, 0, W), (B, H, 0)):
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call("sgic_lpips_head_work_bytes", *args, ctypes.byref(nbytes))
    torch.cuda.synchronize()
    assert bool((planes == FILL).all()) and bool((d == -7.0).all())
