"""GPU: the three kernels of csrc/lpips_alex.hip one by one, each against torch's CPU fp32 for equality: the input layer is the same
single operations, ReLU and max-pool select values, and the three bf16 planes of a normal fp32 value sum to it exactly, so
Planes.float() returns what was written."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_alex_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x1234


def _bits(planes):
    """a Planes' three planes bit for bit, row-major (3, rows, cols) int16 on the host"""
    return planes.rowmajor().cpu()


def _conv1_want(u8):
    """(B, H, W, 3) u8 -> (B h1 w1, 384) fp32: F.unfold of the zero-padded input layer, reordered from (c, ky, kx) to (ky, kx, c)"""
    B = u8.shape[0]
    cols = F.unfold(ref.input_layer(u8, torch.float32), 11, padding=2, stride=4)               # (B, 3 * 121, h1 * w1)
    L = cols.shape[2]
    cols = cols.reshape(B, 3, 121, L).permute(0, 3, 2, 1).reshape(B * L, 363)
    return torch.cat([cols, torch.zeros(B * L, 21)], dim=1)


@pytest.mark.parametrize("B,H,W", [(2, 31, 33), (1, 37, 50)])
def test_conv1_patches(B, H, W):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    rng = np.random.default_rng(H * W)
    a = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    a[0, 0, 0], a[0, 0, 1] = (0, 0, 0), (255, 255, 255)
    h1, w1 = ref.extents(H)[0], ref.extents(W)[0]
    pl = ops.Planes(2 * B * h1 * w1, 384, DEV)
    ops.lpips_alex_conv1_patches(torch.from_numpy(a).to(DEV), pl, 0)
    ops.lpips_alex_conv1_patches(torch.from_numpy(b).to(DEV), pl, B)
    want = _conv1_want(np.concatenate([a, b]))
    got = pl.float().cpu()
    assert got.shape == want.shape == (2 * B * h1 * w1, 384)
    assert torch.equal(got, want)
    assert not bool(_bits(pl)[:, :, 363:].any())                                  # the padding columns hold +0 in every plane
    assert float(want.min()) < -2.0 and float(want.max()) > 2.5                   # the extremes of the u8 range went through
    assert bool((want[:, :363] == 0.0).any())                                     # and some taps fell outside the image


def test_conv1_patches_leave_other_images_alone():
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    B, H, W = 1, 31, 33
    h1, w1 = ref.extents(H)[0], ref.extents(W)[0]
    per = h1 * w1
    u8 = np.random.default_rng(11).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    pl = ops.Planes(3 * per, 384, DEV, buf=torch.full((3 * 3 * per * 384,), SENTINEL, dtype=torch.int16, device=DEV))
    ops.lpips_alex_conv1_patches(torch.from_numpy(u8).to(DEV), pl, 1)
    bits = _bits(pl)
    assert bool((bits[:, :per] == SENTINEL).all()) and bool((bits[:, 2 * per:] == SENTINEL).all())
    assert torch.equal(pl.float().cpu()[per:2 * per], _conv1_want(u8))


@pytest.mark.parametrize("B,H,W,C", [(2, 7, 8, 64), (1, 3, 5, 32)])
def test_relu_maxpool3_patches5(B, H, W, C):
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib, ops
    g = torch.Generator().manual_seed(B * 1000 + C)
    x = torch.randn(B, H, W, C, generator=g)
    assert float(x.min()) < 0.0
    pooled = F.max_pool2d(F.relu(x).permute(0, 3, 1, 2), 3, 2)                                  # (B, C, PH, PW)
    PH, PW = pooled.shape[2:]
    assert (PH, PW) == ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
    if (H, W) == (3, 5):
        assert (PH, PW) == (1, 2)
    cols = F.unfold(pooled, 5, padding=2)                                                        # (B, C * 25, PH * PW)
    want = cols.reshape(B, C, 25, PH * PW).permute(0, 3, 2, 1).reshape(B * PH * PW, 25 * C)
    xd = x.to(DEV).reshape(B * H * W, C)
    pl = ops.relu_maxpool3_patches5(xd, B, H, W, C)
    assert pl.shape == (B * PH * PW, 25 * C)
    assert torch.equal(pl.float().cpu(), want)
    # into a buffer full of a sentinel: every element is written, the zeros of the padding taps too
    pl = ops.Planes(B * PH * PW, 25 * C, DEV, buf=torch.full((3 * B * PH * PW * 25 * C,), SENTINEL, dtype=torch.int16, device=DEV))
    _lib.call("sgic_relu_maxpool3_patches5_split3", xd, B, H, W, C, pl.t)
    assert torch.equal(pl.float().cpu(), want)
    zero = want == 0.0
    assert bool(zero.any()) and not bool(_bits(pl).permute(1, 2, 0)[zero].any())                # the padding taps hold +0 in every plane


@pytest.mark.parametrize("B,H,W,C", [(2, 7, 8, 192), (1, 3, 3, 32)])
def test_relu_maxpool3_halo(B, H, W, C):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + C + 1)
    for use in range(2):                       # the second use of the cached buffer: the interior is replaced, the border still zero
        x = torch.randn(B, H, W, C, generator=g)
        assert float(x.min()) < 0.0
        hp = ops.relu_maxpool3_halo(x.to(DEV).reshape(B * H * W, C), B, H, W, C)
        want = F.max_pool2d(F.relu(x).permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
        assert (hp.B, hp.H, hp.W, hp.C) == (B, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C) == (B,) + tuple(want.shape[1:])
        p = hp.t[:3 * B * (hp.H + 2) * (hp.W + 2) * C].view(3, C // 32, B, hp.H + 2, hp.W + 2, 32)
        p = (p.permute(0, 2, 3, 4, 1, 5).reshape(3, B, hp.H + 2, hp.W + 2, C).to(torch.int32) << 16).view(torch.float32).cpu()
        assert torch.equal(((p[0] + p[1]) + p[2])[:, 1:-1, 1:-1], want), use
        bits = p.view(torch.int32)
        assert not (bool(bits[:, :, 0].any()) or bool(bits[:, :, -1].any()) or bool(bits[:, :, :, 0].any()) or bool(bits[:, :, :, -1].any())), use
    assert ops.halo_planes_buffer(torch.device(DEV), hp.B, hp.H, hp.W, C) is hp


def test_refusals_come_before_any_launch():
    """one case per listed condition and entry: every refused call is stopped by the host-side checks, the outputs keep their fill"""
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib
    B, H, W, C = 1, 9, 11, 64
    planes = torch.full((8 + 3 * 2 * 25 * C * H * W,), SENTINEL, dtype=torch.int16, device=DEV)
    img = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    x = torch.zeros(8 + B * H * W * C, dtype=torch.float32, device=DEV)
    big = 1 << 16                                  # 2^16 images of 2^10 x 2^10: 2^36 pixels, never touched
    bad = {
        "sgic_lpips_alex_conv1_patches_split3": [
            (None, B, H, W, 2, 0, planes), (img, B, H, W, 2, 0, None),                                  # a null pointer
            (img, 0, H, W, 2, 0, planes),                                                               # B < 1
            (img, B, 6, W, 2, 0, planes), (img, B, H, 6, 2, 0, planes),                                 # no output row / column
            (img, B, H, W, 2, 0, planes[1:]),                                                           # 2 bytes off
            (img, B, H, W, 2, 2, planes), (img, B, H, W, 2, -1, planes), (img, 2, H, W, 2, 1, planes),  # slots outside the buffer
            (img, 1, 1 << 10, 1 << 10, big, 0, planes), (img, 1 << 12, 1 << 10, 1 << 10, big, 0, planes)],   # 2^31 rows or more
        "sgic_relu_maxpool3_patches5_split3": [
            (None, B, H, W, C, planes), (x, B, H, W, C, None), (x, 0, H, W, C, planes),
            (x, B, 2, W, C, planes), (x, B, H, 2, C, planes),                                            # the pool leaves nothing
            (x, B, H, W, 48, planes), (x, B, H, W, 0, planes),                                           # C % 32
            (x[1:], B, H, W, C, planes), (x, B, H, W, C, planes[4:]),                                    # 4 and 8 bytes off
            (x, big, 1 << 10, 1 << 10, C, planes)],
        "sgic_relu_maxpool3_halo_split3": [
            (None, B, H, W, C, planes), (x, B, H, W, C, None), (x, 0, H, W, C, planes),
            (x, B, 2, W, C, planes), (x, B, H, 2, C, planes),
            (x, B, H, W, 48, planes), (x, B, H, W, 0, planes),
            (x[1:], B, H, W, C, planes), (x, B, H, W, C, planes[4:]),
            (x, big, 1 << 10, 1 << 10, C, planes)],
    }
    for name, calls in bad.items():
        for args in calls:
            with pytest.raises(_lib.SgicError, match="rc=-1"):
                _lib.call(name, *args)
    torch.cuda.synchronize()
    assert bool((planes == SENTINEL).all())
