"""GPU: the kernels of csrc/dists.hip one by one.  The input layer is compared for equality (torch's CPU fp32 does the same single
operations, and the three bf16 planes of a normal fp32 value sum to it exactly); the u8 moments are integers; the L2 pool against
the fp64 restatement within 1e-6 relative: nine nonnegative fp32 terms (a rounding each for the square; the weights are powers of
two), eight additions, the 1e-12, one square root, no cancellation -- at most 11 roundings of 2^-24 on the radicand, halved by the
root, plus the root's own: below 4e-7.  The moments against numpy fp64 within 1e-12 relative: nonnegative fp64 terms with exact
products, added in another order than numpy."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dists_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOL_TOL = 1e-6
MOM_TOL = 1e-12


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


def _pairs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    a[0, 0, 0], a[0, 0, 1] = (0, 0, 0), (255, 255, 255)
    return a, b


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 16, 16)])
def test_input_layer(B, H, W):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    a, b = _pairs(B, H, W, 3)
    hp = ops.HaloPlanes(torch.zeros(3 * 2 * B * (H + 2) * (W + 2) * 32, dtype=torch.int16, device=DEV), 2 * B, H, W, 32)
    ops.dists_input(torch.from_numpy(b).to(DEV), hp, B)            # the second half alone: the first stays untouched
    p = _planes(hp)
    assert not bool(p[:, :B].view(torch.int32).any())
    ops.dists_input(torch.from_numpy(a).to(DEV), hp, 0)
    p = _planes(hp)
    want = ref.input_layer(np.concatenate([a, b]), torch.float32)[1].permute(0, 2, 3, 1)        # (2B, H, W, 3)
    got = _value(p)[:, 1:-1, 1:-1]
    assert torch.equal(got[..., :3], want)
    assert not bool(p[..., 3:].view(torch.int32).any()) and _border_is_zero(p)
    assert float(want.min()) < -2.0 and float(want.max()) > 2.5       # the extremes of the u8 range went through


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 16, 16), (1, 70, 130)])
def test_moments_u8(B, H, W):
    """(1, 70, 130): 9 100 pixels, three workgroups per pair, the last one partly filled"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    a, b = _pairs(B, H, W, 4)
    a, b = np.concatenate([a, np.full_like(a[:1], 17), a[:1]]), np.concatenate([b, np.full_like(b[:1], 200), a[:1]])    # + flat, + identical
    ai, bi = a.astype(np.int64).reshape(B + 2, -1, 3), b.astype(np.int64).reshape(B + 2, -1, 3)
    want = np.stack([ai.sum(1), bi.sum(1), (ai * ai).sum(1), (bi * bi).sum(1), (ai * bi).sum(1)], axis=2)
    out = torch.full((B + 2, 3, 5), -1, dtype=torch.int64, device=DEV)          # the entry clears it
    got = ops.dists_moments_u8(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    n = H * W
    assert want[B].tolist() == [[17 * n, 200 * n, 289 * n, 40000 * n, 3400 * n]] * 3


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 16, 16), (1, 1, 9)])
def test_relu_l2pool_halo(B, H, W, C):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + C + H)
    for use in range(2):                       # the second use of the cached buffer: the interior is replaced, the border still zero
        x = torch.randn(B, H, W, C, generator=g)
        x[0, 0, W // 2] = -x[0, 0, W // 2].abs()                   # a pixel with no positive value
        x[0, :, :, 5] = -1.0                                       # a channel with none: every output is sqrt(1e-12)
        assert float(x.min()) < 0.0
        hp = ops.relu_l2pool_halo(x.to(DEV).reshape(B * H * W, C), B, H, W, C)
        want = ref.l2pool(torch.relu(x.double()).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        assert (hp.B, hp.H, hp.W, hp.C) == (B, (H + 1) // 2, (W + 1) // 2, C) == (B,) + tuple(want.shape[1:3]) + (C,)
        p = _planes(hp)
        got = _value(p)[:, 1:-1, 1:-1].double()
        err = float(((got - want).abs() / want).max())
        print(f"l2pool {(B, H, W, C)} use {use}: relative error {err:.3e} (bound {POOL_TOL})")
        assert float(want.min()) > 0.999e-6 and float(want[0, ..., 5].max()) < 1.001e-6 and err <= POOL_TOL, use
        assert _border_is_zero(p), use
    assert ops.halo_planes_buffer(torch.device(DEV), hp.B, hp.H, hp.W, C) is hp


def _moments_ref(feat, B):
    f = np.maximum(feat.astype(np.float64), 0.0)
    x, y = f[:B], f[B:]
    return np.stack([x.sum(1), y.sum(1), (x * x).sum(1), (y * y).sum(1), (x * y).sum(1)], axis=1)       # (B, 5, C)


def _head_ref(sums, alpha, beta, n):
    mx, my = sums[:, 0] / n, sums[:, 1] / n
    vx, vy, cxy = sums[:, 2] / n - mx * mx, sums[:, 3] / n - my * my, sums[:, 4] / n - mx * my
    S1 = (2.0 * (mx * my) + 1e-6) / ((mx * mx + my * my) + 1e-6)
    S2 = (2.0 * cxy + 1e-6) / ((vx + vy) + 1e-6)
    return np.stack([(alpha.astype(np.float64) * (1.0 - S1)).sum(1), (beta.astype(np.float64) * (1.0 - S2)).sum(1)], axis=1)


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (40, 72)])
def test_moments_and_head(H, W, C):
    """1, 63 and 2 880 pixels: one partly filled workgroup, and twelve workgroups the last of which is partly filled"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    B, HW = 2, H * W
    rng = np.random.default_rng(HW + C)
    feat = rng.standard_normal((2 * B, HW, C)).astype(np.float32)
    feat[B:] = (feat[:B] + 0.5 * feat[B:]).astype(np.float32)        # correlated sides
    feat[1, HW // 2] = -np.abs(feat[1, HW // 2])                     # a pixel with no positive value
    feat[0, :, 3] = -1.0                                             # a channel that is zero on one side
    want = _moments_ref(feat, B)
    d_feat = torch.from_numpy(feat).to(DEV).reshape(2 * B * HW, C)
    got = ops.dists_moments(d_feat, B, H, W)
    again = ops.dists_moments(d_feat, B, H, W)
    assert got.dtype == torch.float64 and got.shape == (B, 5, C)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                 # the same bits twice
    sums = got.cpu().numpy()
    assert np.all(sums[0, 0, 3] == 0.0) and np.all(sums[0, 2, 3] == 0.0) and np.all(sums[0, 4, 3] == 0.0)
    nz = want != 0.0
    err = float((np.abs(sums - want)[nz] / want[nz]).max())
    print(f"moments {H}x{W} C={C}: relative error {err:.3e} (bound {MOM_TOL})")
    assert np.array_equal(sums == 0.0, ~nz) and err <= MOM_TOL
    # the head on these sums: against numpy on the same sums (the same expression, the channels in another order)
    alpha, beta = rng.uniform(0.0, 0.2, C).astype(np.float32), rng.uniform(0.0, 0.2, C).astype(np.float32)
    d_al, d_be = torch.from_numpy(alpha).to(DEV), torch.from_numpy(beta).to(DEV)
    terms = ops.dists_head(got, d_al, d_be, H, W)
    terms2 = ops.dists_head(got, d_al, d_be, H, W)
    assert terms.shape == (B, 2) and terms.dtype == torch.float64 and torch.equal(terms.view(torch.int64), terms2.view(torch.int64))
    want_t = _head_ref(sums, alpha, beta, float(HW))
    err_t = float(np.abs(terms.cpu().numpy() - want_t).max())
    print(f"head {H}x{W} C={C}: {terms.cpu().numpy().tolist()} absolute error {err_t:.3e}")
    assert err_t <= 1e-12 * max(1.0, float(np.abs(want_t).max()))
    # x == y: exactly 0.0 for both terms
    same = ops.dists_moments(torch.cat([d_feat[:B * HW], d_feat[:B * HW]]), B, H, W)
    assert torch.equal(same[:, 0], same[:, 1]) and torch.equal(same[:, 2], same[:, 3]) and torch.equal(same[:, 2], same[:, 4])
    zero = ops.dists_head(same, d_al, d_be, H, W).cpu().numpy()
    assert np.all(zero == 0.0)


def test_moments_with_a_longer_pixel_range_per_workgroup():
    """257 x 256 = 65 792 pixels: past 256 * 256 a workgroup's range grows to 512 pixels (129 workgroups, the last half filled).  The same bound: on the device a sum passes through 16 + 32 + 17 + 8 additions of nonnegative fp64 terms (1e-14
    relative at the most); numpy adds the 65 792 rows one after the other, whose roundings walk to about sqrt(n) 2^-53 = 3e-14"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    B, H, W, C = 1, 257, 256, 32
    rng = np.random.default_rng(11)
    feat = rng.standard_normal((2 * B, H * W, C)).astype(np.float32)
    want = _moments_ref(feat, B)
    d_feat = torch.from_numpy(feat).to(DEV).reshape(2 * B * H * W, C)
    got = ops.dists_moments(d_feat, B, H, W)
    assert torch.equal(got.view(torch.int64), ops.dists_moments(d_feat, B, H, W).view(torch.int64))
    err = float((np.abs(got.cpu().numpy() - want) / want).max())
    print(f"moments {H}x{W} C={C}: relative error {err:.3e} (bound {MOM_TOL})")
    assert err <= MOM_TOL


def test_refusals_come_before_any_launch():
    """every refused call is stopped by the host-side checks: the outputs keep their fill"""
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib, ops
    size, B, H, W, C = ctypes.c_size_t, 1, 4, 6, 64
    FILL = 0x1234
    planes = torch.full((8 + 3 * 2 * (H + 2) * (W + 2) * C,), FILL, dtype=torch.int16, device=DEV)
    img = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    x = torch.zeros(8 + 2 * B * H * W * C, dtype=torch.float32, device=DEV)
    al = torch.zeros(C, dtype=torch.float32, device=DEV)
    m8 = torch.full((B * 15 + 1,), -7, dtype=torch.int64, device=DEV)
    sums = torch.full((B * 5 * C + 1,), -7.0, dtype=torch.float64, device=DEV)
    terms = torch.full((B * 2 + 1,), -7.0, dtype=torch.float64, device=DEV)
    nbytes = size(0)
    _lib.call("sgic_dists_moments_work_bytes", B, H, W, C, ctypes.byref(nbytes))
    assert nbytes.value == B * 1 * 5 * C * 8
    work = torch.zeros(16 + nbytes.value, dtype=torch.uint8, device=DEV)
    nb = size(nbytes.value)
    m8_off = m8.view(torch.uint8)[4:-4].view(torch.int32)              # 4 bytes off
    sums_off = sums.view(torch.uint8)[4:-4].view(torch.float32)
    bad = {
        "sgic_dists_input_split3": [(None, B, H, W, 2, 0, planes), (img, B, H, W, 2, 0, None), (img, 0, H, W, 2, 0, planes),
                                    (img, B, 0, W, 2, 0, planes), (img, B, H, 0, 2, 0, planes),
                                    (img, B, H, W, 2, 2, planes), (img, B, H, W, 2, -1, planes),        # a slot outside the buffer
                                    (img, B, H, W, 2, 0, planes[1:])],                                  # 2 bytes off
        "sgic_dists_moments_u8": [(None, img, B, H, W, m8), (img, None, B, H, W, m8), (img, img, B, H, W, None), (img, img, 0, H, W, m8),
                                  (img, img, B, 0, W, m8), (img, img, B, H, 0, m8), (img, img, B, H, W, m8_off)],
        "sgic_relu_l2pool_halo_split3": [(None, B, H, W, C, planes), (x, B, H, W, C, None), (x, 0, H, W, C, planes),
                                         (x, B, 0, W, C, planes), (x, B, H, 0, C, planes), (x, B, H, W, 48, planes),
                                         (x, B, H, W, 0, planes), (x[1:], B, H, W, C, planes), (x, B, H, W, C, planes[4:])],
        "sgic_dists_moments": [(None, B, H, W, C, work, nb, sums), (x, B, H, W, C, None, nb, sums), (x, B, H, W, C, work, nb, None),
                               (x, 0, H, W, C, work, nb, sums), (x, B, 0, W, C, work, nb, sums), (x, B, H, 0, C, work, nb, sums),
                               (x, B, H, W, 48, work, nb, sums), (x, B, H, W, 0, work, nb, sums), (x, B, H, W, 2048, work, nb, sums),
                               (x[1:], B, H, W, C, work, nb, sums), (x, B, H, W, C, work[8:], nb, sums),
                               (x, B, H, W, C, work, nb, sums_off),
                               (x, B, H, W, C, work, size(nbytes.value - 1), sums)],                    # a workspace one byte short
        "sgic_dists_head": [(None, al, al, B, H, W, C, terms), (sums, None, al, B, H, W, C, terms), (sums, al, None, B, H, W, C, terms),
                            (sums, al, al, B, H, W, C, None), (sums, al, al, 0, H, W, C, terms), (sums, al, al, B, 0, W, C, terms),
                            (sums, al, al, B, H, 0, C, terms), (sums, al, al, B, H, W, 48, terms), (sums_off, al, al, B, H, W, C, terms)],
    }
    for name, calls in bad.items():
        for args in calls:
            with pytest.raises(_lib.SgicError, match="rc=-1"):
                _lib.call(name, *args)
    for args in ((0, H, W, C), (B, 0, W, C), (B, H, 0, C), (B, H, W, 48), (B, H, W, 2048)):
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call("sgic_dists_moments_work_bytes", *args, ctypes.byref(nbytes))
    # the ops wrappers pass the library's refusal on
    hp = ops.HaloPlanes(planes[8:8 + 3 * 2 * (H + 2) * (W + 2) * 32][1:], 2, H, W, 32)
    with pytest.raises((AssertionError, _lib.SgicError)):
        ops.dists_input(img, hp, 0)
    with pytest.raises(_lib.SgicError, match="rc=-1"):
        ops.dists_moments(torch.zeros(2 * B * H * W, 48, dtype=torch.float32, device=DEV), B, H, W)
    with pytest.raises(_lib.SgicError, match="rc=-1"):
        ops.relu_l2pool_halo(torch.zeros(B * H * W, 48, dtype=torch.float32, device=DEV), B, H, W, 48)
    torch.cuda.synchronize()
    assert bool((planes == FILL).all()) and bool((m8 == -7).all()) and bool((sums == -7.0).all()) and bool((terms == -7.0).all())
