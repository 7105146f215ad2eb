"""GPU: the kernels of csrc/fid.hip one by one: the patch producer and the pools bit for bit against torch
restatements, the mean, the resize and the Gram within bounds that follow from the number formats."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fid_ref import resize_f64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FC1          # a bf16 NaN pattern no split produces


@pytest.fixture(scope="module")
def ops():
    import sgic_amd  # noqa: F401
    from sgic_amd import ops as m
    return m


def _values(shape, seed):
    """fp32 values of mixed sign and magnitude, some exact zeros"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * torch.exp(2 * torch.randn(*shape, generator=g))
    x[torch.rand(*shape, generator=g) < 0.05] = 0.0
    return x


PATCH_CASES = [  # B, H, W, C, kh, kw, sh, sw, ph, pw, relu
    (2, 7, 9, 3, 3, 3, 2, 2, 0, 0, False),       # 27 -> 32 columns, uneven stride cut
    (1, 5, 6, 48, 5, 5, 1, 1, 2, 2, True),       # 1200 -> 1216 columns, mostly padding
    (2, 4, 5, 32, 1, 7, 1, 1, 0, 3, True),
    (2, 5, 4, 32, 7, 1, 1, 1, 3, 0, True),
    (1, 6, 7, 80, 3, 3, 1, 1, 0, 0, True),       # 720 -> 736 columns
    (1, 7, 7, 96, 3, 3, 2, 2, 0, 0, True),
    (1, 3, 3, 384, 1, 3, 1, 1, 0, 1, True),
    (3, 5, 7, 20, 3, 3, 1, 1, 1, 1, True),       # C % 8 != 0 with more than one workgroup: the scalar path
]


def _patch_reference(x_nhwc, kh, kw, sh, sw, ph, pw, relu):
    """(B, H, W, C) -> (B OH OW, kh kw C) in the column order (ky, kx, c): F.unfold's (c, ky, kx) reordered"""
    B, H, W, C = x_nhwc.shape
    x = x_nhwc.permute(0, 3, 1, 2)
    u = F.unfold(F.relu(x) if relu else x, (kh, kw), padding=(ph, pw), stride=(sh, sw))       # (B, C kh kw, L)
    L = u.shape[2]
    return u.view(B, C, kh * kw, L).permute(0, 3, 2, 1).reshape(B * L, kh * kw * C)


def _run_patches(ops, x2d, B, H, W, C, kh, kw, sh, sw, ph, pw, relu, cols=None):
    rows = B * ops.conv_out(H, kh, sh, ph) * ops.conv_out(W, kw, sw, pw)
    Kp = (kh * kw * C + 31) // 32 * 32
    buf = torch.full((3 * rows * Kp + Kp,), SENTINEL, dtype=torch.int16, device=DEV)          # one row longer than needed
    pl = ops.Planes(rows, Kp, DEV, buf=buf)
    ops.patches_split3(x2d, B, H, W, kh, kw, sh, sw, ph, pw, relu=relu, cols=cols, out=pl)
    torch.cuda.synchronize()
    assert bool((buf[3 * rows * Kp:] == SENTINEL).all()), "the extra row was written"
    return pl.float().cpu(), pl.rowmajor().cpu()


@pytest.mark.parametrize("case", PATCH_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_patches_bit_for_bit(ops, case):
    B, H, W, C, kh, kw, sh, sw, ph, pw, relu = case
    x = _values((B, H, W, C), 11 + C)
    got, planes = _run_patches(ops, x.view(B * H * W, C).to(DEV), B, H, W, C, kh, kw, sh, sw, ph, pw, relu)
    want = _patch_reference(x, kh, kw, sh, sw, ph, pw, relu)
    K = kh * kw * C
    assert got.shape[1] == (K + 31) // 32 * 32 and got.shape[0] == want.shape[0]
    assert torch.equal(got[:, :K], want)
    assert not bool(planes[:, :, K:].any()), "padding columns must be exactly 0 in every plane"


def test_patches_1x1_of_a_column_slice(ops):
    B, H, W, ld = 2, 3, 5, 96
    x = _values((B * H * W, ld), 5)
    got, _ = _run_patches(ops, x.to(DEV), B, H, W, 32, 1, 1, 1, 1, 0, 0, True, cols=(32, 32))
    assert torch.equal(got, F.relu(x[:, 32:64]))
    got, _ = _run_patches(ops, x.to(DEV), B, H, W, 30, 1, 1, 1, 1, 0, 0, True, cols=(33, 30))          # an unaligned slice: the scalar path
    assert torch.equal(got[:, :30], F.relu(x[:, 33:63])) and not bool(got[:, 30:].any())


def _pool_reference(x_nhwc, mode):
    """relu, then the pool with the kernel's own tap order (row-major, one fp32 accumulator, one division)"""
    B, H, W, C = x_nhwc.shape
    r = F.relu(x_nhwc)
    st, pad = (2, 0) if mode == "maxs2" else (1, 1)
    OH, OW = (H + 2 * pad - 3) // st + 1, (W + 2 * pad - 3) // st + 1
    out = torch.zeros(B, OH, OW, C)
    for oy in range(OH):
        for ox in range(OW):
            acc, cnt = torch.zeros(B, C), 0
            for dy in range(3):
                for dx in range(3):
                    iy, ix = oy * st - pad + dy, ox * st - pad + dx
                    if 0 <= iy < H and 0 <= ix < W:
                        acc = acc + r[:, iy, ix] if mode == "avg" else torch.maximum(acc, r[:, iy, ix])
                        cnt += 1
            out[:, oy, ox] = acc / cnt if mode == "avg" else acc
    return out


POOL_CASES = [("avg", 2, 5, 6, 32), ("avg", 1, 1, 1, 32), ("max", 1, 2, 3, 64), ("maxs2", 2, 7, 8, 64), ("maxs2", 1, 3, 3, 32)]


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_pools_bit_for_bit_into_a_column_slice(ops, case):
    mode, B, H, W, C = case
    x = _values((B, H, W, C), 23 + H)
    want = _pool_reference(x, mode)
    OH, OW = want.shape[1:3]
    fn = {"avg": ops.relu_avgpool3s1p1, "max": ops.relu_maxpool3s1p1, "maxs2": ops.relu_maxpool3s2}[mode]
    xd = x.view(B * H * W, C).to(DEV)
    dense = fn(xd, B, H, W)
    assert dense.shape == (B * OH * OW, C) and torch.equal(dense.cpu().view(B, OH, OW, C), want)
    wide = torch.full((B * OH * OW + 1, C + 40), -7.5, device=DEV)                             # a wider buffer, one row longer
    fn(xd, B, H, W, out=wide[:B * OH * OW], col0=8)
    wide = wide.cpu()
    assert torch.equal(wide[:-1, 8:8 + C].reshape(B, OH, OW, C), want)
    assert bool((wide[:, :8] == -7.5).all()) and bool((wide[:, 8 + C:] == -7.5).all()) and bool((wide[-1] == -7.5).all())
    xr = F.relu(x).permute(0, 3, 1, 2)
    if mode == "avg":
        t = F.avg_pool2d(xr, 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
        assert bool(((want - t).abs() <= 2 * torch.finfo(torch.float32).eps * t.abs()).all())    # 2 ulp: torch sums in another order
        if H == 1:
            assert torch.equal(want, F.relu(x))                                                  # the divisor is 1
    else:
        t = F.max_pool2d(xr, 3, 2) if mode == "maxs2" else F.max_pool2d(xr, 3, 1, 1)
        assert torch.equal(want, t.permute(0, 2, 3, 1))


@pytest.mark.parametrize("shape", [(2, 8, 8, 2048), (3, 3, 2, 64)], ids=lambda s: "x".join(map(str, s)))
def test_relu_mean_rows(ops, shape):
    B, H, W, C = shape
    x = _values((B * H * W, C), 31)
    got = ops.relu_mean_rows(x.to(DEV), B, H * W).cpu()
    r = F.relu(x).double().view(B, H * W, C)
    bound = (H * W) * 2.0 ** -23 * r.abs().sum(1) / (H * W)          # H W 2^-23 relative of sum |x|, on the mean's scale
    assert got.shape == (B, C) and bool(((got.double() - r.mean(1)).abs() <= bound).all())
    for b in range(B):                                                # a row of the batch = that image alone
        alone = ops.relu_mean_rows(x[b * H * W:(b + 1) * H * W].to(DEV), 1, H * W).cpu()
        assert torch.equal(alone[0], got[b])


def _resize(ops, canvas, desc):
    return ops.fid_resize299(torch.from_numpy(canvas).to(DEV), np.asarray(desc, dtype=np.int32)).cpu().numpy()


def test_resize(ops):
    """|dev - fp64| <= 1e-6: values in [0, 1] (then [-1, 1]) and a handful of fp32 roundings of at most 2^-24 each"""
    rng = np.random.default_rng(8)
    one = rng.integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)
    got = _resize(ops, one, [(0, 0, 0, 256, 256)])
    assert got.shape == (1, 299, 299, 3) and np.abs(got[0] - resize_f64(one[0])).max() <= 1e-6
    canvas = rng.integers(0, 256, (2, 300, 420, 3), dtype=np.uint8)
    desc = [(0, 0, 0, 300, 420), (1, 44, 164, 256, 256), (1, 269, 373, 31, 47), (0, 17, 3, 120, 299), (1, 0, 0, 1, 1)]
    got = _resize(ops, canvas, desc)                              # the second and third touch the bottom-right corner
    for g, (b, y0, x0, h, w) in zip(got, desc):
        assert np.abs(g - resize_f64(canvas[b, y0:y0 + h, x0:x0 + w])).max() <= 1e-6
    for h, w in ((31, 47), (600, 400), (299, 299)):
        img = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        got = _resize(ops, img, [(0, 0, 0, h, w)])
        assert np.abs(got[0] - resize_f64(img[0])).max() <= 1e-6
        if h == 299:                                              # nothing to interpolate: 2 (u / 255) - 1 in fp32 exactly
            assert np.array_equal(got[0], 2 * (img[0].astype(np.float32) / np.float32(255)) - 1)


@pytest.mark.parametrize("n,d", [(3, 32), (70, 96)])
def test_gram_f64(ops, n, d):
    a, b = _values((n, d), 41), _values((n + 5, d), 42)
    a64, b64 = a.double().numpy(), b.double().numpy()
    g = torch.Generator().manual_seed(43)
    ia = torch.randint(0, n, (n + 9,), generator=g, dtype=torch.int32)
    ib = torch.randint(0, n + 5, (2 * n,), generator=g, dtype=torch.int32)
    for ja, jb in ((None, None), (ia, ib), (ia, None)):
        got = ops.gram_f64(a.to(DEV), b.to(DEV), None if ja is None else ja.to(DEV), None if jb is None else jb.to(DEV)).cpu().numpy()
        ra, rb = a64 if ja is None else a64[ja.numpy()], b64 if jb is None else b64[jb.numpy()]
        bound = d * 2.0 ** -52 * (np.abs(ra) @ np.abs(rb).T)
        assert got.shape == (ra.shape[0], rb.shape[0]) and bool((np.abs(got - ra @ rb.T) <= bound).all())
    # the transposed feature matrix against itself, with K no multiple of the tile: second moments; a row of ones: column sums
    at = a.t().contiguous()
    got = ops.gram_f64(at.to(DEV)).cpu().numpy()
    assert bool((np.abs(got - a64.T @ a64) <= n * 2.0 ** -52 * (np.abs(a64).T @ np.abs(a64))).all())
    s = ops.gram_f64(torch.ones(1, n, device=DEV), at.to(DEV)).cpu().numpy()
    assert bool((np.abs(s[0] - a64.sum(0)) <= n * 2.0 ** -52 * np.abs(a64).sum(0)).all())


def test_einval_before_any_launch(ops):
    """every refusal comes back as SgicError (rc SGIC_EINVAL) from the host checks; the output buffers keep their contents"""
    from sgic_amd._lib import SgicError, lib, stream
    x = torch.zeros(2 * 4 * 4, 32, device=DEV)
    out = torch.full((8, 32), 3.0, device=DEV)
    pl = torch.full((3 * 32 * 32 + 64,), SENTINEL, dtype=torch.int16, device=DEV)
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    img = torch.full((1, 299, 299, 3), 3.0, device=DEV)
    null, p = ctypes.c_void_p(0), lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    d_ok = np.array([[0, 0, 0, 8, 8]], dtype=np.int32)
    d_dev = torch.from_numpy(d_ok).to(DEV)

    def resize(desc, canvas=p(u8), n=1):
        h = np.asarray(desc, dtype=np.int32)
        return lib.sgic_fid_resize299(canvas, 1, 8, 8, h.ctypes.data_as(ctypes.c_void_p), p(d_dev), n, p(img), stream())

    calls = [
        lambda: resize(d_ok, canvas=null), lambda: resize(d_ok, n=0),
        lambda: resize([[1, 0, 0, 8, 8]]), lambda: resize([[0, 1, 0, 8, 8]]), lambda: resize([[0, 0, 4, 8, 5]]),
        lambda: resize([[0, 0, 0, 0, 8]]), lambda: resize([[0, -1, 0, 4, 4]]),
        lambda: lib.sgic_patches_split3(null, 32, 0, 2, 4, 4, 32, 1, 1, 1, 1, 0, 0, 1, p(pl), stream()),
        lambda: lib.sgic_patches_split3(p(x), 32, 0, 0, 4, 4, 32, 1, 1, 1, 1, 0, 0, 1, p(pl), stream()),
        lambda: lib.sgic_patches_split3(p(x), 32, 0, 2, 4, 4, 32, 1, 1, 1, 1, 0, 0, 1, p(pl, 2), stream()),        # misaligned planes
        lambda: lib.sgic_patches_split3(p(x), 32, 8, 2, 4, 4, 32, 1, 1, 1, 1, 0, 0, 1, p(pl), stream()),           # slice outside ld
        lambda: lib.sgic_patches_split3(p(x), 32, 0, 2, 4, 4, 32, 7, 1, 1, 1, 0, 0, 1, p(pl), stream()),           # no output row
        lambda: lib.sgic_patches_split3(p(x), 32, 0, 1 << 28, 4, 4, 32, 1, 1, 1, 1, 0, 0, 1, p(pl), stream()),     # 2^32 rows
        lambda: lib.sgic_relu_maxpool3s2(p(x), 2, 2, 8, 32, p(out), 32, 0, stream()),                             # H < 3
        lambda: lib.sgic_relu_avgpool3s1p1(p(x), 2, 4, 4, 30, p(out), 32, 0, stream()),                           # C % 4
        lambda: lib.sgic_relu_maxpool3s1p1(p(x), 2, 4, 4, 32, p(out), 32, 4, stream()),                           # slice outside ldo
        lambda: lib.sgic_relu_maxpool3s1p1(p(x), 2, 4, 4, 32, p(out, 4), 32, 0, stream()),                        # misaligned
        lambda: lib.sgic_relu_mean_rows(p(x), 0, 16, 32, p(out), stream()),
        lambda: lib.sgic_relu_mean_rows(p(x), 2, 16, 32, null, stream()),
        lambda: lib.sgic_gram_f64(p(x), ctypes.c_long(32), null, 32, 0, p(x), ctypes.c_long(32), null, 32, 4, 32, p(out), ctypes.c_long(4), stream()),
        lambda: lib.sgic_gram_f64(p(x), ctypes.c_long(32), null, 32, 33, p(x), ctypes.c_long(32), null, 32, 4, 32, p(out), ctypes.c_long(4), stream()),
        lambda: lib.sgic_gram_f64(p(x), ctypes.c_long(16), null, 32, 4, p(x), ctypes.c_long(32), null, 32, 4, 32, p(out), ctypes.c_long(4), stream()),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, f"call {i}: expected SGIC_EINVAL"
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((pl == SENTINEL).all()) and bool((img == 3.0).all())
    with pytest.raises(SgicError):
        ops.fid_resize299(u8, np.array([[0, 0, 0, 9, 8]], dtype=np.int32))
