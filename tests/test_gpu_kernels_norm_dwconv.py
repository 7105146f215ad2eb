"""GPU tests of LayerNorm (csrc/norm.hip) and the depthwise convolution (csrc/misc.hip) at their branch points, in the sentinel-prefill
style of test_gpu_kernels.py: every output is pre-filled with a bit pattern that must survive wherever the operation does not write.

LayerNorm against torch.nn.functional.layer_norm in fp64: every width class (the register kernel's NV = 1..8, the generic kernel with
idle lanes, one pass, two passes, and above the register path) with a part-full last workgroup, strided x and out, the segment map
with SiLU fused, constant rows, rows whose mean is 30 and 1000 standard deviations away, the planes output at three widths, and the
refusals.  The depthwise kernels against the ordered fp32 restatement kernels_ref.dwconv_ordered32, bit for bit: that pins
dwconv_kernel and dwconv_x4_kernel each, and therefore to each other."""
import pytest
import torch
import torch.nn.functional as F

import kernels_ref as kr
from kernels_ref import from_tm16 as _from_tm16, tm16 as _tm16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BITS = 0x7FA5C3D2                      # a NaN pattern no kernel here produces
PLANE_PAT = 0x7FB7                          # a signalling bf16 NaN: no piece of a split value


def _sent(*shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sent(t):
    return t.cpu().contiguous().view(torch.int32) == SENT_BITS


def _api():
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd._lib import SgicError, call
    return ops, call, SgicError


def _ln64(x, w, b, act):
    ref = F.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), eps=1e-5)
    return F.silu(ref) if act == 2 else ref


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
LN_WIDTHS = [pytest.param(4, id="C4-generic-idle-lanes"), pytest.param(64, id="C64-generic-one-pass"),
             pytest.param(260, id="C260-generic-two-passes"), pytest.param(256, id="C256-NV1"), pytest.param(512, id="C512-NV2"),
             pytest.param(768, id="C768-NV3"), pytest.param(1024, id="C1024-NV4"), pytest.param(1280, id="C1280-NV5"),
             pytest.param(1536, id="C1536-NV6"), pytest.param(1792, id="C1792-NV7"), pytest.param(2048, id="C2048-NV8"),
             pytest.param(2304, id="C2304-generic-above-registers")]


@pytest.mark.parametrize("M", [1, 7])
@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_width_classes_strided(C, M):
    """x and out are column slices of wider buffers (ldx = C + 8, ldy = C + 12); M = 1 and 7 leave the last workgroup (4 rows) part-full;
    everything outside the M x C window keeps the sentinel.  Bound: the 2e-5 of test_layernorm_vs_torch, same data."""
    ops, call, _ = _api()
    g = torch.Generator().manual_seed(C + M)
    wide = torch.randn(M, C + 8, generator=g) * 3 + 1
    x = wide[:, 4:4 + C]
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    for act in (0, 2):
        out = _sent(M + 1, C + 12)
        ops.layernorm(wide.to(DEV)[:, 4:4 + C], w.to(DEV), b.to(DEV), out=out[:M, 8:8 + C], act=act)
        got = out.cpu()
        err = float((got[:M, 8:8 + C].double() - _ln64(x, w, b, act)).abs().max())
        assert err < 2e-5, (act, err)
        written = torch.zeros(got.shape, dtype=torch.bool)
        written[:M, 8:8 + C] = True
        assert bool(_is_sent(got)[~written].all()), act


@pytest.mark.parametrize("C", [pytest.param(260, id="C260-generic"), pytest.param(512, id="C512-NV2")])
@pytest.mark.parametrize("act", [0, 2])
def test_layernorm_segment_maps_keep_unmapped_rows(C, act):
    """rows 0..2 of every 5-row segment of x -> rows 0..2 of every 4-row segment of a strided out, SiLU fused or not; row 3 of every
    segment, the row behind the last segment and the columns beside the window keep the sentinel"""
    ops, call, _ = _api()
    n = 5                                                              # 15 mapped rows: the last workgroup holds 3
    g = torch.Generator().manual_seed(C + act)
    x = torch.randn(n * 5, C, generator=g) * 3 + 1
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = _ln64(x, w, b, act).view(n, 5, C)[:, :3]
    out = _sent(n * 4 + 1, C + 4)
    ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), out=out[:n * 4, :C], M=n * 3, x_seg=(3, 5), y_seg=(3, 4), act=act)
    got = out.cpu()
    o = got[:n * 4, :C].view(n, 4, C)
    assert float((o[:, :3].double() - ref).abs().max()) < 2e-5
    written = torch.zeros(got.shape, dtype=torch.bool)
    written[:n * 4, :C].view(n, 4, C)[:, :3] = True
    assert bool(_is_sent(got)[~written].all())


@pytest.mark.parametrize("C", [pytest.param(1024, id="C1024-NV4"), pytest.param(260, id="C260-generic")])
def test_layernorm_constant_rows_give_beta_exactly(C):
    """every element 3.0: the sums 3 C are exact in fp32, the mean is exactly 3, every difference +0, so with act 0 the output is
    beta bit for bit (0 * rstd * gamma + beta), whatever gamma is"""
    ops, call, _ = _api()
    g = torch.Generator().manual_seed(C)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    out = _sent(6, C)
    ops.layernorm(torch.full((5, C), 3.0, device=DEV), w.to(DEV), b.to(DEV), out=out[:5])
    got = out.cpu()
    assert torch.equal(got[:5], b.expand(5, C)) and bool(_is_sent(got[5]).all())


@pytest.mark.parametrize("C", [pytest.param(1024, id="C1024-NV4"), pytest.param(2048, id="C2048-NV8"), pytest.param(260, id="C260-generic")])
@pytest.mark.parametrize("offset", [30.0, 1000.0])
def test_layernorm_large_mean_no_worse_than_torch_fp32(C, offset):
    """rows with mean / std of about 30 and 1000.  What fp32 can deliver falls with that ratio (the mean itself carries an error of a few
    ulp(offset), 6e-5 at 1000), so the bound is relative to another fp32 LayerNorm: err <= max(2e-5, 4 err_torch), err_torch the
    error of torch.nn.functional.layer_norm in fp32 on the CPU against fp64 on the same input; the factor 4 covers the different
    summation order.  A kernel that took the variance as E[x^2] - mean^2 in fp32 would be off by orders of magnitude here
    (ulp(1e6) = 0.06 against a variance of 1)."""
    ops, call, _ = _api()
    g = torch.Generator().manual_seed(C + int(offset))
    x = torch.randn(7, C, generator=g) + offset
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = _ln64(x, w, b, 0)
    err_torch = float((F.layer_norm(x, (C,), w, b, eps=1e-5).double() - ref).abs().max())
    got = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV)).cpu().double()
    err = float((got - ref).abs().max())
    print(f"[layernorm] C={C} mean/std={offset:g}: worst |err| vs fp64: kernel {err:.3e}, torch fp32 {err_torch:.3e}")
    assert err <= max(2e-5, 4 * err_torch), (err, err_torch)


@pytest.mark.parametrize("C", [pytest.param(256, id="C256-NV1"), pytest.param(1280, id="C1280-NV5"), pytest.param(2048, id="C2048-NV8")])
def test_layernorm_planes_output_equals_fp32_output(C):
    """to_gemm=True under the split precision with an x_seg map: the bf16x3 planes carry the fp32 output exactly"""
    ops, call, _ = _api()
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(3 * 5, C, generator=g) * 3 + 0.5).to(DEV)
    w, b = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    old = ops.PRECISION
    ops.set_precision("split3")
    try:
        for act in (0, 2):
            pl = ops.layernorm(x, w, b, act=act, M=3 * 3, x_seg=(3, 5), to_gemm=True)
            h = ops.layernorm(x, w, b, act=act, M=3 * 3, x_seg=(3, 5))
            assert isinstance(pl, ops.Planes) and torch.is_tensor(h)
            assert torch.equal(pl.float(), h), act
    finally:
        ops.set_precision(old)


def test_layernorm_refusals_leave_the_output_alone():
    """C = 6; ldy < C; x off by one float; act = 1 (GELU is not fused here); planes with C = 260: each an SgicError, nothing written"""
    ops, call, SgicError = _api()
    M = 3
    x = torch.randn(M * 264 + 4, device=DEV)
    w, b = torch.randn(264, device=DEV), torch.randn(264, device=DEV)

    def ln(xp, ldx, out, ldy, C, act):
        call("sgic_layernorm_f32", xp, ldx, 0, 0, w, b, out, ldy, 0, 0, M, C, 1e-5, act)

    out = _sent(M * 264)
    ln(x, 64, out, 64, 64, 0)                                          # the same call shape, valid: it does write
    assert not bool(_is_sent(out[:64]).any())
    for what, args in [("C = 6", (x, 8, 8, 6, 0)), ("ldy < C", (x, 64, 60, 64, 0)), ("x off by one float", (x[1:], 64, 64, 64, 0)),
                       ("act = 1", (x, 64, 64, 64, 1))]:
        out = _sent(M * 264)
        with pytest.raises(SgicError):
            ln(args[0], args[1], out, *args[2:])
        assert bool(_is_sent(out).all()), what
    planes = torch.full((3 * M * 260,), PLANE_PAT, dtype=torch.int16, device=DEV)
    with pytest.raises(SgicError):
        call("sgic_layernorm_split3_f32", x, 260, 0, 0, w, b, planes, M, 260, 1e-5, 0)
    assert bool((planes == PLANE_PAT).all())


# ---- depthwise convolution --------------------------------------------------------------------------------------------------------
# sgic_dwconv_nhwc: W % 4 == 0 and k in {3, 5} -> dwconv_x4_kernel, threads = B H (W / 4) (C / 4), grid = ceil(threads / 256), one pass;
# the kernel remaps its block index over the XCDs when grid % 8 == 0.  Otherwise dwconv_kernel, B H W (C / 4) items, grid-stride.
DW_CASES = [
    # 15 * 5 * 27 = 2025 threads -> grid 8 (remapped), last workgroup 233 / 256
    pytest.param(1, 15, 20, 108, 5, False, id="x4-k5-plain-grid8-remapped-part-full"),
    # 16 * 4 * 31 = 1984 threads -> grid 8 (remapped), last workgroup 192 / 256
    pytest.param(1, 16, 16, 124, 3, True, id="x4-k3-tile16-grid8-remapped-part-full"),
    # 2 * 15 * 5 * 27 = 4050 threads -> grid 16 (remapped, blocks b and b + 8 neighbours), last workgroup 210 / 256
    pytest.param(2, 15, 20, 108, 5, False, id="x4-k5-plain-grid16-remapped-part-full"),
    # 3 * 8 * 2 * 16 = 768 threads -> grid 3 (not remapped), full
    pytest.param(3, 8, 8, 64, 3, False, id="x4-k3-plain-grid3-unremapped"),
    # 2 * 1 * 2 = 4 threads -> grid 1; H = 2 < the 5-row window, W = 4: every output sees taps outside the image
    pytest.param(1, 2, 4, 8, 5, False, id="x4-k5-plain-image-smaller-than-window"),
    pytest.param(1, 16, 16, 8, 7, True, id="generic-k7-tile16"),
    pytest.param(2, 5, 6, 12, 1, False, id="generic-k1-plain-part-full"),       # 180 items
    pytest.param(2, 6, 10, 32, 3, False, id="generic-k3-W10-plain"),            # W % 4 != 0 keeps k = 3 off the x4 kernel
]


@pytest.mark.parametrize("with_bias,with_pre", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B,H,W,C,k,tile16", DW_CASES)
def test_dwconv_bitwise_vs_ordered_fp32(B, H, W, C, k, tile16, with_bias, with_pre):
    ops, call, _ = _api()
    g = torch.Generator().manual_seed(H * W + k + C)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(k * k, C, generator=g)
    bias = torch.randn(C, generator=g) if with_bias else None
    ps = torch.rand(C, generator=g) + 0.5 if with_pre else None
    ref = kr.dwconv_ordered32(x, w, bias, ps, k)
    rows = (_tm16(x) if tile16 else x.reshape(B * H * W, C)).contiguous().to(DEV)
    out = _sent(B * H * W + 1, C)
    ops.dwconv(rows, w.to(DEV), bias.to(DEV) if with_bias else None, ps.to(DEV) if with_pre else None, B, H, W, k, tile16=tile16,
               out=out[:-1])
    got = out.cpu()
    assert bool(_is_sent(got[-1]).all())
    got = _from_tm16(got[:-1], B, H, W) if tile16 else got[:-1].reshape(B, H, W, C)
    assert torch.equal(got, ref)
