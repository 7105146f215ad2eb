"""GPU unit tests of the planes-fed 3x3 convolution chain of the VQGAN decoder and the LPIPS / DISTS towers (csrc/decode.hip,
csrc/gemm_split.hip, csrc/gemm.hip), which the suite otherwise reaches only inside whole blocks at the codec's own shapes:
  a. the producers that write a convolution's operand directly as slice-major zero-halo bf16x3 planes (sgic_groupnorm_nhwc_split3,
     sgic_halo_copy_split3) == the fp32 halo output put through the split pass, bitwise, and they write the INTERIOR only (a stray
     write into the border of the cached planes buffer would corrupt every later convolution of that geometry);
  b. GroupNorm's split reduction (S = HW / 1024 > 1, `per` not dividing HW, the cap at 64 splits, the 4x unrolled loop and its
     tail, one or two pixel lanes per block, one channel per group) against fp64 F.group_norm;
  c. conv3x3 in both arithmetics against fp64 F.conv2d: images narrower than a tile (one M tile spans rows and images), rows longer
     than a tile, Cin % 64 != 0, ragged and scalar-epilogue Cout, SiLU, strided residual and output, every tile mode bitwise equal."""
import functools

import pytest
import torch
import torch.nn.functional as F

import kernels_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BITS = 0x7FA5C3D2                      # a NaN pattern no kernel here produces
PLANE_PAT = 0x7FB7                          # a signalling bf16 NaN: no piece of a split value (the NaN of special_values comes out quiet)
CONV3_TILES = (1, 2, 3, 4, 5, 10, 11, 14, 15, 16, 17, 28, 29, 30, 32)


def _sent(*shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sent(t):
    return t.contiguous().view(torch.int32) == SENT_BITS


def _same_bits(got, ref):
    return torch.equal(kr.bits(got), kr.bits(ref))


def _api():
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd._lib import call
    return ops, call


# ---- a. planes producers ----------------------------------------------------------------------------------------------------------
def _interior_rows(B, OH, OW):
    """bool mask over the B (OH+2) (OW+2) halo rows: True on the interior"""
    m = torch.zeros(B, OH + 2, OW + 2, dtype=torch.bool, device=DEV)
    m[:, 1:-1, 1:-1] = True
    return m.reshape(-1)


def _check_planes_and_conv(ops, call, planes, halo, B, OH, OW, C, seed):
    """planes: the int16 buffer a producer wrote (pre-filled with PLANE_PAT); halo: the zero-halo fp32 buffer the fp32 producer
    wrote from the same input.  Interior == split pass of the fp32 halo; border untouched; then the convolution fed with either."""
    rows = B * (OH + 2) * (OW + 2)
    want = torch.empty(3 * rows * C, dtype=torch.int16, device=DEV)
    call("sgic_split3_pack_f32", halo, C, rows, C, want)
    got4, want4 = planes.view(3, C // 32, rows, 32), want.view(3, C // 32, rows, 32)
    inner = _interior_rows(B, OH, OW)
    assert torch.equal(got4[:, :, inner], want4[:, :, inner]), "interior planes != split pass of the fp32 halo"
    assert bool((got4[:, :, ~inner] == PLANE_PAT).all()), "a producer wrote into the border of the planes buffer"
    got4[:, :, ~inner] = 0                                             # the zero halo the convolution needs
    g = torch.Generator().manual_seed(seed)
    Cout = 8
    w = (torch.randn(Cout, 9 * C, generator=g) / (3.0 * C ** 0.5)).to(DEV)
    bias = torch.randn(Cout, generator=g).to(DEV)
    a = ops.conv3x3(ops.HaloPlanes(planes, B, OH, OW, C), w, bias, B, OH, OW, C, Cout, precision="split3", tile=1)
    b = ops.conv3x3(halo, w, bias, B, OH, OW, C, Cout, precision="split3", tile=1)
    assert _same_bits(a, b), "conv3x3 fed with producer planes != conv3x3 fed with the fp32 halo"


@pytest.mark.parametrize("B,H,W,C,swish", [(2, 6, 10, 32, True), (1, 16, 16, 128, False), (2, 5, 7, 512, True)])
def test_groupnorm_planes_producer_interior_only(B, H, W, C, swish):
    ops, call = _api()
    g = torch.Generator().manual_seed(C + H)
    x = (torch.randn(B * H * W, C, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    ws = torch.empty(B * 64 * C * 2, dtype=torch.float64, device=DEV)
    stats = torch.empty(B * 32 * 2, dtype=torch.float32, device=DEV)
    rows = B * (H + 2) * (W + 2)
    planes = torch.full((3 * rows * C,), PLANE_PAT, dtype=torch.int16, device=DEV)
    call("sgic_groupnorm_nhwc_split3", x, gamma, beta, B, H, W, C, 32, 1e-6, int(swish), ws, stats, planes)
    halo = torch.zeros(B, H + 2, W + 2, C, device=DEV)
    call("sgic_groupnorm_nhwc", x, gamma, beta, B, H, W, C, 32, 1e-6, int(swish), 1, ws, stats, halo)
    _check_planes_and_conv(ops, call, planes, halo, B, H, W, C, seed=C)


@pytest.mark.parametrize("B,H,W,C,upsample,tile16", [(2, 16, 32, 32, False, False), (2, 16, 32, 32, False, True), (2, 16, 32, 32, True, False),
                                                     (2, 16, 32, 32, True, True), (1, 3, 5, 64, False, False), (1, 3, 5, 64, True, False)])
def test_halo_copy_planes_producer_interior_only(B, H, W, C, upsample, tile16):
    ops, call = _api()
    x = kr.special_values(torch.randn(B * H * W, C, generator=torch.Generator().manual_seed(H + C))).to(DEV)
    s = 2 if upsample else 1
    OH, OW = H * s, W * s
    rows = B * (OH + 2) * (OW + 2)
    planes = torch.full((3 * rows * C,), PLANE_PAT, dtype=torch.int16, device=DEV)
    call("sgic_halo_copy_split3", x, B, H, W, C, int(upsample), int(tile16), planes)
    halo = torch.zeros(B, OH + 2, OW + 2, C, device=DEV)
    call("sgic_halo_copy", x, B, H, W, C, int(upsample), int(tile16), halo)
    # the fp32 copy itself against the library restatement (so that the two kernels cannot be wrong together)
    assert _same_bits(halo[:, 1:-1, 1:-1].cpu(), kr.halo_interior(x.cpu(), B, H, W, upsample, tile16).contiguous())
    _check_planes_and_conv(ops, call, planes, halo, B, OH, OW, C, seed=H)


# ---- b. GroupNorm reduction paths -------------------------------------------------------------------------------------------------
GN_CASES = [(2, 48, 44, 32, 32),            # S = 2, per = 1056: the unrolled loop and the tail loop both run
            (1, 260, 256, 32, 32),          # HW / 1024 = 65: the cap at 64 splits
            (1, 8, 8, 1024, 32),            # one pixel lane per block
            (1, 8, 8, 512, 32),             # two pixel lanes
            (3, 4, 4, 64, 32),
            (3, 4, 4, 64, 16)]


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("B,H,W,C,groups", GN_CASES)
def test_groupnorm_reduction_paths_vs_fp64(B, H, W, C, groups, halo):
    """bound 3e-5 and input scale of test_groupnorm_vs_torch; plain output with swish off, halo output with swish on"""
    ops, call = _api()
    g = torch.Generator().manual_seed(C + H + groups)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.5
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.group_norm(x.double(), groups, w.double(), b.double(), eps=1e-6)
    if halo:
        ref = ref * torch.sigmoid(ref)
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous().to(DEV)
    if halo:
        buf = torch.zeros(B, H + 2, W + 2, C, device=DEV)
        ops.groupnorm(rows, w.to(DEV), b.to(DEV), B, H, W, swish=True, halo=True, groups=groups, out=buf)
        border = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
        border[:, 1:-1, 1:-1] = False
        assert bool((buf.view(torch.int32)[border] == 0).all()), "the halo border must stay (+)zero"
        got = buf[:, 1:-1, 1:-1]
    else:
        buf = _sent(B * H * W + 1, C)
        ops.groupnorm(rows, w.to(DEV), b.to(DEV), B, H, W, swish=False, halo=False, groups=groups, out=buf[:-1])
        assert bool(_is_sent(buf[-1]).all())
        got = buf[:-1].view(B, H, W, C)
    err = float((got.cpu().double().permute(0, 3, 1, 2) - ref).abs().max())
    print(f"[groupnorm] B={B} H={H} W={W} C={C} groups={groups} halo={int(halo)}: worst |err| vs fp64 {err:.3e}")
    assert err < 3e-5


# ---- c. conv3x3 -------------------------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, residual variants)
CONV_CASES = [(3, 7, 5, 32, 36, (False, True)),        # a tile spans image rows and images; Cin % 64 != 0
              (1, 2, 300, 32, 8, (False, True)),       # an image row longer than a tile
              (2, 24, 40, 96, 130, (False, True)),     # ragged Cout
              (2, 9, 11, 64, 6, (False, True)),        # scalar epilogue
              (1, 16, 16, 128, 3, (True,))]            # Cout = 3 on the GEMM path (with a residual), not the thin kernel


@functools.lru_cache(maxsize=None)
def _conv_case(case):
    """inputs (CPU) and the fp64 references of one case, computed once: {(act, res): (pre rows, result rows)}"""
    B, H, W, Cin, Cout, res_variants = CONV_CASES[case]
    g = torch.Generator().manual_seed(1000 * case + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=g)
    rw = torch.randn(B * H * W, Cout + 4, generator=g)                 # the residual is its column slice [:, :Cout]: ldr = Cout + 4
    r_nchw = rw[:, :Cout].reshape(B, H, W, Cout).permute(0, 3, 1, 2)
    refs = {(act, res): kr.conv3x3_64(x, w, bias, r_nchw if res else None, act) for act in (0, 2) for res in res_variants}
    halo = torch.zeros(B, H + 2, W + 2, Cin)
    halo[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    wk = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()     # (ky, kx, cin) order
    return halo, wk, bias, rw, refs


@pytest.mark.parametrize("precision", ["f32", "split3"])
@pytest.mark.parametrize("case", range(len(CONV_CASES)))
def test_conv3x3_vs_fp64_all_tile_modes(case, precision):
    """tolerance: the project's GEMM bound 3e-6 sqrt(K) max(1, max|pre-activation|) with K = 9 Cin
    (test_gemm_fuzz_all_tile_modes_identical_and_close_to_fp64).  No tile mode is refused for these shapes: a refusal
    (SgicError) fails the test."""
    ops, call = _api()
    B, H, W, Cin, Cout, res_variants = CONV_CASES[case]
    halo, wk, bias, rw, refs = _conv_case(case)
    halo, wk, bias, rw = halo.to(DEV), wk.to(DEV), bias.to(DEV), rw.to(DEV)
    M = B * H * W
    tiles = CONV3_TILES if precision == "split3" else ops.TUNE_MODES
    written = torch.zeros(M + 1, Cout + 4, dtype=torch.bool, device=DEV)
    written[:M, :Cout] = True
    for (act, res), (pre, ref) in refs.items():
        first = None
        for tile in tiles:
            out = _sent(M + 1, Cout + 4)                                # the kernel gets the column slice: ldc = Cout + 4
            ops.conv3x3(halo, wk, bias, B, H, W, Cin, Cout, residual=rw[:, :Cout] if res else None, act=act, out=out[:M, :Cout],
                        tile=tile, precision=precision)
            if first is None:
                first = out
                assert bool(_is_sent(out)[~written].all()), ("a write outside the Cout columns / the M rows", act, res, tile)
                err = float((out[:M, :Cout].cpu().double() - ref).abs().max())
                bound = 3e-6 * (9 * Cin) ** 0.5 * max(1.0, float(pre.abs().max()))
                print(f"[conv3x3] B={B} H={H} W={W} Cin={Cin} Cout={Cout} act={act} res={int(res)} {precision}: worst |err| vs fp64 "
                      f"{err:.3e} (bound {bound:.3e})")
                assert err < bound, (act, res, tile, err, bound)
            else:
                assert _same_bits(out, first), ("tile modes differ (or one wrote outside its slice)", act, res, tile)
