"""GPU: operands past 2^31 and 2^32 elements in the decoder kernels, the GEMMs and the code search (the shapes a default
decompress.py batch of 1024 x 1024 images and an index of more than 2^23 images reach; tests/wide_shapes.py has the table).

Method: slab equivalence plus a spot reference.  A wide operand is built from independent per-slab data (torch.randn on the device,
the generator seeded with the slab's number), the entry point runs once at the wide shape, and for every probe of the table -- slab 0,
the last slab, the slabs around every width mark (byte offsets and element indices 2^31 and 2^32, in every operand) -- the same entry
point runs on that slab alone with the same forced launch mode: the two must be bitwise equal (batch / M independence is what the
project claims at small sizes).  The last slab's corner is also held against an fp64 restatement computed on the CPU from the
regenerated input, with the bound of the kernel's existing test; a halo stays zero; sentinels around an output the test allocates stay
untouched.  Launch modes are always forced: the tuner has its own tests.

Every test reads torch.cuda.mem_get_info() first and skips when less than its footprint + 8 GB is free (none may skip on an idle
card); it prints its duration and torch.cuda.max_memory_allocated().

Which kernel the split modes run at these widths (read from s3_mode / s3_plan in csrc/gemm_split.hip, not traced): dma_ok holds for every
case (packed operands: 32 elements between rows).  GEMM, M = 2^24 + 288, K = 128: a_plane = M K >= 2^29, so flata_ok is false and mode 32
takes its fallback, the register-staged 64x128 tile, while its 256-row slab runs (a_plane = 2^15) take the LDS-DMA 160x256 kernel: there
the slab comparison is between two kernels.  Mode 1 is the LDS-DMA 128x256 kernel, mode 2 the register-staged 128x128 tile, mode 31 the
256x256 kernel for rows below 2^24 and a second launch of mode 1 with m_base = 2^24 for the last 288 rows.  The convolution's modes 1, 2
and 30 deal no operand over the planes, so the 2.3 x 10^9-element halo plane changes nothing in their choice.

Measured on an idle MI355X (seconds, peak GB of max_memory_allocated), none skipped: groupnorm 1.3-1.8 s, 19.4-45.8 GB (planes, B = 33);
halo_copy 0.02-2.6 s, 13.3-34.2 GB; conv3x3 f32 0.1-2.8 s, 29.6 GB; conv3x3 split 0.1-3.7 s, 24.8-46.3 GB (B = 33); thin 0.02-0.04 s,
10.6-19.4 GB; gemm 0.01-4.2 s, 17.2-38.7 GB (split3 with residual); attention 0.05 s, 13.1 GB; search 0.01-0.5 s (one split: 0.5 s),
4.8 GB; end to end 6 s, 38.2 GB.  The figures above 2 s are supposed to be a kernel's first use in the process.  No test found a wrong offset."""
import ctypes
import gc
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_ref as kr  # noqa: E402
import search_codes_ref as cref  # noqa: E402
import search_range_ref as rgref  # noqa: E402
import search_vectors_ref as vref  # noqa: E402
import wide_shapes as ws  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BITS = 0x7FA5C3D2                      # a NaN pattern no kernel here produces
PLANE_PAT = 0x7FB7                          # a signalling bf16 NaN: no piece of a split value
SGIC_EINVAL = -1
H, W, C, HW, HALO = ws.H, ws.W, ws.C, ws.HW, ws.HALO
WIN = 8                                     # the fp64 window: the last WIN x WIN pixels (or 64 rows) of the last slab


def _api():
    import sgic_amd  # noqa
    from sgic_amd import ops
    return ops


def _drop_caches():
    ops = _api()
    gc.collect()
    for d in (ops._HALO, ops._HALO3, ops._GN_WS, ops._A3_WS):
        d.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _release_wide_buffers():
    """the wrappers' caches keep every shape they ever saw: without this the 26 GB planes buffers stay resident for the rest of the suite"""
    yield
    _drop_caches()


_BUDGET = {}                                # case the running test began -> (the table's footprint, bytes allocated before it began)
_INDEX_BASE = [0]                           # bytes allocated before the search index was built


@pytest.fixture(autouse=True)
def _report(request):
    t0 = time.time()
    _BUDGET.clear()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    base = max([b for _, b in _BUDGET.values()], default=0)     # what earlier modules of the session still hold is not this test's
    print(f"\n[wide] {request.node.name}: {time.time() - t0:.2f} s, max_memory_allocated {(peak - base) / 1e9:.2f} GB above the "
          f"{base / 1e9:.2f} GB allocated before it")
    _drop_caches()
    for name, (budget, b) in _BUDGET.items():
        assert peak - b <= budget <= ws.FOOTPRINT_LIMIT, f"{name}: peak {(peak - b) / 1e9:.2f} GB, the table says {budget / 1e9:.2f} GB"


def _begin(name):
    """-> (case, probes) after the memory condition: skip with the numbers when the card cannot hold the case"""
    case = ws.CASES[name]
    _drop_caches()
    free, total = torch.cuda.mem_get_info()
    need = ws.footprint(case) + ws.HEADROOM
    if free < need:
        pytest.skip(f"{name}: {free / 1e9:.1f} GB free of {total / 1e9:.1f} GB, needs {need / 1e9:.1f} GB (footprint + headroom)")
    torch.cuda.reset_peak_memory_stats()
    _BUDGET[name] = (ws.footprint(case), torch.cuda.memory_allocated())
    return case, ws.probes(case)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(n, dtype=torch.float32, fill=None):
    """-> (whole buffer, the n elements between two guards of ws.GUARD sentinel elements); fill: value of the middle (None: sentinel)"""
    if dtype == torch.float32:
        buf = torch.full((n + 2 * ws.GUARD,), SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    else:
        buf = torch.full((n + 2 * ws.GUARD,), PLANE_PAT, dtype=dtype, device=DEV)
    mid = buf[ws.GUARD:ws.GUARD + n]
    if fill is not None:
        mid.fill_(fill)
    return buf, mid


def _guards_intact(buf):
    if buf.dtype == torch.float32:
        v = buf.view(torch.int32)
        return bool((v[:ws.GUARD] == SENT_BITS).all()) and bool((v[-ws.GUARD:] == SENT_BITS).all())
    return bool((buf[:ws.GUARD] == PLANE_PAT).all()) and bool((buf[-ws.GUARD:] == PLANE_PAT).all())


def _randn(shape, seed, mean=0.0, std=1.0, out=None):
    """a contiguous fp32 device tensor of `shape` from a generator seeded with `seed`: the same call gives the same values again"""
    t = torch.empty(shape, device=DEV) if out is None else out
    assert t.is_contiguous()
    t.normal_(mean, std, generator=torch.Generator(device=DEV).manual_seed(seed))
    return t


def _cpu_randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _planes_f64(p):
    """int16 planes (3, ...) -> the fp64 sum of the three bf16 pieces"""
    f = lambda q: (q.to(torch.int32) << 16).view(torch.float32).double()  # noqa: E731
    return f(p[0]) + f(p[1]) + f(p[2])


# ---- 1. GroupNorm --------------------------------------------------------------------------------------------------------------
def _gn_image(b, rows=HW, out=None):
    """image b: mean 0.1 b, standard deviation 1 + 0.05 b, so that no two images share their statistics"""
    return _randn((rows, C), 100 + b, 0.1 * b, 1.0 + 0.05 * b, out=out)


def _gn_wide(B):
    x = torch.empty(B * HW, C, device=DEV)
    for b in range(B):
        _gn_image(b, out=x[b * HW:(b + 1) * HW])
    return x, _cpu_randn(C, 1), _cpu_randn(C, 2)


def _gn_window64(b, gamma, beta, swish):
    """fp64 GroupNorm (32 groups, eps 1e-6, biased variance) of the regenerated image b on the CPU -> its last WIN x WIN pixels (WIN, WIN, C)"""
    img = _gn_image(b).cpu()
    var, mean = torch.var_mean(img.view(HW, 32, C // 32).double(), dim=(0, 2), unbiased=False)
    win = img.view(H, W, 32, C // 32)[H - WIN:, W - WIN:].double()
    y = (win - mean.view(1, 1, 32, 1)) / torch.sqrt(var.view(1, 1, 32, 1) + 1e-6)
    y = y.reshape(WIN, WIN, C) * gamma.cpu().double() + beta.cpu().double()
    return y * torch.sigmoid(y) if swish else y


def _planes_view(t, B):
    """the int16 planes of a (B, H+2, W+2, C) halo buffer as (3, C/32, B, H+2, W+2, 32)"""
    return t[:3 * B * HALO * C].view(3, C // 32, B, H + 2, W + 2, 32)


def _border_is_zero(img):
    """img (..., H+2, W+2, last): the one-pixel frame of an image, as raw bits"""
    v = img.view(torch.int32) if img.dtype == torch.float32 else img
    return not bool(v[..., 0, :, :].any() or v[..., -1, :, :].any() or v[..., :, 0, :].any() or v[..., :, -1, :].any())


def test_groupnorm_plain():
    """bound: 3e-5, test_gpu_kernels.py::test_groupnorm_vs_torch (swish off, as test_gpu_conv_chain.py runs the plain output)"""
    ops = _api()
    case, probes = _begin("groupnorm_plain")
    B = case["n_units"]
    x, gamma, beta = _gn_wide(B)
    buf, mid = _guarded(B * HW * C)
    y = ops.groupnorm(x, gamma, beta, B, H, W, swish=False, halo=False, out=mid.view(B * HW, C))
    assert _guards_intact(buf)
    for p in probes:
        one = ops.groupnorm(_gn_image(p), gamma, beta, 1, H, W, swish=False, halo=False)
        assert torch.equal(one, y[p * HW:(p + 1) * HW]), f"image {p} of the batch != that image alone"
    assert not torch.equal(y[16 * HW:17 * HW], y[:HW])
    got = y[(B - 1) * HW:].view(H, W, C)[H - WIN:, W - WIN:].cpu().double()
    err = float((got - _gn_window64(B - 1, gamma, beta, False)).abs().max())
    print(f"[groupnorm plain] worst |err| vs fp64 in the last image's corner {err:.3e}")
    assert err < 3e-5


def test_groupnorm_halo_f32():
    """bound: 3e-5, test_gpu_kernels.py::test_groupnorm_vs_torch (halo output with swish)"""
    ops = _api()
    case, probes = _begin("groupnorm_halo")
    B = case["n_units"]
    x, gamma, beta = _gn_wide(B)
    buf, mid = _guarded(B * HALO * C, fill=0.0)
    y = ops.groupnorm(x, gamma, beta, B, H, W, swish=True, halo=True, out=mid.view(B, H + 2, W + 2, C))
    assert _guards_intact(buf)
    one = torch.zeros(1, H + 2, W + 2, C, device=DEV)
    for p in probes:
        ops.groupnorm(_gn_image(p), gamma, beta, 1, H, W, swish=True, halo=True, out=one)
        assert _same_bits(one[0], y[p]), f"image {p} of the batch != that image alone"
        assert _border_is_zero(y[p]), f"halo of image {p}"
    got = y[B - 1, H + 1 - WIN:H + 1, W + 1 - WIN:W + 1].cpu().double()
    err = float((got - _gn_window64(B - 1, gamma, beta, True)).abs().max())
    print(f"[groupnorm halo] worst |err| vs fp64 in the last image's corner {err:.3e}")
    assert err < 3e-5


def _own_halo_planes(ops, B):
    """a guarded, zeroed planes buffer of the test's own put where the wrappers look for the cached one"""
    buf, mid = _guarded(3 * B * HALO * C, dtype=torch.int16, fill=0)
    ops._HALO3[(DEV, B, H, W, C)] = ops.HaloPlanes(mid, B, H, W, C)
    return buf, mid


@pytest.mark.parametrize("tier", ["A", "B"])
def test_groupnorm_planes(tier, monkeypatch):
    """to_conv=(128, False) under the split arithmetic; bound: 3e-5 as above (the planes sum to the fp32 value exactly)"""
    ops = _api()
    monkeypatch.setattr(ops, "PRECISION", "split3")
    case, probes = _begin(f"groupnorm_planes_{tier}")
    B = case["n_units"]
    x, gamma, beta = _gn_wide(B)
    buf, mid = _own_halo_planes(ops, B)
    hp = ops.groupnorm(x, gamma, beta, B, H, W, swish=True, halo=True, to_conv=(C, False))
    assert isinstance(hp, ops.HaloPlanes) and hp.t.data_ptr() == mid.data_ptr() and _guards_intact(buf)
    wide = _planes_view(hp.t, B)
    for p in probes:
        one = ops.groupnorm(_gn_image(p), gamma, beta, 1, H, W, swish=True, halo=True, to_conv=(C, False))
        assert torch.equal(_planes_view(one.t, 1)[:, :, 0], wide[:, :, p]), f"image {p} of the batch != that image alone"
        assert _border_is_zero(wide[:, :, p]), f"halo of image {p}"
    got = _planes_f64(wide[:, :, B - 1, H + 1 - WIN:H + 1, W + 1 - WIN:W + 1].cpu())          # (C/32, WIN, WIN, 32)
    got = got.permute(1, 2, 0, 3).reshape(WIN, WIN, C)
    err = float((got - _gn_window64(B - 1, gamma, beta, True)).abs().max())
    print(f"[groupnorm planes {tier}] worst |err| vs fp64 in the last image's corner {err:.3e}")
    assert err < 3e-5


# ---- 2. halo copies: data movement, exact ----------------------------------------------------------------------------------------
def _hc_image(b, rows):
    return _randn((rows, C), 300 + b)


def _hc_wide(B, rows):
    x = torch.empty(B * rows, C, device=DEV)
    for b in range(B):
        _randn((rows, C), 300 + b, out=x[b * rows:(b + 1) * rows])
    return x


def _hc_interior(img, upsample, tile16):
    h, w = (H // 2, W // 2) if upsample else (H, W)
    return kr.halo_interior(img, 1, h, w, upsample, tile16)[0]


@pytest.mark.parametrize("name,upsample,tile16", [("halo_copy_plain", False, False), ("halo_copy_up_f32", True, False),
                                                  ("halo_copy_tile16", False, True)])
def test_halo_copy_f32(name, upsample, tile16):
    """exact: every probed image equals its own call and the regenerated input put through the library restatement
    (kernels_ref.halo_interior), bit for bit -- the fp64 window of the other tests has nothing to add to a copy"""
    ops = _api()
    case, probes = _begin(name)
    B = case["n_units"]
    h, w = (H // 2, W // 2) if upsample else (H, W)
    x = _hc_wide(B, h * w)
    buf, mid = _guarded(B * HALO * C, fill=0.0)
    y = ops.halo_copy(x, B, h, w, C, upsample=upsample, tile16=tile16, out=mid.view(B, H + 2, W + 2, C))
    assert _guards_intact(buf)
    one = torch.zeros(1, H + 2, W + 2, C, device=DEV)
    for p in probes:
        img = _hc_image(p, h * w)
        ops.halo_copy(img, 1, h, w, C, upsample=upsample, tile16=tile16, out=one)
        assert _same_bits(one[0], y[p]), f"image {p} of the batch != that image alone"
        assert _same_bits(y[p, 1:-1, 1:-1], _hc_interior(img, upsample, tile16)), f"image {p} != its regenerated input"
        assert _border_is_zero(y[p]), f"halo of image {p}"


@pytest.mark.parametrize("tier", ["A", "B"])
def test_halo_copy_upsample_planes(tier, monkeypatch):
    """512^2 -> 1024^2 into planes.  Exact against the own call; against the regenerated input the planes sum back to the value with
    the bound of test_gpu_split3.py::test_split_is_exact (1e-30: a low piece may be a flushed bf16 subnormal)"""
    ops = _api()
    monkeypatch.setattr(ops, "PRECISION", "split3")
    case, probes = _begin(f"halo_copy_up_planes_{tier}")
    B = case["n_units"]
    h, w = H // 2, W // 2
    x = _hc_wide(B, h * w)
    buf, mid = _own_halo_planes(ops, B)
    hp = ops.halo_copy(x, B, h, w, C, upsample=True, to_conv=(C, False))
    assert isinstance(hp, ops.HaloPlanes) and hp.t.data_ptr() == mid.data_ptr() and _guards_intact(buf)
    wide = _planes_view(hp.t, B)
    for p in probes:
        img = _hc_image(p, h * w)
        one = ops.halo_copy(img, 1, h, w, C, upsample=True, to_conv=(C, False))
        assert torch.equal(_planes_view(one.t, 1)[:, :, 0], wide[:, :, p]), f"image {p} of the batch != that image alone"
        assert _border_is_zero(wide[:, :, p]), f"halo of image {p}"
        f = lambda q: (q.to(torch.int32) << 16).view(torch.float32)  # noqa: E731
        pc = wide[:, :, p, 1:-1, 1:-1]
        back = ((f(pc[0]) + f(pc[1])) + f(pc[2])).permute(1, 2, 0, 3).reshape(H, W, C)     # exact in fp32: what ops.Planes.float does
        assert float((back - _hc_interior(img, True, False)).abs().max()) <= 1e-30, f"image {p} != its regenerated input"


# ---- 3. conv3x3 ------------------------------------------------------------------------------------------------------------------
def _conv_weights(Cout):
    w = _cpu_randn((Cout, 9 * C), 11 + Cout, 1.0 / (3.0 * C ** 0.5))
    return w, _cpu_randn(Cout, 12 + Cout)


def _conv_window64(patch, w, bias, res):
    """patch (WIN+2, WIN+2, C) of the zero-halo input around the window, w (Cout, 9 C) in (ky, kx, cin) order -> (pre, out) fp64
    (WIN, WIN, Cout)"""
    Cout = w.shape[0]
    w4 = w.cpu().double().view(Cout, 3, 3, C).permute(0, 3, 1, 2)
    pre = F.conv2d(patch.cpu().double().permute(2, 0, 1)[None], w4, bias.cpu().double())[0].permute(1, 2, 0)
    return pre, (pre + res.cpu().double() if res is not None else pre)


def _halo_wide(B, seed0):
    xh = torch.zeros(B, H + 2, W + 2, C, device=DEV)
    img = torch.empty(HW, C, device=DEV)
    for b in range(B):
        xh[b, 1:-1, 1:-1] = _randn((HW, C), seed0 + b, out=img).view(H, W, C)
    return xh


def _halo_one(b, seed0):
    xh = torch.zeros(1, H + 2, W + 2, C, device=DEV)
    xh[0, 1:-1, 1:-1] = _randn((HW, C), seed0 + b).view(H, W, C)
    return xh


def _res_wide(B, Cout, seed0):
    r = torch.empty(B * HW, Cout, device=DEV)
    for b in range(B):
        _randn((HW, Cout), seed0 + b, out=r[b * HW:(b + 1) * HW])
    return r


@pytest.mark.parametrize("tile", [0, 1, 9, 11])
def test_conv3x3_f32_residual(tile):
    """the built-in heuristic and one mode of each family of gemm_launch (plain 128x128, mixed, persistent).  bound: 3e-6 sqrt(9 Cin)
    max(1, max|pre-activation|), test_gpu_conv_chain.py::test_conv3x3_vs_fp64_all_tile_modes"""
    ops = _api()
    case, probes = _begin("conv_f32")
    B = case["n_units"]
    w, bias = _conv_weights(C)
    xh, r = _halo_wide(B, 500), _res_wide(B, C, 600)
    buf, mid = _guarded(B * HW * C)
    y = ops.conv3x3(xh, w, bias, B, H, W, C, C, residual=r, out=mid.view(B * HW, C), tile=tile, precision="f32")
    assert _guards_intact(buf)
    for p in probes:
        one = ops.conv3x3(_halo_one(p, 500), w, bias, 1, H, W, C, C, residual=_randn((HW, C), 600 + p), tile=tile, precision="f32")
        assert torch.equal(one, y[p * HW:(p + 1) * HW]), f"image {p} of the batch != that image alone (tile {tile})"
    last = _halo_one(B - 1, 500)[0, H - WIN:, W - WIN:]
    rwin = _randn((HW, C), 600 + B - 1).view(H, W, C)[H - WIN:, W - WIN:]
    pre, ref = _conv_window64(last, w, bias, rwin)
    err = float((y[(B - 1) * HW:].view(H, W, C)[H - WIN:, W - WIN:].cpu().double() - ref).abs().max())
    bound = 3e-6 * (9 * C) ** 0.5 * max(1.0, float(pre.abs().max()))
    print(f"[conv3x3 f32 tile {tile}] worst |err| vs fp64 in the last image's corner {err:.3e} (bound {bound:.3e})")
    assert err < bound


@pytest.mark.parametrize("tier,tile,res", [("A", 1, False), ("A", 2, False), ("A", 30, False), ("B", 1, False),
                                           ("A", 1, True), ("A", 2, True), ("A", 30, True)])
def test_conv3x3_split_fed_by_groupnorm_planes(tier, tile, res, monkeypatch):
    """modes 1 (LDS-DMA), 2 (register-staged) and 30 (256x256, single W buffer), fed the HaloPlanes that GroupNorm wrote.  The fp64
    window convolves what the planes hold (their exact sum: the producer has its own test above).  bound: 3e-6 sqrt(9 Cin)
    max(1, max|pre-activation|), test_gpu_conv_chain.py::test_conv3x3_vs_fp64_all_tile_modes"""
    ops = _api()
    monkeypatch.setattr(ops, "PRECISION", "split3")
    case, probes = _begin("conv_split_res" if res else f"conv_split_{tier}")
    B = case["n_units"]
    w, bias = _conv_weights(C)
    x, gamma, beta = _gn_wide(B)
    hp = ops.groupnorm(x, gamma, beta, B, H, W, swish=True, halo=True, to_conv=(C, res))
    assert isinstance(hp, ops.HaloPlanes)
    del x
    r = _res_wide(B, C, 600) if res else None
    buf, mid = _guarded(B * HW * C)
    y = ops.conv3x3(hp, w, bias, B, H, W, C, C, residual=r, out=mid.view(B * HW, C), tile=tile, precision="split3")
    assert _guards_intact(buf)
    for p in probes:
        hp1 = ops.groupnorm(_gn_image(p), gamma, beta, 1, H, W, swish=True, halo=True, to_conv=(C, res))
        one = ops.conv3x3(hp1, w, bias, 1, H, W, C, C, residual=_randn((HW, C), 600 + p) if res else None, tile=tile, precision="split3")
        assert torch.equal(one, y[p * HW:(p + 1) * HW]), f"image {p} of the batch != that image alone (tile {tile})"
    patch = _planes_f64(_planes_view(hp.t, B)[:, :, B - 1, H - WIN:, W - WIN:].cpu()).permute(1, 2, 0, 3).reshape(WIN + 2, WIN + 2, C)
    rwin = _randn((HW, C), 600 + B - 1).view(H, W, C)[H - WIN:, W - WIN:] if res else None
    pre, ref = _conv_window64(patch, w, bias, rwin)
    err = float((y[(B - 1) * HW:].view(H, W, C)[H - WIN:, W - WIN:].cpu().double() - ref).abs().max())
    bound = 3e-6 * (9 * C) ** 0.5 * max(1.0, float(pre.abs().max()))
    print(f"[conv3x3 split {tier} tile {tile} res {int(res)}] worst |err| vs fp64 in the last image's corner {err:.3e} (bound {bound:.3e})")
    assert err < bound


@pytest.mark.parametrize("tier", ["A", "B"])
def test_conv3x3_thin_into_four_columns(tier):
    """Cout = 3 into o[:, :3] of a 4-column buffer, as the decoder's conv_out.  bound: 3e-6 sqrt(9 Cin) max(1, max|pre-activation|),
    test_gpu_conv_chain.py::test_conv3x3_vs_fp64_all_tile_modes"""
    ops = _api()
    case, probes = _begin(f"conv_thin_{tier}")
    B = case["n_units"]
    w, bias = _conv_weights(3)
    xh = _halo_wide(B, 500)
    buf, mid = _guarded(B * HW * 4)
    o = mid.view(B * HW, 4)
    ops.conv3x3(xh, w, bias, B, H, W, C, 3, out=o[:, :3], tile=0, precision="f32")
    assert _guards_intact(buf)
    assert bool((_bits(o[:, 3]) == SENT_BITS).all()), "the fourth column is not the convolution's"
    for p in probes:
        _, m1 = _guarded(HW * 4)
        o1 = m1.view(HW, 4)
        ops.conv3x3(_halo_one(p, 500), w, bias, 1, H, W, C, 3, out=o1[:, :3], tile=0, precision="f32")
        assert _same_bits(o1, o[p * HW:(p + 1) * HW]), f"image {p} of the batch != that image alone"
    pre, ref = _conv_window64(_halo_one(B - 1, 500)[0, H - WIN:, W - WIN:], w, bias, None)
    err = float((o[(B - 1) * HW:].view(H, W, 4)[H - WIN:, W - WIN:, :3].cpu().double() - ref).abs().max())
    bound = 3e-6 * (9 * C) ** 0.5 * max(1.0, float(pre.abs().max()))
    print(f"[conv3x3 thin {tier}] worst |err| vs fp64 in the last image's corner {err:.3e} (bound {bound:.3e})")
    assert err < bound


def test_conv3x3_refuses_2_31_pixels():
    """B = 2^15 images of 256 x 256 are 2^31 pixels: both entry points return SGIC_EINVAL before any launch (the buffers are dummies)"""
    _api()
    from sgic_amd._lib import lib
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)   # noqa: E731
    x = torch.zeros(4096, device=DEV)
    planes = torch.zeros(4096, dtype=torch.int16, device=DEV)
    w = torch.zeros(32 * 288, device=DEV)
    bias = torch.zeros(32, device=DEV)
    out = torch.full((4096,), SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    null = ctypes.c_void_p(0)
    assert lib.sgic_conv3x3_f32(p(x), p(w), p(bias), null, 0, p(out), 32, 1 << 15, 256, 256, 32, 32, 0, null, null) == SGIC_EINVAL
    assert lib.sgic_conv3x3_split3_f32(p(planes), p(planes), p(bias), null, 0, p(out), 32, 1 << 15, 256, 256, 32, 32, 0, null,
                                       null) == SGIC_EINVAL
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENT_BITS).all())


# ---- 4. GEMM ---------------------------------------------------------------------------------------------------------------------
M, K, N, SPAN = ws.GEMM_M, ws.GEMM_K, ws.GEMM_N, ws.GEMM_SPAN
CHUNK = 1 << 20                              # rows generated by one seeded call


def _rows_wide(cols, seed0, scale=1.0):
    a = torch.empty(M, cols, device=DEV)
    for i, r0 in enumerate(range(0, M, CHUNK)):
        r1 = min(M, r0 + CHUNK)
        _randn((r1 - r0, cols), seed0 + i, 0.0, scale, out=a[r0:r1])
    return a


def _rows_tail(cols, seed0, scale=1.0):
    """the regenerated last chunk: rows 2^24 .. M"""
    i = (M - 1) // CHUNK
    return _randn((M - i * CHUNK, cols), seed0 + i, 0.0, scale)


def _gemm_weights():
    return _cpu_randn((N, K), 21, 0.05), _cpu_randn(N, 22)


def _gemm_bound(precision, pre, ref):
    """f32: 3e-6 sqrt(K) max(1, max|pre|), test_gpu_encoder.py::test_gemm_fuzz_all_tile_modes_identical_and_close_to_fp64;
    split3: 2e-5 max(1, max|ref|), test_gpu_split3.py::test_epilogues_vs_torch / test_edge_shapes_every_mode"""
    if precision == "f32":
        return 3e-6 * K ** 0.5 * max(1.0, float(pre.abs().max()))
    return 2e-5 * max(1.0, float(ref.abs().max()))


def _gemm_tail_check(what, precision, got_tail, w, bias, res_seed=None):
    """the last 64 rows against fp64 from the regenerated last chunk of A (and of the residual)"""
    a = _rows_tail(K, 700)[-64:].cpu().double()
    pre = a @ w.cpu().double().T + bias.cpu().double()
    ref = pre + _rows_tail(N, res_seed)[-64:].cpu().double() if res_seed is not None else pre
    err = float((got_tail.cpu().double() - ref).abs().max())
    bound = _gemm_bound(precision, pre, ref)
    print(f"[gemm {what}] worst |err| vs fp64 in the last 64 rows {err:.3e} (bound {bound:.3e})")
    assert err < bound


@pytest.mark.parametrize("precision,tile", [("f32", 0), ("f32", 1), ("f32", 9), ("f32", 11),
                                            ("split3", 1), ("split3", 2), ("split3", 32), ("split3", 31)])
def test_gemm_modes(precision, tile):
    """f32: the heuristic, plain, mixed and persistent launches.  split3: mode 1 (LDS-DMA), 2 (register-staged), 32 (its flat-dealt A
    cannot address a plane of 2^29 elements or more: s3_mode falls back to the register-staged 64x128 tile) and 31 (two launches:
    m_base enters the C row map of the second)"""
    ops = _api()
    case, probes = _begin("gemm_f32" if precision == "f32" else "gemm_split3")
    w, bias = _gemm_weights()
    a = _rows_wide(K, 700)
    buf, mid = _guarded(M * N)
    c = ops.gemm(a, w, bias, out=mid.view(M, N), tile=tile, precision=precision)
    assert _guards_intact(buf)
    for s in probes:
        one = ops.gemm(a[s:s + SPAN].clone(), w, bias, tile=tile, precision=precision)
        assert torch.equal(one, c[s:s + SPAN]), f"rows {s}..{s + SPAN} of the product != those rows alone ({precision} tile {tile})"
    _gemm_tail_check(f"{precision} tile {tile}", precision, c[-64:], w, bias)


@pytest.mark.parametrize("precision,tile", [("f32", 1), ("split3", 1)])
def test_gemm_residual(precision, tile):
    ops = _api()
    case, probes = _begin("gemm_residual")
    w, bias = _gemm_weights()
    a, r = _rows_wide(K, 700), _rows_wide(N, 800)
    buf, mid = _guarded(M * N)
    c = ops.gemm(a, w, bias, residual=r, out=mid.view(M, N), tile=tile, precision=precision)
    assert _guards_intact(buf)
    for s in probes:
        one = ops.gemm(a[s:s + SPAN].clone(), w, bias, residual=r[s:s + SPAN].clone(), tile=tile, precision=precision)
        assert torch.equal(one, c[s:s + SPAN]), f"rows {s}..{s + SPAN} of the product != those rows alone ({precision} tile {tile})"
    _gemm_tail_check(f"residual {precision} tile {tile}", precision, c[-64:], w, bias, res_seed=800)


@pytest.mark.parametrize("precision,tile", [("f32", 9), ("split3", 31)])
def test_gemm_c_seg_into_a_larger_buffer(precision, tile):
    """17 segments of 2^20 rows, 256 rows of padding after each: the padding stays zero, every probed block lands where the map says"""
    ops = _api()
    case, probes = _begin("gemm_c_seg")
    seg = case["operands"]["c"]
    w, bias = _gemm_weights()
    a = _rows_wide(K, 700)
    rows = seg.elems(M) // N
    buf, mid = _guarded(rows * N, fill=0.0)
    cbuf = mid.view(rows, N)
    ops.gemm(a, w, bias, out=cbuf, tile=tile, precision=precision, c_seg=(seg.seg, seg.seg_stride))
    assert _guards_intact(buf)
    for i in range(M // seg.seg):
        gap = cbuf[i * seg.seg_stride + seg.seg:(i + 1) * seg.seg_stride]
        assert not bool(gap.view(torch.int32).any()), f"the padding after segment {i} was written"
    for s in probes:
        one = ops.gemm(a[s:s + SPAN].clone(), w, bias, tile=tile, precision=precision)
        assert torch.equal(one, cbuf[seg.row(s):seg.row(s) + SPAN]), f"rows {s}..{s + SPAN} != those rows alone ({precision} tile {tile})"
    _gemm_tail_check(f"c_seg {precision} tile {tile}", precision, cbuf[-64:], w, bias)


def test_gemm_to_gemm_planes_output():
    ops = _api()
    case, probes = _begin("gemm_to_gemm")
    w, bias = _gemm_weights()
    a = _rows_wide(K, 700)
    buf, mid = _guarded(3 * M * N, dtype=torch.int16)
    pl = ops.gemm(a, w, bias, out=ops.Planes(M, N, DEV, buf=mid), tile=1, precision="split3", to_gemm=True)
    assert isinstance(pl, ops.Planes) and pl.t.data_ptr() == mid.data_ptr() and _guards_intact(buf)
    wide = pl.t[:3 * M * N].view(3, N // 32, M, 32)
    for s in probes:
        one = ops.gemm(a[s:s + SPAN].clone(), w, bias, tile=1, precision="split3", to_gemm=True)
        assert torch.equal(one.t[:3 * SPAN * N].view(3, N // 32, SPAN, 32), wide[:, :, s:s + SPAN]), f"rows {s}..{s + SPAN} != those rows alone"
    tail = _planes_f64(wide[:, :, -64:].cpu()).permute(1, 0, 2).reshape(64, N)
    _gemm_tail_check("to_gemm split3 tile 1", "split3", tail, w, bias)


def test_gemm_pre_split_planes_a():
    ops = _api()
    case, probes = _begin("gemm_planes_a")
    w, bias = _gemm_weights()
    a = _rows_wide(K, 700)
    ap = ops.split3_planes(a)
    wide_a = ap.t[:3 * M * K].view(3, K // 32, M, 32)
    buf, mid = _guarded(M * N)
    c = ops.gemm(ap, w, bias, out=mid.view(M, N), tile=2, precision="split3")
    assert _guards_intact(buf)
    for s in probes:
        one_a = ops.split3_planes(a[s:s + SPAN].clone())
        assert torch.equal(one_a.t[:3 * SPAN * K].view(3, K // 32, SPAN, 32), wide_a[:, :, s:s + SPAN]), f"planes of rows {s}..{s + SPAN}"
        one = ops.gemm(one_a, w, bias, tile=2, precision="split3")
        assert torch.equal(one, c[s:s + SPAN]), f"rows {s}..{s + SPAN} of the product != those rows alone"
    _gemm_tail_check("planes A split3 tile 2", "split3", c[-64:], w, bias)


# ---- 5. VQGAN attention at its production shape ----------------------------------------------------------------------------------
def test_vqgan_attention_batched_gemms_and_softmax():
    """S_b = Q_b K_b^T, softmax in place, O_b = P_b V_b with the strides of decoder._attn, 129 items of L = 4096, c = 512.  bounds:
    3e-6 sqrt(K) max(1, max|pre|) for both products (test_gpu_kernels.py::test_gemm_batched_strides_bias_residual), 1e-6 for the
    softmax (test_gpu_kernels.py::test_softmax_rows_and_topk_vs_torch)"""
    ops = _api()
    case, probes = _begin("vqgan_attention")
    nb, L, c = case["n_units"], ws.ATT_L, ws.ATT_C
    scale = float(c ** -0.5)
    q, k = torch.empty(nb * L, c, device=DEV), torch.empty(nb * L, c, device=DEV)
    vt = torch.empty(nb, c, L, device=DEV)
    for b in range(nb):
        _randn((L, c), 1000 + b, out=q[b * L:(b + 1) * L])
        _randn((L, c), 2000 + b, out=k[b * L:(b + 1) * L])
        _randn((c, L), 3000 + b, out=vt[b])
    bufs, mids = _guarded(nb * L * L)
    S = mids.view(nb, L, L)
    ops.gemm_batched(q, c, L * c, k, c, L * c, S, L, L * L, L, L, c, nb)
    s_tail = S[nb - 1, L - 64:].clone()
    ops.softmax_rows(S, L, scale=scale, out=S)
    bufo, mido = _guarded(nb * L * c)
    o = mido.view(nb * L, c)
    ops.gemm_batched(S, L, L * L, vt, L, c * L, o, c, L * c, L, c, L, nb)
    assert _guards_intact(bufs) and _guards_intact(bufo)
    S1, o1 = torch.empty(1, L, L, device=DEV), torch.empty(L, c, device=DEV)
    for b in probes:
        qb, kb, vb = _randn((L, c), 1000 + b), _randn((L, c), 2000 + b), _randn((c, L), 3000 + b)
        ops.gemm_batched(qb, c, L * c, kb, c, L * c, S1, L, L * L, L, L, c, 1)
        ops.softmax_rows(S1, L, scale=scale, out=S1)
        ops.gemm_batched(S1, L, L * L, vb, L, c * L, o1, c, L * c, L, c, L, 1)
        assert torch.equal(S1[0], S[b]), f"P of item {b} != that item alone"
        assert torch.equal(o1, o[b * L:(b + 1) * L]), f"O of item {b} != that item alone"
    b = nb - 1
    qt, kb, vb = _randn((L, c), 1000 + b)[L - 64:].cpu().double(), _randn((L, c), 2000 + b).cpu().double(), _randn((c, L), 3000 + b).cpu().double()
    s_ref = qt @ kb.T
    e_s = float((s_tail.cpu().double() - s_ref).abs().max())
    b_s = 3e-6 * c ** 0.5 * max(1.0, float(s_ref.abs().max()))
    p_gpu = S[b, L - 64:].cpu().double()
    e_p = float((p_gpu - torch.softmax(s_tail.cpu().double() * scale, dim=-1)).abs().max())
    o_ref = p_gpu @ vb.T
    e_o = float((o[-64:].cpu().double() - o_ref).abs().max())
    b_o = 3e-6 * L ** 0.5 * max(1.0, float(o_ref.abs().max()))
    print(f"[attention] last 64 rows of the last item vs fp64: S {e_s:.3e} (bound {b_s:.3e}), P {e_p:.3e} (bound 1e-6), O {e_o:.3e} (bound {b_o:.3e})")
    assert e_s < b_s and e_p < 1e-6 and e_o < b_o


# ---- 6. search over an index above 2^32 bytes --------------------------------------------------------------------------------------
NQ, TOPK = len(ws.SEARCH_PLANTED), 8
BLK, NROWS, DIM = ws.SEARCH_BLOCK, ws.SEARCH_N, ws.SEARCH_D
POS = np.array(ws.SEARCH_PLANTED, dtype=np.int64)


@pytest.fixture(scope="module")
def index():
    """the index on the device: a 4096-row base block tiled over all rows, with row POS[j] a nudged copy of query j (8 (j + 1) codes moved
    by one step).  The references run on base block + planted rows only (`small`: column 4096 + j is planted row j)"""
    ops = _api()
    from sgic_amd.search import code_rnorm, codes_to_unit
    _drop_caches()
    free, total = torch.cuda.mem_get_info()
    need = ws.footprint(ws.CASES["search_index"]) + ws.HEADROOM
    if free < need:
        pytest.skip(f"search_index: {free / 1e9:.1f} GB free of {total / 1e9:.1f} GB, needs {need / 1e9:.1f} GB (footprint + headroom)")
    _INDEX_BASE[0] = torch.cuda.memory_allocated()
    rng = np.random.default_rng(2024)
    base = cref.quantised_unit_codes(rng, BLK, DIM)
    q = cref.quantised_unit_codes(rng, NQ, DIM)
    planted = np.stack([rgref.nudged(rng, q[j], 8 * (j + 1)) for j in range(NQ)])
    small = np.concatenate([base, planted])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    db = up(base).repeat(NROWS // BLK, 1)
    r_db = up(code_rnorm(base)).repeat(NROWS // BLK)
    pos = torch.from_numpy(POS).to(DEV)
    db[pos] = up(planted)
    r_db[pos] = up(code_rnorm(planted))
    assert db.shape == (NROWS, DIM) and db.is_contiguous() and db.numel() > 1 << 32
    qf = codes_to_unit(q)
    ix = dict(ops=ops, base=base, q=q, qf=qf, planted=planted, small=small, db=db, r_db=r_db, dq=up(q), drq=up(code_rnorm(q)), dqf=up(qf))
    yield ix
    ix.clear()


def _ref(ix, policy):
    """(key, score) (NQ, 4096 + NQ) of the numpy restatements; asserts what the plan rests on: own planted scores strictly descending,
    all above every other score -> (key, score, threshold between the two)"""
    key, score = cref.keys_and_scores(ix["q"], ix["small"]) if policy == "u8" else vref.keys_and_scores(ix["qf"], ix["small"])
    own = score[np.arange(NQ), BLK + np.arange(NQ)]
    rest = score.copy()
    rest[np.arange(NQ), BLK + np.arange(NQ)] = -np.inf
    assert np.all(np.diff(own) < 0) and own.min() > rest.max() + 0.05, (own, rest.max())
    return key, score, float(np.float32(0.5 * (float(own.min()) + float(rest.max()))))


def _col(idx):
    """row of the full index -> its column of `small`"""
    idx = np.asarray(idx, dtype=np.int64)
    hit = idx[..., None] == POS
    return np.where(hit.any(-1), BLK + hit.argmax(-1), idx % BLK)


def _full_topk(key, score, k):
    """top-k of the tiled index from the small reference: planted rows plus the first k + 1 copies of the k + 1 best base rows"""
    out_s, out_i = np.empty((NQ, k), dtype=np.float32), np.empty((NQ, k), dtype=np.int32)
    for j in range(NQ):
        best = np.lexsort((np.arange(BLK), -key[j, :BLK]))[:k + 1]
        cand = (best[:, None] + BLK * np.arange(k + 1)[None, :]).ravel()
        cand = np.concatenate([cand[~np.isin(cand, POS)], POS])
        kk = key[j, _col(cand)]
        order = np.lexsort((cand, -kk))[:k]
        out_i[j], out_s[j] = cand[order], score[j, _col(cand[order])]
    return out_s, out_i


def _full_rank(key, j, target):
    """rows of the tiled index that come before `target` for query j: a higher key, or the same key and a lower index"""
    kt = key[j, _col(target)]
    kb = key[j, :BLK]
    r = np.arange(BLK)
    copies = (NROWS - 1 - r) // BLK + 1 - np.bincount(POS % BLK, minlength=BLK)
    below = np.maximum(0, -(-(target - r) // BLK)) - np.bincount((POS % BLK)[POS < target], minlength=BLK)
    n = int(copies[kb > kt].sum()) + int(below[kb == kt].sum())
    kp = key[j, BLK:]
    return n + int(((kp > kt) | ((kp == kt) & (POS < target))).sum())


@pytest.mark.parametrize("splits", [None, 1, 2048])
@pytest.mark.parametrize("policy", ["u8", "f32q"])
def test_search_topk(index, policy, splits):
    """k = 8 with the default splits, one split and the most splits: scores bit for bit, indices exact"""
    ops = index["ops"]
    torch.cuda.reset_peak_memory_stats()
    _BUDGET["search_index"] = (ws.footprint(ws.CASES["search_index"]), _INDEX_BASE[0])
    key, score, _ = _ref(index, policy)
    want_s, want_i = _full_topk(key, score, TOPK)
    assert want_i[:, 0].tolist() == POS.tolist()
    if policy == "u8":
        s, i = ops.search_codes(index["dq"], index["drq"], index["db"], index["r_db"], TOPK, splits=splits)
    else:
        s, i = ops.search_codes_f32q(index["dqf"], index["db"], index["r_db"], TOPK, splits=splits)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(i, want_i), (policy, splits, i.tolist(), want_i.tolist())
    assert np.array_equal(s.view(np.uint32), want_s.view(np.uint32)), (policy, splits)


@pytest.mark.parametrize("policy", ["u8", "f32q"])
def test_search_range_and_rank(index, policy):
    """threshold between the planted and every other score: the hit list is the planted pairs.  Rank of every query's own planted row
    (0) and of its neighbour's (counted over the tiled index from the small reference)"""
    ops = index["ops"]
    torch.cuda.reset_peak_memory_stats()
    _BUDGET["search_index"] = (ws.footprint(ws.CASES["search_index"]), _INDEX_BASE[0])
    key, score, thr = _ref(index, policy)
    own = score[np.arange(NQ), BLK + np.arange(NQ)]
    if policy == "u8":
        hq, hd, hs, cnt = ops.search_codes_range(index["dq"], index["drq"], index["db"], index["r_db"], thr)
    else:
        hq, hd, hs, cnt = ops.search_codes_range_f32q(index["dqf"], index["db"], index["r_db"], thr)
    assert cnt == NQ and hq.cpu().tolist() == list(range(NQ)) and hd.cpu().tolist() == POS.tolist()
    assert np.array_equal(hs.cpu().numpy().view(np.uint32), own.view(np.uint32))
    for shift in (0, 1):
        targets = np.roll(POS, -shift)
        want_r = np.array([_full_rank(key, j, int(targets[j])) for j in range(NQ)], dtype=np.int64)
        want_s = score[np.arange(NQ), _col(targets)]
        if policy == "u8":
            rk, sc = ops.search_codes_rank(index["dq"], index["drq"], index["db"], index["r_db"], targets)
        else:
            rk, sc = ops.search_codes_rank_f32q(index["dqf"], index["db"], index["r_db"], targets)
        assert np.array_equal(rk.cpu().numpy().astype(np.int64), want_r), (policy, shift, rk.cpu().tolist(), want_r.tolist())
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), want_s.view(np.uint32)), (policy, shift)
        assert shift or not want_r.any()


def test_assign_codes_and_cluster_sums(index):
    """K = 64 centroids.  assign_codes: the 4096-row slabs around the marks and at the end equal the call on those rows alone (ids, the
    integer M and the score bits).  cluster_sums: exact, = tiles x the base block's sums per cluster, corrected for the planted rows"""
    ops = index["ops"]
    torch.cuda.reset_peak_memory_stats()
    _BUDGET["search_index"] = (ws.footprint(ws.CASES["search_index"]), _INDEX_BASE[0])
    db, r_db = index["db"], index["r_db"]
    cent = torch.from_numpy(vref.random_unit(np.random.default_rng(7), ws.SEARCH_K, DIM)).to(DEV)
    oc, sc, oM = ops.assign_codes(cent, db, r_db, return_int=True)
    for u in ws.probes(ws.CASES["search_index"]):
        rows = slice(u * BLK, (u + 1) * BLK)
        c1, s1, m1 = ops.assign_codes(cent, db[rows].clone(), r_db[rows].clone(), return_int=True)
        assert torch.equal(c1, oc[rows]) and torch.equal(m1, oM[rows]) and _same_bits(s1, sc[rows]), f"rows {u * BLK}..{(u + 1) * BLK}"
    tiles = NROWS // BLK
    grid = oc.view(tiles, BLK)
    template = grid[1]                                                  # a tile without a planted row
    odd = torch.nonzero(grid != template).cpu().numpy()
    assert {(int(t), int(r)) for t, r in odd} <= {(int(p // BLK), int(p % BLK)) for p in POS}, "the assignment is not that of the tiles"
    sums, counts = ops.cluster_sums(db, oc, ws.SEARCH_K)
    tb = template.cpu().numpy().astype(np.int64)
    vb = 2 * index["base"].astype(np.int64) - 255
    want = np.zeros((ws.SEARCH_K, DIM), dtype=np.int64)
    np.add.at(want, tb, vb)
    want *= tiles
    wcnt = np.bincount(tb, minlength=ws.SEARCH_K).astype(np.int64) * tiles
    got_c = oc[torch.from_numpy(POS).to(DEV)].cpu().numpy()
    for j, p in enumerate(POS):
        want[tb[p % BLK]] -= vb[p % BLK]
        wcnt[tb[p % BLK]] -= 1
        want[got_c[j]] += 2 * index["planted"][j].astype(np.int64) - 255
        wcnt[got_c[j]] += 1
    assert np.array_equal(counts.cpu().numpy(), wcnt) and np.array_equal(sums.cpu().numpy(), want)


# ---- 7. end to end: the default decompress.py call -------------------------------------------------------------------------------
def test_end_to_end_batch32_of_1024(monkeypatch):
    """SMALL configuration, synthetic weights: encode_batch of 32 distinct 1024 x 1024 images, decode_batch of all 32 (tensors reach
    2^32 bytes), and images 0, 15, 16 and 31 decoded alone equal their rows bitwise.  The launch-mode race is off (cache / heuristic
    only): at these sizes it would run every candidate several times, every mode gives the same bits, and the tuner has its own tests"""
    ops = _api()
    from sgic_amd import weights as Wt
    from sgic_amd.codec import Codec
    from sgic_amd.config import SMALL
    from sgic_amd.data import synth_images
    case, probes = _begin("decode_batch_32x1024")
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    codec = Codec(Wt.synth_weights(Wt.full_spec(SMALL), seed=1234), SMALL, DEV)
    codec.hybrid_codec.quantize_feat.force_zero_thres = 0.12
    codec.hybrid_codec.quantize_feat.update(force=True)
    B = case["n_units"]
    x = synth_images(B, 1024, 1024, seed=4242).to(DEV)
    assert all(not torch.equal(x[0], x[b]) for b in range(1, B))
    encs = codec.encode_batch(x)
    del x
    x_hat = codec.decode_batch(encs)
    assert x_hat.shape == (B, 3, 1024, 1024) and bool(torch.isfinite(x_hat).all()) and codec.bottleneck.last_repairs == 0
    for b in sorted(set(probes) | {0, 15, 16, 31}):
        one = codec.decode_batch([encs[b]])
        assert codec.bottleneck.last_repairs == 0
        assert torch.equal(one[0], x_hat[b]), f"image {b} of the batch != that image decoded alone"
