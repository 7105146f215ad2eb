"""GPU: the luma measures of csrc/hvs.hip (quality.vifp, gmsd, psnr_hvs, measure_hvs) against the fp64 restatement tests/hvs_ref.py.
Both sides are fp64 and differ in summation order only (separable against whole windows, shuffle trees against numpy's sums), so
every value is held to the relative 1e-11 of tests/test_gpu_quality.py; the luma plane itself has to be the restatement's bits."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hvs_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-11
# 41: the smallest VIFp size; 49 x 57: odd both ways, every ::2 sees an odd length; 130 x 70: tile seams of the 16 x 32 tiles inside
# every map (VIFp scale 1: 114 x 54, GMSD: 65 x 35) and four workgroups of 32 DCT blocks; 8 x 8, 15 x 23: one and two whole blocks
# beside partial ones; 9 x 9: GMSD's odd half-size map, the last row and column half padding
SIZES = [(41, 41), (49, 57), (64, 64), (130, 70), (8, 8), (15, 23), (9, 9)]
KINDS = ("noise", "blur")


def _up(x):
    return torch.from_numpy(np.array(x)).to(DEV)[None]        # a copy: the shared cases are read-only


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_parity_with_the_restatement(H, W, kind):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops, quality
    a, b, want = ref.case(kind, H, W)
    da, db = _up(a), _up(b)
    ya = ops.hvs_luma_u8(da)
    assert ya.dtype == torch.float64 and ya.shape == (1, H, W) and np.array_equal(ya[0].cpu().numpy(), ref.luma(a))
    got = quality.measure_hvs(da, db)
    again = quality.measure_hvs(da, db)
    assert list(got) == ["vifp", "gmsd", "psnr_hvs", "psnr_hvs_m"]
    assert np.array_equal(da[0].cpu().numpy(), a) and np.array_equal(db[0].cpu().numpy(), b)            # inputs untouched
    for k, w in want.items():
        if w is None:
            assert got[k] is None
            continue
        assert got[k].dtype == np.float64 and got[k].shape == (1,)
        assert got[k].tobytes() == again[k].tobytes()                                                  # the same bits twice
        err = _rel(float(got[k][0]), w)
        print(f"{H}x{W} {kind} {k}: {float(got[k][0])!r} against {w!r}, relative error {err:.3e}")
    for k, w in want.items():
        if w is not None:
            assert _rel(float(got[k][0]), w) <= TOL, k
    # the single-measure entry points give measure_hvs's bits, or refuse what it reports as None
    assert quality.gmsd(da, db).tobytes() == got["gmsd"].tobytes()
    if want["vifp"] is None:
        with pytest.raises(ValueError, match="41"):
            quality.vifp(da, db)
    else:
        assert quality.vifp(da, db).tobytes() == got["vifp"].tobytes()
    hvs, hvs_m = quality.psnr_hvs(da, db)
    assert hvs.tobytes() == got["psnr_hvs"].tobytes() and hvs_m.tobytes() == got["psnr_hvs_m"].tobytes()
    assert hvs_m[0] >= hvs[0]


def test_a_batch_equals_its_single_calls_bitwise():
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    pairs = [ref.case(kind, 64, 64)[:2] for kind in ("noise", "blur", "offset")]
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
    b = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
    batch = quality.measure_hvs(a, b)
    for j in range(3):
        one = quality.measure_hvs(a[j:j + 1].contiguous(), b[j:j + 1].contiguous())
        for k in batch:
            assert batch[k].shape == (3,) and batch[k][j:j + 1].tobytes() == one[k].tobytes(), (k, j)
    rev = quality.measure_hvs(a.flip(0).contiguous(), b.flip(0).contiguous())      # other neighbours, another slot
    for k in batch:
        assert rev[k][::-1].tobytes() == batch[k].tobytes(), k


def test_special_values():
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    a, b, want = ref.case("identical", 49, 57)
    m = quality.measure_hvs(_up(a), _up(b))
    assert m["gmsd"][0] == 0.0 and math.isinf(m["psnr_hvs"][0]) and math.isinf(m["psnr_hvs_m"][0]) and m["psnr_hvs"][0] > 0
    assert m["vifp"][0] <= 1.0 and 1.0 - m["vifp"][0] < 1e-9 and _rel(m["vifp"][0], want["vifp"]) <= TOL      # eps keeps it below 1
    a, b, _ = ref.case("flat_equal", 49, 57)
    m = quality.measure_hvs(_up(a), _up(b))
    assert m["vifp"][0] == 1.0 and m["gmsd"][0] == 0.0 and math.isinf(m["psnr_hvs"][0]) and math.isinf(m["psnr_hvs_m"][0])
    a, b, want = ref.case("flat", 49, 57)
    m = quality.measure_hvs(_up(a), _up(b))
    assert m["vifp"][0] == 0.0 and _rel(m["gmsd"][0], want["gmsd"]) <= TOL and m["psnr_hvs"][0] == m["psnr_hvs_m"][0]
    a, b, want = ref.case("offset", 49, 57)
    m = quality.measure_hvs(_up(a), _up(b))
    dc = 10.0 * np.log10(255.0 ** 2 / ((3.0 * 8.0 * ref.CSFCOF[0, 0]) ** 2 / 64.0))
    print(f"offset: psnr_hvs {m['psnr_hvs'][0]!r}, psnr_hvs_m {m['psnr_hvs_m'][0]!r} against the DC term's {dc!r}; gmsd {m['gmsd'][0]!r} "
          f"against {want['gmsd']!r}")
    assert _rel(m["psnr_hvs"][0], dc) <= TOL and _rel(m["psnr_hvs_m"][0], dc) <= TOL
    assert _rel(m["gmsd"][0], want["gmsd"]) <= TOL
    # constants 100 and 103 on even sides: GMS is 1 inside and takes two other values on the zero-padded edges and corners
    # (tests/test_hvs_cpu.py works the closed form out)
    c1 = torch.full((1, 20, 28, 3), 100, dtype=torch.uint8, device=DEV)
    got = float(quality.gmsd(c1, c1 + 3)[0])
    y1, y2 = ref.luma(np.full(3, 100, np.uint8)), ref.luma(np.full(3, 103, np.uint8))
    k = np.concatenate([np.zeros(8 * 12), np.ones(2 * 8 + 2 * 12), np.full(4, 8.0 / 9.0)])
    vals = (2.0 * y1 * y2 * k + 170.0) / ((y1 * y1 + y2 * y2) * k + 170.0)
    # the deviations from the mean are about 4e-4 of values near 1 that carry a rounding of 1.1e-16 each: a relative 3e-13 per
    # sample in either computation; 1e-10 leaves the closed form's own rounding (k = 8 / 9, the luma of a grey) far inside
    assert _rel(got, float(np.sqrt(np.mean((vals - vals.mean()) ** 2)))) <= 1e-10


def test_refusals():
    """one less than the smallest sizes: a ValueError that names the side from the wrappers, SGIC_EINVAL before any launch from
    the C entry points; measure_hvs reports None and goes on"""
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib, ops, quality
    for H, W in ((40, 41), (41, 40)):
        a = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match=r"sides >= 41"):
            quality.vifp(a, a)
        m = quality.measure_hvs(a, a)
        assert m["vifp"] is None and m["gmsd"][0] == 0.0 and math.isinf(m["psnr_hvs"][0])
    a = torch.zeros(1, 7, 9, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match=r"sides >= 8"):
        quality.psnr_hvs(a, a)
    m = quality.measure_hvs(a, a)
    assert m["vifp"] is None and m["psnr_hvs"] is None and m["psnr_hvs_m"] is None and m["gmsd"][0] == 0.0
    y = ops.hvs_luma_u8(torch.zeros(1, 41, 41, 3, dtype=torch.uint8, device=DEV))
    nbytes = ctypes.c_size_t(0)
    _lib.call("sgic_hvs_vifp_work_bytes", 1, 41, 41, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 2), -7.0, dtype=torch.float64, device=DEV)
    size = ctypes.c_size_t
    q = np.array(ref.Q_LUMA.ravel(), dtype=np.int32)
    bad = [("sgic_hvs_vifp", (y, y, 1, 40, 41, work, size(nbytes.value), out)),
           ("sgic_hvs_vifp", (y, y, 1, 41, 40, work, size(nbytes.value), out)),
           ("sgic_hvs_vifp", (y, y, 0, 41, 41, work, size(nbytes.value), out)),
           ("sgic_hvs_vifp", (y, y, 1, 41, 41, work, size(nbytes.value - 1), out)),
           ("sgic_hvs_vifp", (None, y, 1, 41, 41, work, size(nbytes.value), out)),
           ("sgic_hvs_vifp", (y, y, 1, 41, 41, None, size(nbytes.value), out)),
           ("sgic_hvs_gmsd", (y, y, 1, 16385, 41, work, size(nbytes.value), out)),
           ("sgic_hvs_gmsd", (y, None, 1, 41, 41, work, size(nbytes.value), out)),
           ("sgic_hvs_gmsd", (y, y, 1, 41, 41, work, size(8), out)),
           ("sgic_hvs_psnr", (y, y, 1, 7, 41, q, work, size(nbytes.value), out)),
           ("sgic_hvs_psnr", (y, y, 1, 41, 41, None, work, size(nbytes.value), out)),
           ("sgic_hvs_psnr", (y, y, 1, 41, 41, np.zeros(64, dtype=np.int32), work, size(nbytes.value), out)),
           ("sgic_hvs_psnr", (y, y, 1, 41, 41, q, work, size(8), out)),
           ("sgic_hvs_luma_u8", (None, 1, 41, 41, y))]
    for name, args in bad:
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call(name, *args)
    for name, args in (("sgic_hvs_vifp_work_bytes", (1, 40, 41)), ("sgic_hvs_psnr_work_bytes", (1, 41, 7)), ("sgic_hvs_gmsd_work_bytes", (0, 41, 41))):
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call(name, *args, ctypes.byref(nbytes))
    assert bool((out == -7.0).all())
