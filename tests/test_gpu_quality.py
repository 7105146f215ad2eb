"""GPU: sgic_quality_u8 (csrc/quality.hip) and quality.measure against the fp64 restatement tests/quality_ref.py.  The squared
error is exact; every level value and ms_ssim is within 1e-11 of the restatement -- about 300 times what a change of summation order
does in fp64 (tests/test_quality_cpu.py prints it) and six orders below the error of an fp32 evaluation."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-11


def _up(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared cases are read-only


@pytest.mark.parametrize("kind", ref.PAIRS)
@pytest.mark.parametrize("H,W,B", ref.SIZES)
def test_parity_with_the_restatement(H, W, B, kind):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops, quality
    a, b, want_sse, want_lv = ref.case(H, W, B, kind)
    da, db = _up(a), _up(b)
    sse, lv = ops.quality_u8(da, db)
    sse2, lv2 = ops.quality_u8(da, db)
    assert sse.dtype == torch.int64 and sse.shape == (B, 3) and lv.dtype == torch.float64 and lv.shape == (B, 3, 5, 2)
    assert torch.equal(sse, sse2) and torch.equal(lv.view(torch.int64), lv2.view(torch.int64))     # the same bits twice
    assert np.array_equal(da.cpu().numpy(), a) and np.array_equal(db.cpu().numpy(), b)            # inputs untouched
    sse, lv = sse.cpu().numpy(), lv.cpu().numpy()
    err = float(np.abs(lv - want_lv).max())
    got, want = quality.combine(sse, lv, H, W), quality.combine(want_sse, want_lv, H, W)
    err_ms = float(np.abs(got["ms_ssim"] - want["ms_ssim"]).max())
    print(f"{H}x{W} B={B} {kind}: level error {err:.3e}, ms_ssim error {err_ms:.3e}, ms_ssim {want['ms_ssim'].tolist()}")
    assert np.array_equal(sse, want_sse)
    assert np.array_equal(got["psnr"], want["psnr"])
    assert err <= TOL and err_ms <= TOL
    m = quality.measure(da, db)
    for k in ("psnr", "ssim", "ms_ssim", "ms_ssim_db"):
        assert np.array_equal(m[k], got[k])
    if kind == "identical":
        assert got["ms_ssim"][0] == 1.0 and np.isinf(got["psnr"][0]) and np.isinf(got["ms_ssim_db"][0])
    if kind == "inverted":
        assert got["ms_ssim"][0] == 0.0


def test_refusals_come_before_any_launch():
    """every refused call is stopped by the host-side checks: the outputs keep their fill"""
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib
    H = W = 200
    a = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    nbytes = ctypes.c_size_t(0)
    _lib.call("sgic_quality_u8_work_bytes", 1, H, W, ctypes.byref(nbytes))
    assert nbytes.value > 0
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    sse = torch.full((1, 3), -7, dtype=torch.int64, device=DEV)
    lv = torch.full((1, 3, 5, 2), -7.0, dtype=torch.float64, device=DEV)
    size = ctypes.c_size_t
    bad = [(a, a, 1, 160, W, work, size(nbytes.value), sse, lv),          # H = 160: no fifth level
           (a, a, 1, H, 160, work, size(nbytes.value), sse, lv),
           (a, a, 0, H, W, work, size(nbytes.value), sse, lv),            # B < 1
           (a, a, 1, 16385, W, work, size(nbytes.value), sse, lv),        # H > 16384
           (a, a, 1, H, W, work, size(nbytes.value - 1), sse, lv),        # a workspace one byte short
           (None, a, 1, H, W, work, size(nbytes.value), sse, lv),         # null pointers
           (a, None, 1, H, W, work, size(nbytes.value), sse, lv),
           (a, a, 1, H, W, None, size(nbytes.value), sse, lv),
           (a, a, 1, H, W, work, size(nbytes.value), None, lv),
           (a, a, 1, H, W, work, size(nbytes.value), sse, None)]
    for args in bad:
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call("sgic_quality_u8", *args)
    for args in ((1, 160, W), (0, H, W), (1, H, 16385)):
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call("sgic_quality_u8_work_bytes", *args, ctypes.byref(nbytes))
    assert bool((sse == -7).all()) and bool((lv == -7.0).all())


def test_measure_small_images_give_psnr_only():
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (2, 100, 120, 3), dtype=np.uint8)
    b = a.copy()
    b[0, 3, 4, 1] ^= 0x10
    m = quality.measure(_up(a), _up(b))
    assert m["ssim"] is None and m["ms_ssim"] is None and m["ms_ssim_db"] is None
    assert m["psnr"][0] == 10.0 * np.log10(65025.0 * 3 * 100 * 120 / 256.0) and np.isinf(m["psnr"][1])
