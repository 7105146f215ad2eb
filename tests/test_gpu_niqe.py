"""GPU: sgic_niqe_u8 (csrc/niqe.hip), niqe.Niqe and the `fit` sub-command against the fp64 restatement tests/niqe_ref.py.  The counts
of negative and positive samples are EQUAL (the MSCN sign comes from exact integer class sums); the sums of squares, of magnitudes
and the sharpness are within 2e-12 relative: they are sums of at most 9216 non-negative fp64 terms, which any order keeps within
(n - 1) u + u < 1.1e-12, and the factor leaves room for a last-bit difference in division and square root.  The alphas are equal
(tests/test_niqe_cpu.py holds every rn at least 1e-9 away from a decision boundary) and the scores are within
niqe_ref.score_tolerance(), ten times what that bound on the sums moves a score by."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niqe_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]


def _up(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared cases are read-only


def _close(got, want, what):
    err = np.abs(got - want)
    worst = float((err / np.where(want == 0.0, 1.0, np.abs(want))).max())
    print(f"{what}: largest relative difference {worst:.3e}")
    assert bool((err <= ref.REL * np.abs(want)).all()), (what, worst)


@pytest.mark.parametrize("name", ref.CASES)
def test_parity_with_the_restatement(name):
    import sgic_amd  # noqa: F401
    from sgic_amd import niqe, ops
    img, want, want_sharp, want_scores = ref.case(name)
    x = _up(img)
    stats, sharp = ops.niqe_blocks_u8(x)
    again, sharp_again = ops.niqe_blocks_u8(x)
    assert torch.equal(stats, again) and torch.equal(sharp, sharp_again), "two runs differ"
    got, got_sharp = stats.cpu().numpy(), sharp.cpu().numpy()
    assert got.shape == want.shape and got_sharp.shape == want_sharp.shape
    assert np.array_equal(got[..., :2], want[..., :2]), "counts of negative / positive samples differ"
    _close(got[..., 2:], want[..., 2:], f"{name} sums")
    _close(got_sharp, want_sharp, f"{name} sharpness")
    fa, fb = niqe.features(got), niqe.features(want)
    assert np.array_equal(np.isnan(fa), np.isnan(fb))
    assert np.array_equal(fa[..., ALPHA_COLS], fb[..., ALPHA_COLS], equal_nan=True), "alphas differ"
    measured = niqe.Niqe(ref.pristine()).measure(x)
    assert measured.dtype == np.float64 and measured.shape == (img.shape[0],)
    tol = ref.score_tolerance()
    for j, w in enumerate(want_scores):
        if w is None:
            assert np.isnan(measured[j])
        else:
            print(f"{name}[{j}]: score {measured[j]!r}, restatement {w!r}, difference {abs(measured[j] - w):.3e}, tolerance {tol:.3e}")
            assert abs(measured[j] - w) <= tol
    if name in ref.NO_SCORE:
        assert all(w is None for w in want_scores)
    if name == "flat":
        assert not got[..., :2].any() and not got[..., 2:].any(), "a flat image has MSCN samples that are not exactly 0"


def test_batch_slots_equal_single_calls():
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    img = ref.case("batch3")[0]
    stats, sharp = ops.niqe_blocks_u8(_up(img))
    for j in range(img.shape[0]):
        s1, h1 = ops.niqe_blocks_u8(_up(img[j:j + 1]))
        assert torch.equal(stats[j], s1[0]) and torch.equal(sharp[j], h1[0]), j


def test_too_small_images_launch_nothing():
    import sgic_amd  # noqa: F401
    from sgic_amd import niqe
    H, W = (int(v) for v in ref.NO_LAUNCH.split("x"))
    out = niqe.Niqe(ref.pristine()).measure(torch.zeros(2, H, W, 3, dtype=torch.uint8, device=DEV))
    assert out.shape == (2,) and np.isnan(out).all()


def test_refusals_come_before_any_launch():
    """every refused call is stopped by the host-side checks: the outputs keep their fill"""
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib, niqe
    H, W = 96, 192
    x = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    nbytes = ctypes.c_size_t(0)
    _lib.call("sgic_niqe_u8_work_bytes", 1, H, W, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value + 16, dtype=torch.uint8, device=DEV)
    stats = torch.full((1, 1, 2, 2, 5, 5), -7.0, dtype=torch.float64, device=DEV)
    sharp = torch.full((1, 1, 2), -7.0, dtype=torch.float64, device=DEV)
    wts = np.array(niqe.window_weights(), dtype=np.float64)
    size = ctypes.c_size_t
    ok = nbytes.value
    bad = [(x, 0, H, W, wts, work, size(ok), stats, sharp),               # B < 1
           (x, 1, 95, W, wts, work, size(ok), stats, sharp),              # H, W outside [96, 16384]
           (x, 1, H, 95, wts, work, size(ok), stats, sharp),
           (x, 1, 16385, W, wts, work, size(ok), stats, sharp),
           (x, 1, H, 16385, wts, work, size(ok), stats, sharp),
           (x, 1, H, W, wts, work[1:], size(ok), stats, sharp),           # misaligned workspace
           (x, 1, H, W, wts, work, size(ok - 1), stats, sharp),           # short workspace
           (None, 1, H, W, wts, work, size(ok), stats, sharp),            # null pointers
           (x, 1, H, W, None, work, size(ok), stats, sharp),
           (x, 1, H, W, wts, None, size(ok), stats, sharp),
           (x, 1, H, W, wts, work, size(ok), None, sharp),
           (x, 1, H, W, wts, work, size(ok), stats, None)]
    for args in bad:
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call("sgic_niqe_u8", *args)
    for args in ((1, 95, W), (0, H, W), (1, H, 16385)):
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call("sgic_niqe_u8_work_bytes", *args, ctypes.byref(nbytes))
    assert bool((stats == -7.0).all()) and bool((sharp == -7.0).all())


def test_fit_reproduces_the_restatement(tmp_path, capsys):
    """`python -m sgic_amd.niqe fit` (called in this process) on six PNGs of three sizes -> the restatement's mu and cov, within ten
    times what the bound on the sums moves an entry by; an unreadable and a too small file are skipped"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import niqe
    src = tmp_path / "imgs"
    src.mkdir()
    for k, img in enumerate(ref.fit_images()):
        Image.fromarray(img).save(src / f"im{k}.png")
    Image.fromarray(ref.natural(95, 120, 1)).save(src / "small.png")
    (src / "broken.png").write_bytes(b"not a png")
    out = tmp_path / "params.npz"
    capsys.readouterr()
    assert niqe.main(["fit", "--images", str(src), "--out", str(out), "--batch_size", "2"]) == 0
    err = capsys.readouterr().err.splitlines()      # the stream of this call, whichever stream the module was imported under
    assert any(ln.startswith("[SKIP] broken: unreadable image") for ln in err)
    assert "[SKIP] small: 95x120 is smaller than one 96x96 block" in err
    mu, cov = niqe.load_params(str(out))
    want_mu, want_cov, tol_mu, tol_cov = ref.fit_case()
    print(f"fit: mu off by {np.abs(mu - want_mu).max():.3e} (tolerance {tol_mu:.3e}), cov by {np.abs(cov - want_cov).max():.3e} "
          f"(tolerance {tol_cov:.3e})")
    assert np.abs(mu - want_mu).max() <= tol_mu and np.abs(cov - want_cov).max() <= tol_cov
