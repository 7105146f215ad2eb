"""GPU: dists.DistsVGG.measure over the shared case list (tests/lpips_ref.py's, through tests/dists_ref.py) against the fp64
restatement.

Tolerances.  Tap 0: |dev - t64| <= 1e-12 for both terms, the flat pairs included: the device forms tap 0 from exact integer sums in
fp64.  Taps 1..5: |dev - t64| <= 8 * E_ABS per term.  E_ABS is the fp32 error of the restatement itself over the same case list, max
|t32 - t64| over the terms of taps 1..5 as printed by tests/test_dists_cpu.py::test_fp32_error_of_the_restatement (torch CPU, seed
1234: 2.091e-08).  The factor 8 covers the other order in which the split convolutions add their 9 Cin products and the deep taps
that average over as few as one pixel (DESIGN.md section 15 has the measured ratios)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dists_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ABS = 2.091e-08
FACTOR = 8.0
TAP0_TOL = 1e-12


def _up(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared cases are read-only


@pytest.fixture(scope="module")
def model():
    import sgic_amd  # noqa: F401
    from sgic_amd import dists
    m = dists.DistsVGG(dists.synth_weights(ref.SEED), DEV)
    assert m.conv[0][0].shape == (64, 9 * 32) and m.conv[0][2] == 32 and m.conv[-1][0].shape == (512, 9 * 512)
    assert [v.numel() for v in m.alpha] == [64, 128, 256, 512, 512] and len(m.alpha0) == 3
    return m


@pytest.mark.parametrize("i", range(len(ref.SIZES)), ids=[f"{b}x{h}x{w}" for b, h, w in ref.SIZES])
def test_measure_against_the_fp64_restatement(model, i):
    case, (want_tot, want) = ref.case_list()[i], ref.reference()[i]
    B = case["size"][0]
    a, b = _up(case["a"]), _up(case["b"])
    tot, terms = model.measure(a, b)
    assert tot.dtype == np.float64 and tot.shape == (5 * B,) and terms.dtype == np.float64 and terms.shape == (5 * B, 6, 2)
    flat = terms.reshape(5 * B, 12)
    acc = np.zeros(5 * B)
    for k in range(12):
        acc += flat[:, k]
    assert np.array_equal(tot, acc)
    err = np.abs(terms - want)
    ratio = float(err[:, 1:].max() / E_ABS)
    print(f"size {case['size']}: tap 0 worst |dev - t64| = {err[:, 0].max():.3e} (bound {TAP0_TOL}; flat pairs {err[4 * B:, 0].max():.3e}); "
          f"taps 1..5 worst |dev - t64| / e_abs = {ratio:.3f} (bound {FACTOR}), per tap {[f'{v / E_ABS:.2f}' for v in err[:, 1:].max(axis=(0, 2))]}; "
          f"dists {tot[B:].min():.3e} .. {tot.max():.4f}")
    assert np.all(terms[:B] == 0.0) and np.all(tot[:B] == 0.0)            # identical pairs: exactly 0.0
    assert np.all(err[:, 0] <= TAP0_TOL)
    assert np.all(err[:, 1:] <= FACTOR * E_ABS)
    assert np.all(np.abs(tot - want_tot) <= 10 * FACTOR * E_ABS + 2 * TAP0_TOL)     # ten such terms and the two of tap 0
    # swapping the sides gives the same bits
    tot_s, terms_s = model.measure(b, a)
    assert np.array_equal(tot, tot_s) and np.array_equal(terms, terms_s)
    # a forced chunk of one pair, and a pair alone: the same bits as inside the batch
    model.max_pixels = 1
    try:
        tot_c, terms_c = model.measure(a, b)
    finally:
        from sgic_amd import dists
        model.max_pixels = dists.MAX_PIXELS
    assert np.array_equal(tot, tot_c) and np.array_equal(terms, terms_c)
    j = 5 * B - 2 if B > 1 else 2
    tot_1, terms_1 = model.measure(a[j:j + 1], b[j:j + 1])
    assert tot_1[0] == tot[j] and np.array_equal(terms_1[0], terms[j])


def test_chunks_follow_the_pixel_bound(model, monkeypatch):
    from sgic_amd import dists, lpips
    seen = []
    monkeypatch.setattr(model, "_chunk", lambda a, b, terms, m0: (seen.append(a.shape[0]), terms.zero_(), m0.zero_()))
    z = torch.zeros(7, 32, 32, 3, dtype=torch.uint8, device=DEV)
    monkeypatch.setattr(model, "max_pixels", 2 * 32 * 32 * 3)
    model.measure(z, z)
    assert seen == [3, 3, 1]
    del seen[:]
    monkeypatch.setattr(model, "max_pixels", dists.MAX_PIXELS)
    model.measure(z, z)
    assert seen == [7] and dists.MAX_PIXELS == lpips.MAX_PIXELS == 1 << 21


def test_small_images_give_none(model):
    z = torch.zeros(1, 15, 40, 3, dtype=torch.uint8, device=DEV)
    assert model.measure(z, z) is None
    z = torch.zeros(1, 40, 15, 3, dtype=torch.uint8, device=DEV)
    assert model.measure(z, z) is None
