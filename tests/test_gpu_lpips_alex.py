"""GPU: lpips_alex.LpipsAlex.measure over the shared case list (tests/lpips_alex_ref.py) against the fp64 restatement.

Tolerance: for every layer value |dev - d64| <= 8 * E_REL * d64.  E_REL is the fp32 error of the restatement itself over the same
case list, max |d32 - d64| / d64 as printed by tests/test_lpips_alex_cpu.py::test_fp32_error_of_the_restatement (torch CPU, seed
1234: 4.022e-06).  The factor 8 is that of tests/test_gpu_lpips.py, for the same reason: the split GEMMs add their K products (here
K <= 3456) in another order, and the deepest taps average over as few as one pixel.  Measured on an MI355X, worst ratio per size:
1.7, 0.7, 2.3, 0.5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_alex_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_REL = 4.022e-06
FACTOR = 8.0


def _up(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared cases are read-only


@pytest.fixture(scope="module")
def model():
    import sgic_amd  # noqa: F401
    from sgic_amd import lpips_alex
    m = lpips_alex.LpipsAlex(lpips_alex.synth_weights(ref.SEED), DEV)
    assert [tuple(c[0].shape) for c in m.conv] == [(64, 384), (192, 1600), (384, 9 * 192), (256, 9 * 384), (256, 9 * 256)]
    assert not bool(m.conv[0][0][:, 363:].any())
    return m


@pytest.mark.parametrize("i", range(len(ref.SIZES)), ids=[f"{b}x{h}x{w}" for b, h, w in ref.SIZES])
def test_measure_against_the_fp64_restatement(model, i):
    case, (want_tot, want_lay) = ref.case_list()[i], ref.reference()[i]
    B = case["size"][0]
    a, b = _up(case["a"]), _up(case["b"])
    tot, lay = model.measure(a, b)
    assert tot.dtype == np.float64 and tot.shape == (5 * B,) and lay.dtype == np.float64 and lay.shape == (5 * B, 5)
    assert np.array_equal(tot, (((lay[:, 0] + lay[:, 1]) + lay[:, 2]) + lay[:, 3]) + lay[:, 4])
    err = np.abs(lay - want_lay)
    per_layer = (err[B:] / (E_REL * want_lay[B:])).max(axis=0)
    ratio = float(per_layer.max())
    print(f"size {case['size']}: worst |dev - d64| / (e_rel d64) = {ratio:.3f} (bound {FACTOR}), per layer "
          f"{', '.join(f'{r:.2f}' for r in per_layer)}; lpips {tot[B:].min():.3e} .. {tot.max():.4f}")
    assert np.all(lay[:B] == 0.0) and np.all(tot[:B] == 0.0)              # identical pairs: exactly 0.0
    assert np.all(err <= FACTOR * E_REL * want_lay)
    assert np.all(np.abs(tot - want_tot) <= FACTOR * E_REL * want_tot)
    # swapping the sides gives the same bits
    tot_s, lay_s = model.measure(b, a)
    assert np.array_equal(tot, tot_s) and np.array_equal(lay, lay_s)
    # a forced chunk of one pair, and a pair alone: the same bits as inside the batch
    model.max_pixels = 1
    try:
        tot_c, lay_c = model.measure(a, b)
    finally:
        from sgic_amd import lpips_alex
        model.max_pixels = lpips_alex.MAX_PIXELS
    assert np.array_equal(tot, tot_c) and np.array_equal(lay, lay_c)
    j = 5 * B - 2 if B > 1 else 2
    tot_1, lay_1 = model.measure(a[j:j + 1], b[j:j + 1])
    assert tot_1[0] == tot[j] and np.array_equal(lay_1[0], lay[j])


def test_chunks_follow_the_pixel_bound(model, monkeypatch):
    from sgic_amd import lpips_alex
    seen = []
    monkeypatch.setattr(model, "_chunk", lambda a, b, out: (seen.append(a.shape[0]), out.zero_()))
    z = torch.zeros(7, 32, 32, 3, dtype=torch.uint8, device=DEV)
    monkeypatch.setattr(model, "max_pixels", 2 * 32 * 32 * 3)
    model.measure(z, z)
    assert seen == [3, 3, 1]
    del seen[:]
    monkeypatch.setattr(model, "max_pixels", lpips_alex.MAX_PIXELS)
    model.measure(z, z)
    assert seen == [7] and lpips_alex.MAX_PIXELS == 1 << 21


def test_small_images_give_none(model):
    z = torch.zeros(1, 30, 40, 3, dtype=torch.uint8, device=DEV)
    assert model.measure(z, z) is None
    z = torch.zeros(1, 40, 30, 3, dtype=torch.uint8, device=DEV)
    assert model.measure(z, z) is None
