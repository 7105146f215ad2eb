"""CPU: the definition of NIQE in DESIGN.md section 19 piece by piece -- the restatement tests/niqe_ref.py against independent forms
of each step (the float luma, the cubic kernel, scipy's convolution), the host functions of sgic_amd.niqe, and the two figures the GPU
tests lean on: how far every rn lies from an alpha decision boundary, and how far the bound on the block sums moves a score."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niqe_ref as ref  # noqa: E402


def test_window_weights_are_the_fspecial_window():
    import sgic_amd  # noqa: F401
    from sgic_amd.niqe import window_weights
    w = window_weights()
    sig = 7.0 / 6.0
    h = np.array([[math.exp(-(i * i + j * j) / (2.0 * sig * sig)) for j in range(-3, 4)] for i in range(-3, 4)])
    h /= h.sum()                                            # fspecial('gaussian', 7, 7/6)
    worst = max(abs(h[3 + di, 3 + dj] - w[ref.class_of(di, dj)]) for di in range(-3, 4) for dj in range(-3, 4))
    total = sum(w[ref.class_of(di, dj)] for di in range(-3, 4) for dj in range(-3, 4))
    print(f"largest difference to the 2-D window {worst:.3e}, sum of the 49 weights - 1 = {total - 1.0:.3e}")
    assert len(w) == 10 and worst <= 1e-16 and abs(total - 1.0) <= 1e-15
    assert [ref.class_of(0, 0), ref.class_of(-1, 0), ref.class_of(1, -1), ref.class_of(3, -2), ref.class_of(3, 3)] == [0, 1, 4, 8, 9]


def test_luma_integers_against_the_float_formula():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (50000, 3), dtype=np.uint8)
    rgb[:4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    y = ref.luma(rgb)
    f = (65.481 * rgb[:, 0].astype(np.float64) + 128.553 * rgb[:, 1] + 24.966 * rgb[:, 2]) / 255.0 + 16.0
    away = np.abs(f - np.floor(f) - 0.5) > 1e-9             # away from ties the float formula rounds the same way
    assert away.sum() > 49000 and np.array_equal(y[away], np.rint(f[away]).astype(np.int64))
    assert y[0] == 16 and y[1] == 235 and y.min() >= 16 and y.max() <= 235
    # an exact tie goes to the even level: N = 255000 q + 127500
    assert ref.luma(np.array([[0, 0, 0]], dtype=np.uint8))[0] == 16


def _cubic(x):
    x = abs(x)
    if x <= 1.0:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
    if x <= 2.0:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
    return 0.0


def test_half_size_numerators_are_imresize():
    """imresize(., 0.5): output i sits at u = 2 i + 0.5 of the input and weighs input k by 0.5 cubic(0.5 (u - k)), normalised"""
    w = np.array([0.5 * _cubic(0.5 * (0.5 - (k - 3))) for k in range(8)])        # inputs 2 i - 3 .. 2 i + 4
    w = w / w.sum()
    assert np.array_equal(w * 256.0, ref.TAPS.astype(np.float64)) and ref.TAPS.sum() == 256
    rng = np.random.default_rng(8)
    y = rng.integers(16, 236, (20, 26)).astype(np.int64)

    def axis(x):            # along the last axis, floats, symmetric extension
        n = x.shape[-1]
        out = np.zeros(x.shape[:-1] + (n // 2,))
        for i in range(n // 2):
            for k in range(8):
                j = 2 * i - 3 + k
                j = -j - 1 if j < 0 else (2 * n - 1 - j if j >= n else j)
                out[..., i] += w[k] * x[..., j]
        return out

    want = axis(axis(y.astype(np.float64)).T).T                                 # dyadic weights on integers: exact in fp64
    assert np.array_equal(ref.half(y).astype(np.float64), want * 65536.0)


@pytest.mark.parametrize("name", ["200x300", "noise", "halfflat", "ramp", "checker"])
def test_mscn_against_the_convolution_form(name):
    """(x - mu) / (sigma + 1) with mu = conv(x), sigma = sqrt(|conv(x^2) - mu^2|): the usual code.  The two agree to rounding; the
    cancellation is in the other form's conv(x^2) - mu^2."""
    from scipy.ndimage import convolve
    sig = 7.0 / 6.0
    h = np.array([[math.exp(-(i * i + j * j) / (2.0 * sig * sig)) for j in range(-3, 4)] for i in range(-3, 4)])
    h /= h.sum()
    img = ref.case(name)[0][0]
    for x, p in ref.planes(img):
        got, _ = ref.mscn(x, p)
        xf = x.astype(np.float64) * 2.0 ** -p
        mu = convolve(xf, h, mode="nearest")
        sigma = np.sqrt(np.abs(convolve(xf * xf, h, mode="nearest") - mu * mu))
        worst = float(np.abs(got - (xf - mu) / (sigma + 1.0)).max())
        print(f"{name} scale {1 + (p > 0)}: largest difference to the convolution form {worst:.3e}")
        assert worst <= 1e-10


def test_flat_and_antisymmetric_neighbourhoods_give_exact_zeros():
    n, sigma = ref.mscn(np.full((40, 40), 77, dtype=np.int64), 0)
    assert not n.any() and not sigma.any()
    ramp = np.broadcast_to(3 * np.arange(40, dtype=np.int64)[None, :] * 65536, (40, 40))
    n, _ = ref.mscn(ramp, 16)
    assert not n[:, 3:-3].any() and n[:, :3].all() and n[:, -3:].all()       # only the replicated border breaks the symmetry
    img = ref.case("halfflat")[0][0]
    x = ref.planes(img)[0][0]
    n, _ = ref.mscn(x, 0)
    assert not n[:, 96 + 3:].any() and np.count_nonzero(n[:, :96]) > 9000
    stats = ref.case("flat")[1]
    assert not stats.any() and ref.case("flat")[3] == [None]


def test_aggd_of_gaussian_noise():
    import sgic_amd  # noqa: F401
    from sgic_amd.niqe import features
    blk = np.random.default_rng(2).normal(size=(96, 96))
    stats = np.zeros((2, 5, 5))
    stats[:] = 1.0                                   # the other maps: anything finite
    stats[0, 0] = ref.map_stats(blk)
    f = features(stats)
    print(f"alpha of a 96 x 96 Gaussian block: {f[0]}, scale (beta_l + beta_r) / 2: {f[1]}")
    assert abs(f[0] - 2.0) <= 0.15 and abs(f[1] - math.sqrt(2.0)) <= 0.1
    stats[0, 0, 0] = 0.0                             # no negative sample: NaN, for that map only
    f = features(stats)
    assert np.isnan(f[:2]).all() and np.isfinite(f[2:]).all()


def test_scores_of_the_case_list():
    for name in ref.CASES:
        sc = ref.case(name)[3]
        print(name, sc)
        if name in ref.NO_SCORE:
            assert sc == [None] * len(sc)
        elif name != "ramp":                         # the ramp's blocks are mostly exact zeros: whatever the definition gives
            assert all(v is not None and math.isfinite(v) and v > 0.0 for v in sc)
    b3 = ref.case("batch3")[3]
    assert len(set(b3)) == 3


def test_score_matches_the_product_host_functions():
    import sgic_amd  # noqa: F401
    from sgic_amd import niqe
    mu_p, cov_p = ref.pristine()
    for name in ("200x300", "batch3", "96x100"):
        _, stats, _, want = ref.case(name)
        feat = niqe.features(stats)
        got = [niqe.score(feat[b].reshape(-1, 36), mu_p, cov_p) for b in range(feat.shape[0])]
        assert got == want


def test_load_params(tmp_path):
    import sgic_amd  # noqa: F401
    from sgic_amd import niqe
    mu, cov = ref.pristine()
    good = tmp_path / "good.npz"
    np.savez(good, mu_pris_param=mu.reshape(1, 36), cov_pris_param=cov)          # BasicSR's file holds a (1, 36) row
    m, c = niqe.load_params(str(good))
    assert m.shape == (36,) and np.array_equal(m, mu) and np.array_equal(c, cov)
    bad_mu = mu.copy()
    bad_mu[3] = np.nan
    for k, kw in enumerate([{"mu_pris_param": mu}, {"cov_pris_param": cov}, {"mu_pris_param": mu[:35], "cov_pris_param": cov},
                            {"mu_pris_param": mu, "cov_pris_param": cov[:35]}, {"mu_pris_param": bad_mu, "cov_pris_param": cov},
                            {"mu_pris_param": mu, "cov_pris_param": np.full((36, 36), np.inf)}]):
        path = tmp_path / f"bad{k}.npz"
        np.savez(path, **kw)
        with pytest.raises(ValueError):
            niqe.load_params(str(path))
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"not an archive")
    with pytest.raises(ValueError):
        niqe.load_params(str(junk))
    from scipy.io import savemat
    mat = tmp_path / "model.mat"
    savemat(mat, {"mu_prisparam": mu.reshape(1, 36), "cov_prisparam": cov})
    m, c = niqe.load_params(str(mat))
    assert np.array_equal(m, mu) and np.array_equal(c, cov)


def test_fit_keeps_the_sharp_blocks():
    import sgic_amd  # noqa: F401
    from sgic_amd import niqe
    assert niqe.select_sharp([4.0, 3.0, 3.0001, 1.0, 2.9999]).tolist() == [True, False, True, False, False]   # strictly above 0.75 x 4
    stats, sharp = ref.blocks(ref.fit_images()[3][None])
    rows = niqe.fit_rows(stats, sharp)
    keep = sharp.reshape(-1) > 0.75 * sharp.max()
    assert 1 <= keep.sum() and rows.shape == (int(keep.sum()), 36)
    assert np.array_equal(rows, niqe.features(stats).reshape(-1, 36)[keep], equal_nan=True)
    mu, cov, tol_mu, tol_cov = ref.fit_case()
    print(f"fit of six images: tolerance on mu {tol_mu:.3e}, on cov {tol_cov:.3e}")
    assert mu.shape == (36,) and cov.shape == (36, 36) and np.isfinite(mu).all() and np.isfinite(cov).all()
    assert 0.0 < tol_mu < 1e-9 and 0.0 < tol_cov < 1e-9


def test_every_rn_is_away_from_an_alpha_boundary():
    """alpha changes where rn crosses the midpoint of two neighbouring r_gam entries.  The device's sums are within 2e-12 of the
    restatement's, which moves rn by a few times that; every rn of the case list and of the fit images is at least 1e-9 (relative)
    from the nearest midpoint, so the GPU tests may ask for equal alphas."""
    import sgic_amd  # noqa: F401
    from sgic_amd import niqe
    _, r_gam = niqe._gamma_table()
    assert bool((np.diff(r_gam) > 0).all())
    mids = (r_gam[1:] + r_gam[:-1]) / 2.0
    all_stats = [ref.case(name)[1] for name in ref.CASES] + [ref.blocks(img[None])[0] for img in ref.fit_images()]
    smallest = math.inf
    for stats in all_stats:
        flat = stats.reshape(-1, 2, 5, 5)
        for s in range(2):
            rn = niqe.aggd_rn(flat[:, s], float((96 >> s) ** 2))[2].reshape(-1)
            rn = rn[np.isfinite(rn)]
            if rn.size:
                k = np.clip(np.searchsorted(mids, rn), 1, mids.size - 1)
                dist = np.minimum(np.abs(rn - mids[k - 1]), np.abs(rn - mids[k])) / rn
                smallest = min(smallest, float(dist.min()))
    print(f"smallest relative distance of an rn from an alpha boundary: {smallest:.3e}")
    assert smallest > 1e-9


def test_score_tolerance():
    change = ref.score_change()
    print(f"largest change of a score when every block sum moves by +-{ref.REL}: {change:.3e}; "
          f"the GPU tests hold scores to {ref.score_tolerance():.3e}")
    assert 0.0 < change < 1e-9 and ref.score_tolerance() == 10.0 * change
