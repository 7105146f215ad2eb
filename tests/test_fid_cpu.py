"""CPU: the host side of FID / KID (sgic_amd/fid.py) and the reference of the GPU tests (tests/fid_ref.py); DESIGN.md section 17."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref  # noqa: E402


@pytest.fixture(scope="module")
def fid():
    import sgic_amd  # noqa: F401
    from sgic_amd import fid as m
    return m


@pytest.fixture(scope="module")
def sd(fid):
    return fid.synth_weights(1234)


def test_load_weights_round_trip(fid, sd, tmp_path):
    p = str(tmp_path / "inception.pth")
    fid.synth_weights(1234, path=p)
    got = fid.load_weights(p)
    assert list(got) == list(fid.expected_shapes()) and len(got) == 94 * 5
    assert all(torch.equal(got[k], sd[k]) for k in got)
    # nesting is unwrapped; fc.*, AuxLogits.*, num_batches_tracked and foreign keys are ignored, whatever their shape
    extra = dict(sd)
    extra.update({"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(3), "AuxLogits.conv0.conv.weight": torch.zeros(1),
                  "Conv2d_1a_3x3.bn.num_batches_tracked": torch.tensor(7), "something.else": torch.zeros(2)})
    got = fid.load_weights({"state_dict": extra})
    assert list(got) == list(fid.expected_shapes()) and all(torch.equal(got[k], sd[k]) for k in got)
    # two files that together hold everything
    keys = list(sd)
    got = fid.load_weights([{k: sd[k] for k in keys[:100]}, {k: sd[k] for k in keys[100:]}])
    assert all(torch.equal(got[k], sd[k]) for k in got)


def test_load_weights_names_a_missing_key_and_refuses_a_wrong_shape(fid, sd):
    part = {k: v for k, v in sd.items() if k != "Mixed_6c.branch7x7dbl_3.bn.running_var"}
    with pytest.raises(KeyError, match="Mixed_6c.branch7x7dbl_3.bn.running_var"):
        fid.load_weights(part)
    bad = dict(sd)
    bad["Mixed_7c.branch3x3_2b.conv.weight"] = torch.zeros(384, 384, 1, 3)       # the 3x1 kernel transposed
    with pytest.raises(ValueError, match="Mixed_7c.branch3x3_2b.conv.weight"):
        fid.load_weights(bad)


def test_architecture_tables(fid):
    specs = fid.conv_specs()
    assert len(specs) == 94
    assert specs["Mixed_6c.branch7x7dbl_3"] == (160, 160, 1, 7, 1, 0, 3) and specs["Mixed_7a.branch7x7x3_4"] == (192, 192, 3, 3, 2, 0, 0)
    assert [fid.block_out_channels(k, c, p) for _, k, c, p in fid.BLOCKS] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    assert max(kh * kw * cin for cin, _, kh, kw, _, _, _ in specs.values()) == 4032       # the largest K of a GEMM


def test_reference_extents_and_channels(sd):
    shapes = []
    f = fid_ref.Ref(sd, torch.float32).features(fid_ref.ref_images()[3][1], shapes)
    assert f.shape == (2048,)
    assert [s[0] for s in shapes[:7]] == [149, 147, 147, 73, 73, 71, 35]
    assert [s[0] for s in shapes[7:]] == [35, 35, 35, 17, 17, 17, 17, 17, 8, 8, 8]
    assert [s[1] for s in shapes[7:]] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]


def test_reference_conditioning(sd):
    """the synthetic weights must leave a usable signal at pool3: on the fp64 reference, for the GPU test's images, at least half of
    the 2048 features are non-zero and none is above 1e4"""
    r = fid_ref.Ref(sd, torch.float64)
    for im in fid_ref.ref_images()[3]:
        f = r.features(im)
        assert int((f > 0).sum()) >= 1024 and float(f.max()) <= 1e4 and bool(torch.isfinite(f).all())


def test_reference_input_rule():
    """Ties the two references of the GPU tests together (it needs no product code, so it does not show the feature):
    F.interpolate in the reference is the rule section 17 writes out: src = max((dst + 0.5) in / 299 - 0.5, 0), floor, neighbour
    clamped, within rows, then between rows; 2 x - 1 also at 299"""
    rng = np.random.default_rng(3)
    for h, w in ((31, 47), (299, 299), (600, 400)):
        u = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = fid_ref.Ref({}, torch.float64).input(u)[0].permute(1, 2, 0).numpy()
        assert np.abs(got - fid_ref.resize_f64(u)).max() <= 1e-12


def test_patch_grid(fid):
    assert fid.patch_grid(256, 256, 256) == [(0, 0, 256, 256)]
    g = fid.patch_grid(512, 768, 256)
    assert len(g) == 6 + 2 and g[:6] == [(y, x, 256, 256) for y in (0, 256) for x in (0, 256, 512)]
    assert g[6:] == [(128, 128, 256, 256), (128, 384, 256, 256)]
    assert fid.patch_grid(255, 400, 256) == [] and fid.patch_grid(400, 255, 256) == []
    assert fid.patch_grid(255, 400, 0) == [(0, 0, 255, 400)]
    d = fid.descriptors(2, 512, 768, 256)
    assert d.shape == (16, 5) and d.dtype == np.int32 and d[8].tolist() == [1, 0, 0, 256, 256]
    assert all(0 <= y and y + h <= 512 and 0 <= x and x + w <= 768 for _, y, x, h, w in d.tolist())


def _cov(rng, d, cond=1e3):
    """a random full-rank covariance of condition number <= cond"""
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    lam = np.exp(rng.uniform(0, np.log(cond), d))
    return (q * lam) @ q.T


@pytest.mark.parametrize("d", [48, 64])
def test_fid_from_stats_against_sqrtm(fid, d):
    """against pytorch-fid's form tr sqrtm(cov_x cov_y), within 1e-9 relative (fp64 eigen-solvers, condition <= 1e3); scipy's two
    forms, sqrtm(cov_x cov_y) and sqrtm(cov_y cov_x), bound what the comparison can resolve and are asserted to agree as well"""
    from scipy import linalg
    rng = np.random.default_rng(d)
    cx, cy = _cov(rng, d), _cov(rng, d)
    mx, my = rng.normal(size=d), rng.normal(size=d)
    diff = mx - my
    forms = [float(diff @ diff + np.trace(cx) + np.trace(cy) - 2 * np.trace(linalg.sqrtm(a @ b)).real) for a, b in ((cx, cy), (cy, cx))]
    got = fid.fid_from_stats(mx, cx, my, cy)
    spread = abs(forms[0] - forms[1]) / abs(forms[0])
    print(f"d={d}: fid {got!r}, sqrtm forms {forms!r}, their relative gap {spread:.3e}, ours to the first {abs(got - forms[0]) / abs(forms[0]):.3e}")
    assert spread <= 1e-9
    assert abs(got - forms[0]) <= 1e-9 * abs(forms[0])


def test_fid_identical_and_rank_deficient(fid):
    rng = np.random.default_rng(9)
    X = rng.normal(size=(500, 48)).astype(np.float32)
    n, mu, cov = fid.moments(X)
    assert n == 500 and np.allclose(mu, X.astype(np.float64).mean(0), rtol=0, atol=1e-12)
    assert np.allclose(cov, np.cov(X.astype(np.float64), rowvar=False, ddof=1), rtol=0, atol=1e-12)
    assert abs(fid.fid_from_stats(mu, cov, mu, cov)) <= 1e-9 * np.trace(cov)
    assert abs(fid.fid(X, X)) <= 1e-9 * np.trace(cov)
    A, B = X[:20], (X[20:40] * 1.5 + 0.3).astype(np.float32)           # n = 20 < d = 48: covariances of rank 19
    v = fid.fid(A, B)
    assert np.isfinite(v) and v >= 0
    assert abs(fid.fid(A, A)) <= 1e-9 * np.trace(fid.moments(A)[2])
    with pytest.raises(ValueError):
        fid.moments(X[:1])


def test_kid_against_numpy(fid):
    rng = np.random.default_rng(4)
    X = np.abs(rng.normal(size=(60, 96))).astype(np.float32)
    Y = np.abs(rng.normal(0.2, 1.1, size=(45, 96))).astype(np.float32)
    idx = fid.kid_indices(60, 45, subsets=7, subset_size=30, seed=5)
    assert len(idx) == 7 and all(len(ix) == 30 and len(set(ix.tolist())) == 30 and ix.max() < 60 and iy.max() < 45 for ix, iy in idx)
    rng2 = np.random.default_rng(5)                   # the draws: X's rows, then Y's, subset after subset, from default_rng(seed)
    assert np.array_equal(idx[0][0], rng2.choice(60, 30, replace=False)) and np.array_equal(idx[0][1], rng2.choice(45, 30, replace=False))
    got, want = fid.kid(X, Y, subsets=7, subset_size=30, seed=5), fid_ref.kid_numpy(X, Y, idx)
    assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]) and abs(got[1] - want[1]) <= 1e-12 * abs(want[1])
    # subset size min(1000, n, m) and seed 0 by default
    got = fid.kid(X, Y, subsets=3)
    want = fid_ref.kid_numpy(X, Y, fid.kid_indices(60, 45, 3, 1000, 0))
    assert len(fid.kid_indices(60, 45, 3)[0][0]) == 45 and abs(got[0] - want[0]) <= 1e-12 * abs(want[0])
    assert fid.kid(X[:1], Y) == (None, None)


def test_kid_identical_sets_with_identical_indices(fid, monkeypatch):
    """Identical sets with identical indices: the three kernel matrices of a subset are one matrix K, bit for bit, so the estimate is
    exactly 2 (sum K - tr K) / (s (s-1)) - 2 sum K / s^2.  That is not 0: the within-set terms leave the diagonal out and the cross
    term keeps it (for s = 2 it is K_ab - (K_aa + K_bb) / 2 <= 0), which is what makes the estimate unbiased for independent sets.
    Only sets of equal vectors give exactly 0, and the biased form (diagonals kept) would."""
    rng = np.random.default_rng(6)
    X = np.abs(rng.normal(size=(40, 64))).astype(np.float32)
    same = [(ix, ix) for ix, _ in fid.kid_indices(40, 40, 5, 25, 0)]
    monkeypatch.setattr(fid, "kid_indices", lambda *a, **k: same)
    est = []
    for ix, _ in same:
        K = (X[ix].astype(np.float64) @ X[ix].astype(np.float64).T / 64 + 1.0) ** 3
        w = (K.sum() - np.trace(K)) / (25 * 24)
        est.append(w + w - 2.0 * K.sum() / (25 * 25))
    assert fid.kid(X, X.copy(), subsets=5, subset_size=25) == (float(np.mean(est)), float(np.std(est)))
    assert all(e <= 0 for e in est)
    const = np.tile(X[:1], (40, 1))                   # equal vectors: every kernel value is the same number c, c + c - 2 c
    k, k_std = fid.kid(const, const.copy(), subsets=5, subset_size=25)
    c = float((const[0].astype(np.float64) @ const[0].astype(np.float64) / 64 + 1) ** 3)
    assert abs(k) <= 1e-13 * c and k_std <= 1e-13 * c      # the sums of 625 and 600 copies of c round a few times
