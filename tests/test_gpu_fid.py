"""GPU: fid.InceptionFID.features against the fp64 restatement (tests/fid_ref.py), its invariance under chunking, batching and
descriptors, and FID / KID from the device's own features against numpy on the same features.

Tolerance of the features: per image, |dev - f64|_2 / |f64|_2 <= 8 * e_rel, e_rel being the same distance between the
restatement's own fp32 and fp64 runs on that image, measured here (torch CPU, synth_weights(1234): 1.5e-07, 1.6e-07, 1.7e-07).  The
factor 8 is that of tests/test_gpu_lpips.py: the split GEMMs add their K products (here K <= 4032) in another order than the
reference.  Measured on an MI355X: 1.16e-06, 1.08e-06, 1.10e-06, ratios 7.8, 6.6, 6.5: inside the factor, but
using most of it.  Layer by layer no convolution's output is past 2.7 times the reference's fp32 error; the margin goes in the
final mean over 64 positions, where the reference's error averages out by 5.5 and the device's by 1.8."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234
FACTOR = 8.0


@pytest.fixture(scope="module")
def fid():
    import sgic_amd  # noqa: F401
    from sgic_amd import fid as m
    return m


@pytest.fixture(scope="module")
def model(fid):
    """the launch modes are bitwise equivalent (ops.py), so the tests do not spend their seconds racing them"""
    from sgic_amd import ops
    old, ops.AUTOTUNE = ops.AUTOTUNE, False
    yield fid.InceptionFID(fid.synth_weights(SEED), DEV)
    ops.AUTOTUNE = old


@pytest.fixture(scope="module")
def reference(fid):
    """(f32 (3, 2048), f64 (3, 2048)) of the restatement on fid_ref.ref_images(), computed once"""
    sd = fid.synth_weights(SEED)
    imgs = fid_ref.ref_images()[3]
    return tuple(torch.stack([fid_ref.Ref(sd, dt).features(im).double() for im in imgs]).numpy() for dt in (torch.float32, torch.float64))


@pytest.fixture(scope="module")
def device_features(model):
    big, small, desc, _ = fid_ref.ref_images()
    a = model.features(torch.from_numpy(big).to(DEV))
    b = model.features(torch.from_numpy(small).to(DEV), desc)
    return torch.cat([a, b]).cpu()


def test_features_against_the_fp64_restatement(device_features, reference):
    f32, f64 = reference
    got = device_features.double().numpy()
    assert got.shape == (3, 2048) and np.isfinite(got).all()
    for i in range(3):
        e_rel = np.linalg.norm(f32[i] - f64[i]) / np.linalg.norm(f64[i])
        dev = np.linalg.norm(got[i] - f64[i]) / np.linalg.norm(f64[i])
        print(f"image {i}: e_rel {e_rel:.3e}, device {dev:.3e}, ratio {dev / e_rel:.2f}")
    for i in range(3):
        e_rel = np.linalg.norm(f32[i] - f64[i]) / np.linalg.norm(f64[i])
        assert 0 < e_rel < 1e-5
        assert np.linalg.norm(got[i] - f64[i]) <= FACTOR * e_rel * np.linalg.norm(f64[i])


def test_chunking_batching_and_descriptors_give_identical_bits(model, device_features):
    big, small, desc, imgs = fid_ref.ref_images()
    old = model.max_operand_bytes
    try:
        model.max_operand_bytes = 1                                   # chunks of one window
        one = model.features(torch.from_numpy(small).to(DEV), desc).cpu()
    finally:
        model.max_operand_bytes = old
    assert torch.equal(one, device_features[1:])
    # every window as a canvas of its own, whole-image descriptors by default
    for i, im in enumerate(imgs):
        alone = model.features(torch.from_numpy(np.ascontiguousarray(im)[None]).to(DEV)).cpu()
        assert torch.equal(alone[0], device_features[i]), i
    # the windows in another order and slot of a larger batch
    two = np.concatenate([small, small[:, ::-1].copy()])
    d = np.array([(1, 0, 0, 64, 80), (0, 11, 27, 40, 53), (1, 3, 3, 20, 20), (0, 0, 0, 64, 64)], dtype=np.int32)
    mixed = model.features(torch.from_numpy(two).to(DEV), d).cpu()
    assert torch.equal(mixed[1], device_features[2]) and torch.equal(mixed[3], device_features[1])


@pytest.fixture(scope="module")
def two_sets(model):
    """X, Y (24, 2048) on the device: windows of 24 images and of their perturbed versions"""
    rng = np.random.default_rng(29)
    yy, xx = np.mgrid[0:64, 0:80]
    base = np.stack([np.stack([128 + 100 * np.sin(xx / (3.0 + i % 5) + c) * np.cos(yy / (2.5 + i % 7)) for c in range(3)], -1)
                     for i in range(24)]) + rng.normal(0, 10, (24, 64, 80, 3))
    a = np.clip(base, 0, 255).astype(np.uint8)
    b = np.clip(base * 0.9 + rng.normal(0, 25, base.shape), 0, 255).astype(np.uint8)
    desc = np.array([(i, (5 * i) % 24, (7 * i) % 40, 40, 40) for i in range(24)], dtype=np.int32)
    return model.features(torch.from_numpy(a).to(DEV), desc), model.features(torch.from_numpy(b).to(DEV), desc)


def test_fid_and_kid_from_device_features_against_numpy(fid, two_sets):
    """The device's Gram sums differ from numpy's by at most K 2^-52 sum |a||b| per element (tests/test_gpu_fid_kernels.py).
    KID: K = d = 2048, the cube triples the relative error and the estimate is a signed sum of three means of positive kernel
    values, so |dev - numpy| <= 4 * 3 * 2048 * 2^-52 * (mean K_XX + mean K_YY + 2 mean K_XY) (5.5e-12 of that scale).
    FID: K = n = 24, so a second moment moves by at most 24 * 2^-52 = 5e-15 of sum |x_i||x_j|; the same host code then turns both
    sets of moments into the number, and the eigenvalues that fid_from_stats keeps amplify that perturbation by far less than the
    four orders of magnitude left to the bound the issue states: 1e-10 of tr cov_x + tr cov_y + |mu_x - mu_y|^2.  Moments summed in
    fp32 (6e-8) or a gathered row off by one would miss it.  Both figures are printed."""
    X, Y = two_sets
    Xn, Yn = X.cpu().numpy(), Y.cpu().numpy()
    n, d = Xn.shape
    assert (n, d) == (24, 2048) and np.isfinite(Xn).all() and np.isfinite(Yn).all() and not np.array_equal(Xn, Yn)
    got = fid.fid(X, Y)
    _, mx, cx = fid.moments(Xn)
    _, my, cy = fid.moments(Yn)
    want = fid.fid_from_stats(mx, cx, my, cy)
    scale = np.trace(cx) + np.trace(cy) + float((mx - my) @ (mx - my))
    print(f"fid device {got!r} numpy {want!r} relative to the scale {abs(got - want) / scale:.3e}")
    assert want > 0 and abs(got - want) <= 1e-10 * scale
    k, k_std = fid.kid(X, Y, subsets=10, subset_size=16, seed=0)
    idx = fid.kid_indices(n, n, 10, 16, 0)
    wk, wk_std = fid_ref.kid_numpy(Xn, Yn, idx)
    x64, y64 = Xn.astype(np.float64), Yn.astype(np.float64)
    kscale = sum(w * float(((a @ b.T / d + 1) ** 3).mean()) for w, a, b in ((1, x64, x64), (1, y64, y64), (2, x64, y64)))
    print(f"kid device {k!r} numpy {wk!r} std {k_std!r} {wk_std!r} relative to the scale {abs(k - wk) / kscale:.3e}")
    assert abs(k - wk) <= 12 * d * 2.0 ** -52 * kscale and abs(k_std - wk_std) <= 12 * d * 2.0 ** -52 * kscale


def test_fid_of_a_set_with_itself_is_zero(fid, two_sets):
    X, _ = two_sets
    _, _, cov = fid.moments(X)
    assert abs(fid.fid(X, X.clone())) <= 1e-9 * np.trace(cov)


def test_feature_stats_accumulates_on_the_device(fid, two_sets):
    X, Y = two_sets
    st = fid.FeatureStats()
    st.add(X[:10])
    st.add(X[10:])
    assert st.n == 24 and st.features().is_cuda and torch.equal(st.features(), X)
    n, mu, cov = st.moments()
    n2, mu2, cov2 = fid.moments(X)
    assert n == n2 == 24 and np.array_equal(mu, mu2) and np.array_equal(cov, cov2)
