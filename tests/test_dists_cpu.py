"""CPU: the DISTS weight loader, the properties of the definition on its restatement (tests/dists_ref.py), and the fp32 error of the
restatement per tap-term, which sets the tolerance of the GPU test (tests/test_gpu_dists.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dists_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def D():
    import __graft_entry__ as g
    g.build()
    import sgic_amd  # noqa: F401
    from sgic_amd import dists
    return dists


def _same(x, y):
    assert list(x) == list(y)
    for k in x:
        assert x[k].dtype == torch.float32 and torch.equal(x[k], y[k]), k


def test_synth_weights_recipe(D):
    sd = D.synth_weights(ref.SEED)
    _same(sd, ref.synth_state(ref.SEED))
    assert {k: tuple(v.shape) for k, v in sd.items()} == D.expected_shapes()
    assert D.N_CH == ref.N_CH == sum(D.TAP_CH) == 1475 and D.TAP_CH == ref.TAP_CH
    for k in ("alpha", "beta"):
        assert 0.0 < float(sd[k].min()) and float(sd[k].max()) <= 0.2
    assert not torch.equal(sd["alpha"], sd["beta"])


@pytest.mark.parametrize("style", ["torchvision", "dists_pytorch", "piq"])
def test_loader_key_spellings(D, tmp_path, style):
    sd = D.synth_weights(7, path=tmp_path / "w.pt", style=style)
    raw = torch.load(tmp_path / "w.pt", weights_only=True)
    first = {"torchvision": ("features.0.weight", "features.28.bias"), "dists_pytorch": ("stage1.0.weight", "stage5.28.bias"),
             "piq": ("model.0.weight", "model.28.bias")}[style]
    assert all(k in raw for k in first) and len(raw) == 28
    if style == "dists_pytorch":
        assert "stage2.5.weight" in raw and "stage3.14.bias" in raw and "stage4.17.weight" in raw
    assert tuple(raw["alpha"].shape) == ((1475,) if style == "torchvision" else (1, 1475, 1, 1))
    _same(D.load_weights(tmp_path / "w.pt"), sd)
    _same(D.load_weights([str(tmp_path / "w.pt")]), sd)


def test_loader_merges_files_and_ignores_foreign_keys(D, tmp_path):
    sd = D.synth_weights(7)
    other = D.synth_weights(8)
    trunk = {k: v for k, v in sd.items() if k.startswith("features")}
    trunk["classifier.0.weight"] = torch.zeros(4, 4)                       # torchvision's vgg16 carries a classifier
    heads = {"alpha": sd["alpha"].reshape(1, -1, 1, 1), "beta": sd["beta"], "mean": torch.zeros(1, 3, 1, 1), "std": torch.ones(1, 3, 1, 1),
             "stage2.4.filter": torch.zeros(64, 1, 3, 3)}                  # DISTS_pytorch's buffers
    torch.save(trunk, tmp_path / "trunk.pt")
    torch.save({"state_dict": heads}, tmp_path / "heads.pt")
    _same(D.load_weights([tmp_path / "trunk.pt", tmp_path / "heads.pt"]), sd)
    _same(D.load_weights(sd), sd)
    # later files win
    got = D.load_weights([sd, {"alpha": other["alpha"], "model.12.bias": other["features.12.bias"]}])
    assert torch.equal(got["alpha"], other["alpha"]) and torch.equal(got["features.12.bias"], other["features.12.bias"])
    assert torch.equal(got["beta"], sd["beta"]) and torch.equal(got["features.12.weight"], sd["features.12.weight"])


def test_loader_names_missing_and_misshaped_keys(D, tmp_path):
    sd = D.synth_weights(7)
    part = {k: v for k, v in sd.items() if k not in ("features.17.bias", "beta")}
    torch.save(part, tmp_path / "part.pt")
    with pytest.raises(KeyError) as e:
        D.load_weights(tmp_path / "part.pt")
    assert "features.17.bias" in str(e.value) and "beta" in str(e.value) and "features.19" not in str(e.value) and "alpha" not in str(e.value)
    bad = D.to_style(sd, "dists_pytorch")
    bad["stage3.12.weight"] = torch.zeros(256, 128, 3, 3)
    with pytest.raises(ValueError) as e:
        D.load_weights(bad)
    assert "stage3.12.weight" in str(e.value) and "(256, 128, 3, 3)" in str(e.value) and "(256, 256, 3, 3)" in str(e.value)
    for shape in ((1, 1475), (1474,), (1, 1475, 1, 2)):
        bad = dict(sd)
        bad["alpha"] = torch.zeros(shape)
        with pytest.raises(ValueError) as e:
            D.load_weights(bad)
        assert "alpha" in str(e.value) and "(1475,)" in str(e.value) and "(1, 1475, 1, 1)" in str(e.value)


def test_layer_tables_agree(D):
    from sgic_amd import lpips
    assert lpips.CONV_IDX == ref.CONV_IDX
    assert tuple(lpips.CONV_IDX[j] for j in lpips.TAP_AFTER) == ref.TAP_AFTER
    assert tuple(lpips.CONV_IDX[j + 1] for j in lpips.POOL_AFTER) == ref.POOL_BEFORE
    assert (3,) + tuple(c[1] for j, c in enumerate(lpips.CONV_CH) if j in lpips.TAP_AFTER) == D.TAP_CH
    assert (D.C1, D.C2) == (ref.C1, ref.C2) == (1e-6, 1e-6)


def test_tap0_from_integers(D):
    """the host half of tap 0: integer sums -> the terms of x = u / 255, against the restatement's fp64 head; a flat pair has
    variance exactly 0"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    a[1], b[1] = 17, 200
    b[2] = a[2]
    ai, bi = a.astype(np.int64).reshape(3, -1, 3), b.astype(np.int64).reshape(3, -1, 3)
    m = np.stack([ai.sum(1), bi.sum(1), (ai * ai).sum(1), (bi * bi).sum(1), (ai * bi).sum(1)], axis=2)      # (B, 3, 5)
    al, be = [0.11, 0.02, 0.19], [0.07, 0.2, 0.01]
    got = D.tap0_terms(m, 99, al, be)
    xa, _ = ref.input_layer(a, torch.float64)
    xb, _ = ref.input_layer(b, torch.float64)
    want = ref.head(xa, xb, torch.tensor(al, dtype=torch.float64), torch.tensor(be, dtype=torch.float64)).numpy()
    print(f"tap 0 from integers against the fp64 head: {np.abs(got - want).max(axis=1)}")
    assert np.abs(got - want)[[0, 2]].max() <= 1e-12
    assert got[2, 0] == 0.0 and got[2, 1] == 0.0
    # flat 17 against flat 200: S2 = c2 / c2 = 1 exactly, the structure term is what the two means give.  The fp64 head is the one that
    # errs here: its E[x^2] - E[x]^2 leaves about 1e-17 next to c2, 1e-10 in the texture sum (1e-12 is asked after the division by W)
    assert np.abs(got - want)[1].max() <= 1e-9
    mx, my = 17 / 255, 200 / 255
    assert got[1, 1] == 0.0 and abs(got[1, 0] - sum(al) * (1.0 - (2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6))) <= 1e-15


def test_l2pool_keeps_an_odd_last_row_and_column():
    f = torch.rand(1, 2, 5, 7, dtype=torch.float64)
    p = ref.l2pool(f)
    assert tuple(p.shape) == (1, 2, 3, 4)
    # the corner output sees four input cells: weights 4, 2, 2, 1 over 16
    want = torch.sqrt((4 * f[0, 0, 0, 0] ** 2 + 2 * f[0, 0, 0, 1] ** 2 + 2 * f[0, 0, 1, 0] ** 2 + f[0, 0, 1, 1] ** 2) / 16 + 1e-12)
    assert abs(float(p[0, 0, 0, 0] - want)) <= 1e-15
    assert abs(float(ref.l2pool(torch.ones(1, 1, 8, 8, dtype=torch.float64))[0, 0, 2, 2]) - 1.0) <= 1e-12      # the window sums to 1
    assert float(ref.l2pool(torch.zeros(1, 1, 1, 1, dtype=torch.float64))) == 1e-6


def test_properties_of_the_definition():
    sd = ref.synth_state()
    case = ref.case_list()[1]
    B = case["size"][0]
    a, b = case["a"], case["b"]
    for dtype in (torch.float32, torch.float64):
        tot, terms = ref.dists(a, b, sd, dtype)
        assert terms.shape == (5 * B, 6, 2) and np.all(np.isfinite(terms))
        assert np.all(tot[:B] == 0.0) and np.all(terms[:B] == 0.0)           # identical images: exactly 0
        assert np.all(tot[B:] > 0.0)
        tot_s, terms_s = ref.dists(b, a, sd, dtype)
        assert np.array_equal(tot, tot_s) and np.array_equal(terms, terms_s)   # S1 and S2 are symmetric
    # the ordering of the pair kinds, per image: identical < noise 5 < noise 40 < independent, and flat 17 against flat 200 far off
    k = tot.reshape(5, B)
    print("dists per kind:", {name: k[i].tolist() for i, name in enumerate(ref.KINDS)})
    assert np.all(k[0] < k[1]) and np.all(k[1] < k[2]) and np.all(k[2] < k[3]) and np.all(k[4] > k[2])
    assert np.all(k <= 1.0)


def test_fp32_error_of_the_restatement():
    """e_abs = max over all cases and the terms of taps 1..5 of |t32 - t64|: the yardstick of the device's tolerance.  Tap 0 is left
    out: fp32 loses a flat image's zero variance next to c2 = 1e-6 (printed), which is why the device takes tap 0 from integers."""
    sd = ref.synth_state()
    e_abs, e_tap0 = 0.0, 0.0
    for case, (tot64, terms64) in zip(ref.case_list(), ref.reference()):
        B = case["size"][0]
        tot32, terms32 = ref.dists(case["a"], case["b"], sd, torch.float32)
        assert np.all(terms32[:B] == 0.0) and np.all(terms64[:B] == 0.0)
        d = np.abs(terms32 - terms64)
        print(f"size {case['size']}: e_abs per tap 1..5 {[f'{v:.2e}' for v in d[:, 1:].max(axis=(0, 2))]}, tap 0 {d[:, 0].max():.2e}, "
              f"total {np.abs(tot32 - tot64).max():.2e}; dists {tot64[B:].min():.3e} .. {tot64.max():.4f}")
        e_abs = max(e_abs, float(d[:, 1:].max()))
        e_tap0 = max(e_tap0, float(d[:, 0].max()))
    print(f"e_abs = {e_abs:.3e} (tap 0 in fp32: {e_tap0:.3e})")
    assert e_abs < 1e-6
