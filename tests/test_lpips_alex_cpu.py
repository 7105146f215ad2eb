"""CPU: the LPIPS-Alex weight loader, the properties of the definition on its restatement (tests/lpips_alex_ref.py), the conditioning
of the shared case list, and the fp32 error of the restatement, which sets the tolerance of the GPU test
(tests/test_gpu_lpips_alex.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_alex_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    import sgic_amd  # noqa: F401
    from sgic_amd import lpips_alex
    return lpips_alex


def _same(x, y):
    assert list(x) == list(y)
    for k in x:
        assert x[k].dtype == torch.float32 and torch.equal(x[k], y[k]), k


def test_synth_weights_recipe(L):
    sd = L.synth_weights(ref.SEED)
    _same(sd, ref.synth_state(ref.SEED))
    assert {k: tuple(v.shape) for k, v in sd.items()} == L.expected_shapes()
    assert sd["features.0.weight"].shape == (64, 3, 11, 11) and sd["features.3.weight"].shape == (192, 64, 5, 5)
    for k, v in sd.items():
        if k.endswith("bias"):
            assert 0.0 <= float(v.min()) and float(v.max()) <= 0.05
        elif k.startswith("lin"):
            assert 0.0 <= float(v.min()) and float(v.max()) <= 2.0 / v.numel()
    for key, fan in (("features.3.weight", 25 * 64), ("features.8.weight", 9 * 384)):
        assert abs(float(sd[key].std()) / (2.0 / fan) ** 0.5 - 1.0) < 0.01       # >= 307k samples: the sample std is within 0.4 %


def test_loader_key_spellings_and_split(L, tmp_path):
    sd = L.synth_weights(7, path=tmp_path / "tv.pt")
    L.synth_weights(7, path=tmp_path / "ref.pt", style="reference")
    raw = torch.load(tmp_path / "ref.pt", weights_only=True)
    assert sorted(k for k in raw if k.startswith("net.")) == sorted(
        f"net.slice{s}.{i}.{p}" for s, i in ((1, 0), (2, 3), (3, 6), (4, 8), (5, 10)) for p in ("weight", "bias"))
    assert "lin4.model.1.weight" in raw
    _same(L.load_weights(tmp_path / "tv.pt"), sd)
    _same(L.load_weights([str(tmp_path / "ref.pt")]), sd)
    # the trunk from a torchvision file, the lin layers from a file without the dropout slot, plus keys that are not LPIPS's
    trunk = {k: v for k, v in sd.items() if k.startswith("features")}
    trunk["classifier.1.weight"] = torch.zeros(4, 4)
    lins = {k.replace("model.1", "model.0"): v for k, v in sd.items() if k.startswith("lin")}
    lins["scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)
    torch.save(trunk, tmp_path / "trunk.pt")
    torch.save({"state_dict": lins}, tmp_path / "lins.pt")
    _same(L.load_weights([tmp_path / "trunk.pt", tmp_path / "lins.pt"]), sd)
    _same(L.load_weights(sd), sd)


def test_loader_names_missing_and_misshaped_keys(L, tmp_path):
    sd = L.synth_weights(7)
    part = {k: v for k, v in sd.items() if k not in ("features.8.bias", "lin3.model.1.weight")}
    torch.save(part, tmp_path / "part.pt")
    with pytest.raises(KeyError) as e:
        L.load_weights(tmp_path / "part.pt")
    assert "features.8.bias" in str(e.value) and "lin3.model.1.weight" in str(e.value) and "features.10" not in str(e.value)
    bad = dict(L.to_reference_keys(sd))
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError) as e:
        L.load_weights(bad)
    assert "net.slice2.3.weight" in str(e.value) and "(192, 64, 3, 3)" in str(e.value) and "(192, 64, 5, 5)" in str(e.value)


def test_layer_tables_agree(L):
    assert L.CONV_IDX == tuple(c[0] for c in ref.CONV)
    assert L.CONV_CFG == tuple(c[1:] for c in ref.CONV)
    assert tuple(L.CONV_IDX[j] for j in L.POOL_BEFORE) == ref.POOL_BEFORE
    assert L.TAP_CH == ref.TAP_CH == tuple(c[2] for c in ref.CONV)
    for n in (31, 35, 67, 64, 48, 95, 130, 256):
        assert L.extents(n) == ref.extents(n)
    assert L.extents(L.MIN_SIDE) == (7, 3, 1) and L.extents(L.MIN_SIDE - 1)[2] == 0


def test_properties_of_the_definition():
    sd = ref.synth_state()
    case = ref.case_list()[1]
    B = case["size"][0]
    a, b = case["a"], case["b"]
    for dtype in (torch.float32, torch.float64):
        tot, lay = ref.lpips(a, b, sd, dtype)
        assert np.all(tot[:B] == 0.0) and np.all(lay[:B] == 0.0)             # identical images: exactly 0
        assert np.all(lay[B:] > 0.0) and np.all(np.isfinite(lay))
        tot_s, lay_s = ref.lpips(b, a, sd, dtype)
        assert np.array_equal(tot, tot_s) and np.array_equal(lay, lay_s)     # (u_a - u_b)^2 is symmetric
    with torch.no_grad():
        shapes = [tuple(f.shape[1:]) for f in ref.taps(a, sd, torch.float32)]
    (h1, h2, h3), (w1, w2, w3) = ref.extents(35), ref.extents(67)
    assert shapes == [(64, h1, w1), (192, h2, w2), (384, h3, w3), (256, h3, w3), (256, h3, w3)]


def test_case_list_shapes_reach_every_path():
    for case, (B, H, W) in zip(ref.case_list(), ref.SIZES):
        assert case["a"].shape == (5 * B, H, W, 3) and case["a"].dtype == np.uint8 and case["b"].shape == case["a"].shape
        assert np.array_equal(case["a"][:B], case["b"][:B]) and int(np.abs(case["a"][B:2 * B].astype(int) - case["b"][B:2 * B]).max()) <= 5
        assert int(np.abs(case["a"][2 * B:3 * B].astype(int) - case["b"][2 * B:3 * B]).max()) > 5
        assert np.all(case["a"][4 * B:] == 17) and np.all(case["b"][4 * B:] == 200)
    assert ref.extents(ref.SIZES[0][1]) == (7, 3, 1) and ref.extents(ref.SIZES[0][2]) == (7, 3, 1)      # a 1x1 deepest tap
    ext = [ref.extents(n) for s in ref.SIZES for n in s[1:]]
    assert any(n1 == 8 and n2 == 3 for n1, n2, _ in ext)                          # 8 -> 3: the first pool drops a column
    assert any((n - 7) % 4 for s in ref.SIZES for n in s[1:])                     # the stride-4 layer cuts unevenly
    assert any(s[1] != s[2] for s in ref.SIZES) and any(s[0] > 1 for s in ref.SIZES)


def test_case_list_is_well_conditioned():
    """a condition on the inputs, on the fp64 restatement alone: at every tap the smallest channel norm over the pixels is at least
    0.05 of the median, so no pixel's unit vector amplifies the rounding of its features"""
    sd = ref.synth_state()
    worst = np.inf
    for case in ref.case_list():
        for side in ("a", "b"):
            with torch.no_grad():
                for f in ref.taps(case[side], sd, torch.float64):
                    n = torch.sqrt((f * f).sum(dim=1)).reshape(f.shape[0], -1)
                    worst = min(worst, float((n.min(dim=1).values / n.median(dim=1).values).min()))
    print(f"smallest norm / median norm over the case list: {worst:.4f}")
    assert worst >= 0.05


def test_fp32_error_of_the_restatement():
    """e_rel = max over the non-identical cases and the layers of |d32 - d64| / d64: the yardstick of the device's tolerance"""
    sd = ref.synth_state()
    e_rel = 0.0
    for case, (tot64, lay64) in zip(ref.case_list(), ref.reference()):
        B = case["size"][0]
        _, lay32 = ref.lpips(case["a"], case["b"], sd, torch.float32)
        assert np.all(lay32[:B] == 0.0) and np.all(lay64[:B] == 0.0)
        e = float((np.abs(lay32[B:] - lay64[B:]) / lay64[B:]).max())
        print(f"size {case['size']}: e_rel {e:.3e}, largest layer value {lay64.max():.4f}, smallest non-identical {lay64[B:].min():.3e}")
        e_rel = max(e_rel, e)
    print(f"e_rel = {e_rel:.3e}")
    assert e_rel < 1e-5
