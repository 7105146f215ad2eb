"""GPU: the JPEG anchor at reduced resolution (evaluate.jpeg_anchors(scales=...), evaluate.py --anchor_scales) against the Pillow
restatement of tests/anchor_scales_ref.py: scale, quality, file size, coded size and over_rate for equality, the numbers within the
tolerance of tests/test_gpu_evaluate_anchor.py; and decompress.py --max_side against Pillow's Lanczos resize."""
import io
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor_scales_ref as ar  # noqa: E402
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(256, 256)] * 3 + [(200, 300)]
SCALES = (1, 2, 3, 4, 6, 8)
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
SCALE_KEYS = ANCHOR_KEYS[:3] + ["scale", "coded_height", "coded_width"] + ANCHOR_KEYS[3:]
SUMMARY_ANCHOR = ["anchor_bpp", "anchor_psnr", "anchor_ms_ssim", "anchor_ms_ssim_db", "anchor_over_rate"]
MIN_LEAD_DB = 0.01      # the choice of a scale must not hang on the last digits of two PSNRs


def _num(v):
    return math.inf if v == "inf" else v


@pytest.fixture(scope="module")
def textures():
    return [ref.texture(np.random.default_rng(40 + i), h, w) for i, (h, w) in enumerate(SIZES)]


def _anchors(images, budgets, **kw):
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    return evaluate.jpeg_anchors(torch.from_numpy(np.stack(images)).cuda(), list(budgets), 2, **kw)


def _check(an, original, want, lead, budget, optimize, keys=None):
    """an: an anchor record; want: the restatement's kept scale"""
    print(an, {k: want[k] for k in ("scale", "quality", "coded", "over_rate", "psnr")}, len(want["data"]), lead)
    assert lead is None or lead > MIN_LEAD_DB, lead
    keys = keys or (SCALE_KEYS[:3] + (["optimize"] if optimize else []) + SCALE_KEYS[3:])
    assert list(an) == keys
    assert (an["codec"], an["subsampling"]) == ("jpeg", 2) and an.get("optimize", False) == optimize
    h, w, _ = original.shape
    assert (an["scale"], an["quality"], an["bytes"]) == (want["scale"], want["quality"], len(want["data"]))
    assert (an["coded_height"], an["coded_width"]) == want["coded"]
    assert an["bpp"] == 8 * len(want["data"]) / (h * w)
    assert an["over_rate"] == bool(want["over_rate"])
    m = ref.measure(original[None], want["decoded"][None])
    assert _num(an["psnr"]) == m["psnr"][0]
    assert abs(an["ms_ssim"] - m["ms_ssim"][0]) <= 1e-11 and abs(an["ssim"] - m["ssim"][0]) <= 1e-11
    assert _num(an["ms_ssim_db"]) == float(0.0 - 10.0 * np.log10(1.0 - an["ms_ssim"]))


def test_budgets_of_the_small_model(textures):
    """the container sizes of the four textures: Pillow keeps scales 2, 3, 3, 1 at q = 50, 77, 77, 34"""
    budgets = (2848, 2848, 2848, 5037)
    want = [ar.anchor(a, SCALES, b, optimize=True) for a, b in zip(textures, budgets)]
    assert [(w["scale"], w["quality"]) for w, _ in want] == [(2, 50), (3, 77), (3, 77), (1, 34)]
    got = _anchors(textures[:3], budgets[:3], scales=SCALES, optimize=True) + _anchors(textures[3:], budgets[3:], scales=SCALES, optimize=True)
    for an, a, (w, lead), b in zip(got, textures, want, budgets):
        _check(an, a, w, lead, b, True)


def test_low_budget_needs_a_reduced_anchor(textures):
    """600 bytes: full resolution is over rate for every image (q = 1 is 964, 995, 995, 908 bytes); Pillow keeps scales 8, 8, 8, 6"""
    want = [ar.anchor(a, SCALES, 600, optimize=True) for a in textures]
    assert [w["scale"] for w, _ in want] == [8, 8, 8, 6]
    full = [ar.at_scale(a, 1, 600, optimize=True) for a in textures]
    assert [(f["over_rate"], f["quality"], len(f["data"])) for f in full] == [(True, 1, 964), (True, 1, 995), (True, 1, 995), (True, 1, 908)]
    got = _anchors(textures[:3], [600] * 3, scales=SCALES, optimize=True) + _anchors(textures[3:], [600], scales=SCALES, optimize=True)
    for an, a, (w, lead) in zip(got, textures, want):
        _check(an, a, w, lead, 600, True)
        assert an["over_rate"] is False


def test_apple_at_the_rate_of_the_reference_container():
    """the 859 x 1000 apple at the size of tests/golden/ref_apple.c2df: no JPEG at full resolution, scale 4 at q = 15 with the scales"""
    from PIL import Image
    a = np.array(Image.open(os.path.join(GOLDEN, "ref_apple.jpg")).convert("RGB"))
    budget = os.path.getsize(os.path.join(GOLDEN, "ref_apple.c2df"))
    assert budget == 2486
    want, lead = ar.anchor(a, SCALES, budget, optimize=True)
    assert (want["scale"], want["quality"], len(want["data"]), want["over_rate"]) == (4, 15, 2398, False)
    an = _anchors([a], [budget], scales=SCALES, optimize=True)[0]
    _check(an, a, want, lead, budget, True)
    plain = _anchors([a], [budget], optimize=True)[0]
    assert plain["over_rate"] is True and plain["quality"] == 1 and "scale" not in plain


def test_no_scale_fits(textures):
    """100 bytes: nothing fits; the smallest file over all scales is kept and over_rate is set"""
    want, _ = ar.anchor(textures[0], SCALES, 100, optimize=True)
    assert want["over_rate"] is True
    an = _anchors(textures[:1], [100], scales=SCALES, optimize=True)[0]
    _check(an, textures[0], want, None, 100, True)
    assert an["over_rate"] is True and an["bytes"] > 100


def test_choose_scale_rule():
    import sgic_amd  # noqa: F401
    from sgic_amd.evaluate import choose_scale
    inf = math.inf
    assert choose_scale([(1, True, 900, 30.0), (2, False, 500, 24.0), (3, False, 400, 25.0)]) == 2          # the best PSNR that fits
    assert choose_scale([(1, False, 900, 24.0), (2, False, 500, 24.0)]) == 0                                 # a tie: the smaller scale
    assert choose_scale([(1, False, 900, 50.0), (2, False, 500, inf), (3, False, 400, inf)]) == 1             # an infinite PSNR wins
    assert choose_scale([(1, True, 900, 30.0), (2, True, 500, 24.0), (3, True, 500, 25.0)]) == 1             # no fit: the smallest file
    assert choose_scale([(2, True, 500, 24.0)]) == 0


# ---- through the command line, with the SMALL architecture ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def run(tmp_path_factory, textures):
    """compress and decompress (PNG) the four textures once; the plain report and the report with the unscaled anchor"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate
    root = tmp_path_factory.mktemp("anchor_scales")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, a in enumerate(textures):
        Image.fromarray(a).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    base = ["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small"]
    plain, anchor = root / "plain.jsonl", root / "anchor.jsonl"
    assert evaluate.main(base + ["--out", str(plain)]) == 0
    assert evaluate.main(base + ["--anchor", "jpeg", "--out", str(anchor)]) == 0
    return {"root": root, "src": src, "out": out, "base": base, "plain": plain.read_text().splitlines(),
            "anchor": anchor.read_text().splitlines()}


def _report(run, name, extra):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / name
    assert evaluate.main(run["base"] + extra + ["--out", str(rep)]) == 0
    lines = rep.read_text().splitlines()
    return [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])


def test_cli_scales_against_the_restatement(run, textures, capsys):
    recs, summary = _report(run, "scales.jsonl", ["--anchor", "jpeg", "--anchor_scales", "3", "1", "2"])
    capsys.readouterr()
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == 4
    for r, p, a in zip(recs, plain[:-1], textures):
        assert list(r) == KEYS + ["anchor"] and {k: r[k] for k in KEYS} == p
        want, lead = ar.anchor(a, (1, 2, 3), r["bytes"])
        _check(r["anchor"], a, want, lead, r["bytes"], False, SCALE_KEYS)
    anchors = [r["anchor"] for r in recs]
    assert list(summary) == list(plain[-1]) + SUMMARY_ANCHOR + ["anchor_scale_counts"]
    assert summary["anchor_scale_counts"] == {str(s): sum(1 for a in anchors if a["scale"] == s) for s in sorted({a["scale"] for a in anchors})}
    assert sum(summary["anchor_scale_counts"].values()) == 4
    assert summary["anchor_bpp"] == float(np.mean(np.array([a["bpp"] for a in anchors], dtype=np.float64)))
    assert summary["anchor_psnr"] == float(np.mean(np.array([a["psnr"] for a in anchors], dtype=np.float64)))
    assert summary["anchor_over_rate"] == sum(1 for a in anchors if a["over_rate"])


def test_cli_lines_without_the_flag_keep_their_form(run, capsys):
    """without --anchor_scales no record and no summary carries a new key; scale 1 alone is the same anchor plus the three keys"""
    old = [json.loads(ln) for ln in run["anchor"]]
    for r in old[:-1]:
        assert list(r) == KEYS + ["anchor"] and list(r["anchor"]) == ANCHOR_KEYS
    assert list(old[-1]) == list(json.loads(run["plain"][-1])) + SUMMARY_ANCHOR
    recs, summary = _report(run, "scale1.jsonl", ["--anchor", "jpeg", "--anchor_scales", "1"])
    capsys.readouterr()
    for r, o in zip(recs, old[:-1]):
        assert list(r["anchor"]) == SCALE_KEYS
        assert (r["anchor"]["scale"], r["anchor"]["coded_height"], r["anchor"]["coded_width"]) == (1, r["height"], r["width"])
        assert {k: r["anchor"][k] for k in ANCHOR_KEYS} == o["anchor"]
    assert {k: summary[k] for k in old[-1]} == old[-1] and summary["anchor_scale_counts"] == {"1": 4}


@pytest.mark.parametrize("extra, word", [(["--anchor_scales", "2"], "--anchor jpeg"),
                                         (["--anchor_quality", "50", "--anchor_scales", "1", "2"], "exactly one"),
                                         (["--anchor", "jpeg", "--anchor_scales", "2", "2"], "distinct"),
                                         (["--anchor", "jpeg", "--anchor_scales", "17"], "1..16")])
def test_cli_refuses(run, capsys, monkeypatch, extra, word):
    import sgic_amd  # noqa: F401
    from sgic_amd import codec, evaluate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(codec, "Codec", no_model)
    with pytest.raises(SystemExit) as e:
        evaluate.main(run["base"] + extra)
    assert e.value.code not in (0, None)
    assert word in capsys.readouterr().err


def test_cli_fixed_quality_and_scale(run, textures, capsys):
    recs, summary = _report(run, "fixed.jsonl", ["--anchor_quality", "50", "--anchor_scales", "2"])
    capsys.readouterr()
    for r, a in zip(recs, textures):
        want = ar.at_scale(a, 2, r["bytes"], fixed_quality=50)
        assert (r["anchor"]["scale"], r["anchor"]["quality"]) == (2, 50)
        _check(r["anchor"], a, want, None, r["bytes"], False, SCALE_KEYS)
    assert summary["anchor_scale_counts"] == {"2": 4}


@pytest.mark.parametrize("fmt", ["png", "jpg"])
def test_decompress_max_side(run, fmt):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import decompress
    from sgic_amd.resize import max_side_size
    dst = run["root"] / f"side_{fmt}"
    assert decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(dst), "--small", "--format", fmt,
                            "--max_side", "100"]) == 0
    assert sorted(os.listdir(dst / "results")) == [f"im{i}.{fmt}" for i in range(4)]
    for i, (h, w) in enumerate(SIZES):
        oh, ow = max_side_size(h, w, 100)
        assert (oh, ow) == ((100, 100) if h == w else (67, 100))
        full = Image.open(run["out"] / "results" / f"im{i}.png")
        want = np.asarray(full.resize((ow, oh), Image.LANCZOS))
        if fmt == "png":
            assert np.array_equal(np.asarray(Image.open(dst / "results" / f"im{i}.png")), want), i
        else:
            buf = io.BytesIO()
            Image.fromarray(want).save(buf, format="JPEG", quality=90, subsampling=2)
            assert (dst / "results" / f"im{i}.jpg").read_bytes() == buf.getvalue(), i


def test_decompress_max_side_leaves_small_results_alone(run):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import decompress
    dst = run["root"] / "side_big"
    assert decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(dst), "--small", "--max_side", "300"]) == 0
    for i in range(4):
        assert np.array_equal(np.asarray(Image.open(dst / "results" / f"im{i}.png")), np.asarray(Image.open(run["out"] / "results" / f"im{i}.png")))


def test_decompress_refuses_a_bad_side(run, capsys, monkeypatch):
    import sgic_amd  # noqa: F401
    from sgic_amd import decompress, filemaker

    def no_read(*a, **k):
        raise AssertionError("a container was read")
    monkeypatch.setattr(filemaker, "unpack_c2df", no_read)
    for bad in ("0", "16385"):
        with pytest.raises(SystemExit) as e:
            decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(run["root"] / "never"), "--max_side", bad])
        assert e.value.code not in (0, None)
        assert "--max_side" in capsys.readouterr().err
