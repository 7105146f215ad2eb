"""GPU: the users of the JPEG encoder end to end with the SMALL model: evaluate.py --anchor jpeg (the anchor's quality, size and
numbers are those that Pillow's files and the fp64 restatement give) and decompress.py --format jpg (Pillow's files of the PNG
run's pixels)."""
import io
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(256, 256)] * 3 + [(200, 300)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]


def _num(v):
    return math.inf if v == "inf" else v


def _pillow(a, q, sub=2):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=q, subsampling=sub)
    return buf.getvalue()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """compress and decompress (PNG) the four images of tests/test_gpu_evaluate.py once; the plain report of the containers"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate
    root = tmp_path_factory.mktemp("anchor")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(plain)]) == 0
    return {"root": root, "src": src, "out": out, "plain": plain.read_text().splitlines()}


def _check_anchor(an, original, quality, budget):
    from PIL import Image
    data = _pillow(original, quality)
    assert list(an) == ANCHOR_KEYS
    assert (an["codec"], an["quality"], an["subsampling"]) == ("jpeg", quality, 2)
    h, w, _ = original.shape
    assert an["bytes"] == len(data) and an["bpp"] == 8 * len(data) / (h * w)
    want = ref.measure(original[None], np.array(Image.open(io.BytesIO(data)).convert("RGB"))[None])
    print(an, {k: float(v[0]) for k, v in want.items()})
    assert _num(an["psnr"]) == want["psnr"][0]
    assert abs(an["ms_ssim"] - want["ms_ssim"][0]) <= 1e-11 and abs(an["ssim"] - want["ssim"][0]) <= 1e-11
    assert _num(an["ms_ssim_db"]) == float(0.0 - 10.0 * np.log10(1.0 - an["ms_ssim"]))
    assert an["over_rate"] == (budget is not None and len(data) > budget)


def test_anchor_at_matched_rate(run, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    from sgic_amd.jpeg_enc import pick_quality
    rep = run["root"] / "anchor.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--anchor", "jpeg",
                          "--out", str(rep)]) == 0
    capsys.readouterr()
    lines = rep.read_text().splitlines()
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    assert len(recs) == 4
    plain = [json.loads(ln) for ln in run["plain"]]
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + ["anchor"]
        assert {k: r[k] for k in KEYS} == p                     # the record itself is the one of the run without --anchor
        a = np.array(Image.open(run["src"] / f"{r['name']}.png").convert("RGB"))
        sizes = {q: len(_pillow(a, q)) for q in range(1, 96)}
        q, over = pick_quality(sizes, r["bytes"])
        assert r["anchor"]["quality"] == q and r["anchor"]["over_rate"] == over
        _check_anchor(r["anchor"], a, q, r["bytes"])
    anchors = [r["anchor"] for r in recs]
    assert list(summary) == list(plain[-1]) + ["anchor_bpp", "anchor_psnr", "anchor_ms_ssim", "anchor_ms_ssim_db", "anchor_over_rate"]
    assert {k: summary[k] for k in plain[-1]} == plain[-1]
    assert summary["anchor_bpp"] == float(np.mean(np.array([a["bpp"] for a in anchors], dtype=np.float64)))
    assert summary["anchor_psnr"] == float(np.mean(np.array([a["psnr"] for a in anchors], dtype=np.float64)))
    assert summary["anchor_ms_ssim"] == float(np.mean(np.array([a["ms_ssim"] for a in anchors], dtype=np.float64)))
    assert _num(summary["anchor_ms_ssim_db"]) == float(0.0 - 10.0 * np.log10(1.0 - summary["anchor_ms_ssim"]))
    assert summary["anchor_over_rate"] == sum(1 for a in anchors if a["over_rate"])


def test_lines_without_anchor_are_unchanged(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "recon.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams",
                          str(run["out"] / "bitstreams"), "--out", str(rep)]) == 0
    capsys.readouterr()
    assert rep.read_text().splitlines() == run["plain"]
    for ln in run["plain"][:-1]:
        assert list(json.loads(ln)) == KEYS
    assert list(json.loads(run["plain"][-1])) == ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]


def test_fixed_quality_without_bitstreams(run, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "fixed.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor_quality", "50",
                          "--out", str(rep)]) == 0
    capsys.readouterr()
    lines = rep.read_text().splitlines()
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    assert len(recs) == 4 and summary["anchor_over_rate"] == 0
    for r in recs:
        assert r["bytes"] is None and r["bpp"] is None
        a = np.array(Image.open(run["src"] / f"{r['name']}.png").convert("RGB"))
        _check_anchor(r["anchor"], a, 50, None)


def test_anchor_search_needs_bitstreams(run, capsys, monkeypatch):
    import sgic_amd  # noqa: F401
    from sgic_amd import codec, evaluate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(codec, "Codec", no_model)
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor", "jpeg"])
    assert e.value.code not in (0, None)
    assert "--bitstreams" in capsys.readouterr().err


def test_decompress_to_jpeg(run):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import decompress
    dst = run["root"] / "jpg"
    assert decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(dst), "--small", "--format", "jpg",
                            "--quality", "80"]) == 0
    assert sorted(os.listdir(dst / "results")) == [f"im{i}.jpg" for i in range(4)]
    for i in range(4):
        pixels = np.array(Image.open(run["out"] / "results" / f"im{i}.png").convert("RGB"))
        assert (dst / "results" / f"im{i}.jpg").read_bytes() == _pillow(pixels, 80), i
    sub = run["root"] / "jpg444"
    assert decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(sub), "--small", "--format", "jpg",
                            "--subsampling", "0"]) == 0
    pixels = np.array(Image.open(run["out"] / "results" / "im3.png").convert("RGB"))
    assert (sub / "results" / "im3.jpg").read_bytes() == _pillow(pixels, 90, 0)
