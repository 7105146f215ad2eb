"""GPU: the command lines of the JPEG encoder's optimised Huffman tables with the SMALL model: evaluate.py --anchor_optimize (the
anchor's quality, size and numbers are those of Pillow's optimize=True files and the fp64 restatement) and decompress.py --format
jpg --optimize (Pillow's optimize=True files of the PNG run's pixels).  Without the flags the records are those of before."""
import io
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_opt_ref as oref  # noqa: E402
import jpeg_enc_ref as eref  # noqa: E402
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(256, 256)] * 3 + [(200, 300)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
OPT_KEYS = ANCHOR_KEYS[:3] + ["optimize"] + ANCHOR_KEYS[3:]


def _num(v):
    return math.inf if v == "inf" else v


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """compress and decompress (PNG) the four images of tests/test_gpu_evaluate_anchor.py once"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress
    root = tmp_path_factory.mktemp("anchor_opt")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    return {"root": root, "src": src, "out": out}


def _check_anchor(an, original, quality, budget, optimize):
    from PIL import Image
    data = oref.pillow_bytes(original, quality, 2) if optimize else eref.pillow_bytes(original, quality, 2)
    assert list(an) == (OPT_KEYS if optimize else ANCHOR_KEYS)
    assert (an["codec"], an["quality"], an["subsampling"]) == ("jpeg", quality, 2)
    assert "optimize" not in an or an["optimize"] is True
    h, w, _ = original.shape
    assert an["bytes"] == len(data) and an["bpp"] == 8 * len(data) / (h * w)
    want = ref.measure(original[None], np.array(Image.open(io.BytesIO(data)).convert("RGB"))[None])
    print(an, {k: float(v[0]) for k, v in want.items()})
    assert _num(an["psnr"]) == want["psnr"][0]
    assert abs(an["ms_ssim"] - want["ms_ssim"][0]) <= 1e-11 and abs(an["ssim"] - want["ssim"][0]) <= 1e-11
    assert _num(an["ms_ssim_db"]) == float(0.0 - 10.0 * np.log10(1.0 - an["ms_ssim"]))
    assert an["over_rate"] == (budget is not None and len(data) > budget)


@pytest.mark.parametrize("optimize", [True, False])
def test_anchor_at_matched_rate(run, capsys, optimize):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    from sgic_amd.jpeg_enc import pick_quality
    rep = run["root"] / f"anchor{int(optimize)}.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--anchor", "jpeg",
                          "--out", str(rep)] + (["--anchor_optimize"] if optimize else [])) == 0
    capsys.readouterr()
    lines = rep.read_text().splitlines()
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    assert len(recs) == 4
    pillow = oref.pillow_bytes if optimize else eref.pillow_bytes
    for r in recs:
        assert list(r) == KEYS + ["anchor"]
        a = np.array(Image.open(run["src"] / f"{r['name']}.png").convert("RGB"))
        q, over = pick_quality({q: len(pillow(a, q, 2)) for q in range(1, 96)}, r["bytes"])
        assert r["anchor"]["quality"] == q and r["anchor"]["over_rate"] == over
        _check_anchor(r["anchor"], a, q, r["bytes"], optimize)
    assert "optimize" not in summary
    assert summary["anchor_over_rate"] == sum(1 for r in recs if r["anchor"]["over_rate"])
    assert summary["anchor_bpp"] == float(np.mean(np.array([r["anchor"]["bpp"] for r in recs], dtype=np.float64)))


def test_fixed_quality_with_optimize(run, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "fixed.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor_quality", "50",
                          "--anchor_optimize", "--out", str(rep)]) == 0
    capsys.readouterr()
    recs = [json.loads(ln) for ln in rep.read_text().splitlines()[:-1]]
    assert len(recs) == 4
    for r in recs:
        _check_anchor(r["anchor"], np.array(Image.open(run["src"] / f"{r['name']}.png").convert("RGB")), 50, None, True)


def test_flags_need_their_subject(run, capsys, monkeypatch):
    import sgic_amd  # noqa: F401
    from sgic_amd import codec, decompress, evaluate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(codec, "Codec", no_model)
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor_optimize"])
    assert e.value.code not in (0, None) and "--anchor" in capsys.readouterr().err
    for fmt in (["--format", "png"], []):
        with pytest.raises(SystemExit) as e:
            decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(run["root"] / "no"), "--small", "--optimize"] + fmt)
        assert e.value.code not in (0, None) and "--format jpg" in capsys.readouterr().err
    assert not (run["root"] / "no").exists()


def test_decompress_to_optimised_jpeg(run):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import decompress
    dst = run["root"] / "jpg"
    assert decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(dst), "--small", "--format", "jpg",
                            "--quality", "80", "--optimize"]) == 0
    assert sorted(os.listdir(dst / "results")) == [f"im{i}.jpg" for i in range(4)]
    for i in range(4):
        pixels = np.array(Image.open(run["out"] / "results" / f"im{i}.png").convert("RGB"))
        assert (dst / "results" / f"im{i}.jpg").read_bytes() == oref.pillow_bytes(pixels, 80, 2), i
    plain = run["root"] / "jpg_plain"          # without the flag: Pillow's default file
    assert decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(plain), "--small", "--format", "jpg",
                            "--quality", "80"]) == 0
    pixels = np.array(Image.open(run["out"] / "results" / "im3.png").convert("RGB"))
    assert (plain / "results" / "im3.jpg").read_bytes() == eref.pillow_bytes(pixels, 80, 2)
