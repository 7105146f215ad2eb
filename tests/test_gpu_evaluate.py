"""GPU: evaluate.py end to end with the SMALL model: compress -> decompress -> the report from the containers alone and the report
from decompress.py's PNGs must be the same lines, and their numbers those of the fp64 restatement on (original, PNG)."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _num(v):
    return math.inf if v == "inf" else v


def test_evaluate_cli(tmp_path, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate
    src = tmp_path / "imgs"
    src.mkdir()
    sizes = [(256, 256)] * 3 + [(200, 300)]
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    out = tmp_path / "out"
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    # a stem without a partner on either side
    Image.fromarray(np.zeros((200, 200, 3), np.uint8)).save(src / "lonely.png")
    Image.fromarray(np.zeros((200, 200, 3), np.uint8)).save(out / "results" / "orphan.png")
    # a pair of different sizes and a reconstruction that is no image
    for stem, shape in (("mis", (210, 200, 3)), ("bad", None)):
        Image.fromarray(np.zeros((200, 200, 3), np.uint8)).save(src / f"{stem}.png")
        if shape:
            Image.fromarray(np.zeros(shape, np.uint8)).save(out / "results" / f"{stem}.png")
        else:
            (out / "results" / f"{stem}.png").write_bytes(b"not a png")
    capsys.readouterr()
    rep_a, rep_b = tmp_path / "a.jsonl", tmp_path / "b.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(rep_a)]) == 0
    err_a = capsys.readouterr().err.splitlines()
    assert evaluate.main(["--originals", str(src), "--recon_dir", str(out / "results"), "--bitstreams", str(out / "bitstreams"),
                          "--out", str(rep_b)]) == 0
    err_b = capsys.readouterr().err.splitlines()
    lines = rep_a.read_text().splitlines()
    assert lines == rep_b.read_text().splitlines()
    assert "[SKIP] lonely: no reconstruction for this original" in err_a and "[SKIP] lonely: no reconstruction for this original" in err_b
    assert any(ln.startswith("[SKIP] orphan:") for ln in err_b) and not any("orphan" in ln for ln in err_a)
    assert "[SKIP] mis: original is 200x200, reconstruction 210x200" in err_b
    assert any(ln.startswith("[SKIP] bad: unreadable reconstruction") for ln in err_b)
    assert err_a[-1] == lines[-1] and err_b[-1] == lines[-1]
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    assert [r["name"] for r in recs] == [f"im{i}" for i in range(4)]
    for r, (h, w) in zip(recs, sizes):
        assert list(r) == ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
        size = os.path.getsize(out / "bitstreams" / f"{r['name']}.c2df")
        assert (r["height"], r["width"], r["bytes"]) == (h, w, size) and r["bpp"] == 8 * size / (h * w)
        a = np.array(Image.open(src / f"{r['name']}.png").convert("RGB"))
        b = np.array(Image.open(out / "results" / f"{r['name']}.png").convert("RGB"))
        want = ref.measure(a[None], b[None])
        print(r, {k: float(v[0]) for k, v in want.items()})
        assert _num(r["psnr"]) == want["psnr"][0]
        assert abs(r["ms_ssim"] - want["ms_ssim"][0]) <= 1e-11 and abs(r["ssim"] - want["ssim"][0]) <= 1e-11
    assert summary["images"] == 4
    assert summary["bpp"] == float(np.mean(np.array([r["bpp"] for r in recs], dtype=np.float64)))
    assert summary["psnr"] == float(np.mean(np.array([r["psnr"] for r in recs if r["psnr"] != "inf"], dtype=np.float64)))
    assert summary["ms_ssim"] == float(np.mean(np.array([r["ms_ssim"] for r in recs], dtype=np.float64)))
    assert _num(summary["ms_ssim_db"]) == float(-10.0 * np.log10(1.0 - summary["ms_ssim"]))
