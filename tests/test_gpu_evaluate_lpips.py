"""GPU: evaluate.py --lpips_ckpt end to end with the SMALL model and a synthetic LPIPS state dict: every record's "lpips" is what
lpips.LpipsVGG.measure gives for the same u8 pair, the other keys and the lines without the flag are what they were, and the JPEG
anchor and the summary carry it too."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(256, 256)] * 3 + [(200, 300)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
SUMMARY_KEYS = ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]


def _rgb(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """compress and decompress (PNG) the four images of tests/test_gpu_evaluate.py once; the plain report; the LPIPS model"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate, lpips
    root = tmp_path_factory.mktemp("lpips")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(plain)]) == 0
    # the state dict in two files, one per key spelling
    sd = lpips.to_reference_keys(lpips.synth_weights(99))
    torch.save({k: v for k, v in sd.items() if k.startswith("net.")}, root / "trunk.pt")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, root / "lins.pt")
    model = lpips.LpipsVGG([root / "trunk.pt", root / "lins.pt"], DEV)
    return {"root": root, "src": src, "out": out, "plain": plain.read_text().splitlines(), "ckpt": [str(root / "trunk.pt"), str(root / "lins.pt")],
            "model": model}


def _lpips_of(model, a, b):
    tot, _ = model.measure(torch.from_numpy(a[None]).to(DEV), torch.from_numpy(b[None]).to(DEV))
    return float(tot[0])


def test_records_carry_lpips(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "lpips.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--out", str(rep),
                          "--lpips_ckpt"] + run["ckpt"]) == 0
    err = capsys.readouterr().err.splitlines()
    lines = rep.read_text().splitlines()
    assert err[-1] == lines[-1]
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == 4
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + ["lpips"]
        assert {k: r[k] for k in KEYS} == p                      # the other keys are those of the run without the flag
        want = _lpips_of(run["model"], _rgb(run["src"] / f"{r['name']}.png"), _rgb(run["out"] / "results" / f"{r['name']}.png"))
        print(r["name"], r["lpips"], want)
        assert isinstance(r["lpips"], float) and r["lpips"] == want and want > 0.0
    assert list(summary) == SUMMARY_KEYS + ["lpips"] and {k: summary[k] for k in SUMMARY_KEYS} == plain[-1]
    assert summary["lpips"] == float(np.mean(np.array([r["lpips"] for r in recs], dtype=np.float64)))


def test_lines_without_the_flag_are_unchanged(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "recon.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams",
                          str(run["out"] / "bitstreams"), "--out", str(rep)]) == 0
    capsys.readouterr()
    assert rep.read_text().splitlines() == run["plain"]
    for ln in run["plain"][:-1]:
        assert list(json.loads(ln)) == KEYS
    assert list(json.loads(run["plain"][-1])) == SUMMARY_KEYS


def test_anchor_and_summary_carry_lpips(run, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    base, rep = run["root"] / "fixed.jsonl", run["root"] / "fixed_lpips.jsonl"
    args = ["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor_quality", "50"]
    assert evaluate.main(args + ["--out", str(base)]) == 0
    assert evaluate.main(args + ["--out", str(rep), "--lpips_ckpt"] + run["ckpt"]) == 0
    capsys.readouterr()
    old = [json.loads(ln) for ln in base.read_text().splitlines()]
    new = [json.loads(ln) for ln in rep.read_text().splitlines()]
    assert len(new) == 5
    for r, p in zip(new[:-1], old[:-1]):
        assert list(p) == KEYS + ["anchor"] and list(p["anchor"]) == ANCHOR_KEYS
        assert list(r) == KEYS + ["lpips", "anchor"] and list(r["anchor"]) == ANCHOR_KEYS[:-1] + ["lpips", "over_rate"]
        assert {k: r[k] for k in KEYS} == {k: p[k] for k in KEYS} and {k: r["anchor"][k] for k in ANCHOR_KEYS} == p["anchor"]
        a = _rgb(run["src"] / f"{r['name']}.png")
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=50, subsampling=2)
        assert r["anchor"]["lpips"] == _lpips_of(run["model"], a, np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
        assert r["lpips"] == _lpips_of(run["model"], a, _rgb(run["out"] / "results" / f"{r['name']}.png"))
    keys = list(old[-1])
    assert list(new[-1]) == SUMMARY_KEYS + ["lpips"] + keys[len(SUMMARY_KEYS):] + ["anchor_lpips"]
    assert {k: new[-1][k] for k in keys} == old[-1]
    assert new[-1]["anchor_lpips"] == float(np.mean(np.array([r["anchor"]["lpips"] for r in new[:-1]], dtype=np.float64)))
    assert new[-1]["lpips"] == float(np.mean(np.array([r["lpips"] for r in new[:-1]], dtype=np.float64)))
