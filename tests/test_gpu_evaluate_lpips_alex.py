"""GPU: evaluate.py --lpips_alex_ckpt end to end with the SMALL model and a synthetic LPIPS-Alex state dict: every record's
"lpips_alex" is what lpips_alex.LpipsAlex.measure gives for the same u8 pair, the other keys and the lines without the flag are what
they were, the JPEG anchor and the summary carry it too, and with --lpips_ckpt as well both fields are there, "lpips" first."""
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
    """compress and decompress (PNG) the four images of tests/test_gpu_evaluate.py once; the plain report; the two models"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate, lpips, lpips_alex
    root = tmp_path_factory.mktemp("lpips_alex")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--recon_dir", str(out / "results"), "--bitstreams", str(out / "bitstreams"), "--out",
                          str(plain)]) == 0
    # the state dict in two files, one per key spelling
    sd = lpips_alex.to_reference_keys(lpips_alex.synth_weights(99))
    torch.save({k: v for k, v in sd.items() if k.startswith("net.")}, root / "trunk.pt")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, root / "lins.pt")
    ckpt = [str(root / "trunk.pt"), str(root / "lins.pt")]
    lpips.synth_weights(98, path=root / "vgg.pt")
    return {"root": root, "src": src, "out": out, "plain": plain.read_text().splitlines(), "ckpt": ckpt, "vgg": str(root / "vgg.pt"),
            "model": lpips_alex.LpipsAlex(ckpt, DEV), "vgg_model": lpips.LpipsVGG(str(root / "vgg.pt"), DEV)}


def _measure(model, a, b):
    tot, _ = model.measure(torch.from_numpy(a[None]).to(DEV), torch.from_numpy(b[None]).to(DEV))
    return float(tot[0])


def test_records_carry_lpips_alex(run, capsys):
    """decoded from the containers: the measured tensor is the u8 image that decompress.py writes"""
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "alex.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--out", str(rep),
                          "--lpips_alex_ckpt"] + run["ckpt"]) == 0
    err = capsys.readouterr().err.splitlines()
    lines = rep.read_text().splitlines()
    assert err[-1] == lines[-1]
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == 4
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + ["lpips_alex"]                  # where "lpips" would stand
        assert {k: r[k] for k in KEYS} == p                      # the other keys are those of the run without the flag
        want = _measure(run["model"], _rgb(run["src"] / f"{r['name']}.png"), _rgb(run["out"] / "results" / f"{r['name']}.png"))
        print(r["name"], r["lpips_alex"], want)
        assert isinstance(r["lpips_alex"], float) and r["lpips_alex"] == want and want > 0.0
    assert list(summary) == SUMMARY_KEYS + ["lpips_alex"] and {k: summary[k] for k in SUMMARY_KEYS} == plain[-1]
    assert summary["lpips_alex"] == float(np.mean(np.array([r["lpips_alex"] for r in recs], dtype=np.float64)))
    for ln in run["plain"][:-1]:
        assert list(json.loads(ln)) == KEYS
    assert list(json.loads(run["plain"][-1])) == SUMMARY_KEYS


def test_anchor_summary_and_both_flags(run, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    base, rep, both = run["root"] / "fixed.jsonl", run["root"] / "fixed_alex.jsonl", run["root"] / "fixed_both.jsonl"
    args = ["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor_quality", "50"]
    assert evaluate.main(args + ["--out", str(base)]) == 0
    assert evaluate.main(args + ["--out", str(rep), "--lpips_alex_ckpt"] + run["ckpt"]) == 0
    assert evaluate.main(args + ["--out", str(both), "--lpips_alex_ckpt"] + run["ckpt"] + ["--lpips_ckpt", run["vgg"]]) == 0
    capsys.readouterr()
    old = [json.loads(ln) for ln in base.read_text().splitlines()]
    new = [json.loads(ln) for ln in rep.read_text().splitlines()]
    two = [json.loads(ln) for ln in both.read_text().splitlines()]
    assert len(new) == 5 and len(two) == 5
    for r, t, p in zip(new[:-1], two[:-1], old[:-1]):
        assert list(p) == KEYS + ["anchor"] and list(p["anchor"]) == ANCHOR_KEYS
        assert list(r) == KEYS + ["lpips_alex", "anchor"] and list(r["anchor"]) == ANCHOR_KEYS[:-1] + ["lpips_alex", "over_rate"]
        assert list(t) == KEYS + ["lpips", "lpips_alex", "anchor"]
        assert list(t["anchor"]) == ANCHOR_KEYS[:-1] + ["lpips", "lpips_alex", "over_rate"]
        assert {k: r[k] for k in KEYS} == {k: p[k] for k in KEYS} and {k: r["anchor"][k] for k in ANCHOR_KEYS} == p["anchor"]
        a = _rgb(run["src"] / f"{r['name']}.png")
        rec = _rgb(run["out"] / "results" / f"{r['name']}.png")
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=50, subsampling=2)
        jpg = np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        assert r["anchor"]["lpips_alex"] == _measure(run["model"], a, jpg) and r["lpips_alex"] == _measure(run["model"], a, rec)
        assert t["lpips_alex"] == r["lpips_alex"] and t["anchor"]["lpips_alex"] == r["anchor"]["lpips_alex"]
        assert t["lpips"] == _measure(run["vgg_model"], a, rec) and t["anchor"]["lpips"] == _measure(run["vgg_model"], a, jpg)
        assert t["lpips"] != t["lpips_alex"]
    keys = list(old[-1])
    assert list(new[-1]) == SUMMARY_KEYS + ["lpips_alex"] + keys[len(SUMMARY_KEYS):] + ["anchor_lpips_alex"]
    assert list(two[-1]) == SUMMARY_KEYS + ["lpips", "lpips_alex"] + keys[len(SUMMARY_KEYS):] + ["anchor_lpips", "anchor_lpips_alex"]
    assert {k: new[-1][k] for k in keys} == old[-1]
    assert new[-1]["anchor_lpips_alex"] == float(np.mean(np.array([r["anchor"]["lpips_alex"] for r in new[:-1]], dtype=np.float64)))
    assert new[-1]["lpips_alex"] == float(np.mean(np.array([r["lpips_alex"] for r in new[:-1]], dtype=np.float64)))
    assert two[-1]["lpips_alex"] == new[-1]["lpips_alex"] and two[-1]["anchor_lpips_alex"] == new[-1]["anchor_lpips_alex"]
