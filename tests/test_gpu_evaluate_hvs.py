"""GPU: evaluate.py --hvs end to end with the SMALL model on four images, one of them (32 x 48) too small for VIFp: the new keys stand
where DESIGN.md section 20 puts them, their values are quality.measure_hvs's on the written PNGs, the small image carries null and
is counted, and a report without the flag is the one it was."""
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

SIZES = [(256, 256)] * 2 + [(200, 300), (32, 48)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
HVS = ["vifp", "gmsd", "psnr_hvs", "psnr_hvs_m"]
SUMMARY = ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
ANCHOR_SUMMARY = ["anchor_bpp", "anchor_psnr", "anchor_ms_ssim", "anchor_ms_ssim_db", "anchor_over_rate"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate
    root = tmp_path_factory.mktemp("hvs")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(60 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(plain)]) == 0
    return {"root": root, "src": src, "out": out, "plain": plain.read_text().splitlines()}


def _load(path):
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(path).convert("RGB"))[None]).to("cuda:0")


def _measure(orig, recon):
    """quality.measure_hvs of one pair as the report prints it"""
    from sgic_amd import evaluate, quality
    m = quality.measure_hvs(_load(orig), _load(recon))
    return {k: None if m[k] is None else evaluate._json_number(m[k][0]) for k in HVS}


def _mean(vals):
    vals = [v for v in vals if isinstance(v, float)]
    return float(np.mean(np.array(vals, dtype=np.float64))) if vals else None


def test_records_and_summary_carry_the_keys(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep_a, rep_b = run["root"] / "a.jsonl", run["root"] / "b.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--hvs",
                          "--out", str(rep_a)]) == 0
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams",
                          str(run["out"] / "bitstreams"), "--hvs", "--out", str(rep_b)]) == 0
    capsys.readouterr()
    lines = rep_a.read_text().splitlines()
    assert lines == rep_b.read_text().splitlines()                  # --recon_dir gives the same report
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == 4
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + HVS                                 # directly after "ms_ssim_db"
        assert {k: r[k] for k in KEYS} == p
        want = _measure(run["src"] / f"{r['name']}.png", run["out"] / "results" / f"{r['name']}.png")
        assert {k: r[k] for k in HVS} == want
        small = min(r["height"], r["width"]) < 41
        assert (r["vifp"] is None) == small
        assert r["gmsd"] > 0.0 and r["psnr_hvs_m"] >= r["psnr_hvs"] and (small or r["vifp"] >= 0.0)
    assert sum(1 for r in recs if r["vifp"] is None) == 1
    assert list(summary) == SUMMARY + HVS + ["hvs_skipped"]
    assert {k: summary[k] for k in SUMMARY} == plain[-1]
    assert summary["hvs_skipped"] == 1
    for k in HVS:
        assert summary[k] == _mean([r[k] for r in recs])           # the means over the rest


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
    assert list(json.loads(run["plain"][-1])) == SUMMARY


def test_anchor_carries_the_keys(run, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep, rep_plain = run["root"] / "anchor.jsonl", run["root"] / "anchor_plain.jsonl"
    common = ["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams", str(run["out"] / "bitstreams"),
              "--anchor", "jpeg"]
    assert evaluate.main(common + ["--hvs", "--out", str(rep)]) == 0
    assert evaluate.main(common + ["--out", str(rep_plain)]) == 0
    capsys.readouterr()
    lines, plain = rep.read_text().splitlines(), [json.loads(ln) for ln in rep_plain.read_text().splitlines()]
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    assert len(recs) == 4
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + HVS + ["anchor"]
        assert list(r["anchor"]) == ANCHOR_KEYS[:-1] + HVS + ["over_rate"]
        assert {k: v for k, v in r["anchor"].items() if k not in HVS} == p["anchor"]      # the anchor is otherwise the one it was
        buf = io.BytesIO()       # the anchor's file is Pillow's (tests/test_gpu_evaluate_anchor.py), so its pixels are too
        Image.open(run["src"] / f"{r['name']}.png").convert("RGB").save(buf, format="JPEG", quality=r["anchor"]["quality"], subsampling=2)
        assert {k: r["anchor"][k] for k in HVS} == _measure(run["src"] / f"{r['name']}.png", io.BytesIO(buf.getvalue()))
    assert list(summary) == SUMMARY + HVS + ["hvs_skipped"] + ANCHOR_SUMMARY + ["anchor_" + k for k in HVS]
    assert {k: v for k, v in summary.items() if k in plain[-1]} == plain[-1]
    for k in HVS:
        assert summary["anchor_" + k] == _mean([r["anchor"][k] for r in recs])
