"""GPU: evaluate.py --fsim end to end with the SMALL model on three images, plus a 1-pixel-wide one that only --recon_dir sees: the
two keys stand where DESIGN.md section 21 puts them (with and without --hvs), their values are quality.fsim's on the written PNGs,
the thin image carries null and is counted, and a report without the flag is the one it was."""
import io
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(256, 256)] * 2 + [(200, 300)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
HVS = ["vifp", "gmsd", "psnr_hvs", "psnr_hvs_m"]
FSIM = ["fsim", "fsimc"]
SUMMARY = ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
ANCHOR_SUMMARY = ["anchor_bpp", "anchor_psnr", "anchor_ms_ssim", "anchor_ms_ssim_db", "anchor_over_rate"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate
    root = tmp_path_factory.mktemp("fsim")
    src, out, src_all, recon_all = root / "imgs", root / "out", root / "imgs_all", root / "recon_all"
    for d in (src, src_all, recon_all):
        d.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(80 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    # the same three pairs and a 48 x 1 image with a reconstruction of its own, which has no container
    for i in range(len(SIZES)):
        shutil.copy(src / f"im{i}.png", src_all / f"im{i}.png")
        shutil.copy(out / "results" / f"im{i}.png", recon_all / f"im{i}.png")
    thin = np.ascontiguousarray(ref.texture(np.random.default_rng(90), 48, 8)[:, :1])
    Image.fromarray(thin).save(src_all / "thin.png")
    Image.fromarray(255 - thin).save(recon_all / "thin.png")
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(plain)]) == 0
    return {"root": root, "src": src, "out": out, "src_all": src_all, "recon_all": recon_all, "plain": plain.read_text().splitlines()}


def _load(path):
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(path).convert("RGB"))[None]).to("cuda:0")


def _measure(orig, recon):
    """quality.measure_fsim of one pair as the report prints it"""
    from sgic_amd import evaluate, quality
    m = quality.measure_fsim(_load(orig), _load(recon))
    return {k: None if m[k] is None else evaluate._json_number(m[k][0]) for k in FSIM}


def _mean(vals):
    vals = [v for v in vals if isinstance(v, float)]
    return float(np.mean(np.array(vals, dtype=np.float64))) if vals else None


def _read(path):
    lines = path.read_text().splitlines()
    return lines, [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])


def test_records_and_summary_carry_the_keys(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep_a, rep_b, rep_h = run["root"] / "a.jsonl", run["root"] / "b.jsonl", run["root"] / "h.jsonl"
    bits = str(run["out"] / "bitstreams")
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", bits, "--small", "--fsim", "--out", str(rep_a)]) == 0
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams", bits, "--fsim",
                          "--out", str(rep_b)]) == 0
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams", bits, "--fsim",
                          "--hvs", "--out", str(rep_h)]) == 0
    capsys.readouterr()
    lines, recs, summary = _read(rep_a)
    assert lines == rep_b.read_text().splitlines()                  # --recon_dir gives the same report
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == 3
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + FSIM                                # directly after "ms_ssim_db"
        assert {k: r[k] for k in KEYS} == p
        assert {k: r[k] for k in FSIM} == _measure(run["src"] / f"{r['name']}.png", run["out"] / "results" / f"{r['name']}.png")
        assert 0.0 < r["fsimc"] < r["fsim"] < 1.0
    assert list(summary) == SUMMARY + FSIM + ["fsim_skipped"]
    assert {k: summary[k] for k in SUMMARY} == plain[-1] and summary["fsim_skipped"] == 0
    for k in FSIM:
        assert summary[k] == _mean([r[k] for r in recs])
    _, recs_h, summary_h = _read(rep_h)                              # with --hvs: directly after "psnr_hvs_m"
    for r, q in zip(recs_h, recs):
        assert list(r) == KEYS + HVS + FSIM and {k: r[k] for k in KEYS + FSIM} == q
    assert list(summary_h) == SUMMARY + HVS + ["hvs_skipped"] + FSIM + ["fsim_skipped"]
    assert {k: summary_h[k] for k in SUMMARY + FSIM + ["fsim_skipped"]} == summary


def test_a_thin_image_carries_null_and_is_counted(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "thin.jsonl"
    assert evaluate.main(["--originals", str(run["src_all"]), "--recon_dir", str(run["recon_all"]), "--bitstreams",
                          str(run["out"] / "bitstreams"), "--fsim", "--out", str(rep)]) == 0
    capsys.readouterr()
    _, recs, summary = _read(rep)
    assert [r["name"] for r in recs] == ["im0", "im1", "im2", "thin"]
    thin = recs[3]
    assert list(thin) == KEYS + FSIM and (thin["height"], thin["width"]) == (48, 1)
    assert thin["fsim"] is None and thin["fsimc"] is None and isinstance(thin["psnr"], float)
    assert all(isinstance(r["fsim"], float) and isinstance(r["fsimc"], float) for r in recs[:3])
    assert summary["fsim_skipped"] == 1 and summary["images"] == 4
    for k in FSIM:
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
    rep, rep_h, rep_plain = run["root"] / "anchor.jsonl", run["root"] / "anchor_h.jsonl", run["root"] / "anchor_plain.jsonl"
    common = ["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams", str(run["out"] / "bitstreams"),
              "--anchor", "jpeg"]
    assert evaluate.main(common + ["--fsim", "--out", str(rep)]) == 0
    assert evaluate.main(common + ["--fsim", "--hvs", "--out", str(rep_h)]) == 0
    assert evaluate.main(common + ["--out", str(rep_plain)]) == 0
    capsys.readouterr()
    plain = [json.loads(ln) for ln in rep_plain.read_text().splitlines()]
    _, recs, summary = _read(rep)
    assert len(recs) == 3
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + FSIM + ["anchor"]
        assert list(r["anchor"]) == ANCHOR_KEYS[:-1] + FSIM + ["over_rate"]
        assert {k: v for k, v in r["anchor"].items() if k not in FSIM} == p["anchor"]      # the anchor is otherwise the one it was
        buf = io.BytesIO()       # the anchor's file is Pillow's (tests/test_gpu_evaluate_anchor.py), so its pixels are too
        Image.open(run["src"] / f"{r['name']}.png").convert("RGB").save(buf, format="JPEG", quality=r["anchor"]["quality"], subsampling=2)
        assert {k: r["anchor"][k] for k in FSIM} == _measure(run["src"] / f"{r['name']}.png", io.BytesIO(buf.getvalue()))
    assert list(summary) == SUMMARY + FSIM + ["fsim_skipped"] + ANCHOR_SUMMARY + ["anchor_" + k for k in FSIM]
    assert {k: v for k, v in summary.items() if k in plain[-1]} == plain[-1]
    for k in FSIM:
        assert summary["anchor_" + k] == _mean([r["anchor"][k] for r in recs])
    _, recs_h, summary_h = _read(rep_h)      # with --hvs: after the last hand-crafted key, before "over_rate" and the other anchor_* keys' end
    for r, q in zip(recs_h, recs):
        assert list(r["anchor"]) == ANCHOR_KEYS[:-1] + HVS + FSIM + ["over_rate"]
        assert {k: r["anchor"][k] for k in FSIM} == {k: q["anchor"][k] for k in FSIM}
    assert list(summary_h) == (SUMMARY + HVS + ["hvs_skipped"] + FSIM + ["fsim_skipped"] + ANCHOR_SUMMARY + ["anchor_" + k for k in HVS]
                               + ["anchor_" + k for k in FSIM])
