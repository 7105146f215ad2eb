"""GPU: evaluate.py --niqe_params end to end with the SMALL model and the four images of tests/test_gpu_evaluate.py: the new keys
stand where DESIGN.md section 19 puts them, their values are niqe.Niqe.measure's on the u8 images, and a report without the flag is
the one it was."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niqe_ref  # noqa: E402
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(256, 256)] * 3 + [(200, 300)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
SUMMARY = ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
ANCHOR_SUMMARY = ["anchor_bpp", "anchor_psnr", "anchor_ms_ssim", "anchor_ms_ssim_db", "anchor_over_rate"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate
    root = tmp_path_factory.mktemp("niqe")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(plain)]) == 0
    params = root / "params.npz"
    mu, cov = niqe_ref.pristine()
    np.savez(params, mu_pris_param=mu, cov_pris_param=cov)
    return {"root": root, "src": src, "out": out, "plain": plain.read_text().splitlines(), "params": params}


def _measure(path):
    from PIL import Image
    from sgic_amd import niqe
    x = torch.from_numpy(np.array(Image.open(path).convert("RGB"))[None]).to("cuda:0")
    v = niqe.Niqe(niqe_ref.pristine()).measure(x)[0]
    return None if np.isnan(v) else float(v)


def _mean(vals):
    vals = [v for v in vals if v is not None]
    return float(np.mean(np.array(vals, dtype=np.float64))) if vals else None


def test_records_and_summary_carry_niqe(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep_a, rep_b = run["root"] / "a.jsonl", run["root"] / "b.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--niqe_params",
                          str(run["params"]), "--out", str(rep_a)]) == 0
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams",
                          str(run["out"] / "bitstreams"), "--niqe_params", str(run["params"]), "--out", str(rep_b)]) == 0
    capsys.readouterr()
    lines = rep_a.read_text().splitlines()
    assert lines == rep_b.read_text().splitlines()                  # --recon_dir gives the same report
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == 4
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + ["niqe", "niqe_orig"]
        assert {k: r[k] for k in KEYS} == p
        assert r["niqe"] == _measure(run["out"] / "results" / f"{r['name']}.png")
        assert r["niqe_orig"] == _measure(run["src"] / f"{r['name']}.png")
        assert r["niqe"] is not None and r["niqe_orig"] is not None and r["niqe"] > 0.0
    assert list(summary) == SUMMARY + ["niqe", "niqe_orig"]
    assert {k: summary[k] for k in SUMMARY} == plain[-1]
    assert summary["niqe"] == _mean([r["niqe"] for r in recs]) and summary["niqe_orig"] == _mean([r["niqe_orig"] for r in recs])


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


def test_anchor_carries_niqe_before_over_rate(run, capsys):
    import io
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "fixed.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor_quality", "50",
                          "--niqe_params", str(run["params"]), "--out", str(rep)]) == 0
    capsys.readouterr()
    lines = rep.read_text().splitlines()
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    assert len(recs) == 4
    for r in recs:
        assert list(r) == KEYS + ["niqe", "niqe_orig", "anchor"]
        assert list(r["anchor"]) == ANCHOR_KEYS[:-1] + ["niqe", "over_rate"]
        buf = io.BytesIO()       # the anchor's file is Pillow's (tests/test_gpu_evaluate_anchor.py), so its pixels are too
        Image.open(run["src"] / f"{r['name']}.png").convert("RGB").save(buf, format="JPEG", quality=50, subsampling=2)
        assert r["anchor"]["niqe"] == _measure(io.BytesIO(buf.getvalue()))
    assert list(summary) == SUMMARY + ANCHOR_SUMMARY + ["niqe", "niqe_orig", "anchor_niqe"]
    assert summary["anchor_niqe"] == _mean([r["anchor"]["niqe"] for r in recs])


def test_bad_params_end_the_command_before_any_model(run, capsys, monkeypatch):
    import sgic_amd  # noqa: F401
    from sgic_amd import codec, evaluate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(codec, "Codec", no_model)
    bad = run["root"] / "bad.npz"
    np.savez(bad, mu_pris_param=np.zeros(35), cov_pris_param=np.eye(36))
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--niqe_params",
                       str(bad)])
    assert e.value.code not in (0, None)
    assert "--niqe_params" in capsys.readouterr().err
