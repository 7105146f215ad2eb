"""GPU: evaluate.py --clip_ckpt end to end with the SMALL model and a synthetic CLIP state dict written here: every record's
"clip_sim" is the fp64 cosine of what ClipCodec.u8_to_codes gives for the same u8 pair, the retrieval figures of the summary are
retrieval_summary of the restated ranks (tests/search_rank_ref.py), "clip_code_match" tells the tower of the archive from another,
the anchor carries the same keys, and the lines without the flag are what they were."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as ref  # noqa: E402
import search_rank_ref as rref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(256, 256)] * 3 + [(200, 300)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
SUMMARY_KEYS = ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]
CLIP_SUMMARY = ["clip_sim", "clip_recall@1", "clip_recall@5", "clip_recall@10", "clip_mrr", "clip_median_rank"]


def _rgb(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """compress and decompress (PNG) four images once with the default test tower; the plain report; that tower's state dict and
    another one as files; the tower itself"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, evaluate, weights as W
    from sgic_amd.codec import ClipCodec
    from sgic_amd.config import CLIP_TINY
    root = tmp_path_factory.mktemp("clip_eval")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(60 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(plain)]) == 0
    same = W.synth_weights(W.clip_spec(CLIP_TINY), seed=4321)          # the tower compress.py --small uses without --clip_ckpt
    torch.save(same, root / "clip_same.pt")
    torch.save({k[len("clip."):]: v for k, v in W.synth_weights(W.clip_spec(CLIP_TINY), seed=777).items()}, root / "clip_other.pt")
    return {"root": root, "src": src, "out": out, "plain": plain.read_text().splitlines(), "same": str(root / "clip_same.pt"),
            "other": str(root / "clip_other.pt"), "clipc": ClipCodec(same, CLIP_TINY, DEV)}


def _embed(clipc, img):
    """one image (H, W, 3) u8 -> (unit (D,) fp32, code (D,) u8) through ClipCodec.u8_to_codes, alone in its batch"""
    u, q = clipc.u8_to_codes(torch.from_numpy(img[None]).to(DEV), np.array([img.shape[:2]]))
    return u[0].cpu().numpy(), q[0].cpu().numpy()


def _cos(u, v):
    u, v = u.astype(np.float64), v.astype(np.float64)
    return float((u * v).sum() / (np.sqrt((u * u).sum()) * np.sqrt((v * v).sum())))


def _retrieval(units, codes):
    """the restated summary figures: query j against all codes, target j"""
    from sgic_amd.search import retrieval_summary
    rank, score = rref.rank_vectors(np.stack(units), np.stack(codes), np.arange(len(units)))
    s = retrieval_summary(rank, score)
    return {"recall@1": s["recall@1"], "recall@5": s["recall@5"], "recall@10": s["recall@10"], "mrr": s["mrr"],
            "median_rank": s["median_rank"]}


def test_records_and_summary_carry_the_clip_figures(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "clip.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--out", str(rep),
                          "--clip_ckpt", run["same"]]) == 0
    err = capsys.readouterr().err.splitlines()
    lines = rep.read_text().splitlines()
    assert err[-1] == lines[-1]
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == 4
    units, codes = [], []
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + ["clip_sim", "clip_code_match"]
        assert {k: r[k] for k in KEYS} == p                      # the other keys are those of the run without the flag
        ua, qa = _embed(run["clipc"], _rgb(run["src"] / f"{r['name']}.png"))
        ub, _ = _embed(run["clipc"], _rgb(run["out"] / "results" / f"{r['name']}.png"))
        want = _cos(ua, ub)
        print(r["name"], r["clip_sim"], want, r["clip_code_match"])
        assert isinstance(r["clip_sim"], float) and r["clip_sim"] == want and -1.0 <= want <= 1.0 + 1e-6
        assert r["clip_code_match"] is True                      # written by compress.py with this tower
        units.append(ub)
        codes.append(qa)
    assert list(summary) == SUMMARY_KEYS + CLIP_SUMMARY + ["clip_code_mismatch"]
    assert {k: summary[k] for k in SUMMARY_KEYS} == plain[-1]
    assert summary["clip_sim"] == float(np.mean(np.array([r["clip_sim"] for r in recs], dtype=np.float64)))
    want = _retrieval(units, codes)
    print(summary, want)
    assert {k[len("clip_"):]: summary[k] for k in CLIP_SUMMARY[1:]} == want
    assert summary["clip_code_mismatch"] == 0


def test_another_tower_is_told_apart(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "clip_other.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--bitstreams",
                          str(run["out"] / "bitstreams"), "--small", "--out", str(rep), "--clip_ckpt", run["other"]]) == 0
    capsys.readouterr()
    lines = [json.loads(ln) for ln in rep.read_text().splitlines()]
    assert len(lines) == 5 and all(r["clip_code_match"] is False for r in lines[:-1])
    assert lines[-1]["clip_code_mismatch"] == 4


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


def test_anchor_carries_the_clip_figures(run, capsys):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    base, rep = run["root"] / "fixed.jsonl", run["root"] / "fixed_clip.jsonl"
    args = ["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--small", "--anchor_quality", "50"]
    assert evaluate.main(args + ["--out", str(base)]) == 0
    assert evaluate.main(args + ["--out", str(rep), "--clip_ckpt", run["same"]]) == 0
    capsys.readouterr()
    old = [json.loads(ln) for ln in base.read_text().splitlines()]
    new = [json.loads(ln) for ln in rep.read_text().splitlines()]
    assert len(new) == 5
    units, codes = [], []
    for r, p in zip(new[:-1], old[:-1]):
        assert list(p) == KEYS + ["anchor"] and list(p["anchor"]) == ANCHOR_KEYS
        assert list(r) == KEYS + ["clip_sim", "anchor"] and list(r["anchor"]) == ANCHOR_KEYS[:-1] + ["clip_sim", "over_rate"]   # no containers
        assert {k: r[k] for k in KEYS} == {k: p[k] for k in KEYS} and {k: r["anchor"][k] for k in ANCHOR_KEYS} == p["anchor"]
        a = _rgb(run["src"] / f"{r['name']}.png")
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=50, subsampling=2)
        ua, qa = _embed(run["clipc"], a)
        uj, _ = _embed(run["clipc"], np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
        assert r["anchor"]["clip_sim"] == _cos(ua, uj)
        units.append(uj)
        codes.append(qa)
    keys = list(old[-1])
    anchor_clip = ["anchor_" + k for k in CLIP_SUMMARY]
    assert list(new[-1]) == SUMMARY_KEYS + CLIP_SUMMARY + keys[len(SUMMARY_KEYS):] + anchor_clip
    assert {k: new[-1][k] for k in keys} == old[-1]
    assert new[-1]["anchor_clip_sim"] == float(np.mean(np.array([r["anchor"]["clip_sim"] for r in new[:-1]], dtype=np.float64)))
    assert {k[len("anchor_clip_"):]: new[-1][k] for k in anchor_clip[1:]} == _retrieval(units, codes)
