"""GPU: evaluate.py --dists_ckpt end to end with the SMALL model and a synthetic DISTS state dict: every record's "dists" is what
dists.DistsVGG.measure gives for the same u8 pair, the other keys and the lines without the flag are what they were, the JPEG anchor
and the summary carry it too, and with --lpips_ckpt as well it comes after "lpips"."""
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
SIZES = [(256, 256)] * 2 + [(200, 300)]
KEYS = ["name", "height", "width", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db"]
ANCHOR_KEYS = ["codec", "quality", "subsampling", "bytes", "bpp", "psnr", "ssim", "ms_ssim", "ms_ssim_db", "over_rate"]
SUMMARY_KEYS = ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]


def _rgb(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """compress and decompress (PNG) three images once; the plain report; the DISTS model and an LPIPS state dict"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress, dists, evaluate, lpips
    root = tmp_path_factory.mktemp("dists")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    plain = root / "plain.jsonl"
    assert evaluate.main(["--originals", str(src), "--bitstreams", str(out / "bitstreams"), "--small", "--out", str(plain)]) == 0
    # the state dict in two files: the trunk under piq's keys, alpha and beta as DISTS_pytorch stores them
    sd = dists.to_style(dists.synth_weights(99), "piq")
    torch.save({k: v for k, v in sd.items() if k.startswith("model.")}, root / "trunk.pt")
    torch.save({k: v for k, v in sd.items() if k in ("alpha", "beta")}, root / "ab.pt")
    model = dists.DistsVGG([root / "trunk.pt", root / "ab.pt"], DEV)
    lpips.synth_weights(98, path=root / "lpips.pt")
    return {"root": root, "src": src, "out": out, "plain": plain.read_text().splitlines(), "ckpt": [str(root / "trunk.pt"), str(root / "ab.pt")],
            "lpips_ckpt": str(root / "lpips.pt"), "model": model}


def _dists_of(model, a, b):
    tot, _ = model.measure(torch.from_numpy(a[None]).to(DEV), torch.from_numpy(b[None]).to(DEV))
    return float(tot[0])


def test_records_carry_dists(run, capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    rep = run["root"] / "dists.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--bitstreams", str(run["out"] / "bitstreams"), "--small", "--out", str(rep),
                          "--dists_ckpt"] + run["ckpt"]) == 0
    err = capsys.readouterr().err.splitlines()
    lines = rep.read_text().splitlines()
    assert err[-1] == lines[-1]
    recs, summary = [json.loads(ln) for ln in lines[:-1]], json.loads(lines[-1])
    plain = [json.loads(ln) for ln in run["plain"]]
    assert len(recs) == len(SIZES)
    for r, p in zip(recs, plain[:-1]):
        assert list(r) == KEYS + ["dists"]
        assert {k: r[k] for k in KEYS} == p                      # the other keys are those of the run without the flag
        want = _dists_of(run["model"], _rgb(run["src"] / f"{r['name']}.png"), _rgb(run["out"] / "results" / f"{r['name']}.png"))
        print(r["name"], r["dists"], want)
        assert isinstance(r["dists"], float) and r["dists"] == want and 0.0 < want < 1.0
    assert list(summary) == SUMMARY_KEYS + ["dists"] and {k: summary[k] for k in SUMMARY_KEYS} == plain[-1]
    assert summary["dists"] == float(np.mean(np.array([r["dists"] for r in recs], dtype=np.float64)))


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


@pytest.mark.parametrize("with_lpips", [False, True], ids=["dists", "lpips+dists"])
def test_anchor_and_summary_carry_dists(run, capsys, with_lpips):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    base, rep = run["root"] / f"fixed{int(with_lpips)}.jsonl", run["root"] / f"fixed_dists{int(with_lpips)}.jsonl"
    args = ["--originals", str(run["src"]), "--recon_dir", str(run["out"] / "results"), "--anchor_quality", "50"]
    if with_lpips:
        args += ["--lpips_ckpt", run["lpips_ckpt"]]
    lp = ["lpips"] if with_lpips else []
    assert evaluate.main(args + ["--out", str(base)]) == 0
    assert evaluate.main(args + ["--out", str(rep), "--dists_ckpt"] + run["ckpt"]) == 0
    capsys.readouterr()
    assert base.read_text().splitlines() != rep.read_text().splitlines()
    old = [json.loads(ln) for ln in base.read_text().splitlines()]
    new = [json.loads(ln) for ln in rep.read_text().splitlines()]
    assert len(new) == len(SIZES) + 1
    for r, p in zip(new[:-1], old[:-1]):
        assert list(p) == KEYS + lp + ["anchor"] and list(p["anchor"]) == ANCHOR_KEYS[:-1] + lp + ["over_rate"]
        assert list(r) == KEYS + lp + ["dists", "anchor"] and list(r["anchor"]) == ANCHOR_KEYS[:-1] + lp + ["dists", "over_rate"]
        assert {k: r[k] for k in p if k != "anchor"} == {k: p[k] for k in p if k != "anchor"}
        assert {k: r["anchor"][k] for k in p["anchor"]} == p["anchor"]
        a = _rgb(run["src"] / f"{r['name']}.png")
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=50, subsampling=2)
        assert r["anchor"]["dists"] == _dists_of(run["model"], a, np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
        assert r["dists"] == _dists_of(run["model"], a, _rgb(run["out"] / "results" / f"{r['name']}.png"))
    keys = list(old[-1])
    n = len(SUMMARY_KEYS + lp)
    assert keys[:n] == SUMMARY_KEYS + lp and (not with_lpips or keys[-1] == "anchor_lpips")
    assert list(new[-1]) == keys[:n] + ["dists"] + keys[n:] + ["anchor_dists"]
    assert {k: new[-1][k] for k in keys} == old[-1]
    assert new[-1]["anchor_dists"] == float(np.mean(np.array([r["anchor"]["dists"] for r in new[:-1]], dtype=np.float64)))
    assert new[-1]["dists"] == float(np.mean(np.array([r["dists"] for r in new[:-1]], dtype=np.float64)))
