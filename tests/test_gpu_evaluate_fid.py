"""GPU: evaluate.py --fid_ckpt in --recon_dir mode (no codec) on six synthetic PNG pairs: three of 256 x 384, two of 512 x 256 and
one of 200 x 300, which gives no 256 x 256 window."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = {"a0": (256, 384), "a1": (256, 384), "a2": (256, 384), "b0": (512, 256), "b1": (512, 256), "c0": (200, 300)}


def _pair(name, h, w):
    rng = np.random.default_rng(sum(map(ord, name)))
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / (9.0 + 2 * c) + len(name) + rng.uniform(0, 3)) * np.cos(yy / (7.0 + c)) for c in range(3)], -1)
    a = np.clip(base + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8)
    b = np.clip(base * 0.95 + 5 + rng.normal(0, 14, base.shape), 0, 255).astype(np.uint8)
    return a, b


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate, fid, ops
    root = tmp_path_factory.mktemp("evaluate_fid")
    src, rec = root / "imgs", root / "results"
    src.mkdir()
    rec.mkdir()
    pairs = {}
    for name, (h, w) in SIZES.items():
        pairs[name] = _pair(name, h, w)
        Image.fromarray(pairs[name][0]).save(src / f"{name}.png")
        Image.fromarray(pairs[name][1]).save(rec / f"{name}.png")
    ckpt = str(root / "inception.pth")
    fid.synth_weights(1234, path=ckpt)
    old, ops.AUTOTUNE = ops.AUTOTUNE, False      # the launch modes are bitwise equivalent; the test does not spend its seconds racing them
    yield {"src": src, "rec": rec, "root": root, "ckpt": ckpt, "pairs": pairs, "evaluate": evaluate, "fid": fid}
    ops.AUTOTUNE = old


def _lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_summary_gains_fid_and_kid_and_the_lines_do_not_change(run, capsys):
    evaluate, fid = run["evaluate"], run["fid"]
    base = ["--originals", str(run["src"]), "--recon_dir", str(run["rec"])]
    plain, rep = run["root"] / "plain.jsonl", run["root"] / "fid.jsonl"
    assert evaluate.main(base + ["--out", str(plain)]) == 0
    assert evaluate.main(base + ["--out", str(rep), "--fid_ckpt", run["ckpt"]]) == 0
    err = capsys.readouterr().err
    assert "[WARN] FID over 7 windows" in err                     # fewer than 2048 samples: the number is biased, and says so
    a, b = _lines(plain), _lines(rep)
    assert len(a) == len(b) == 7 and a[:-1] == b[:-1]             # per-image lines byte for byte
    s0, s1 = json.loads(a[-1]), json.loads(b[-1])
    new = ["fid", "kid", "kid_std", "fid_patches", "fid_skipped"]
    assert not any(k in s0 for k in new + ["anchor_fid"])
    assert list(s1)[:len(s0)] == list(s0) and list(s1)[len(s0):] == new and all(s1[k] == s0[k] for k in s0)
    assert s1["fid_patches"] == 3 * 1 + 2 * 2 and s1["fid_skipped"] == 1
    # the direct API on the same windows: the groups in the order evaluate.py meets them, image-major within a group
    model = fid.InceptionFID(run["ckpt"], DEV)
    X, Y = [], []
    for names in (("a0", "a1", "a2"), ("b0", "b1")):
        h, w = SIZES[names[0]]
        desc = fid.descriptors(len(names), h, w, 256)
        X.append(model.features(torch.from_numpy(np.stack([run["pairs"][n][0] for n in names])).to(DEV), desc))
        Y.append(model.features(torch.from_numpy(np.stack([run["pairs"][n][1] for n in names])).to(DEV), desc))
    X, Y = torch.cat(X), torch.cat(Y)
    k, k_std = fid.kid(X, Y)
    assert X.shape == (7, 2048) and s1["fid"] == fid.fid(X, Y) and s1["kid"] == k and s1["kid_std"] == k_std
    assert s1["fid"] > 0 and np.isfinite(s1["kid"])


def test_whole_images_and_anchor(run, capsys):
    evaluate = run["evaluate"]
    rep = run["root"] / "anchor.jsonl"
    assert evaluate.main(["--originals", str(run["src"]), "--recon_dir", str(run["rec"]), "--anchor_quality", "50", "--out", str(rep),
                          "--fid_ckpt", run["ckpt"], "--fid_patch", "0"]) == 0
    capsys.readouterr()
    s = json.loads(_lines(rep)[-1])
    assert s["fid_patches"] == 6 and s["fid_skipped"] == 0        # whole images: one window each
    assert list(s)[-8:] == ["fid", "kid", "kid_std", "fid_patches", "fid_skipped", "anchor_fid", "anchor_kid", "anchor_kid_std"]
    assert all(isinstance(s[k], float) and np.isfinite(s[k]) for k in ("fid", "kid", "kid_std", "anchor_fid", "anchor_kid", "anchor_kid_std"))
    assert s["anchor_fid"] > 0 and "anchor" in json.loads(_lines(rep)[0])
