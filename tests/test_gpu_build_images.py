"""GPU: `search.py build-images` -- a folder of ordinary images indexed with the CLIP tower alone -- and `compress.py --write_codes`.
One folder (baseline JPEG decoded on the GPU, progressive JPEG / PNG / BMP decoded on the host, a broken file, a text file), one
run of the command, and every output file checked; then the code search and the vector search on that directory."""
import contextlib
import io
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases  # noqa: E402

pytestmark = pytest.mark.gpu

# (relative path, H, W, kind): every size distinct, 17..400 a side.  The five baseline JPEGs pad to 512 x 512 and fill batches of
# their own (GPU decode, mixed sizes in one canvas); everything else pads to 256 x 256 and is decoded on the host
SPEC = [("a/p0.png", 17, 200, "png"), ("a/p1.png", 200, 240, "png"), ("a/p2.png", 255, 129, "png"),
        ("a/q0.jpg", 131, 77, "prog"), ("a/q1.jpg", 250, 190, "prog"), ("a/r0.bmp", 100, 150, "bmp"),
        ("b/s0.jpg", 300, 400, "base"), ("b/s1.jpg", 400, 257, "base"), ("b/s2.jpeg", 257, 300, "base"), ("b/s3.JPG", 333, 390, "base"),
        ("b/s4.jpg", 390, 333, "base")]
BROKEN, TEXT = "b/broken.jpg", "b/readme.txt"


def _run(argv):
    """search.main(argv) -> (return code, everything it printed)"""
    from sgic_amd import search
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = search.main([str(a) for a in argv])
    return rc, out.getvalue()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from PIL import Image
    import sgic_amd  # noqa: F401
    root = tmp_path_factory.mktemp("build_images")
    src = root / "imgs"
    rng = np.random.default_rng(61)
    for rel, h, w, kind in SPEC:
        p = src / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        im = Image.fromarray(jpeg_cases.natural_like(h, w, rng))
        if kind in ("base", "prog"):
            im.save(p, "JPEG", quality=88, progressive=(kind == "prog"))
        else:
            im.save(p)
    (src / BROKEN).write_bytes(rng.integers(0, 256, 40, dtype=np.uint8).tobytes())
    (src / TEXT).write_text("not an image\n")
    index = root / "index"
    rc, text = _run(["build-images", "--image_dir", src, "--index_dir", index, "--small", "--batch_size", "4"])
    assert rc == 0
    valid = sorted(src / rel for rel, *_ in SPEC)
    return dict(root=root, src=src, index=index, text=text, valid=valid, listed=sorted(valid + [src / BROKEN]))


def test_skips_the_broken_file_and_lists_the_valid_ones_sorted(built):
    skips = [ln for ln in built["text"].splitlines() if ln.startswith("[SKIP]")]
    assert len(skips) == 1 and "broken.jpg" in skips[0]
    want = [str(p) for p in built["valid"]]
    assert len(want) == 11
    assert (built["index"] / "ids.txt").read_text(encoding="utf-8").split("\n") == want
    assert json.loads((built["index"] / "paths.json").read_text(encoding="utf-8")) == want
    rec = json.loads(built["text"].strip().splitlines()[-1])
    assert rec["images"] == 11 and rec["cli_images_per_s"] > 0 and set(rec["host_ms_per_batch"]) >= {"wait_loader", "submit"}
    # the five baseline JPEGs: batches of 4 + 1 decoded on the GPU; the six others: 4 + 2 on the host
    assert (rec["gpu_jpeg_batches"], rec["gpu_scan_jpeg_batches"], rec["host_decoded_batches"]) == (2, 0, 2), rec
    meta = json.loads((built["index"] / "meta.json").read_text(encoding="utf-8"))
    assert meta["dim"] == 64 and meta["model_id"].startswith("ViT-B-32")


def test_both_index_files_hold_each_image_s_own_vector(built):
    from PIL import Image
    from sgic_amd import search
    from sgic_amd import weights as W
    from sgic_amd.codec import ClipCodec
    from sgic_amd.config import CLIP_TINY
    a, b = (built["index"] / "faiss.index").read_bytes(), (built["index"] / "index.faiss").read_bytes()
    assert a == b
    vecs, ids = search.load_index(built["index"])
    assert vecs.shape == (11, 64) and vecs.dtype == np.float32 and ids == [str(p) for p in built["valid"]]
    clipc = ClipCodec(W.synth_weights(W.clip_spec(CLIP_TINY), seed=4321), CLIP_TINY, "cuda:0")
    for i, p in enumerate(built["valid"]):
        u8 = np.asarray(Image.open(p).convert("RGB"))
        unit, _ = clipc.u8_to_codes(torch.from_numpy(u8.copy())[None].cuda(), [u8.shape[:2]])
        err = float(np.abs(unit[0].cpu().numpy() - vecs[i]).max())
        print(p.name, "max |row - alone|", err)
        assert err <= 1e-6, (p.name, err)


def test_codes_are_the_tower_s_u8_output(built):
    from sgic_amd import search
    codes = np.load(built["index"] / "codes.npy")
    assert codes.shape == (11, 64) and codes.dtype == np.uint8
    vecs, _ = search.load_index(built["index"])
    t = (vecs.astype(np.float64) * 0.5 + 0.5) * 255.0
    host = np.clip(np.round(t), 0, 255)
    assert np.abs(codes.astype(np.float64) - host).max() <= 1
    clear = np.abs(t - np.floor(t) - 0.5) > 1e-3
    assert clear.mean() > 0.9 and np.array_equal(codes[clear].astype(np.float64), host[clear])


def test_queries_and_neighbours_work_on_the_image_index(built):
    png = built["src"] / "a/p1.png"
    for extra in (["--codes"], []):
        rc, text = _run(["query-image", "--index_dir", built["index"], "--image", png, "--topk", "3", "--small"] + extra)
        hits = json.loads(text)
        assert rc == 0 and len(hits) == 3 and hits[0]["path"] == str(png), (extra, hits)
    rc, text = _run(["neighbours", "--index_dir", built["index"], "--topk", "3"])
    rows = [json.loads(ln) for ln in text.splitlines()]
    assert rc == 0 and [r["path"] for r in rows] == [str(p) for p in built["valid"]] and all(len(r["neighbours"]) == 3 for r in rows)


def test_limit_and_random_selection(built):
    """the selection comes first, as in the reference, and the header pass drops the unreadable file from what was selected"""
    from sgic_amd import search
    first = built["root"] / "first5"
    rc, _ = _run(["build-images", "--image_dir", built["src"], "--index_dir", first, "--small", "--batch_size", "4", "--limit", "5"])
    assert rc == 0
    want = built["listed"][:5]
    assert built["src"] / BROKEN not in want
    assert search.load_index(first)[1] == [str(p) for p in want] and np.load(first / "codes.npy").shape == (5, 64)
    rnd = built["root"] / "random5"
    rc, _ = _run(["build-images", "--image_dir", built["src"], "--index_dir", rnd, "--small", "--batch_size", "4", "--limit", "5",
                  "--random", "--seed", "3"])
    assert rc == 0
    want = [p for p in random.Random(3).sample(built["listed"], 5) if p != built["src"] / BROKEN]
    assert search.load_index(rnd)[1] == [str(p) for p in want]
    # rows follow the ids whatever the batch plan was: each is the row the full index holds for that file
    full_vecs, full_ids = search.load_index(built["index"])
    got = search.load_index(rnd)[0]
    for i, p in enumerate(want):
        assert np.abs(got[i] - full_vecs[full_ids.index(str(p))]).max() <= 1e-6


def test_downloader_flags_and_other_towers_are_refused(built, capsys):
    from sgic_amd import search
    nowhere = built["root"] / "never"
    for extra, word in ((["--auto_download"], "no downloader"), (["--download_size", "64"], "no downloader"), (["--model_id", "RN50"], "ViT-B-32")):
        with pytest.raises(SystemExit) as e:
            search.main(["build-images", "--image_dir", str(built["src"]), "--index_dir", str(nowhere), "--small"] + extra)
        assert e.value.code != 0 and word in capsys.readouterr().err
        assert not nowhere.exists()


def test_compress_write_codes_is_opt_in_and_matches_build(built):
    from sgic_amd import compress, search
    src, root = built["src"] / "a", built["root"]
    out = root / "c_codes"
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4", "--write_codes"]) == 0
    other = root / "c_build"
    search.build_index(out / "bitstreams", other, log=lambda *_: None)
    got, want = np.load(out / "faiss" / "codes.npy"), np.load(other / "codes.npy")
    assert got.dtype == np.uint8 and got.shape == (6, 64) and got.tobytes() == want.tobytes()
    ids = [ln for ln in (out / "faiss" / "ids.txt").read_text(encoding="utf-8").splitlines() if ln]
    assert ids == (other / "ids.txt").read_text(encoding="utf-8").split("\n") and len(ids) == 6
    plain = root / "c_plain"
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(plain), "--small", "--batch_size", "4"]) == 0
    assert (plain / "faiss" / "index.faiss").exists() and not (plain / "faiss" / "codes.npy").exists()
