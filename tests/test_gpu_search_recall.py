"""GPU: `search.py recall` end to end -- two `build-images` indexes of one small folder (TINY tower, a synthetic CLIP state dict
written here), then the same with one query picture swapped for a copy of another; the per-query lines and the summary against the
numpy restatement (tests/search_rank_ref.py) on the index files themselves."""
import contextlib
import io
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases  # noqa: E402
import search_rank_ref as rref  # noqa: E402

pytestmark = pytest.mark.gpu
N = 6


def _run(argv):
    """search.main(argv) -> (return code, everything it printed)"""
    from sgic_amd import search
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = search.main([str(a) for a in argv])
    return rc, out.getvalue()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """corpus: six PNGs; `same`: the same files in another folder; `swapped`: im3 replaced by a copy of im1, and one more picture
    that the corpus does not have"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import weights as W
    from sgic_amd.config import CLIP_TINY
    root = tmp_path_factory.mktemp("recall")
    ckpt = root / "clip.pt"
    torch.save(W.synth_weights(W.clip_spec(CLIP_TINY), seed=99), ckpt)
    rng = np.random.default_rng(71)
    src = root / "orig"
    src.mkdir()
    for j in range(N):
        Image.fromarray(jpeg_cases.natural_like(96 + 16 * j, 128 + 8 * j, rng)).save(src / f"im{j}.png")
    shutil.copytree(src, root / "same")
    shutil.copytree(src, root / "swapped")
    shutil.copyfile(src / "im1.png", root / "swapped" / "im3.png")
    Image.fromarray(jpeg_cases.natural_like(100, 100, rng)).save(root / "swapped" / "stranger.png")
    index = {}
    for name, folder in (("corpus", src), ("same", root / "same"), ("swapped", root / "swapped")):
        index[name] = root / f"index_{name}"
        rc, _ = _run(["build-images", "--image_dir", folder, "--index_dir", index[name], "--small", "--batch_size", "4", "--clip_ckpt", ckpt])
        assert rc == 0
    return dict(root=root, index=index)


def _summary(text):
    lines = text.strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0])


def test_an_index_finds_itself(built):
    out = built["root"] / "same.jsonl"
    rc, text = _run(["recall", "--index_dir", built["index"]["corpus"], "--queries_dir", built["index"]["same"], "--out", out])
    assert rc == 0
    rec = _summary(text)
    assert list(rec) == ["queries", "recall@1", "recall@5", "recall@10", "mrr", "mean_rank", "median_rank", "mean_score", "corpus",
                         "unmatched", "policy"]
    assert rec["queries"] == N and rec["corpus"] == N and rec["unmatched"] == 0 and rec["policy"] == "u8"
    assert rec["recall@1"] == 1.0 and rec["mrr"] == 1.0 and rec["mean_rank"] == 0.0 and rec["median_rank"] == 0.0
    rows = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert len(rows) == N and all(r["rank"] == 0 and list(r) == ["query", "target", "rank", "score"] for r in rows)
    assert [os.path.basename(r["query"]) for r in rows] == [os.path.basename(r["target"]) for r in rows] == [f"im{j}.png" for j in range(N)]
    assert all(abs(r["score"] - 1.0) <= 2.0 ** -22 for r in rows)


def _restated(built, vectors, ks):
    from sgic_amd.search import CodeIndex, load_index, pair_by_stem, retrieval_summary
    corpus = CodeIndex.load(built["index"]["corpus"])
    if vectors:
        q, qids = load_index(built["index"]["swapped"])
    else:
        qi = CodeIndex.load(built["index"]["swapped"])
        q, qids = qi.codes, qi.ids
    qrows, targets, unmatched = pair_by_stem(qids, corpus.ids)
    assert unmatched == 1 and qrows.size == N
    rank, score = (rref.rank_vectors if vectors else rref.rank_codes)(q[qrows], corpus.codes, targets)
    rec = retrieval_summary(rank, score, ks)
    rec.update({"corpus": N, "unmatched": 1, "policy": "f32q" if vectors else "u8"})
    rows = [{"query": qids[i], "target": corpus.ids[t], "rank": int(r), "score": float(s)}
            for i, t, r, s in zip(qrows.tolist(), targets.tolist(), rank, score)]
    return rec, rows


@pytest.mark.parametrize("vectors", [False, True])
def test_a_swapped_picture_against_the_restatement(built, vectors):
    out = built["root"] / f"swapped_{int(vectors)}.jsonl"
    argv = ["recall", "--index_dir", built["index"]["corpus"], "--queries_dir", built["index"]["swapped"], "--out", out, "--k", "1", "2", "6"]
    rc, text = _run(argv + (["--vectors"] if vectors else []))
    assert rc == 0
    want, want_rows = _restated(built, vectors, (1, 2, 6))
    got = _summary(text)
    print(got)
    assert got == want and list(got)[:4] == ["queries", "recall@1", "recall@2", "recall@6"]
    rows = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert rows == want_rows
    swapped = [r for r in rows if os.path.basename(r["query"]) == "im3.png"]
    assert len(swapped) == 1 and swapped[0]["rank"] >= 1 and os.path.basename(swapped[0]["target"]) == "im3.png"
    assert all(r["rank"] == 0 for r in rows if r is not swapped[0])
    assert got["recall@1"] == (N - 1) / N and got["recall@6"] == 1.0 and got["unmatched"] == 1
