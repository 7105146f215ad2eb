"""CPU side of the rank-of-target search: the numpy restatement (tests/search_rank_ref.py) against the `search` of the two modules it
is built on, retrieval_summary on hand-made ranks, the stem pairing of `search.py recall`, and the refusals of the CLI and of
CodeIndex.rank / rank_vectors that need no GPU."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as cref  # noqa: E402
import search_rank_ref as rref  # noqa: E402
import search_vectors_ref as vref  # noqa: E402


@pytest.mark.parametrize("dim,n", [(64, 1), (64, 67), (128, 300)])
def test_restatement_is_the_position_in_the_full_search(dim, n):
    """k = n: for every query and EVERY target t, idx[q][rank] == t and the score bits are those of that entry"""
    rng = np.random.default_rng(dim + n)
    db = cref.quantised_unit_codes(rng, n, dim)
    if n > 10:
        db[[5, 9, n - 1]] = db[2]                                     # equal keys: the index decides
    qc = np.concatenate([db[min(2, n - 1):][:1], cref.quantised_unit_codes(rng, 3, dim)])
    qv = vref.random_unit(rng, 4, dim)
    for q, mod, rank_of in ((qc, cref, rref.rank_codes), (qv, vref, rref.rank_vectors)):
        s, idx = mod.search(q, db, n)
        seen = np.zeros((q.shape[0], n), dtype=bool)
        for t in range(n):
            rank, score = rank_of(q, db, np.full(q.shape[0], t))
            assert rank.dtype == np.int32 and score.dtype == np.float32
            rows = np.arange(q.shape[0])
            assert np.array_equal(idx[rows, rank], np.full(q.shape[0], t)), t
            assert np.array_equal(s[rows, rank].view(np.uint32), score.view(np.uint32)), t
            seen[rows, rank] = True
        assert seen.all()                                             # the ranks of the n targets are a permutation of 0 .. n - 1
    if n > 10:
        rank, _ = rref.rank_codes(qc[:1], db, [2])
        assert rank[0] == 0                                           # its own code, the lowest index among the copies
        assert [int(rref.rank_codes(qc[:1], db, [t])[0][0]) for t in (5, 9, n - 1)] == [1, 2, 3]


def test_rank_below_k_iff_in_the_top_k():
    rng = np.random.default_rng(3)
    db = cref.quantised_unit_codes(rng, 200, 64)
    q = vref.random_unit(rng, 6, 64)
    targets = rng.integers(0, 200, 6)
    rank, score = rref.rank_vectors(q, db, targets)
    for k in (1, 10, 128, 200):
        s, idx = vref.search(q, db, k)
        for j in range(6):
            assert (rank[j] < k) == (targets[j] in idx[j])
            if rank[j] < k:
                assert idx[j, rank[j]] == targets[j] and s[j, rank[j]].view(np.uint32) == score[j].view(np.uint32)


def test_retrieval_summary_hand_made():
    import sgic_amd  # noqa
    from sgic_amd.search import retrieval_summary
    got = retrieval_summary(np.array([0, 0, 3, 9, 40], dtype=np.int32), np.array([1.0, 0.5, 0.25, 0.25, 0.0], dtype=np.float32))
    assert list(got) == ["queries", "recall@1", "recall@5", "recall@10", "mrr", "mean_rank", "median_rank", "mean_score"]
    assert got["queries"] == 5 and got["recall@1"] == 0.4 and got["recall@5"] == 0.6 and got["recall@10"] == 0.8
    assert got["mrr"] == pytest.approx((1 + 1 + 1 / 4 + 1 / 10 + 1 / 41) / 5, rel=1e-15, abs=0)
    assert got["mean_rank"] == 52 / 5 and got["median_rank"] == 3.0 and got["mean_score"] == 0.4
    assert all(isinstance(v, float) for k, v in got.items() if k != "queries")
    even = retrieval_summary([0, 1, 2, 7], [0.5] * 4, ks=(2, 3))     # an even count: the median lies between the middle two
    assert even["median_rank"] == 1.5 and even["recall@2"] == 0.5 and even["recall@3"] == 0.75 and "recall@1" not in even
    tied = retrieval_summary([4, 4, 4, 4, 0, 9], [0.0] * 6)          # ties at the median
    assert tied["median_rank"] == 4.0 and tied["recall@5"] == 5 / 6
    none = retrieval_summary(np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert none == {"queries": 0, "recall@1": None, "recall@5": None, "recall@10": None, "mrr": None, "mean_rank": None,
                    "median_rank": None, "mean_score": None}
    json.dumps(got), json.dumps(none)
    with pytest.raises(ValueError):
        retrieval_summary([0, 1], [0.0, 0.0], ks=(0,))
    with pytest.raises(ValueError):
        retrieval_summary([0, 1], [0.0])
    with pytest.raises(ValueError):
        retrieval_summary([0, -1], [0.0, 0.0])


def test_stem_pairing():
    import sgic_amd  # noqa
    from sgic_amd.search import pair_by_stem
    corpus = ["/data/orig/a.png", "/data/orig/sub/b.jpg", "/data/orig/c.tar.png", "d"]
    queries = ["/out/results/b.png", "/elsewhere/zz.png", "c.tar.jpeg", "/out/results/a.c2df", "a.png", "d.webp", "c.png"]
    qrows, targets, unmatched = pair_by_stem(queries, corpus)
    assert qrows.tolist() == [0, 2, 3, 4, 5] and targets.tolist() == [1, 2, 0, 0, 3] and unmatched == 2
    assert qrows.dtype == np.int64 and targets.dtype == np.int64
    qrows, targets, unmatched = pair_by_stem([], corpus)
    assert qrows.size == 0 and targets.size == 0 and unmatched == 0
    with pytest.raises(ValueError) as e:
        pair_by_stem(queries, corpus + ["/other/b.png"])
    assert "/data/orig/sub/b.jpg" in str(e.value) and "/other/b.png" in str(e.value)
    qrows, targets, _ = pair_by_stem(["x/q.png", "y/q.png"], ["q.jpg"])    # two queries may share a target
    assert qrows.tolist() == [0, 1] and targets.tolist() == [0, 0]


def _index_dir(root, codes, ids):
    from sgic_amd.search import CodeIndex
    CodeIndex(codes, ids).save(root)
    return root


def test_recall_cli_refusals_before_any_load(tmp_path, capsys, monkeypatch):
    import sgic_amd  # noqa
    from sgic_amd import search
    rng = np.random.default_rng(1)
    good = _index_dir(tmp_path / "good", cref.quantised_unit_codes(rng, 4, 64), [f"im{j}.png" for j in range(4)])
    empty = tmp_path / "empty"
    empty.mkdir()
    loaded = []

    def no_load(*a, **k):
        loaded.append(a)
        raise AssertionError("an index file was read before the refusal")

    monkeypatch.setattr(np, "load", no_load)
    base = ["recall", "--index_dir", str(good), "--queries_dir", str(good)]
    for bad_k in (["0"], ["1", "5", "-3"]):
        with pytest.raises(SystemExit) as e:
            search.main(base + ["--k"] + bad_k)
        assert e.value.code == 2 and "at least 1" in capsys.readouterr().err
    for idx, qs, flags, word in ((empty, good, [], "codes.npy"), (good, empty, [], "codes.npy"), (good, tmp_path / "absent", [], "codes.npy"),
                                 (good, good, ["--vectors"], "faiss.index"), (empty, good, ["--vectors"], "codes.npy")):
        with pytest.raises(SystemExit) as e:
            search.main(["recall", "--index_dir", str(idx), "--queries_dir", str(qs)] + flags)
        assert e.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(FileNotFoundError):
        search.write_recall(good, empty)
    with pytest.raises(ValueError):
        search.write_recall(good, good, ks=(0,))
    assert not loaded
    with pytest.raises(SystemExit) as e:
        search.main(["recall", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--queries_dir" in text and "--vectors" in text and "--out" in text


def test_recall_cli_ambiguous_stem_and_no_partner_need_no_device(tmp_path, capsys):
    import sgic_amd  # noqa
    from sgic_amd import search
    rng = np.random.default_rng(2)
    codes = cref.quantised_unit_codes(rng, 3, 64)
    twice = _index_dir(tmp_path / "twice", codes, ["a/x.png", "b/x.jpg", "c/y.png"])
    qs = _index_dir(tmp_path / "qs", codes[:2], ["r/x.png", "r/y.png"])
    with pytest.raises(ValueError) as e:
        search.main(["recall", "--index_dir", str(twice), "--queries_dir", str(qs)])
    assert "a/x.png" in str(e.value) and "b/x.jpg" in str(e.value)
    other = _index_dir(tmp_path / "other", codes, ["p.png", "q.png", "r.png"])     # no query has a partner: nothing is launched
    capsys.readouterr()
    out = tmp_path / "per_query.jsonl"
    assert search.main(["recall", "--index_dir", str(other), "--queries_dir", str(qs), "--k", "1", "3", "--out", str(out)]) == 0
    rec = json.loads(capsys.readouterr().out)
    assert rec == {"queries": 0, "recall@1": None, "recall@3": None, "mrr": None, "mean_rank": None, "median_rank": None,
                   "mean_score": None, "corpus": 3, "unmatched": 2, "policy": "u8"}
    assert out.read_text() == ""
    wide = _index_dir(tmp_path / "wide", cref.quantised_unit_codes(rng, 2, 128), ["x.png", "y.png"])
    with pytest.raises(ValueError, match="dim"):
        search.main(["recall", "--index_dir", str(other), "--queries_dir", str(wide)])


def test_rank_argument_errors_need_no_device():
    import sgic_amd  # noqa
    from sgic_amd.search import CodeIndex
    rng = np.random.default_rng(5)
    db = cref.quantised_unit_codes(rng, 20, 64)
    ci = CodeIndex(db, [f"id{j}" for j in range(20)])
    qv, qc = vref.random_unit(rng, 3, 64), db[:3]
    for fn, q in ((ci.rank, qc), (ci.rank_vectors, qv)):
        for bad in ([0, 1], [0, 1, 2, 3], [[0, 1, 2]], 5):
            with pytest.raises(ValueError, match="targets"):
                fn(q, bad)
        for bad in ([0, 1, 20], [-1, 0, 0], [0, 2 ** 31, 0]):
            with pytest.raises(ValueError, match="outside"):
                fn(q, bad)
        with pytest.raises(ValueError, match="targets"):
            fn(q, [0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="dim"):
        ci.rank(cref.quantised_unit_codes(rng, 3, 128), [0, 1, 2])
    bad = qv.copy()
    bad[1, 7] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ci.rank_vectors(bad, [0, 1, 2])
    with pytest.raises(ValueError, match="unit"):
        ci.rank_vectors(2.0 * qv, [0, 1, 2])
    with pytest.raises(ValueError, match="dim"):
        ci.rank_vectors(vref.random_unit(rng, 3, 128), [0, 1, 2])
    big = CodeIndex(rng.integers(0, 256, (4, 2112), dtype=np.uint8), list("abcd"))
    with pytest.raises(ValueError, match="faiss.index"):
        big.rank_vectors(vref.random_unit(rng, 1, 2112), [0])
    assert ci._dev is None and big._dev is None                     # nothing was sent to a device


def test_exported_from_the_library():
    import sgic_amd  # noqa
    from sgic_amd import _lib, ops
    for name in ("sgic_search_rank_u8", "sgic_search_rank_f32q", "sgic_search_rank_work_bytes"):
        assert hasattr(_lib.lib, name)
    assert callable(ops.search_codes_rank) and callable(ops.search_codes_rank_f32q)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgic.h")).read()
    assert "int sgic_search_rank_u8(" in header and "int sgic_search_rank_f32q(" in header
