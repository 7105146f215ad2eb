"""GPU: the fused u8 code search (csrc/search.hip through ops.search_codes / search.CodeIndex / the CLI) against its numpy
restatement (tests/search_codes_ref.py).  Ids and scores are compared bit for bit everywhere; only the cross-check against the
existing fp32 path has a tolerance, the one that path's own 10k test uses."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(q, db, k, splits=None):
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    s, i = ops.search_codes(up(q), up(code_rnorm(q)), up(db), up(code_rnorm(db)), k, splits=splits)
    return s.cpu().numpy(), i.cpu().numpy()


def _same(got, want, what):
    (gs, gi), (ws, wi) = got, want
    assert gi.dtype == np.int32 and gs.dtype == np.float32 and gi.shape == wi.shape and gs.shape == ws.shape, what
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:4].tolist())
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, np.argwhere(gs != ws)[:4].tolist())


def _check(q, db, k, what, splits=None):
    _same(_gpu(q, db, k, splits), ref.search(q, db, k), (what, k, splits))


@pytest.mark.parametrize("dim", [64, 512])
@pytest.mark.parametrize("n", [1, 17, 1000])
def test_random_unit_codes_bit_equal(dim, n):
    rng = np.random.default_rng(1000 * dim + n)
    db = ref.quantised_unit_codes(rng, n, dim)
    for nq in (1, 5, 33):
        q = ref.quantised_unit_codes(rng, nq, dim)
        q[0] = db[n // 2]                                   # one query that is in the database
        key, score = ref.keys_and_scores(q, db)
        ids = np.arange(n)
        order = np.stack([np.lexsort((ids, -key[r])) for r in range(nq)])
        for k in sorted({1, min(10, n), min(128, n)}):
            want = (np.take_along_axis(score, order[:, :k], axis=1), order[:, :k].astype(np.int32))
            _same(_gpu(q, db, k), want, (dim, n, nq, k))


def _edge_rows(dim):
    alt = np.tile(np.array([0, 255], dtype=np.uint8), dim // 2)
    return np.stack([np.zeros(dim, np.uint8), np.full(dim, 255, np.uint8), alt, alt[::-1]])


@pytest.mark.parametrize("dim", [64, 512, 4096])
def test_sign_and_edge_rows(dim):
    """-128 * -128 accumulated over the whole row, +127 * +127, and the mixed signs: the largest |N| int32 has to hold"""
    rng = np.random.default_rng(dim)
    db = np.concatenate([_edge_rows(dim), ref.quantised_unit_codes(rng, 30, dim), _edge_rows(dim)])
    q = np.concatenate([_edge_rows(dim), ref.quantised_unit_codes(rng, 2, dim)])
    assert np.abs(ref.int_scores(q, db)).max() == 255 * 255 * dim
    _check(q, db, db.shape[0], "edge")
    _check(q, db, 3, "edge")


@pytest.mark.parametrize("nq", [17, 33])
def test_three_steps_one_load_per_round_wide_tile(nq):
    """D = 192: three 64-byte steps, not a multiple of eight, so one load per round (U = 1) with more than one step, under the
    64-query tile -- the query fragment index (f * steps + step) of every fragment f > 0.  nq = 17 / 33: the last live fragment
    (f = 1 / f = 2) holds one query, the fragments after it only clamped rows; n = 65: a one-row tail tile, which splits = 2 makes a split of its own"""
    rng = np.random.default_rng(192 + nq)
    db = ref.quantised_unit_codes(rng, 65, 192)
    q = ref.quantised_unit_codes(rng, nq, 192)
    q[nq - 1] = db[64]
    for k in (1, 10):
        want = ref.search(q, db, k)
        assert want[1][nq - 1, 0] == 64
        for splits in (1, 2):
            _same(_gpu(q, db, k, splits), want, ("D = 192", nq, k, splits))


def test_operand_placement_identity_queries_asymmetric_database():
    """query i is the unit step at coordinate p_i (a = 1 there, 0 elsewhere), so S(i, j) = a_db[j][p_i]: a row/column swap or a
    lane-map error of either MFMA operand shows as a wrong integer, the database being asymmetric in (row, coordinate)"""
    dim, n = 512, 48
    pos = (np.arange(16) * 37 + 5) % dim
    q = np.full((16, dim), 128, np.uint8)
    q[np.arange(16), pos] = 129
    j, c = np.meshgrid(np.arange(n), np.arange(dim), indexing="ij")
    db = ((7 * j * j + 3 * c + 11 * j * c + (c >> 4)) % 256).astype(np.uint8)
    big = ref.int_scores(q, db)
    a_db = db.astype(np.int64) - 128
    assert np.array_equal(big, 4 * a_db[:, pos].T + 2 + 2 * a_db.sum(axis=1)[None, :] + dim)
    _check(q, db, n, "identity")
    _check(q[:3], db, n, "identity")


def test_ties_across_tile_and_split_boundaries():
    """exact duplicates on both sides of a 16-row tile boundary, of a 64-row block step and of the split boundaries that
    splits = 3 (384 rows each) and splits = 7 (192 rows each) give on n = 1000: equal keys resolve to the lower index"""
    rng = np.random.default_rng(5)
    db = ref.quantised_unit_codes(rng, 1000, 512)
    dup = [15, 16, 63, 64, 191, 192, 383, 384, 999]
    db[dup] = db[15]
    q = np.concatenate([db[15:16], ref.quantised_unit_codes(rng, 4, 512)])
    for splits in (1, 3, 7, None):
        s, i = _gpu(q, db, 12, splits)
        assert i[0, :len(dup)].tolist() == dup, splits
        _same((s, i), ref.search(q, db, 12), splits)
        _check(q, db, 128, "ties", splits)


def test_identical_rows_return_first_ids():
    rng = np.random.default_rng(6)
    row = ref.quantised_unit_codes(rng, 1, 512)
    db = np.repeat(row, 300, axis=0)
    q = np.concatenate([row, ref.quantised_unit_codes(rng, 2, 512)])
    for splits in (1, 3):
        s, i = _gpu(q, db, 10, splits)
        assert np.array_equal(i, np.tile(np.arange(10, dtype=np.int32), (3, 1))), splits
        _same((s, i), ref.search(q, db, 10), splits)


@pytest.mark.parametrize("k", [10, 128])
def test_threshold_filter_worst_cases(k):
    """rows ordered by ascending score for query 0: every row beats the running k-th best, so the candidate buffer fills and is
    pruned at every step; descending: nothing after the first k passes"""
    rng = np.random.default_rng(7)
    db = ref.quantised_unit_codes(rng, 4096, 512)
    q = ref.quantised_unit_codes(rng, 3, 512)
    key, _ = ref.keys_and_scores(q[:1], db)
    asc = db[np.argsort(key[0], kind="stable")]
    for name, rows in (("ascending", asc), ("descending", asc[::-1].copy())):
        want = ref.search(q, rows, k)
        for splits in (1, None):
            _same(_gpu(q, rows, k, splits), want, (name, k, splits))


def test_unsupported_shapes_raise():
    rng = np.random.default_rng(8)
    db = ref.quantised_unit_codes(rng, 300, 512)
    with pytest.raises(RuntimeError):
        _gpu(db[:2], db, 129)
    db96 = rng.integers(0, 256, (300, 96), dtype=np.uint8)
    with pytest.raises(RuntimeError):
        _gpu(db96[:2], db96, 5)
    _check(db[:2], db, 128, "largest k")


def test_cross_check_with_fp32_path_10k():
    """the path that exists today on the same vectors: search_gpu(codes_to_unit(q), codes_to_unit(db)); scores within 1e-5, ids
    equal except where the fp64 scores of the swapped entries differ by less than 1e-6 (test_search_topk_parity_10k_corpus)"""
    import sgic_amd  # noqa
    from sgic_amd import search
    rng = np.random.default_rng(9)
    db = ref.quantised_unit_codes(rng, 10000, 512)
    db[4321] = db[1234]
    q = np.concatenate([db[[1234, 17, 9999]], ref.quantised_unit_codes(rng, 13, 512)])
    s, i = _gpu(q, db, 10)
    _same((s, i), ref.search(q, db, 10), "10k")
    uq, udb = search.codes_to_unit(q), search.codes_to_unit(db)
    s32, i32 = search.search_gpu(uq, udb, 10)
    full = uq.astype(np.float64) @ udb.astype(np.float64).T
    assert i[0, 0] == 1234 and i[0, 1] == 4321 and i[1, 0] == 17 and i[2, 0] == 9999
    for r in range(q.shape[0]):
        if not np.array_equal(i[r], i32[r]):
            assert np.abs(np.sort(full[r, i[r]])[::-1] - np.sort(full[r, i32[r]])[::-1]).max() < 1e-6, r
        assert np.abs(s[r].astype(np.float64) - full[r, i[r]]).max() <= 1e-5 and np.abs(s[r] - s32[r]).max() <= 1e-5, r


def test_no_score_matrix_in_device_memory():
    """n = 100 000, nq = 1024, k = 10: the call may allocate less than half of what the (nq, n) fp32 score matrix alone takes"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    rng = np.random.default_rng(10)
    n, nq, k = 100000, 1024, 10
    db = rng.integers(0, 256, (n, 512), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 512), dtype=np.uint8)
    dq, ddb = torch.from_numpy(q).to(DEV), torch.from_numpy(db).to(DEV)
    rq, rdb = torch.from_numpy(code_rnorm(q)).to(DEV), torch.from_numpy(code_rnorm(db)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    s, i = ops.search_codes(dq, rq, ddb, rdb, k)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < nq * n * 4 // 2, rise
    rows = [0, 15, 16, 1023]
    _same((s.cpu().numpy()[rows], i.cpu().numpy()[rows]), ref.search(q[rows], db, k), "100k")


def test_cli_build_query_neighbours(tmp_path, capsys):
    import sgic_amd  # noqa
    from sgic_amd import search
    from sgic_amd.filemaker import pack_c2df
    from sgic_amd.zstd import Compressor
    rng = np.random.default_rng(11)
    codes = ref.quantised_unit_codes(rng, 40, 512)
    codes[6] = codes[5]                                      # a duplicate ranks above the query's own id
    src = tmp_path / "c2df"
    src.mkdir()
    zc = Compressor(3)
    for j in range(40):
        enc = {"clip_stream": zc.compress(codes[j].tobytes()), "clip_meta": {"model_id": "m", "dim": 512}}
        (src / f"im{j:02d}.c2df").write_bytes(pack_c2df(enc, {"version": 2}))
    ids = [str(src / f"im{j:02d}.c2df") for j in range(40)]
    out = tmp_path / "index"
    assert search.main(["build", "--c2df_dir", str(src), "--index_dir", str(out)]) == 0
    capsys.readouterr()
    ws, wi = ref.search(codes, codes, 5)
    want = [[{"path": ids[i], "score": float(v)} for i, v in zip(wi[j], ws[j])] for j in range(40)]
    # one file through the code index, and through the fp32 files `build` wrote (the existing path, unchanged)
    assert search.main(["query-c2df", "--codes", "--index_dir", str(out), "--c2df", ids[7], "--topk", "5"]) == 0
    assert json.loads(capsys.readouterr().out) == want[7]
    assert search.main(["query-c2df", "--index_dir", str(out), "--c2df", ids[7], "--topk", "5"]) == 0
    old = json.loads(capsys.readouterr().out)
    assert old[0]["path"] == ids[7] and all(abs(a["score"] - b["score"]) <= 1e-5 for a, b in zip(old, want[7]))
    # the whole directory in one call
    assert search.main(["query-c2df", "--codes", "--index_dir", str(out), "--c2df", str(src), "--topk", "5"]) == 0
    assert json.loads(capsys.readouterr().out) == dict(zip(ids, want))
    # neighbours
    nb = tmp_path / "nb.jsonl"
    assert search.main(["neighbours", "--index_dir", str(out), "--topk", "3", "--out", str(nb)]) == 0
    lines = [json.loads(ln) for ln in nb.read_text().splitlines()]
    ws, wi = ref.search(codes, codes, 4)
    assert [ln["path"] for ln in lines] == ids
    for j, ln in enumerate(lines):
        keep = [(int(i), float(v)) for i, v in zip(wi[j], ws[j]) if i != j][:3]
        assert len(keep) == 3 and ids[j] not in [e["path"] for e in ln["neighbours"]]
        assert ln["neighbours"] == [{"path": ids[i], "score": v} for i, v in keep], j
    assert lines[6]["neighbours"][0]["path"] == ids[5] and lines[5]["neighbours"][0]["path"] == ids[6]
