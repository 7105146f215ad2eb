"""GPU: the threshold (range) search over u8 codes (csrc/search.hip search_range_kernel through ops.search_codes_range,
search.CodeIndex and the CLI) against its numpy restatement (tests/search_range_ref.py): the same pairs, the same score bits, the
exact count, everywhere."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as ref  # noqa: E402
import search_range_ref as rref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Dev:
    """one (queries, database) pair on the device with its restated scores, shared by every threshold tried on it"""

    def __init__(self, q, db, self_join=False):
        import sgic_amd  # noqa
        from sgic_amd.search import code_rnorm
        self.self_join = self_join
        self.db, self.r_db = _up(db), _up(code_rnorm(db))
        self.q, self.r_q = (self.db, self.r_db) if self_join else (_up(q), _up(code_rnorm(q)))
        self.score = ref.keys_and_scores(db if self_join else q, db)[1]
        self.upper = np.triu(np.ones(self.score.shape, dtype=bool), 1) if self_join else None

    def want(self, T):
        hit = self.score >= np.float32(T)
        if self.self_join:
            hit &= self.upper
        hq, hd = np.nonzero(hit)
        return hq.astype(np.int32), hd.astype(np.int32), self.score[hq, hd], int(hq.size)

    def got(self, T, **kw):
        from sgic_amd import ops
        hq, hd, hs, count = ops.search_codes_range(self.q, self.r_q, self.db, self.r_db, T, self_join=self.self_join, **kw)
        return hq.cpu().numpy(), hd.cpu().numpy(), hs.cpu().numpy(), count

    def check(self, T, what, **kw):
        _same(self.got(T, **kw), self.want(T), (what, T, kw))


def _same(got, want, what):
    (gq, gd, gs, gc), (wq, wd, ws, wc) = got, want
    assert gc == wc, (what, gc, wc)
    assert gq.dtype == np.int32 and gd.dtype == np.int32 and gs.dtype == np.float32 and gq.shape == gd.shape == gs.shape == (wc,), what
    assert np.array_equal(gq, wq) and np.array_equal(gd, wd), (what, np.argwhere((gq != wq) | (gd != wd))[:4].tolist())
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, np.argwhere(gs != ws)[:4].tolist())


def _planted_case(rng, nq, n, dim):
    """random codes; database rows copied into the queries exactly (twice) and with 1, 8 and 64 codes moved by +-1.
    -> (q, db, [(query, row)] of the plants that survive: with few queries a later plant overwrites an earlier one)"""
    db = ref.quantised_unit_codes(rng, n, dim)
    q = ref.quantised_unit_codes(rng, nq, dim)
    owner = {}
    for t, moved in enumerate((0, 0, 1, 8, 64)):
        qi, di = (5 * t) % nq, (37 * t + n // 2) % n
        q[qi] = rref.nudged(rng, db[di], min(moved, dim)) if moved else db[di]
        owner[qi] = di
    return q, db, sorted(owner.items())


@pytest.mark.parametrize("dim", [64, 192, 512])      # U = 1 with one step, U = 1 with three steps, U = 8
def test_variants_bit_equal(dim):
    """nq 1 / 16 -> the 16-query tile, 17 / 70 -> the 64-query tile with a ragged last tile; n around one 64-row step and many steps;
    splits chosen, one, three.  T: the three documented thresholds, one pair's own score (>= keeps it) and the next float above it
    (drops it)"""
    rng = np.random.default_rng(dim)
    for nq in (1, 16, 17, 70):
        for n in (1, 63, 64, 65, 1000):
            q, db, plants = _planted_case(rng, nq, n, dim)
            case = _Dev(q, db)
            pq, pd = plants[-1]
            own = case.score[pq, pd]
            above = np.nextafter(own, np.float32(np.inf))
            assert own in case.want(own)[2] and (case.score >= above).sum() < (case.score >= own).sum()
            for splits in (None, 1, 3):
                for T in (0.99999, 0.999, 0.99, own, above):
                    case.check(T, (dim, nq, n), splits=splits)
            hq, hd, _, _ = case.got(own)
            assert (pq, pd) in set(zip(hq.tolist(), hd.tolist()))
            hq, hd, _, _ = case.got(above)
            assert (pq, pd) not in set(zip(hq.tolist(), hd.tolist()))
            exact = [(a, b) for a, b in plants if np.array_equal(q[a], db[b])]
            hq, hd, _, _ = case.got(0.99999)
            assert set(exact) <= set(zip(hq.tolist(), hd.tolist()))


@pytest.mark.parametrize("dim,nq,n", [(64, 70, 1000), (512, 70, 1000), (192, 17, 65), (64, 1, 1)])
def test_dense_emission_every_pair_once(dim, nq, n):
    """T = -2: every lane of every wave emits in every step, masked rows and queries included; each (q, d) exactly once"""
    rng = np.random.default_rng(dim + n)
    case = _Dev(ref.quantised_unit_codes(rng, nq, dim), ref.quantised_unit_codes(rng, n, dim))
    for splits in (None, 1, 3):
        hq, hd, hs, count = case.got(-2.0, splits=splits)
        assert count == nq * n
        assert np.array_equal(hq, np.repeat(np.arange(nq, dtype=np.int32), n)) and np.array_equal(hd, np.tile(np.arange(n, dtype=np.int32), nq))
        assert np.array_equal(hs.view(np.uint32), case.score.reshape(-1).view(np.uint32))


def test_overflow_count_exact_nothing_past_capacity():
    import sgic_amd  # noqa
    from sgic_amd import ops
    rng = np.random.default_rng(20)
    case = _Dev(ref.quantised_unit_codes(rng, 70, 64), ref.quantised_unit_codes(rng, 1000, 64))
    T = 0.25                                           # D = 64: a few hundred of the 70 000 random pairs
    wq, wd, ws, total = case.want(T)
    assert 100 < total < 5000
    members = {(a, b): v for a, b, v in zip(wq.tolist(), wd.tolist(), ws.view(np.uint32).tolist())}
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for capacity, thr, full in ((37, T, total), (64, -2.0, 70000), (total, T, total)):
        pad = 4096                                     # canaries behind the `capacity` entries the call may write
        bq = torch.full((capacity + pad,), -7, dtype=torch.int32, device=DEV)
        bd = torch.full((capacity + pad,), -7, dtype=torch.int32, device=DEV)
        bs = torch.full((capacity + pad,), -7.0, dtype=torch.float32, device=DEV)
        count.zero_()
        ops.search_codes_range_launch(case.q, case.r_q, case.db, case.r_db, thr, False, None, capacity, count, bq, bd, bs)
        assert int(count.item()) == full
        assert bool((bq[capacity:] == -7).all()) and bool((bd[capacity:] == -7).all()) and bool((bs[capacity:] == -7.0).all())
        gq, gd, gs = bq[:capacity].cpu().numpy(), bd[:capacity].cpu().numpy(), bs[:capacity].cpu().numpy()
        pairs = list(zip(gq.tolist(), gd.tolist()))
        assert len(set(pairs)) == capacity             # all slots written, with distinct pairs
        if thr == T:
            assert all(members.get(p) == v for p, v in zip(pairs, gs.view(np.uint32).tolist()))
        else:
            assert np.array_equal(gs.view(np.uint32), case.score[gq, gd].view(np.uint32))
        count.zero_()                                  # count only
        ops.search_codes_range_launch(case.q, case.r_q, case.db, case.r_db, thr, False, None, 0, count, None, None, None)
        assert int(count.item()) == full
    # the counter is added to, not overwritten: it still holds the last count-only call's `total`
    ops.search_codes_range_launch(case.q, case.r_q, case.db, case.r_db, T, False, 3, 0, count, None, None, None)
    assert int(count.item()) == 2 * total
    # the wrapper retries once with exactly `count` entries and returns the full sorted set
    case.check(T, "retry", capacity=10)
    case.check(T, "retry", capacity=total - 1)
    case.check(T, "count only, then all", capacity=0)
    with pytest.raises(ValueError, match=str(total)):
        case.got(T, capacity=10, max_pairs=total - 1)
    case.check(T, "max_pairs met", max_pairs=total)


def test_refusals_of_the_entry_point():
    import sgic_amd  # noqa
    from sgic_amd import ops
    rng = np.random.default_rng(21)
    case = _Dev(ref.quantised_unit_codes(rng, 5, 64), ref.quantised_unit_codes(rng, 70, 64))
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):                  # self_join needs nq == n
        ops.search_codes_range_launch(case.q, case.r_q, case.db, case.r_db, 0.9, True, None, 0, count, None, None, None)
    with pytest.raises(RuntimeError):                  # a NaN reaches the library only past the wrapper: refused there too
        ops.search_codes_range_launch(case.q, case.r_q, case.db, case.r_db, float("nan"), False, None, 0, count, None, None, None)
    with pytest.raises(ValueError):
        case.got(float("nan"))
    q96 = _up(rng.integers(0, 256, (5, 96), dtype=np.uint8))
    with pytest.raises(RuntimeError):                  # D % 64
        ops.search_codes_range_launch(q96, case.r_q, q96, case.r_q, 0.9, False, None, 0, count, None, None, None)
    assert int(count.item()) == 0


def _self_join_corpus(rng, n, dim):
    """identical rows across the ends, a 64-row step edge, a 16-row tile edge, and three in one 16-row tile"""
    db = ref.quantised_unit_codes(rng, n, dim)
    for a, b in ((0, n - 1), (63, 64), (15, 16)):
        if b < n:
            db[b] = db[a]
    if n > 45:
        db[35] = db[40] = db[33]
    return db


@pytest.mark.parametrize("dim", [64, 512])
@pytest.mark.parametrize("n", [2, 16, 17, 64, 65, 130, 1000])
def test_self_join_upper_triangle(n, dim):
    rng = np.random.default_rng(100 * n + dim)
    db = _self_join_corpus(rng, n, dim)
    case = _Dev(None, db, self_join=True)
    loose = 0.3 if dim == 64 else 0.12                 # a threshold that random pairs pass too
    for splits in (None, 1, 3):
        for T in (0.99999, loose):
            case.check(T, ("self", n, dim), splits=splits)
        hq, hd, _, count = case.got(-2.0, splits=splits)
        assert count == n * (n - 1) // 2 and bool((hq < hd).all())
        assert len(set(zip(hq.tolist(), hd.tolist()))) == count
    hq, hd, _, _ = case.got(0.99999)
    found = set(zip(hq.tolist(), hd.tolist()))
    for a, b in ((0, n - 1), (63, 64), (15, 16)):     # at n = 17 and 65 the later plant overwrites row n - 1 of the first
        assert b >= n or not np.array_equal(db[a], db[b]) or (a, b) in found
    assert (15, 16) in found or n < 17
    if n > 45:
        assert {(33, 35), (33, 40), (35, 40)} <= found


def test_code_index_matches_the_top_k_kernel():
    """n <= 128: range_search(q, T) is CodeIndex.search(q, k = n) filtered by score >= T, ids and score bits; duplicate_pairs and
    duplicate_groups are the restatement's"""
    import sgic_amd  # noqa
    from sgic_amd import search
    rng = np.random.default_rng(30)
    db = _self_join_corpus(rng, 128, 64)
    q = np.concatenate([db[[0, 63, 33]], ref.quantised_unit_codes(rng, 17, 64)])
    ci = search.CodeIndex(db, [f"f{j}" for j in range(128)]).to(DEV)
    s, idx = ci.search(q, 128)
    for T in (0.99999, 0.2, -2.0):
        lims, rs, ri = ci.range_search(q, T)
        assert lims.dtype == np.int64 and lims.shape == (21,) and lims[0] == 0 and lims[-1] == rs.size == ri.size
        for j in range(20):
            keep = s[j] >= np.float32(T)
            order = np.argsort(idx[j][keep], kind="stable")
            assert np.array_equal(ri[lims[j]:lims[j + 1]], idx[j][keep][order]), (T, j)
            assert np.array_equal(rs[lims[j]:lims[j + 1]].view(np.uint32), s[j][keep][order].view(np.uint32)), (T, j)
        wl, ws, wi = rref.range_search(q, db, T)
        assert np.array_equal(lims, wl) and np.array_equal(ri, wi) and np.array_equal(rs.view(np.uint32), ws.view(np.uint32))
    wi, wj, ws, _ = rref.range_hits(db, db, 0.99999, self_join=True)
    gi, gj, gs = ci.duplicate_pairs(0.99999)
    assert np.array_equal(gi, wi) and np.array_equal(gj, wj) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    assert ci.duplicate_groups(0.99999) == rref.groups(wi, wj) == [[0, 127], [15, 16], [33, 35, 40], [63, 64]]
    with pytest.raises(ValueError, match="8128"):
        ci.duplicate_pairs(-2.0, max_pairs=1000)


def test_cli_duplicates_and_min_score(tmp_path, capsys):
    import sgic_amd  # noqa
    from sgic_amd import search
    from sgic_amd.filemaker import pack_c2df
    from sgic_amd.zstd import Compressor
    rng = np.random.default_rng(31)
    codes = ref.quantised_unit_codes(rng, 40, 512)
    codes[6] = codes[5]
    codes[20] = rref.nudged(rng, codes[5], 8)
    codes[31] = rref.nudged(rng, codes[30], 64)
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
    _, score = ref.keys_and_scores(codes, codes)
    link = lambda a, b: {"a": ids[a], "b": ids[b], "score": float(score[a, b])}   # noqa: E731
    dup = tmp_path / "dup.jsonl"
    assert search.main(["duplicates", "--index_dir", str(out), "--threshold", "0.99", "--out", str(dup)]) == 0
    lines = [json.loads(ln) for ln in dup.read_text().splitlines()]
    assert lines == [{"paths": [ids[5], ids[6], ids[20]], "links": [link(5, 6), link(5, 20), link(6, 20)]},
                     {"paths": [ids[30], ids[31]], "links": [link(30, 31)]}]
    err = capsys.readouterr().err.strip().splitlines()[-1]
    assert "40 rows" in err and "4 pairs" in err and "2 groups" in err and "5 files" in err
    assert search.main(["duplicates", "--index_dir", str(out), "--threshold", "0.99999"]) == 0     # identical codes only, to stdout
    assert [json.loads(ln) for ln in capsys.readouterr().out.splitlines()] == [{"paths": [ids[5], ids[6]], "links": [link(5, 6)]}]
    with pytest.raises(ValueError, match="780"):
        search.main(["duplicates", "--index_dir", str(out), "--threshold", "-2", "--max_pairs", "100"])
    capsys.readouterr()
    # query-c2df --codes --min_score: every hit, score descending, ties to the lower index; --topk is ignored
    assert search.main(["query-c2df", "--codes", "--index_dir", str(out), "--c2df", ids[5], "--min_score", "0.99", "--topk", "1"]) == 0
    assert json.loads(capsys.readouterr().out) == [{"path": ids[j], "score": float(score[5, j])} for j in (5, 6, 20)]
    assert score[5, 5] == score[5, 6] > score[5, 20]
    assert search.main(["query-c2df", "--codes", "--index_dir", str(out), "--c2df", str(src), "--min_score", "0.99"]) == 0
    got = json.loads(capsys.readouterr().out)
    assert list(got) == ids and [e["path"] for e in got[ids[31]]] == [ids[31], ids[30]] and [e["path"] for e in got[ids[0]]] == [ids[0]]
    # without the flag: the top k, as before
    ws, wi = ref.search(codes, codes, 5)
    want = [[{"path": ids[i], "score": float(v)} for i, v in zip(wi[j], ws[j])] for j in range(40)]
    assert search.main(["query-c2df", "--codes", "--index_dir", str(out), "--c2df", ids[7], "--topk", "5"]) == 0
    text = capsys.readouterr().out
    assert text == json.dumps(want[7], ensure_ascii=False, indent=2) + "\n"
