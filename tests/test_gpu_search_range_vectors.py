"""GPU: the threshold (range) search of fp32 queries over u8 codes (csrc/search.hip search_range_kernel with F32Query through
ops.search_codes_range_f32q, search.CodeIndex.range_search_vectors, the CLI and the resident service) against its numpy restatement
(tests/search_range_vectors_ref.py): the same pairs, the same score bits, the exact count, everywhere."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as cref  # noqa: E402
import search_range_ref as crref  # noqa: E402
import search_range_vectors_ref as rref  # noqa: E402
import search_vectors_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_TOKENS = "1,17,300,511"          # within the TINY text tower's vocabulary (512) and context (16)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Dev:
    """one (queries, database) pair on the device with its restated scores, shared by every threshold tried on it"""

    def __init__(self, q, db):
        import sgic_amd  # noqa
        from sgic_amd.search import code_rnorm
        self.q, self.db, self.r_db = _up(np.asarray(q, dtype=np.float32)), _up(db), _up(code_rnorm(db))
        self.score = ref.keys_and_scores(q, db)[1]

    def want(self, T):
        return rref.hits_of(self.score, T)

    def got(self, T, **kw):
        from sgic_amd import ops
        hq, hd, hs, count = ops.search_codes_range_f32q(self.q, self.db, self.r_db, T, **kw)
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
    """random unit queries; the dequantised vectors of database rows planted among them, exactly (twice) and with 1, 8 and 64 codes
    moved by +-1 first.  -> (q, db, [(query, row)] of the plants that survive: with few queries a later one overwrites an earlier)"""
    from sgic_amd.search import codes_to_unit
    db = ref.quantised_unit_codes(rng, n, dim)
    q = ref.random_unit(rng, nq, dim)
    owner = {}
    for t, moved in enumerate((0, 0, 1, 8, 64)):
        qi, di = (5 * t) % nq, (37 * t + n // 2) % n
        q[qi] = codes_to_unit(crref.nudged(rng, db[di], min(moved, dim)) if moved else db[di])
        owner[qi] = di
    return q, db, sorted(owner.items())


@pytest.mark.parametrize("dim", [64, 192, 512])      # U = 1 with one step, U = 1 with three steps, U = 8
def test_variants_bit_equal(dim):
    """nq 1 / 16 -> the 16-query tile, 17 / 40 -> the 32-query tile with a ragged last tile; n around one 64-row step and many steps;
    splits chosen, one, three.  T: two documented thresholds, one planted pair's own score (>= keeps it) and the next float above
    it (drops it)"""
    import sgic_amd  # noqa
    rng = np.random.default_rng(dim)
    for nq in (1, 16, 17, 40):
        for n in (1, 63, 64, 65, 1000):
            q, db, plants = _planted_case(rng, nq, n, dim)
            case = _Dev(q, db)
            pq, pd = plants[-1]
            own = case.score[pq, pd]
            above = np.nextafter(own, np.float32(np.inf))
            assert own in case.want(own)[2] and (case.score >= above).sum() < (case.score >= own).sum()
            assert case.want(0.99)[3] >= 1                          # even with all of 64 codes one step off a plant scores 0.998
            for splits in (None, 1, 3):
                for T in (0.999, 0.99, own, above):
                    case.check(T, (dim, nq, n), splits=splits)
            hq, hd, _, _ = case.got(own)
            assert (pq, pd) in set(zip(hq.tolist(), hd.tolist()))
            hq, hd, _, _ = case.got(above)
            assert (pq, pd) not in set(zip(hq.tolist(), hd.tolist()))


def test_largest_dim_raised_lds_and_narrow_tile():
    """D = 2048, nq = 17: three planes of 16 queries take 96.1 KiB of LDS (above the 64 KiB default), and the 32-query tile does not
    fit, so two 16-query tiles run, the second with one live row"""
    import sgic_amd  # noqa
    rng = np.random.default_rng(2048)
    q, db, plants = _planted_case(rng, 17, 130, 2048)
    case = _Dev(q, db)
    own = case.score[plants[-1]]
    for splits in (None, 1, 3):
        for T in (0.999, own, np.nextafter(own, np.float32(np.inf)), -2.0):
            case.check(T, "D = 2048", splits=splits)
    assert case.want(-2.0)[3] == 17 * 130 and case.want(0.999)[3] >= 1


def test_digit_edges_and_nan_coordinate():
    """fixed-point values whose digits carry, borrow, change sign or sit at a range end, and a NaN coordinate (the device takes it
    as 0): only reachable at the ops level, CodeIndex refuses such a query"""
    import sgic_amd  # noqa
    rng = np.random.default_rng(13)
    db = np.concatenate([ref.quantised_unit_codes(rng, 80, 64), rng.integers(0, 256, (20, 64), dtype=np.uint8)])
    q = ref.random_unit(rng, 3, 64)
    q[1] = np.resize(np.array(ref.EDGE_Q, dtype=np.float64) / ref.SCALE, 64).astype(np.float32)
    q[1, 40] = np.nan
    assert ref.quantise(q)[1, 40] == 0                  # 0x7F7F7F is past the clamp and becomes 2^22
    assert set(np.clip(ref.EDGE_Q, -ref.SCALE, ref.SCALE).tolist()) <= set(ref.quantise(q)[1].tolist())
    case = _Dev(q, db)
    for splits in (None, 1):
        case.check(-2.0, "digit edges", splits=splits)
    assert case.want(-2.0)[3] == 300


@pytest.mark.parametrize("dim,nq,n", [(64, 40, 1000), (512, 40, 1000), (192, 17, 65), (64, 1, 1)])
def test_dense_emission_every_pair_once(dim, nq, n):
    """T = -2: every lane of every wave emits in every step, masked rows and queries included; each (q, d) exactly once"""
    rng = np.random.default_rng(dim + n)
    case = _Dev(ref.random_unit(rng, nq, dim), ref.quantised_unit_codes(rng, n, dim))
    for splits in (None, 1, 3):
        hq, hd, hs, count = case.got(-2.0, splits=splits)
        assert count == nq * n
        assert np.array_equal(hq, np.repeat(np.arange(nq, dtype=np.int32), n)) and np.array_equal(hd, np.tile(np.arange(n, dtype=np.int32), nq))
        assert np.array_equal(hs.view(np.uint32), case.score.reshape(-1).view(np.uint32))


def test_overflow_count_exact_nothing_past_capacity():
    import sgic_amd  # noqa
    from sgic_amd import ops
    rng = np.random.default_rng(20)
    case = _Dev(ref.random_unit(rng, 40, 64), ref.quantised_unit_codes(rng, 1000, 64))
    T = 0.25                                           # D = 64: scores of random pairs spread with sigma 1/8, two sigma pass
    wq, wd, ws, total = case.want(T)
    assert 100 < total < 5000
    members = {(a, b): v for a, b, v in zip(wq.tolist(), wd.tolist(), ws.view(np.uint32).tolist())}
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for capacity in (37, 64, total):
        pad = 4096                                     # canaries behind the `capacity` entries the call may write
        bq = torch.full((capacity + pad,), -7, dtype=torch.int32, device=DEV)
        bd = torch.full((capacity + pad,), -7, dtype=torch.int32, device=DEV)
        bs = torch.full((capacity + pad,), -7.0, dtype=torch.float32, device=DEV)
        count.zero_()
        ops.search_codes_range_f32q_launch(case.q, case.db, case.r_db, T, None, capacity, count, bq, bd, bs)
        assert int(count.item()) == total
        assert bool((bq[capacity:] == -7).all()) and bool((bd[capacity:] == -7).all()) and bool((bs[capacity:] == -7.0).all())
        gq, gd, gs = bq[:capacity].cpu().numpy(), bd[:capacity].cpu().numpy(), bs[:capacity].cpu().numpy()
        pairs = list(zip(gq.tolist(), gd.tolist()))
        assert len(set(pairs)) == capacity             # all slots written, with distinct pairs ...
        assert all(members.get(p) == v for p, v in zip(pairs, gs.view(np.uint32).tolist()))     # ... each a true hit, its own bits
        count.zero_()                                  # count only
        ops.search_codes_range_f32q_launch(case.q, case.db, case.r_db, T, None, 0, count, None, None, None)
        assert int(count.item()) == total
    # the counter is added to, not overwritten: it still holds the last count-only call's `total`
    ops.search_codes_range_f32q_launch(case.q, case.db, case.r_db, T, 3, 0, count, None, None, None)
    assert int(count.item()) == 2 * total
    # the wrapper launches once more with exactly `count` entries and returns the full sorted set
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
    case = _Dev(ref.random_unit(rng, 5, 64), ref.quantised_unit_codes(rng, 70, 64))
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):                  # a NaN reaches the library only past the wrapper: refused there too
        ops.search_codes_range_f32q_launch(case.q, case.db, case.r_db, float("nan"), None, 0, count, None, None, None)
    with pytest.raises(ValueError):
        case.got(float("inf"))
    for dim in (96, 2112):                             # D % 64, D > 2048
        qd, dbd = _up(ref.random_unit(rng, 5, dim)), _up(rng.integers(0, 256, (70, dim), dtype=np.uint8))
        with pytest.raises(RuntimeError):
            ops.search_codes_range_f32q_launch(qd, dbd, case.r_db, 0.9, None, 0, count, None, None, None)
    assert int(count.item()) == 0


def test_consistent_with_the_top_k_search():
    """every (idx, score) of search_codes_f32q(k = 10) with score >= T is in the range result with the same score bits"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    rng = np.random.default_rng(22)
    q, db, _ = _planted_case(rng, 20, 3000, 512)
    case = _Dev(q, db)
    s, i = ops.search_codes_f32q(case.q, case.db, case.r_db, 10)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    T = 0.12                                           # D = 512: sigma 0.044, a few random pairs per query pass as well
    hq, hd, hs, count = case.got(T)
    found = {(a, b): v for a, b, v in zip(hq.tolist(), hd.tolist(), hs.view(np.uint32).tolist())}
    kept = 0
    for r in range(20):
        for idx, sc in zip(i[r].tolist(), s[r]):
            if sc >= np.float32(T):
                assert found.get((r, idx)) == int(sc.view(np.uint32)), (r, idx)
                kept += 1
    assert 5 <= kept <= count


def test_code_index_range_search_vectors():
    import sgic_amd  # noqa
    from sgic_amd.search import CodeIndex, codes_to_unit
    rng = np.random.default_rng(30)
    db = ref.quantised_unit_codes(rng, 300, 512)
    db[200] = db[10]
    ci = CodeIndex(db, [str(j) for j in range(300)])
    q = np.concatenate([codes_to_unit(db[10:11]), ref.random_unit(rng, 2, 512)])
    for T in (0.999, 0.1, -2.0):
        want = rref.range_search(q, db, T)
        for form in (q, torch.from_numpy(q), torch.from_numpy(q).to(DEV)):
            lims, s, idx = ci.range_search_vectors(form, T)
            assert lims.dtype == np.int64 and lims.shape == (4,) and lims[0] == 0 and lims[-1] == s.size == idx.size
            assert s.dtype == np.float32 and idx.dtype == np.int32
            assert np.array_equal(lims, want[0]) and np.array_equal(idx, want[2]) and np.array_equal(s.view(np.uint32), want[1].view(np.uint32))
            assert all(np.all(np.diff(idx[lims[j]:lims[j + 1]]) > 0) for j in range(3))
    lims, s, idx = ci.range_search_vectors(q, 0.999)
    assert lims.tolist() == [0, 2, 2, 2] and idx.tolist() == [10, 200]       # two queries with zero hits
    lims, s, idx = ci.range_search_vectors(q[1], 0.999)                      # one vector, no hit at all
    assert lims.tolist() == [0, 0] and s.shape == (0,) and idx.shape == (0,)
    with pytest.raises(ValueError, match="900"):
        ci.range_search_vectors(q, -2.0, max_pairs=899)
    with pytest.raises(ValueError):
        ci.range_search_vectors(torch.from_numpy(2 * q).to(DEV), 0.5)


# ---------------------------------------------------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def cli_index(tmp_path_factory):
    """an index directory built from 40 synthetic containers of dim 64, the width of the TINY towers (`--small`)"""
    import sgic_amd  # noqa
    from sgic_amd import search
    from sgic_amd.filemaker import pack_c2df
    from sgic_amd.zstd import Compressor
    root = tmp_path_factory.mktemp("range_vec_cli")
    rng = np.random.default_rng(11)
    codes = ref.quantised_unit_codes(rng, 40, 64)
    src = root / "c2df"
    src.mkdir()
    zc = Compressor(3)
    for j in range(40):
        enc = {"clip_stream": zc.compress(codes[j].tobytes()), "clip_meta": {"model_id": "m", "dim": 64}}
        (src / f"im{j:02d}.c2df").write_bytes(pack_c2df(enc, {"version": 2}))
    ids = [str(src / f"im{j:02d}.c2df") for j in range(40)]
    out = root / "index"
    assert search.main(["build", "--c2df_dir", str(src), "--index_dir", str(out)]) == 0
    return root, out, codes, ids


def _spy(monkeypatch, name):
    """records the vector handed to CodeIndex.<name>, which then runs as it is"""
    from sgic_amd.search import CodeIndex
    seen = []
    real = getattr(CodeIndex, name)

    def spy(self, q, *a, **kw):
        seen.append(np.array(q.cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float32, copy=True))
        return real(self, q, *a, **kw)

    monkeypatch.setattr(CodeIndex, name, spy)
    return seen


def _by_score(ids, hd, hs):
    order = np.lexsort((hd, -hs))
    return [{"path": ids[i], "score": float(v)} for i, v in zip(hd[order], hs[order])]


def _cli_threshold_and_top_k(argv, cli_index, capsys, monkeypatch):
    from sgic_amd import search
    _, out, codes, ids = cli_index
    ranged, topped = _spy(monkeypatch, "range_search_vectors"), _spy(monkeypatch, "search_vectors")
    capsys.readouterr()
    T = 0.05                                            # D = 64: sigma 1/8, about a third of the 40 rows pass
    assert search.main(argv + ["--min_score", str(T), "--topk", "1"]) == 0
    got = json.loads(capsys.readouterr().out)
    assert len(ranged) == 1 and ranged[0].shape == (1, 64) and not topped
    _, hd, hs, count = rref.range_hits(ranged[0], codes, T)
    assert 1 < count < 40                               # more than --topk 1, fewer than all
    assert got == _by_score(ids, hd, hs) and len(got) == count
    assert [e["score"] for e in got] == sorted((e["score"] for e in got), reverse=True)
    with pytest.raises(ValueError, match=str(count)):   # a larger count than --max_pairs names it
        search.main(argv + ["--min_score", str(T), "--max_pairs", str(count - 1)])
    capsys.readouterr()
    assert search.main(argv + ["--topk", "5"]) == 0     # without the flag: the top k of search_vectors, as before
    text = capsys.readouterr().out
    assert len(topped) == 1 and np.array_equal(topped[0], ranged[0])
    ws, wi = ref.search(topped[0], codes, 5)
    assert text == json.dumps([{"path": ids[i], "score": float(v)} for i, v in zip(wi[0], ws[0])], ensure_ascii=False, indent=2) + "\n"


def test_cli_query_text_min_score(cli_index, capsys, monkeypatch):
    argv = ["query-text", "--codes", "--small", "--index_dir", str(cli_index[1]), "--text", "a dog", "--token_ids", TINY_TOKENS]
    _cli_threshold_and_top_k(argv, cli_index, capsys, monkeypatch)


def test_cli_query_image_min_score(cli_index, capsys, monkeypatch):
    from PIL import Image
    from sgic_amd.data import synth_images
    png = cli_index[0] / "query.png"
    x = synth_images(1, 256, 256, 77)[0, :, :96, :128]
    Image.fromarray(((x * 0.5 + 0.5) * 255).round().byte().permute(1, 2, 0).numpy()).save(png)
    argv = ["query-image", "--codes", "--small", "--index_dir", str(cli_index[1]), "--image", str(png)]
    _cli_threshold_and_top_k(argv, cli_index, capsys, monkeypatch)


# ------------------------------------------------------------------------------------------------------------ service
def _png(h, w, seed):
    from PIL import Image
    from sgic_amd.data import synth_images
    x = synth_images(1, 256 * ((h + 255) // 256), 256 * ((w + 255) // 256), seed)[0, :, :h, :w]
    buf = io.BytesIO()
    Image.fromarray(((x * 0.5 + 0.5) * 255).round().byte().permute(1, 2, 0).numpy()).save(buf, format="PNG")
    return buf.getvalue()


@pytest.fixture(scope="module")
def svc(tmp_path_factory):
    import sgic_amd  # noqa
    from sgic_amd import compress, search
    from sgic_amd.service import ResidentService
    root = tmp_path_factory.mktemp("range_vec_svc")
    src = root / "imgs"
    src.mkdir()
    for i in range(6):
        (src / f"im{i}.png").write_bytes(_png(256, 256, 900 + i))
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(root / "out"), "--small", "--batch_size", "4"]) == 0
    index = root / "index"
    ci = search.build_index(root / "out" / "bitstreams", index, log=lambda *_: None)
    kw = dict(small=True, index_dir=str(index), preview_cache=str(root / "previews"), media_roots=[str(root)])
    return ResidentService(code_index=True, **kw), ResidentService(**kw), root, ci


def _lines(it):
    return [json.loads(ln) for ln in b"".join(it).decode().splitlines()]


def _timeless(ev):
    return [{k: v for k, v in e.items() if k != "elapsed_ms"} for e in ev]


def _check_stream(ev, start, want_items):
    assert ev[0] == dict({"type": "meta", "stage": "start"}, **start)
    assert ev[1]["type"] == "meta" and ev[1]["stage"] == "searched" and ev[1]["count"] == len(want_items)
    assert [(e["path"], e["score"]) for e in ev[2:-1]] == [(w["path"], w["score"]) for w in want_items]
    assert all(e["type"] == "item" and "preview_url" in e for e in ev[2:-1]) and ev[-1]["type"] == "done"


def test_service_min_score_streams(svc, monkeypatch):
    s, plain, root, ci = svc
    c2df = root / "out" / "bitstreams" / "im3.c2df"
    row = ci.ids.index(str(c2df))
    # c2df stream: the embedded u8 code through the u8 range kernel; T = the third best score of the restatement keeps three rows
    _, score = cref.keys_and_scores(ci.codes[row:row + 1], ci.codes)
    T = float(np.sort(score[0])[-3])
    _, hd, hs, count = crref.range_hits(ci.codes[row:row + 1], ci.codes, T)
    assert 3 <= count <= 6
    ev = _lines(s.search_c2df("im3.c2df", c2df.read_bytes(), topk=1, min_score=T))
    _check_stream(ev, {"query_type": "c2df", "filename": "im3.c2df", "topk": 1, "min_score": T}, _by_score(ci.ids, hd, hs))
    assert ev[2]["path"] == str(c2df)
    # text stream: the restatement on exactly the vector the service's own tower produced
    seen = _spy(monkeypatch, "range_search_vectors")
    for T in (0.0, -2.0):
        ev = _lines(s.search_text({"text": "a dog", "topk": 2, "token_ids": TINY_TOKENS, "min_score": T}))
        _, hd, hs, count = rref.range_hits(seen[-1], ci.codes, T)
        _check_stream(ev, {"query_type": "text", "query": "a dog", "topk": 2, "min_score": T}, _by_score(ci.ids, hd, hs))
    assert count == 6 and len(seen) == 2 and seen[0].shape == (1, ci.dim)
    # image stream: the uploaded image of corpus item 2 scores (nearly) 1 against its own code, nothing else passes 0.99
    ev = _lines(s.search_image("q.png", (root / "imgs" / "im2.png").read_bytes(), topk=5, min_score=0.99))
    _, hd, hs, _ = rref.range_hits(seen[-1], ci.codes, 0.99)
    _check_stream(ev, {"query_type": "image", "filename": "q.png", "topk": 5, "min_score": 0.99}, _by_score(ci.ids, hd, hs))
    assert len(seen) == 3 and os.path.basename(ev[2]["path"]) == "im2.c2df"
    # in-band errors: a non-finite value, a count above the service's cap
    for bad in (float("nan"), float("inf"), "high"):
        ev = _lines(s.search_c2df("im3.c2df", c2df.read_bytes(), min_score=bad))
        assert [e["type"] for e in ev] == ["meta", "error"] and ("min_score" in ev[1]["detail"] or "float" in ev[1]["detail"])
    assert len(seen) == 3
    monkeypatch.setattr(type(s), "MAX_RANGE_HITS", 4)
    ev = _lines(s.search_text({"text": "a dog", "token_ids": TINY_TOKENS, "min_score": -2.0}))
    assert [e["type"] for e in ev] == ["meta", "error"] and "6" in ev[1]["detail"] and "max_pairs = 4" in ev[1]["detail"]


def test_service_min_score_needs_the_code_index(svc):
    s, plain, root, ci = svc
    c2df = (root / "out" / "bitstreams" / "im3.c2df").read_bytes()
    tower = plain._text
    for ev in (_lines(plain.search_c2df("im3.c2df", c2df, min_score=0.5)),
               _lines(plain.search_text({"text": "a dog", "token_ids": TINY_TOKENS, "min_score": 0.5})),
               _lines(s.search_c2df("im3.c2df", c2df, min_score=0.5, index_dir=str(root / "out" / "faiss")))):   # no codes.npy there
        assert [e["type"] for e in ev] == ["meta", "error"] and ev[0]["min_score"] == 0.5 and "codes.npy" in ev[1]["detail"]
    assert plain._text is tower                         # refused before the query is made: no text tower was built for it


def test_service_without_min_score_is_unchanged(svc):
    """the lines of today: no new key in the start line, the top k of the same kernels as before"""
    s, plain, root, ci = svc
    c2df = root / "out" / "bitstreams" / "im3.c2df"
    row = ci.ids.index(str(c2df))
    for service in (s, plain):
        ev = _lines(service.search_c2df("im3.c2df", c2df.read_bytes(), topk=4))
        assert ev[0] == {"type": "meta", "stage": "start", "query_type": "c2df", "filename": "im3.c2df", "topk": 4}
        assert [e["type"] for e in ev] == ["meta", "meta"] + ["item"] * 4 + ["done"] and set(ev[1]) == {"type", "stage", "count", "elapsed_ms"}
        assert _timeless(ev) == _timeless(_lines(service.search_c2df("im3.c2df", c2df.read_bytes(), topk=4, min_score=None)))
        ev = _lines(service.search_text({"text": "a dog", "topk": 2, "token_ids": TINY_TOKENS}))
        assert ev[0] == {"type": "meta", "stage": "start", "query_type": "text", "query": "a dog", "topk": 2}
        assert _timeless(ev) == _timeless(_lines(service.search_text({"text": "a dog", "topk": 2, "token_ids": TINY_TOKENS, "min_score": None})))
    ev = _lines(s.search_c2df("im3.c2df", c2df.read_bytes(), topk=4))
    ws, wi = cref.search(ci.codes[row:row + 1], ci.codes, 4)
    assert [(e["path"], e["score"]) for e in ev[2:-1]] == [(ci.ids[i], float(v)) for i, v in zip(wi[0], ws[0])]


def test_http_adapter_passes_min_score(svc):
    """the stdlib handler hands the `min_score` query field (c2df, image) and body key (text) to the service; driven with in-memory
    request / response files, as tests/test_gpu_service.py drives it"""
    from sgic_amd.service import http_handler
    s, plain, root, ci = svc
    H = http_handler(s)
    c2df = (root / "out" / "bitstreams" / "im3.c2df").read_bytes()

    class _Sock:
        def __init__(self, data):
            self.r, self.w = io.BytesIO(data), io.BytesIO()

        def makefile(self, mode, *a, **k):
            return self.r if "r" in mode else self.w

        def sendall(self, b):
            self.w.write(b)

    def post(url, ctype, body):
        sock = _Sock(b"POST " + url.encode() + b" HTTP/1.1\r\nHost: x\r\nContent-Type: " + ctype + b"\r\nContent-Length: "
                     + str(len(body)).encode() + b"\r\n\r\n" + body)
        h = H.__new__(H)
        h.request, h.client_address, h.server = sock, ("127.0.0.1", 0), None
        h.rfile, h.wfile = sock.r, sock.w
        h.handle_one_request()
        head, _, payload = sock.w.getvalue().partition(b"\r\n\r\n")
        assert b" 200" in head.splitlines()[0] and b"application/x-ndjson" in head
        return [json.loads(ln) for ln in payload.decode().splitlines()]

    form = b"--BOUND\r\nContent-Disposition: form-data; name=\"file\"; filename=\"im3.c2df\"\r\n\r\n" + c2df + b"\r\n--BOUND--\r\n"
    ev = post("/search/stream/c2df?topk=1&min_score=-2", b"multipart/form-data; boundary=BOUND", form)
    assert ev[0]["min_score"] == -2.0 and ev[1]["count"] == len(ci) and ev[-1]["type"] == "done"
    assert _timeless(ev) == _timeless(_lines(s.search_c2df("im3.c2df", c2df, topk=1, min_score=-2.0)))
    ev = post("/search/stream/c2df?topk=1&min_score=nan", b"multipart/form-data; boundary=BOUND", form)
    assert [e["type"] for e in ev] == ["meta", "error"] and ev[0]["min_score"] == "nan"
    ev = post("/search/stream/c2df?topk=2", b"multipart/form-data; boundary=BOUND", form)          # no field: the top k, no new key
    assert "min_score" not in ev[0] and ev[1]["count"] == 2
    body = json.dumps({"text": "a dog", "topk": 1, "token_ids": TINY_TOKENS, "min_score": -2.0}).encode()
    ev = post("/search/stream/text", b"application/json", body)
    assert ev[0]["min_score"] == -2.0 and ev[1]["count"] == len(ci) and ev[-1]["type"] == "done"
