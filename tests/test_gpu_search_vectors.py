"""GPU: fp32 text / image queries against the u8 code index (csrc/search.hip search_topk_kernel with F32Query through
ops.search_codes_f32q / CodeIndex.search_vectors / the CLI / ResidentService) against the numpy restatement (tests/search_vectors_ref.py).  Ids and scores
are compared bit for bit everywhere; only the cross-check against the fp32 path has tolerances, those of that path's own 10k test,
plus the derived bound against fp64."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as cref  # noqa: E402
import search_vectors_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOKENS = "49406,320,3055,49407"


def _gpu(q, db, k, splits=None):
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    s, i = ops.search_codes_f32q(up(np.asarray(q, dtype=np.float32)), up(db), up(code_rnorm(db)), k, splits=splits)
    return s.cpu().numpy(), i.cpu().numpy()


def _same(got, want, what):
    (gs, gi), (ws, wi) = got, want
    assert gi.dtype == np.int32 and gs.dtype == np.float32 and gi.shape == wi.shape and gs.shape == ws.shape, what
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:4].tolist())
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, np.argwhere(gs != ws)[:4].tolist())


def _check(q, db, k, what, splits=None):
    _same(_gpu(q, db, k, splits), ref.search(q, db, k), (what, k, splits))


def _unit_of(codes):
    import sgic_amd  # noqa
    from sgic_amd.search import codes_to_unit
    return codes_to_unit(codes)


@pytest.mark.parametrize("dim", [64, 512, 2048])
@pytest.mark.parametrize("n", [1, 17, 1000])
def test_random_unit_queries_bit_equal(dim, n):
    rng = np.random.default_rng(1000 * dim + n)
    db = ref.quantised_unit_codes(rng, n, dim)
    ids = np.arange(n)
    for nq in (1, 5, 33):
        q = ref.random_unit(rng, nq, dim)
        q[0] = _unit_of(db[n // 2])                         # one query that is in the database
        key, score = ref.keys_and_scores(q, db)
        order = np.stack([np.lexsort((ids, -key[r])) for r in range(nq)])
        assert order[0, 0] == n // 2
        for k in sorted({1, min(10, n), min(128, n)}):
            want = (np.take_along_axis(score, order[:, :k], axis=1), order[:, :k].astype(np.int32))
            _same(_gpu(q, db, k), want, (dim, n, nq, k))


def test_every_score_compared_n100_k100():
    rng = np.random.default_rng(21)
    db = ref.quantised_unit_codes(rng, 100, 512)
    for nq in (5, 33):
        _check(ref.random_unit(rng, nq, 512), db, 100, ("all", nq))


@pytest.mark.parametrize("nq", [17, 33])
def test_three_steps_one_load_per_round_wide_tile(nq):
    """D = 192: three 64-byte steps, not a multiple of eight, so one load per round (U = 1) with more than one step, under the
    32-query tile -- the query fragment index (f * steps + step) of fragment f = 1 in each plane.  nq = 17 / 33: one full and one
    partial wide tile, two full and one partial; n = 65: a one-row tail tile, which splits = 2 makes a split of its own"""
    rng = np.random.default_rng(192 + nq)
    db = ref.quantised_unit_codes(rng, 65, 192)
    q = ref.random_unit(rng, nq, 192)
    q[nq - 1] = _unit_of(db[64])
    for k in (1, 10):
        want = ref.search(q, db, k)
        assert want[1][nq - 1, 0] == 64
        for splits in (1, 2):
            _same(_gpu(q, db, k, splits), want, ("D = 192", nq, k, splits))


def test_plane_placement_one_hot_queries_asymmetric_database():
    """query 16 b + i holds 256^b * 2^-22 at coordinate p_i and 0 elsewhere: digit plane b is 1 there and every other digit of every
    plane is 0, so M(16 b + i, j) = 256^b (2 c[j][p_i] - 255).  A swapped plane, a wrong plane weight or a lane-map error of either
    MFMA operand gives a wrong integer, the database being asymmetric in (row, coordinate)"""
    dim, n = 512, 48
    pos = (np.arange(16) * 37 + 5) % dim
    q = np.zeros((48, dim), np.float32)
    for b, val in enumerate((2.0 ** -22, 2.0 ** -14, 2.0 ** -6)):
        q[16 * b + np.arange(16), pos] = val
    j, c = np.meshgrid(np.arange(n), np.arange(dim), indexing="ij")
    db = ((7 * j * j + 3 * c + 11 * j * c + (c >> 4)) % 256).astype(np.uint8)
    Q = ref.quantise(q)
    planes = ref.digits(Q)
    for b in range(3):
        for p in range(3):
            blk = planes[p][16 * b:16 * b + 16]
            assert blk.sum() == (16 if p == b else 0) and np.abs(blk).sum() == (16 if p == b else 0)
    v = 2 * db.astype(np.int64) - 255
    want = np.concatenate([256 ** b * v[:, pos].T for b in range(3)])
    assert np.array_equal(ref.int_scores(Q, db), want)
    _check(q, db, n, "planes, 32-query tiles")
    for b in range(3):
        _check(q[16 * b:16 * b + 16], db, n, ("plane", b))
    _check(q[30:33], db, n, "planes, 3 queries")


def test_carries_and_signs():
    """coordinates hold Q * 2^-22 for the Q whose digits carry, borrow or sit at a range end (0x7F7F7F is past the clamp and becomes
    2^22); all other coordinates are zero; an all-zero query gives equal keys everywhere"""
    dim = 512
    rng = np.random.default_rng(22)
    edge = np.array(ref.EDGE_Q, dtype=np.float64) * 2.0 ** -22
    at = (np.arange(len(edge)) * 37 + 11) % dim
    q = np.zeros((6, dim), np.float32)
    q[0, at] = edge
    q[1, at] = -edge
    q[2, (at + 3) % dim] = edge * np.where(np.arange(len(edge)) % 2, -1.0, 1.0)
    q[3, at[::-1]] = edge
    q[4] = np.resize(edge, dim) * np.where(np.arange(dim) % 3, 1.0, -1.0)       # every coordinate an edge value
    assert np.array_equal(ref.quantise(q[:1])[0, at], np.clip(ref.EDGE_Q, -ref.SCALE, ref.SCALE))
    db = np.concatenate([rng.integers(0, 256, (60, dim), dtype=np.uint8), ref.quantised_unit_codes(rng, 40, dim)])
    _check(q, db, 100, "carries")
    s, i = _gpu(q, db, 10)
    assert i[5].tolist() == list(range(10)) and not s[5].any()


def test_magnitude_needs_int64():
    dim = 2048
    rng = np.random.default_rng(23)
    alt = np.tile(np.array([0, 255], dtype=np.uint8), dim // 2)
    db = np.concatenate([np.stack([np.zeros(dim, np.uint8), np.full(dim, 255, np.uint8), alt, alt[::-1]]),
                         ref.quantised_unit_codes(rng, 13, dim)])
    sign = np.where(np.arange(dim) % 2, -1.0, 1.0)
    q = np.stack([np.ones(dim), -np.ones(dim), sign, -sign]).astype(np.float32)
    big = ref.int_scores(ref.quantise(q), db)
    assert np.abs(big).max() == ref.SCALE * 255 * dim > 2 ** 31
    assert big[0, 1] == -big[0, 0] == big[2, 3] == -big[2, 2] == ref.SCALE * 255 * dim
    _check(q, db, db.shape[0], "magnitude")
    _check(q, db, 3, "magnitude")


def test_ties_across_tile_and_split_boundaries():
    """exact duplicates on both sides of a 16-row tile boundary, of a 64-row block step and of the split boundaries that
    splits = 3 (384 rows each) and splits = 7 (192 rows each) give on n = 1000: equal keys resolve to the lower index"""
    rng = np.random.default_rng(5)
    db = ref.quantised_unit_codes(rng, 1000, 512)
    dup = [15, 16, 63, 64, 191, 192, 383, 384, 999]
    db[dup] = db[15]
    q = np.concatenate([_unit_of(db[15:16]), ref.random_unit(rng, 4, 512)])
    for splits in (1, 3, 7, None):
        for k in (12, 128):
            s, i = _gpu(q, db, k, splits)
            assert i[0, :len(dup)].tolist() == dup, (splits, k)
            _same((s, i), ref.search(q, db, k), (splits, k))


def test_identical_rows_return_first_ids():
    rng = np.random.default_rng(6)
    row = ref.quantised_unit_codes(rng, 1, 512)
    db = np.repeat(row, 300, axis=0)
    q = np.concatenate([_unit_of(row), ref.random_unit(rng, 2, 512)])
    for splits in (1, 3):
        s, i = _gpu(q, db, 10, splits)
        assert np.array_equal(i, np.tile(np.arange(10, dtype=np.int32), (3, 1))), splits
        _same((s, i), ref.search(q, db, 10), splits)


def test_one_hot_query_many_equal_keys():
    """rows that are permutations of one row share r_d, so a one-hot query ranks them by a single code: at most 256 distinct keys
    over 1000 rows"""
    rng = np.random.default_rng(24)
    row = ref.quantised_unit_codes(rng, 1, 512)[0]
    db = np.stack([rng.permutation(row) for _ in range(1000)])
    q = np.zeros((2, 512), np.float32)
    q[0, 5] = 1.0
    q[1, 300] = -1.0
    key, _ = ref.keys_and_scores(q, db)
    assert len(np.unique(key[0])) <= 256 and len(np.unique(key[0, np.argsort(-key[0])[:128]])) < 64
    for splits in (1, 7, None):
        _check(q, db, 128, "one-hot", splits)
        _check(q, db, 10, "one-hot", splits)


@pytest.mark.parametrize("k", [10, 128])
def test_threshold_filter_worst_cases(k):
    """rows ordered by ascending score for query 0: every row beats the running k-th best, so the candidate buffer fills and is
    pruned at every step; descending: nothing after the first k passes"""
    rng = np.random.default_rng(7)
    db = ref.quantised_unit_codes(rng, 4096, 512)
    q = ref.random_unit(rng, 3, 512)
    key, _ = ref.keys_and_scores(q[:1], db)
    asc = db[np.argsort(key[0], kind="stable")]
    for name, rows in (("ascending", asc), ("descending", asc[::-1].copy())):
        want = ref.search(q, rows, k)
        for splits in (1, None):
            _same(_gpu(q, rows, k, splits), want, (name, k, splits))


def test_unsupported_shapes_raise():
    rng = np.random.default_rng(8)
    db = ref.quantised_unit_codes(rng, 300, 512)
    q = ref.random_unit(rng, 2, 512)
    with pytest.raises(RuntimeError):
        _gpu(q, db, 129)
    with pytest.raises(RuntimeError):
        _gpu(ref.random_unit(rng, 2, 96), rng.integers(0, 256, (300, 96), dtype=np.uint8), 5)
    with pytest.raises(RuntimeError):
        _gpu(ref.random_unit(rng, 2, 4096), rng.integers(0, 256, (300, 4096), dtype=np.uint8), 5)
    _check(q, db, 128, "largest k")
    _check(ref.random_unit(rng, 2, 2048), ref.quantised_unit_codes(rng, 300, 2048), 128, "largest D and k")


def test_cross_check_with_fp32_path_10k():
    """the path that serves these queries today on the same vectors: search_gpu(q, codes_to_unit(db)); scores within 1e-5, ids equal
    except where the fp64 scores of the swapped entries differ by less than 1e-6 (test_cross_check_with_fp32_path_10k of the u8
    search); and the derived bound against fp64"""
    import sgic_amd  # noqa
    from sgic_amd import search
    rng = np.random.default_rng(9)
    db = ref.quantised_unit_codes(rng, 10000, 512)
    db[4321] = db[1234]
    udb = search.codes_to_unit(db)
    q = np.concatenate([udb[[1234, 17, 9999]], ref.random_unit(rng, 13, 512)])
    s, i = _gpu(q, db, 10)
    _same((s, i), ref.search(q, db, 10), "10k")
    s32, i32 = search.search_gpu(q, udb, 10)
    full = q.astype(np.float64) @ udb.astype(np.float64).T
    exact = ref.fp64_scores(q, db)
    assert i[0, 0] == 1234 and i[0, 1] == 4321 and i[1, 0] == 17 and i[2, 0] == 9999
    for r in range(q.shape[0]):
        if not np.array_equal(i[r], i32[r]):
            assert np.abs(np.sort(full[r, i[r]])[::-1] - np.sort(full[r, i32[r]])[::-1]).max() < 1e-6, r
        assert np.abs(s[r].astype(np.float64) - full[r, i[r]]).max() <= 1e-5 and np.abs(s[r] - s32[r]).max() <= 1e-5, r
        assert np.abs(s[r].astype(np.float64) - exact[r, i[r]]).max() <= ref.error_bound(512), r


def test_no_score_matrix_in_device_memory():
    """n = 100 000, nq = 256, k = 10: the call may allocate less than half of what the (nq, n) fp32 score matrix alone takes"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    rng = np.random.default_rng(10)
    n, nq, k = 100000, 256, 10
    db = rng.integers(0, 256, (n, 512), dtype=np.uint8)
    q = ref.random_unit(rng, nq, 512)
    dq, ddb, rdb = torch.from_numpy(q).to(DEV), torch.from_numpy(db).to(DEV), torch.from_numpy(code_rnorm(db)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    s, i = ops.search_codes_f32q(dq, ddb, rdb, k)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < nq * n * 4 // 2, rise
    rows = [0, 15, 16, 31, 32, 255]
    _same((s.cpu().numpy()[rows], i.cpu().numpy()[rows]), ref.search(q[rows], db, k), "100k")


def test_search_vectors_takes_host_and_device_queries():
    import sgic_amd  # noqa
    from sgic_amd.search import CodeIndex
    rng = np.random.default_rng(25)
    db = ref.quantised_unit_codes(rng, 300, 512)
    ci = CodeIndex(db, [str(j) for j in range(300)])
    q = ref.random_unit(rng, 3, 512)
    want = ref.search(q, db, 7)
    _same(ci.search_vectors(q, 7), want, "numpy")
    _same(ci.search_vectors(torch.from_numpy(q), 7), want, "host tensor")
    _same(ci.search_vectors(torch.from_numpy(q).to(DEV), 7), want, "device tensor")
    small = CodeIndex(db[:100], [str(j) for j in range(100)])   # k is clipped to n, and n <= 128 is within the kernel's limit
    _same(small.search_vectors(q[0], 500), ref.search(q[:1], db[:100], 100), "one vector, k clipped to n")
    with pytest.raises(RuntimeError):                            # clipped to n = 300 > 128: refused, not truncated
        ci.search_vectors(q[0], 500)
    with pytest.raises(ValueError):
        ci.search_vectors(torch.from_numpy(2 * q).to(DEV), 7)


# ---------------------------------------------------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def cli_index(tmp_path_factory):
    """an index directory built from 40 synthetic containers of dim 512 (as test_cli_build_query_neighbours does)"""
    import sgic_amd  # noqa
    from sgic_amd import search
    from sgic_amd.filemaker import pack_c2df
    from sgic_amd.zstd import Compressor
    root = tmp_path_factory.mktemp("vec_cli")
    rng = np.random.default_rng(11)
    codes = ref.quantised_unit_codes(rng, 40, 512)
    src = root / "c2df"
    src.mkdir()
    zc = Compressor(3)
    for j in range(40):
        enc = {"clip_stream": zc.compress(codes[j].tobytes()), "clip_meta": {"model_id": "m", "dim": 512}}
        (src / f"im{j:02d}.c2df").write_bytes(pack_c2df(enc, {"version": 2}))
    ids = [str(src / f"im{j:02d}.c2df") for j in range(40)]
    out = root / "index"
    assert search.main(["build", "--c2df_dir", str(src), "--index_dir", str(out)]) == 0
    return root, out, codes, ids


def _spy_on_query(monkeypatch):
    """records the vector the CLI / the service hands to CodeIndex.search_vectors, which then runs as it is"""
    from sgic_amd.search import CodeIndex
    seen = []
    real = CodeIndex.search_vectors

    def spy(self, q, k):
        seen.append(np.array(q.cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float32, copy=True))
        return real(self, q, k)

    monkeypatch.setattr(CodeIndex, "search_vectors", spy)
    return seen


def _cli_pair(flagged_argv, q_expected, cli_index, capsys, monkeypatch):
    from sgic_amd import search
    _, out, codes, ids = cli_index
    seen = _spy_on_query(monkeypatch)
    capsys.readouterr()
    assert search.main(flagged_argv + ["--codes"]) == 0
    got = json.loads(capsys.readouterr().out)
    assert len(seen) == 1 and seen[0].shape == (1, 512)
    assert np.abs(seen[0] - q_expected).max() <= 1e-5               # it is the tower's vector for this input ...
    ws, wi = ref.search(seen[0], codes, 5)                          # ... and the answer is the restatement on exactly that vector
    assert got == [{"path": ids[i], "score": float(v)} for i, v in zip(wi[0], ws[0])]
    assert search.main(flagged_argv) == 0                           # the fp32 files of the same index, the route without the flag
    old = json.loads(capsys.readouterr().out)
    assert len(seen) == 1 and len(old) == 5 and old[0]["path"] == got[0]["path"]
    assert all(abs(a["score"] - b["score"]) <= 1e-5 for a, b in zip(old, got))


def test_cli_query_text_codes(cli_index, capsys, monkeypatch):
    import sgic_amd  # noqa
    from sgic_amd import search, weights as W
    from sgic_amd.clip import ClipTextHIP
    from sgic_amd.compress import load_state
    from sgic_amd.config import CLIP_B32
    model = ClipTextHIP(load_state(None, W.clip_text_spec, CLIP_B32, 4321), CLIP_B32, DEV)
    q = search.encode_text(search.tokenize("ignored", CLIP_B32.ctx, TOKENS), model)
    argv = ["query-text", "--index_dir", str(cli_index[1]), "--text", "an apple", "--token_ids", TOKENS, "--topk", "5"]
    _cli_pair(argv, q, cli_index, capsys, monkeypatch)


def test_cli_query_image_codes(cli_index, capsys, monkeypatch):
    import sgic_amd  # noqa
    from PIL import Image
    from sgic_amd import weights as W
    from sgic_amd.codec import ClipCodec
    from sgic_amd.compress import load_image, load_state
    from sgic_amd.config import CLIP_B32
    from sgic_amd.data import synth_images
    png = cli_index[0] / "query.png"
    x = synth_images(1, 256, 256, 77)[0, :, :96, :128]
    Image.fromarray(((x * 0.5 + 0.5) * 255).round().byte().permute(1, 2, 0).numpy()).save(png)
    q = ClipCodec(load_state(None, W.clip_spec, CLIP_B32, 4321), CLIP_B32, DEV).image_to_unit_vec(load_image(str(png)))[None, :]
    argv = ["query-image", "--index_dir", str(cli_index[1]), "--image", str(png), "--topk", "5"]
    _cli_pair(argv, q, cli_index, capsys, monkeypatch)


def test_cli_query_c2df_codes_route_untouched(cli_index, capsys):
    from sgic_amd import search
    _, out, codes, ids = cli_index
    assert search.main(["query-c2df", "--codes", "--index_dir", str(out), "--c2df", ids[7], "--topk", "5"]) == 0
    ws, wi = cref.search(codes[7:8], codes, 5)
    assert json.loads(capsys.readouterr().out) == [{"path": ids[i], "score": float(v)} for i, v in zip(wi[0], ws[0])]


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
    root = tmp_path_factory.mktemp("vec_svc")
    src = root / "imgs"
    src.mkdir()
    for i in range(6):
        (src / f"im{i}.png").write_bytes(_png(256, 256, 900 + i))
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(root / "out"), "--small", "--batch_size", "4"]) == 0
    index = root / "index"
    ci = search.build_index(root / "out" / "bitstreams", index, log=lambda *_: None)
    s = ResidentService(small=True, index_dir=str(index), preview_cache=str(root / "previews"), media_roots=[str(root)], code_index=True)
    return s, root, index, ci


def _items(it):
    ev = [json.loads(ln) for ln in b"".join(it).decode().splitlines()]
    assert ev[-1]["type"] == "done", ev[-1]
    return [(e["path"], e["score"]) for e in ev if e["type"] == "item"]


def test_service_code_index_streams(svc, monkeypatch):
    s, root, index, ci = svc
    seen = _spy_on_query(monkeypatch)
    got = _items(s.search_text({"text": "an apple", "topk": 4, "token_ids": TOKENS}))
    assert len(seen) == 1 and seen[0].shape == (1, ci.dim)
    from sgic_amd.search import encode_text, tokenize
    again = encode_text(tokenize("an apple", s.ccfg.ctx, TOKENS), s._text)       # the service's own text tower, same tokens
    assert np.abs(seen[0] - again).max() <= 1e-5
    ws, wi = ref.search(seen[0], ci.codes, 4)
    assert got == [(ci.ids[i], float(v)) for i, v in zip(wi[0], ws[0])]
    # image stream: fp32 vector route as well; the uploaded image of corpus item 2 retrieves item 2 first
    got = _items(s.search_image("q.png", (root / "imgs" / "im2.png").read_bytes(), topk=3))
    assert len(seen) == 2 and os.path.basename(got[0][0]) == "im2.c2df"
    ws, wi = ref.search(seen[1], ci.codes, 3)
    assert got == [(ci.ids[i], float(v)) for i, v in zip(wi[0], ws[0])]
    # c2df stream: the embedded u8 code through the u8 kernel, no fp32 vector involved
    c2df = root / "out" / "bitstreams" / "im3.c2df"
    got = _items(s.search_c2df("im3.c2df", c2df.read_bytes(), topk=4))
    row = ci.ids.index(str(c2df))
    ws, wi = cref.search(ci.codes[row:row + 1], ci.codes, 4)
    assert len(seen) == 2 and got == [(ci.ids[i], float(v)) for i, v in zip(wi[0], ws[0])] and got[0][0] == str(c2df)
    # what is resident is the u8 matrix and its reciprocal norms
    stamp, mat, ids, held = s._index[str(index.resolve())]
    assert mat.dtype == torch.uint8 and mat.is_cuda and tuple(mat.shape) == ci.codes.shape and ids == ci.ids
    assert held._dev[0] is mat and held._dev[1].dtype == torch.float32 and np.array_equal(held._dev[1].cpu().numpy(), ci.r)
    # the stamp-based reload applies: a rewritten codes.npy is picked up
    ci2 = type(ci)(ci.codes[::-1].copy(), ci.ids[::-1])
    ci2.save(index)
    got2 = _items(s.search_c2df("im3.c2df", c2df.read_bytes(), topk=4))
    assert s._index[str(index.resolve())][1] is not mat and got2[0][0] == str(c2df)
    assert np.array_equal(s._index[str(index.resolve())][1].cpu().numpy(), ci2.codes)
    ci.save(index)


def test_service_default_keeps_the_fp32_matrix(svc):
    """without code_index the resident tensor is the fp32 matrix, as before -- and so is a directory without codes.npy with it"""
    from sgic_amd.service import ResidentService
    s, root, index, ci = svc
    plain = ResidentService(small=True, index_dir=str(index), preview_cache=str(root / "previews"), media_roots=[str(root)])
    assert plain.code_index is False
    got = _items(plain.search_c2df("im3.c2df", (root / "out" / "bitstreams" / "im3.c2df").read_bytes(), topk=4))
    mat = plain._index[str(index.resolve())][1]
    assert mat.dtype == torch.float32 and tuple(mat.shape) == ci.codes.shape and os.path.basename(got[0][0]) == "im3.c2df"
    faiss_dir = root / "out" / "faiss"                              # compress.py's own index: index.faiss + ids.txt, no codes.npy
    got = _items(s.search_c2df("im3.c2df", (root / "out" / "bitstreams" / "im3.c2df").read_bytes(), topk=2, index_dir=str(faiss_dir)))
    assert s._index[str(faiss_dir.resolve())][1].dtype == torch.float32 and len(got) == 2
