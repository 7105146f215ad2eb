"""GPU: the rank-of-target sink of the fused code search (csrc/search.hip search_rank_kernel, both query policies, through
ops.search_codes_rank / search_codes_rank_f32q / CodeIndex.rank / rank_vectors) against the numpy restatement
(tests/search_rank_ref.py) and against the top-k kernels.  Ranks are compared as integers, scores bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as cref  # noqa: E402
import search_rank_ref as rref  # noqa: E402
import search_vectors_ref as vref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SGIC_EINVAL = -1
U8_SHAPES = [(1, 1, 64), (3, 65, 64), (17, 130, 128), (33, 1000, 512), (16, 4097, 512), (64, 20000, 512)]
F32_SHAPES = [(1, 1, 64), (5, 67, 64), (17, 1000, 512), (16, 300, 2048)]


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu_u8(q, db, targets, splits=0):
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    r, s = ops.search_codes_rank(_up(q), _up(code_rnorm(q)), _up(db), _up(code_rnorm(db)), targets, splits=splits)
    return r.cpu().numpy(), s.cpu().numpy()


def _gpu_f32(q, db, targets, splits=0):
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    r, s = ops.search_codes_rank_f32q(_up(np.asarray(q, dtype=np.float32)), _up(db), _up(code_rnorm(db)), targets, splits=splits)
    return r.cpu().numpy(), s.cpu().numpy()


def _same(got, want, what):
    (gr, gs), (wr, ws) = got, want
    assert gr.dtype == np.int32 and gs.dtype == np.float32 and gr.shape == wr.shape and gs.shape == ws.shape, what
    assert np.array_equal(gr, wr), (what, np.argwhere(gr != wr)[:4].tolist(), gr[:8].tolist(), wr[:8].tolist())
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, np.argwhere(gs != ws)[:4].tolist())


def _target_sets(rng, nq, n):
    """random targets, and every query forced to the first and to the last row"""
    return [rng.integers(0, n, nq), np.zeros(nq, dtype=np.int64), np.full(nq, n - 1, dtype=np.int64)]


def _in_topk(rank, score, topk, targets, what):
    """rank < k <=> the target is in the top-k result; then it stands at position `rank` with the same score bits"""
    s, idx = topk
    k = idx.shape[1]
    for j, t in enumerate(np.asarray(targets).tolist()):
        assert (rank[j] < k) == (t in idx[j].tolist()), (what, j, int(rank[j]))
        if rank[j] < k:
            assert idx[j, rank[j]] == t and s[j, rank[j]].view(np.uint32) == score[j].view(np.uint32), (what, j)


@pytest.mark.parametrize("nq,n,dim", U8_SHAPES)
def test_u8_restatement_splits_and_topk(nq, n, dim):
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    rng = np.random.default_rng(nq * 100003 + n)
    db = cref.quantised_unit_codes(rng, n, dim)
    q = cref.quantised_unit_codes(rng, nq, dim)
    q[0] = db[n // 2]                                                 # a query equal to a database code
    key, score = cref.keys_and_scores(q, db)
    k = min(n, 128)
    ts, ti = ops.search_codes(_up(q), _up(code_rnorm(q)), _up(db), _up(code_rnorm(db)), k)
    topk = (ts.cpu().numpy(), ti.cpu().numpy())
    for targets in _target_sets(rng, nq, n):
        want = rref.rank_from_keys(key, score, targets)
        got = _gpu_u8(q, db, targets)
        _same(got, want, (nq, n, dim, "auto"))
        _same(_gpu_u8(q, db, targets), got, "a second run")
        for splits in (1, 2, 7):
            _same(_gpu_u8(q, db, targets, splits), want, (nq, n, dim, splits))
        _in_topk(*got, topk, targets, (nq, n, dim))
    own = _gpu_u8(q[:1], db, [n // 2])
    assert own[0][0] == int((key[0] > key[0, n // 2]).sum()) and own[0][0] == 0


@pytest.mark.parametrize("nq,n,dim", F32_SHAPES)
def test_f32_restatement_splits_and_topk(nq, n, dim):
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm, codes_to_unit
    rng = np.random.default_rng(nq * 100003 + n + 1)
    db = vref.quantised_unit_codes(rng, n, dim)
    q = vref.random_unit(rng, nq, dim)
    q[0] = codes_to_unit(db[n // 2])
    key, score = vref.keys_and_scores(q, db)
    k = min(n, 128)
    ts, ti = ops.search_codes_f32q(_up(q), _up(db), _up(code_rnorm(db)), k)
    topk = (ts.cpu().numpy(), ti.cpu().numpy())
    for targets in _target_sets(rng, nq, n):
        want = rref.rank_from_keys(key, score, targets)
        got = _gpu_f32(q, db, targets)
        _same(got, want, (nq, n, dim, "auto"))
        _same(_gpu_f32(q, db, targets), got, "a second run")
        for splits in (1, 2, 7):
            _same(_gpu_f32(q, db, targets, splits), want, (nq, n, dim, splits))
        _in_topk(*got, topk, targets, (nq, n, dim))


@pytest.mark.parametrize("policy", ["u8", "f32"])
def test_ties_only_lower_copies_count(policy):
    """copies of the target row planted below and above it, across 16-row tile, 64-row step and split boundaries: exactly the
    lower ones come before it.  The query is the target's own code (its dequantised vector), so nothing else scores higher"""
    import sgic_amd  # noqa
    from sgic_amd.search import codes_to_unit
    rng = np.random.default_rng(5)
    n, dim = 1000, 512
    db = cref.quantised_unit_codes(rng, n, dim)
    dup = [15, 16, 63, 64, 191, 192, 383, 384, 999]
    db[dup] = db[15]
    q = np.repeat(db[15:16], len(dup), axis=0)
    gpu = _gpu_u8 if policy == "u8" else _gpu_f32
    qq = q if policy == "u8" else codes_to_unit(q)
    want = (rref.rank_codes if policy == "u8" else rref.rank_vectors)(qq, db, dup)
    assert want[0].tolist() == list(range(len(dup)))
    for splits in (0, 1, 3, 7):
        _same(gpu(qq, db, dup, splits), want, (policy, splits))


@pytest.mark.parametrize("policy", ["u8", "f32"])
def test_identical_rows_rank_is_the_target(policy):
    rng = np.random.default_rng(6)
    row = cref.quantised_unit_codes(rng, 1, 512)
    db = np.repeat(row, 300, axis=0)
    targets = np.array([0, 1, 15, 16, 63, 64, 65, 128, 255, 256, 299])
    if policy == "u8":
        q = cref.quantised_unit_codes(rng, len(targets), 512)
        gpu, want = _gpu_u8, rref.rank_codes(q, db, targets)
    else:
        q = vref.random_unit(rng, len(targets), 512)
        gpu, want = _gpu_f32, rref.rank_vectors(q, db, targets)
    assert want[0].tolist() == targets.tolist()
    for splits in (0, 1, 3):
        _same(gpu(q, db, targets, splits), want, (policy, splits))


def test_f32_nan_coordinate_and_plus_minus_one():
    """a NaN coordinate counts as 0 (the staging rule); a coordinate at +-1 is the end of the fixed-point range"""
    rng = np.random.default_rng(7)
    n, dim = 300, 512
    db = vref.quantised_unit_codes(rng, n, dim)
    q = np.zeros((4, dim), dtype=np.float32)
    q[0] = vref.random_unit(rng, 1, dim)[0]
    q[0, 7] = np.nan
    q[1, 100] = 1.0
    q[2, 511] = -1.0
    q[3] = vref.random_unit(rng, 1, dim)[0]
    q[3, [0, 64, 200]] = [np.nan, np.nan, 0.5]
    assert vref.quantise(q)[0, 7] == 0 and vref.quantise(q)[1, 100] == vref.SCALE and vref.quantise(q)[2, 511] == -vref.SCALE
    for targets in _target_sets(rng, 4, n):
        want = rref.rank_vectors(q, db, targets)
        for splits in (0, 2):
            _same(_gpu_f32(q, db, targets, splits), want, splits)


def test_abi_refusals_leave_the_outputs_untouched():
    import sgic_amd  # noqa
    from sgic_amd import _lib
    from sgic_amd.search import code_rnorm
    lib = _lib.lib
    rng = np.random.default_rng(8)
    n, nq, dim = 100, 3, 64
    db = cref.quantised_unit_codes(rng, n, dim)
    q = cref.quantised_unit_codes(rng, nq, dim)
    qf = _up(vref.random_unit(rng, nq, dim))
    dq, drq, ddb, drdb = _up(q), _up(code_rnorm(q)), _up(db), _up(code_rnorm(db))
    tgt = _up(np.array([0, 5, 99], dtype=np.int32))
    work = torch.zeros(64, dtype=torch.uint8, device=DEV)
    rank = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    score = torch.full((nq,), -7.0, dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)   # noqa: E731

    def u8(q=dq, rq=drq, db_=ddb, rdb=drdb, t=tgt, nq_=nq, n_=n, D=dim, splits=0, w=work, wb=64, r=rank, s=score):
        return lib.sgic_search_rank_u8(p(q), p(rq), p(db_), p(rdb), p(t), nq_, n_, D, splits, p(w), ctypes.c_size_t(wb), p(r), p(s),
                                       ctypes.c_void_p(0))

    def f32(q=qf, db_=ddb, rdb=drdb, t=tgt, nq_=nq, n_=n, D=dim, splits=0, w=work, wb=64, r=rank, s=score):
        return lib.sgic_search_rank_f32q(p(q), p(db_), p(rdb), p(t), nq_, n_, D, splits, p(w), ctypes.c_size_t(wb), p(r), p(s),
                                         ctypes.c_void_p(0))

    bad = [dict(D=96), dict(D=0), dict(D=8192), dict(nq_=0), dict(n_=0), dict(splits=4096), dict(wb=8), dict(q=None), dict(db_=None),
           dict(rdb=None), dict(t=None), dict(w=None), dict(r=None), dict(s=None)]
    for kw in bad:
        assert f32(**kw) == SGIC_EINVAL, ("f32q", kw)
        assert u8(**kw) == SGIC_EINVAL, ("u8", kw)
    assert u8(rq=None) == SGIC_EINVAL
    assert f32(D=4096) == SGIC_EINVAL                                 # fp32 queries: D <= 2048
    nbytes = ctypes.c_size_t(0)
    assert lib.sgic_search_rank_work_bytes(0, ctypes.byref(nbytes)) == SGIC_EINVAL
    assert lib.sgic_search_rank_work_bytes(nq, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * nq
    torch.cuda.synchronize()
    assert rank.cpu().tolist() == [-7] * nq and score.cpu().tolist() == [-7.0] * nq
    assert u8() == 0                                                  # the same arguments without a fault are served
    torch.cuda.synchronize()
    _same((rank.cpu().numpy(), score.cpu().numpy()), rref.rank_codes(q, db, [0, 5, 99]), "after the refusals")


def test_target_and_shape_refusals_before_a_launch():
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import CodeIndex, code_rnorm
    rng = np.random.default_rng(9)
    db = cref.quantised_unit_codes(rng, 50, 64)
    q = cref.quantised_unit_codes(rng, 3, 64)
    qv = vref.random_unit(rng, 3, 64)
    dq, drq, ddb, drdb = _up(q), _up(code_rnorm(q)), _up(db), _up(code_rnorm(db))
    for bad in ([0, 1], [0, 1, 2, 3], [0, 1, 50], [-1, 0, 0], torch.tensor([0, 1, 50], device=DEV), torch.tensor([0, 1], device=DEV)):
        with pytest.raises(ValueError):
            ops.search_codes_rank(dq, drq, ddb, drdb, bad)
        with pytest.raises(ValueError):
            ops.search_codes_rank_f32q(_up(qv), ddb, drdb, bad)
    ci = CodeIndex(db, [str(j) for j in range(50)])
    for bad in ([0, 1], [0, 1, 50], [-1, 0, 0]):
        with pytest.raises(ValueError):
            ci.rank(q, bad)
        with pytest.raises(ValueError):
            ci.rank_vectors(qv, bad)
    assert ci._dev is None
    big = CodeIndex(rng.integers(0, 256, (4, 2112), dtype=np.uint8), list("abcd"))
    with pytest.raises(ValueError, match="faiss.index"):
        big.rank_vectors(vref.random_unit(rng, 1, 2112), [0])
    assert big._dev is None
    _same(big.rank(big.codes[:2], [1, 3]), rref.rank_codes(big.codes[:2], big.codes, [1, 3]), "u8 queries at D = 2112")


def test_code_index_rank_host_and_device_queries():
    import sgic_amd  # noqa
    from sgic_amd.search import CodeIndex
    rng = np.random.default_rng(10)
    db = cref.quantised_unit_codes(rng, 300, 512)
    ci = CodeIndex(db, [str(j) for j in range(300)])
    q = cref.quantised_unit_codes(rng, 5, 512)
    qv = vref.random_unit(rng, 5, 512)
    targets = [0, 299, 17, 17, 150]
    _same(ci.rank(q, targets), rref.rank_codes(q, db, targets), "codes")
    want = rref.rank_vectors(qv, db, targets)
    _same(ci.rank_vectors(qv, np.array(targets)), want, "numpy")
    _same(ci.rank_vectors(torch.from_numpy(qv).to(DEV), targets), want, "device tensor")
    _same(ci.rank_vectors(qv[0], [299]), rref.rank_vectors(qv[:1], db, [299]), "one vector")
    s, idx = ci.search_vectors(qv, 128)
    _in_topk(*want, (s, idx), targets, "search_vectors")
    s, idx = ci.search(q, 128)
    _in_topk(*ci.rank(q, targets), (s, idx), targets, "search")
