"""CPU side of the fp32-query search over u8 codes: the digit identity behind the three i8 planes, the int64 combine, the derived
error bound and the ranking of the restatement (tests/search_vectors_ref.py) against fp64, the limits the library enforces before
any launch, and the argument checks of CodeIndex.search_vectors that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_vectors_ref as ref  # noqa: E402


def test_digit_identity_and_ranges():
    rng = np.random.default_rng(0)
    Q = np.concatenate([np.array(ref.EDGE_Q), -np.array(ref.EDGE_Q), rng.integers(-ref.SCALE, ref.SCALE + 1, 200000),
                        np.arange(-70000, 70000), ref.SCALE - np.arange(70000), np.arange(70000) - ref.SCALE])
    d0, d1, d2 = ref.digits(Q)
    assert np.array_equal(65536 * d2 + 256 * d1 + d0, Q)
    assert d0.min() == -128 and d0.max() == 127 and d1.min() == -128 and d1.max() == 127
    inside = np.abs(Q) <= ref.SCALE                                 # 0x7F7F7F is past the clamp: its digits fit i8 all the same
    assert d2[inside].min() == -64 and d2[inside].max() == 64 and np.abs(d2).max() == 127
    # at scale 2^23 the top digit of q = 1 would be 128, which is no i8
    assert ref.digits(np.array([2 * ref.SCALE]))[2][0] == 128
    # the named values, digit by digit
    want = {0: (0, 0, 0), 1: (1, 0, 0), -1: (-1, 0, 0), 127: (127, 0, 0), 128: (-128, 1, 0), -128: (-128, 0, 0), -129: (127, -1, 0),
            32767: (-1, -128, 1), 32768: (0, -128, 1), -32768: (0, -128, 0), -32769: (-1, -128, 0), 0x7F7F7F: (127, 127, 127),
            ref.SCALE: (0, 0, 64), -ref.SCALE: (0, 0, -64)}
    assert sorted(want) == sorted(ref.EDGE_Q)
    for q, d in want.items():
        assert tuple(int(x[0]) for x in ref.digits(np.array([q]))) == d, q


def test_quantise_rounding_clamp_and_nan():
    s = np.float32(2.0 ** -22)
    q = np.array([[0.5 * s, 1.5 * s, 2.5 * s, -0.5 * s, -1.5 * s, 1.0, -1.0, 1.5, -7.0, np.inf, -np.inf, np.nan, 0.0, 127 * s, 3e-8, -3e-8]],
                 dtype=np.float32)
    assert ref.quantise(q)[0].tolist() == [0, 2, 2, 0, -2, ref.SCALE, -ref.SCALE, ref.SCALE, -ref.SCALE, ref.SCALE, -ref.SCALE, 0, 0, 127,
                                           0, 0]


@pytest.mark.parametrize("dim", [64, 512, 2048])
def test_combine_equals_direct_product(dim):
    rng = np.random.default_rng(dim)
    Q = np.concatenate([np.full((1, dim), ref.SCALE), np.full((1, dim), -ref.SCALE), rng.integers(-ref.SCALE, ref.SCALE + 1, (6, dim)),
                        ref.quantise(ref.random_unit(rng, 6, dim))])
    Q[2, :len(ref.EDGE_Q)] = ref.EDGE_Q
    alt = np.tile(np.array([0, 255], dtype=np.uint8), dim // 2)
    db = np.concatenate([np.stack([np.zeros(dim, np.uint8), np.full(dim, 255, np.uint8), alt]),
                         rng.integers(0, 256, (9, dim), dtype=np.uint8), ref.quantised_unit_codes(rng, 9, dim)])
    direct = Q @ (2 * db.astype(np.int64) - 255).T
    assert np.array_equal(ref.int_scores(Q, db), direct)
    assert direct[0, 1] == ref.SCALE * 255 * dim and direct[0, 0] == -ref.SCALE * 255 * dim     # the bound on |M| is reached
    assert dim < 2048 or direct[0, 1] > 2 ** 31                                               # and int32 cannot hold it


@pytest.mark.parametrize("dim", [64, 512, 2048])
def test_error_bound_against_fp64(dim):
    rng = np.random.default_rng(100 + dim)
    db = np.concatenate([ref.quantised_unit_codes(rng, 1500, dim), rng.integers(0, 256, (500, dim), dtype=np.uint8)])
    q = ref.random_unit(rng, 33, dim)
    q[0] = 0.0
    q[0, 3] = 1.0                                                   # a coordinate at the end of the fixed-point range
    q[1] = np.sign(q[1]) / np.float32(np.sqrt(dim))                 # |q|_1 as large as a unit vector allows
    _, score = ref.keys_and_scores(q, db)
    err = np.abs(score.astype(np.float64) - ref.fp64_scores(q, db)).max()
    assert err <= ref.error_bound(dim), (err, ref.error_bound(dim))
    assert dim != 512 or abs(ref.error_bound(dim) - 2.94e-6) < 1e-8


@pytest.mark.parametrize("dim,seed", [(64, 1), (512, 2), (512, 3), (2048, 4)])
def test_ranking_against_fp64(dim, seed):
    """ids equal the fp64 ranking except where the fp64 scores of the swapped entries differ by less than the error bound -- and on
    these seeds nothing needs the excuse: the ids are equal"""
    rng = np.random.default_rng(seed)
    db = ref.quantised_unit_codes(rng, 2000, dim)
    q = ref.random_unit(rng, 33, dim)
    k = 10
    s, i = ref.search(q, db, k)
    full = ref.fp64_scores(q, db)
    ids = np.arange(db.shape[0])
    want = np.stack([np.lexsort((ids, -full[r]))[:k] for r in range(q.shape[0])])
    excused = 0
    for r in range(q.shape[0]):
        for j in np.flatnonzero(i[r] != want[r]):
            assert abs(full[r, i[r, j]] - full[r, want[r, j]]) < ref.error_bound(dim), (r, j)
            excused += 1
    assert excused == 0
    assert np.abs(s.astype(np.float64) - np.take_along_axis(full, want, axis=1)).max() <= ref.error_bound(dim)


def test_work_bytes_limits_through_the_library():
    import sgic_amd  # noqa
    from sgic_amd import _lib

    def plan(nq, n, dim, k, splits=0):
        used, nbytes = ctypes.c_int(-1), ctypes.c_size_t(0)
        _lib.call("sgic_search_codes_f32q_work_bytes", nq, n, dim, k, splits, ctypes.byref(used), ctypes.byref(nbytes))
        return used.value, nbytes.value

    for bad in ((4, 1000, 4096, 10), (4, 1000, 96, 10), (4, 1000, 512, 129), (4, 5, 512, 6)):
        with pytest.raises(RuntimeError):
            plan(*bad)
    used, nbytes = plan(4, 1000, 2048, 128)
    assert used >= 1 and nbytes == (4 * used * 128 * 8 if used > 1 else 0)
    assert plan(4, 1000, 512, 10, 1) == (1, 0)
    used, nbytes = plan(33, 100000, 512, 10, 7)
    assert 1 < used <= 7 and nbytes == 33 * used * 10 * 8
    # the u8 entry keeps its own limit
    used = ctypes.c_int(-1)
    _lib.call("sgic_search_codes_u8_work_bytes", 4, 1000, 4096, 10, 0, ctypes.byref(used), ctypes.byref(ctypes.c_size_t(0)))
    assert used.value >= 1


def test_search_vectors_argument_errors_need_no_device():
    import sgic_amd  # noqa
    from sgic_amd.search import CodeIndex
    rng = np.random.default_rng(5)
    ci = CodeIndex(ref.quantised_unit_codes(rng, 20, 64), [f"id{j}" for j in range(20)])
    q = ref.random_unit(rng, 3, 64)
    bad = q.copy()
    bad[1, 7] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ci.search_vectors(bad, 5)
    bad[1, 7] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ci.search_vectors(bad, 5)
    with pytest.raises(ValueError, match="unit"):
        ci.search_vectors(2.0 * q, 5)
    with pytest.raises(ValueError, match="dim"):
        ci.search_vectors(ref.random_unit(rng, 3, 128), 5)
    with pytest.raises(ValueError, match="dim"):
        ci.search_vectors(np.zeros((2, 3, 64), np.float32), 5)
    big = CodeIndex(rng.integers(0, 256, (4, 4096), dtype=np.uint8), list("abcd"))
    with pytest.raises(ValueError, match="faiss.index"):
        big.search_vectors(ref.random_unit(rng, 1, 4096), 2)
    assert ci._dev is None and big._dev is None                     # nothing was sent to a device
