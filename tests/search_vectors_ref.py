"""numpy restatement of the fp32-query search over u8 codes (csrc/search.hip search_topk_kernel with F32Query, CodeIndex.search_vectors), every
bit of it.

Query to fixed point: Q = clamp(rint(float32(q) * 2^22), -2^22, 2^22) as an integer (round to nearest even, NaN -> 0).  Balanced
base-256 digits: d0 = ((Q + 128) & 255) - 128, Q' = (Q - d0) >> 8, d1 = ((Q' + 128) & 255) - 128, d2 = (Q' - d1) >> 8, so
Q = 65536 d2 + 256 d1 + d0 with d0, d1 in [-128, 127], d2 in [-64, 64].  With a = c - 128: S_p = sum d_p a,
M = 2 (65536 S_2 + 256 S_1 + S_0) + sum Q  (== sum Q (2c - 255)) in int64, ranking key = float32(M) * r_d, reported score =
key * 2^-22.  Order: key descending, equal keys -> lower database index."""
import numpy as np

from search_codes_ref import quantised_unit_codes, rnorm  # noqa: F401

SCALE = 1 << 22
# the Q values whose digits carry or borrow, change sign or sit at a range end (both tests use them)
EDGE_Q = [0, 1, -1, 127, 128, -128, -129, 32767, 32768, -32768, -32769, 0x7F7F7F, SCALE, -SCALE]


def error_bound(dim):
    """|score - fp64(q . v / |v|)| for finite |q_j| <= 1: query rounding of at most 2^-23 per coordinate times |v|_1 / |v| <= sqrt(D),
    plus three fp32 roundings of at most 2^-24 relative on |score| <= 1, with slack"""
    return 2.0 ** -23 * np.sqrt(dim) + 2.0 ** -22


def quantise(q):
    """(nq, D) float -> Q int64"""
    t = np.asarray(q, dtype=np.float32) * np.float32(SCALE)
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.rint(np.clip(t, -SCALE, SCALE)).astype(np.int64)


def digits(Q):
    Q = np.asarray(Q, dtype=np.int64)
    d0 = ((Q + 128) & 255) - 128
    Q1 = (Q - d0) >> 8
    d1 = ((Q1 + 128) & 255) - 128
    d2 = (Q1 - d1) >> 8
    return d0, d1, d2


def int_scores(Q, db):
    """M (nq, n) int64 by the digit-plane route the kernel takes, each S_p checked against int32"""
    Q, db = np.asarray(Q, dtype=np.int64), np.asarray(db)
    planes = digits(Q)
    big = np.empty((Q.shape[0], db.shape[0]), dtype=np.int64)
    for j in range(0, db.shape[0], 8192):                   # database chunks: the int64 copy of a large corpus stays small
        a = db[j:j + 8192].astype(np.int64) - 128
        S = [d @ a.T for d in planes]
        assert max(np.abs(s).max() for s in S) < 2 ** 31
        big[:, j:j + 8192] = 2 * (65536 * S[2] + 256 * S[1] + S[0]) + Q.sum(axis=1)[:, None]
    return big


def keys_and_scores(q, db):
    key = int_scores(quantise(q), db).astype(np.float32) * rnorm(db)[None, :]
    return key, key * np.float32(2.0 ** -22)


def search(q, db, k):
    """-> (scores (nq,k) fp32, idx (nq,k) int32)"""
    key, score = keys_and_scores(q, db)
    ids = np.arange(db.shape[0])
    idx = np.stack([np.lexsort((ids, -key[r]))[:k] for r in range(key.shape[0])])
    return np.take_along_axis(score, idx, axis=1), idx.astype(np.int32)


def random_unit(rng, n, dim):
    v = rng.standard_normal((n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def fp64_scores(q, db):
    """q . v / |v| in fp64, v = 2c - 255: what the search approximates"""
    v = 2.0 * np.asarray(db).astype(np.float64) - 255.0
    return np.asarray(q).astype(np.float64) @ (v / np.linalg.norm(v, axis=1, keepdims=True)).T
