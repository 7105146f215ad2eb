"""numpy restatement of the u8 code search (csrc/search.hip, sgic_amd.search.CodeIndex), every bit of it.

For codes c in u8^D: a = c - 128, S = sum a_q a_d, s_x = sum a_x, N = 4 S + 2 s_q + 2 s_d + D  (== sum (2c_q - 255)(2c_d - 255)),
r_x = float32(1 / sqrt(float64(sum (2c_x - 255)^2))), ranking key = float32(N) * r_d, reported score = key * r_q.  Order: key
descending, equal keys -> lower database index.  The integer part runs in int64, the float part is two fp32 multiplies."""
import numpy as np


def quantised_unit_codes(rng, n, dim):
    """what the compress side stores: random unit vectors through its u8 quantiser round((z * 0.5 + 0.5) * 255)"""
    v = rng.standard_normal((n, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.round((v * 0.5 + 0.5) * 255).astype(np.uint8)


def rnorm(codes):
    v = 2 * np.asarray(codes).astype(np.int64) - 255
    return (1.0 / np.sqrt((v * v).sum(axis=1).astype(np.float64))).astype(np.float32)


def int_scores(q, db):
    """N (nq, n) int64 by the a = c - 128 route the kernel takes; checked against the int32 bound"""
    q, db = np.asarray(q), np.asarray(db)
    dim = q.shape[1]
    aq = q.astype(np.int64) - 128
    big = np.empty((q.shape[0], db.shape[0]), dtype=np.int64)
    for j in range(0, db.shape[0], 8192):                   # database chunks: the int64 copy of a large corpus stays small
        ad = db[j:j + 8192].astype(np.int64) - 128
        big[:, j:j + 8192] = 4 * (aq @ ad.T) + 2 * aq.sum(axis=1)[:, None] + 2 * ad.sum(axis=1)[None, :] + dim
    assert np.abs(big).max() <= 255 * 255 * dim < 2 ** 31
    return big


def keys_and_scores(q, db):
    key = int_scores(q, db).astype(np.float32) * rnorm(db)[None, :]
    return key, key * rnorm(q)[:, None]


def search(q, db, k):
    """-> (scores (nq,k) fp32, idx (nq,k) int32)"""
    key, score = keys_and_scores(q, db)
    ids = np.arange(db.shape[0])
    idx = np.stack([np.lexsort((ids, -key[r]))[:k] for r in range(key.shape[0])])
    return np.take_along_axis(score, idx, axis=1), idx.astype(np.int32)
