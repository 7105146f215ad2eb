"""numpy restatement of the rank-of-target sink (csrc/search.hip search_rank_kernel, CodeIndex.rank / rank_vectors), every bit.

For a query q and a target database row t, with the ranking key of the top-k searches (search_codes_ref / search_vectors_ref:
float32(N) * r_d, resp. float32(M) * r_d):
    rank(q, t)  = #{ d in [0, n) : key(q, d) > key(q, t)  or  (key(q, d) == key(q, t) and d < t) }
    score(q, t) = the score those modules report for the pair (key * r_q, resp. key * 2^-22)
i.e. the position of t in the full ordering that their `search` truncates at k."""
import numpy as np

import search_codes_ref as cref
import search_vectors_ref as vref


def rank_from_keys(key, score, targets):
    """key, score (nq, n) fp32, targets (nq,) -> (rank (nq,) int32, score (nq,) fp32)"""
    targets = np.asarray(targets, dtype=np.int64)
    rows = np.arange(key.shape[0])
    tk = key[rows, targets][:, None]
    d = np.arange(key.shape[1])[None, :]
    before = (key > tk) | ((key == tk) & (d < targets[:, None]))
    return before.sum(axis=1).astype(np.int32), score[rows, targets].astype(np.float32)


def rank_codes(q, db, targets):
    """u8 queries"""
    return rank_from_keys(*cref.keys_and_scores(q, db), targets)


def rank_vectors(q, db, targets):
    """fp32 queries"""
    return rank_from_keys(*vref.keys_and_scores(q, db), targets)
