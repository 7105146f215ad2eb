"""numpy restatement of the threshold (range) search of fp32 queries over u8 codes (csrc/search.hip search_range_kernel with F32Query,
ops.search_codes_range_f32q, sgic_amd.search.CodeIndex.range_search_vectors), built on search_vectors_ref.keys_and_scores.

A pair (q, d) is a hit iff score(q, d) >= float32(T), score being the fp32 value the top-k search of fp32 queries reports,
(float32(M) * r_d) * 2^-22.  Hits are listed by (q, d) ascending."""
import numpy as np

import search_vectors_ref as ref


def hits_of(score, threshold):
    """the hits of a ready score matrix -> (q int32, d int32, score fp32, count), sorted by (q, d)"""
    hq, hd = np.nonzero(score >= np.float32(threshold))       # row-major: (q, d) ascending
    return hq.astype(np.int32), hd.astype(np.int32), score[hq, hd], int(hq.size)


def range_hits(q, db, threshold):
    return hits_of(ref.keys_and_scores(q, db)[1], threshold)


def range_search(q, db, threshold):
    """the FAISS shape: (lims (nq + 1,) int64, scores, indices)"""
    hq, hd, hs, _ = range_hits(q, db, threshold)
    lims = np.zeros(np.atleast_2d(q).shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(hq, minlength=lims.size - 1), out=lims[1:])
    return lims, hs, hd
