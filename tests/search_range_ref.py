"""numpy restatement of the threshold (range) search over u8 codes (csrc/search.hip search_range_kernel, ops.search_codes_range,
sgic_amd.search.CodeIndex.range_search / duplicate_pairs / duplicate_groups), built on search_codes_ref.keys_and_scores.

A pair (q, d) is a hit iff score(q, d) >= float32(T), score being the fp32 value the top-k search reports, (float32(N) * r_d) * r_q.
Hits are listed by (q, d) ascending.  The self-join keeps the upper triangle d > q of the index against itself."""
import numpy as np

import search_codes_ref as ref


def range_hits(q, db, threshold, self_join=False):
    """-> (q int32, d int32, score fp32, count), sorted by (q, d)"""
    _, score = ref.keys_and_scores(q, db)
    hit = score >= np.float32(threshold)
    if self_join:
        assert q.shape == db.shape
        hit &= np.triu(np.ones(hit.shape, dtype=bool), 1)
    hq, hd = np.nonzero(hit)                      # row-major: (q, d) ascending
    return hq.astype(np.int32), hd.astype(np.int32), score[hq, hd], int(hq.size)


def range_search(q, db, threshold):
    """the FAISS shape: (lims (nq + 1,) int64, scores, indices)"""
    hq, hd, hs, _ = range_hits(q, db, threshold)
    lims = np.zeros(q.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(hq, minlength=q.shape[0]), out=lims[1:])
    return lims, hs, hd


def groups(i, j):
    """connected components with at least two members, members ascending, groups ordered by first member (union-find)"""
    parent = {}

    def find(a):
        while parent.setdefault(a, a) != a:
            a = parent[a]
        return a

    for a, b in zip(i, j):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[rb] = ra
    comp = {}
    for a in parent:
        comp.setdefault(find(a), []).append(a)
    return sorted((sorted(g) for g in comp.values() if len(g) > 1), key=lambda g: g[0])


def nudged(rng, row, count):
    """a copy of a code row with `count` distinct codes moved by +-1 (away from the u8 range's ends)"""
    out = row.copy()
    pos = rng.choice(row.size, size=count, replace=False)
    step = rng.choice(np.array([-1, 1]), size=count)
    step = np.where(out[pos] == 0, 1, np.where(out[pos] == 255, -1, step))
    out[pos] = (out[pos].astype(np.int64) + step).astype(np.uint8)
    return out
