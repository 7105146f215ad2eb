"""numpy restatement of the clustering over u8 codes (csrc/search.hip assign_codes_kernel / cluster_sums_kernel, ops.assign_codes,
ops.cluster_sums, sgic_amd.search.CodeIndex.assign / kmeans), built on search_vectors_ref.

Assignment: M(c, d) = int_scores(quantise(centroids), db), the integer of the fp32-query search; a row goes to the centroid with the
largest M, equal M -> the lower centroid index; its score is (float32(M) * r_d) * 2^-22.  Sums: per cluster the int64 sum of the
members' 2 code - 255 and their number.  lloyd: the loop of CodeIndex.kmeans around the two, the update step being the package's own
centroids_from_sums (host code, held to its contract by tests/test_cluster_codes_cpu.py)."""
import numpy as np

import search_vectors_ref as ref


def assign(cent, db, with_int=False):
    """-> (cluster (n,) int32, score (n,) fp32[, M (n,) int64])"""
    M = ref.int_scores(ref.quantise(np.atleast_2d(cent)), db)
    best = np.argmax(M, axis=0)                              # the first of equal maxima: the lower centroid index
    Mb = M[best, np.arange(M.shape[1])]
    score = (Mb.astype(np.float32) * ref.rnorm(db)) * np.float32(2.0 ** -22)
    return (best.astype(np.int32), score, Mb) if with_int else (best.astype(np.int32), score)


def sums(db, assign_, K):
    """-> (sums (K, D) int64, counts (K,) int64)"""
    a = np.asarray(assign_).astype(np.int64)
    assert a.min() >= 0 and a.max() < K
    order = np.argsort(a, kind="stable")
    v = 2 * np.asarray(db)[order].astype(np.int64) - 255
    ids, start = np.unique(a[order], return_index=True)
    out = np.zeros((K, v.shape[1]), dtype=np.int64)
    out[ids] = np.add.reduceat(v, start, axis=0)
    return out, np.bincount(a, minlength=K).astype(np.int64)


def lloyd(db, init, iters):
    """-> {"centroids", "assign", "score", "counts", "moved", "iters_run"}: each pass assigns, counts the rows that changed
    cluster (all of them in the first pass) and, unless none did, updates; a loop that used up `iters` ends with one more assign"""
    from sgic_amd.search import centroids_from_sums
    cent = np.array(init, dtype=np.float32, copy=True)
    k = cent.shape[0]
    previous, moved, settled = np.full(db.shape[0], -1, dtype=np.int32), [], False
    for _ in range(iters):
        a, s = assign(cent, db)
        moved.append(int((a != previous).sum()))
        if moved[-1] == 0:
            settled = True
            break
        cent = centroids_from_sums(*sums(db, a, k), cent)
        previous = a
    if not settled:
        a, s = assign(cent, db)
    return {"centroids": cent, "assign": a, "score": s, "counts": np.bincount(a, minlength=k).astype(np.int64), "moved": moved,
            "iters_run": len(moved)}


def default_init(db, k, seed):
    """the initial centroids of CodeIndex.kmeans without `init`"""
    from sgic_amd.search import codes_to_unit
    return codes_to_unit(db[np.sort(np.random.default_rng(seed).choice(db.shape[0], k, replace=False))])


def planted_corpus(rng, n, dim, k, noise=0.02):
    """k random unit directions, each row one of them plus noise (per coordinate, against 1 / sqrt(dim) of the signal), through the
    compress side's u8 quantiser -> (codes (n, dim) u8, group (n,), directions (k, dim) fp32).  Rows 0 .. k - 1 are one member of
    each group, in group order"""
    dirs = ref.random_unit(rng, k, dim)
    group = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
    v = dirs[group].astype(np.float64) + noise * rng.standard_normal((n, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.round((v * 0.5 + 0.5) * 255).astype(np.uint8), group, dirs
