#!/usr/bin/env python3
"""Counterpart of the reference src/search.py: query a FAISS IndexFlatIP built by compress.py.
`query-c2df` needs no CLIP model (zstd-decode the embedded u8 code, q/255*2-1, l2-normalise; search.py:20-41);
`query-image` / `query-text` run the MI355X CLIP image / text towers (clip.py).  The BPE tokenizer is open_clip's
(third-party, its vocabulary file is not in the reference tree): `query-text` uses `open_clip.get_tokenizer` when the
package is importable and otherwise takes ready-made ids via --token_ids.  The search itself is exact inner product: one fp32 MFMA GEMM (queries x
database^T) + a top-k kernel on the GPU.
`build` makes an index directory from a directory of containers (the reference's `build.py build`); besides the fp32 index it
writes the u8 codes themselves (codes.npy), which `--codes` (on all three query commands) and `neighbours` search with the fused
i8 kernels (csrc/search.hip): integer inner products, no fp32 database and no score matrix on the device.  A u8 query code is used
as it is; an fp32 text / image vector is taken to 2^-22 fixed point and searched as three i8 digit planes.
`duplicates --threshold T` lists the groups of rows whose codes score >= T against each other (a threshold search over the same
codes, each pair computed once), and `--codes --min_score T` on any of the three query commands returns every hit with score >= T
instead of the top k (`--max_pairs` bounds their number): u8 queries through the range kernel, text / image vectors through its
fp32-query sibling.
`clusters --k K` groups the code index into K themes: spherical k-means over the u8 codes (assignment on the i8 kernels' integer
score, exact integer sums per cluster, the corpus never leaving its one byte per coordinate) and one JSON line per cluster with its
representative and best members.
`build-images` (the reference's `build.py build-images`) indexes a folder of ordinary images with the CLIP tower alone: no codec, no
container.  The decoded bytes go to the tower as they are (clip.py preprocess_u8), and the index directory carries the same files
as `build`, the tower's own u8 codes included.
`recall --index_dir CORPUS --queries_dir QUERIES` measures retrieval between two index directories: every query row is paired
with the corpus row of the same file stem, the rank kernel (csrc/search.hip, search_rank_kernel) gives the position of that row
in the query's full result list, and one JSON line reports recall@k, MRR and the mean / median rank."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch


class NotSearchable(ValueError):
    """a .c2df whose embedded CLIP code is absent or inconsistent with its own metadata"""


def unit_rows(x, floor=1e-9):
    """rows scaled to unit length; a zero row stays zero instead of dividing by zero"""
    x = np.asarray(x, dtype=np.float32)
    length = np.sqrt(np.sum(x * x, axis=-1, keepdims=True))
    return x / np.maximum(length, floor)


def codes_to_unit(codes_u8):
    """inverse of the compress side's u8 quantiser (compress.py:77, `round((z*0.5+0.5)*255)`): code c -> c/255*2-1 in the
    reference's operation order (search.py:21: divide, then scale, then shift -- `c * (2/255) - 1` differs by one fp32 ulp for 111
    of the 256 codes, enough to reorder near-ties), then back onto the unit sphere (the quantiser moved the vector off it by up
    to half a step per coordinate)"""
    return unit_rows((np.asarray(codes_u8).astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0))


def embedded_clip_codes(path):
    """the u8 CLIP code a .c2df carries -- entry `clip_stream` is a zstd frame of `dim` u8 codes, `clip_meta["dim"]` says how
    many.  -> (codes (dim,) u8, container header, clip_meta)"""
    from .filemaker import unpack_c2df
    from .zstd import decompress
    entries, header = unpack_c2df(path)
    path = path if isinstance(path, (str, os.PathLike)) else "<c2df bytes>"    # unpack_c2df also takes the file's bytes
    stream, meta = entries.get("clip_stream"), entries.get("clip_meta")
    if stream is None or meta is None:
        raise NotSearchable(f"{path}: container has no embedded CLIP code (entries clip_stream / clip_meta), it cannot be used as a query")
    want = int((meta or {}).get("dim", 0) or 0)
    if want <= 0:
        raise NotSearchable(f"{path}: clip_meta carries no positive 'dim'")
    codes = np.frombuffer(decompress(stream), dtype=np.uint8)
    if codes.size != want:
        raise NotSearchable(f"{path}: clip_stream decodes to {codes.size} codes but clip_meta.dim says {want}")
    return codes, header, meta


def embedded_clip_vector(path):
    """query-c2df (search.py:20-41): the CLIP vector a .c2df carries, dequantised -> (unit vector (dim,) fp32, container header)"""
    codes, header, _ = embedded_clip_codes(path)
    return codes_to_unit(codes), header


# names of the reference script (search.py:16-41), kept so that code written against it keeps importing
l2n = unit_rows
dequantize_clip_u8 = codes_to_unit
decode_clip_from_c2df = embedded_clip_vector

# the two on-disk layouts the reference's tools produce: build.py writes (faiss.index, paths.json), compress.py writes
# (index.faiss, ids.txt) -- search.py:65-88 accepts either
_INDEX_LAYOUTS = (("faiss.index", "paths.json", lambda t: list(json.loads(t))),
                  ("index.faiss", "ids.txt", lambda t: [ln.strip() for ln in t.splitlines() if ln.strip()]))


def load_index(index_dir):
    """-> (database (n, d) fp32, doc ids [n]) from whichever layout is present in index_dir"""
    from .faiss_io import read_index_flat_ip
    root = Path(index_dir)
    for index_name, ids_name, parse in _INDEX_LAYOUTS:
        fi, fp = root / index_name, root / ids_name
        if fi.exists() and fp.exists():
            vecs, ids = read_index_flat_ip(str(fi)), parse(fp.read_text(encoding="utf-8"))
            if len(ids) != vecs.shape[0]:
                raise ValueError(f"{root}: {index_name} holds {vecs.shape[0]} vectors but {ids_name} lists {len(ids)} ids")
            return vecs, ids
    raise FileNotFoundError(f"no FAISS index in {root}: expected " + " or ".join(f"{a} + {b}" for a, b, _ in _INDEX_LAYOUTS))


def tokenize(text, ctx=77, token_ids=None):
    """search.py:93-94 `tokenizer([query])` -> (1, ctx) int64.  open_clip's tokenizer when available; `token_ids`
    (already BPE-encoded, <start> ... <end>) is the offline route."""
    if token_ids is not None:
        ids = [int(t) for t in (token_ids.split(",") if isinstance(token_ids, str) else token_ids)]
        if not 0 < len(ids) <= ctx:
            raise ValueError(f"need 1..{ctx} token ids, got {len(ids)}")
        out = np.zeros((1, ctx), dtype=np.int64)
        out[0, :len(ids)] = ids
        return out
    try:
        import open_clip
    except ImportError as e:
        raise RuntimeError("query-text needs open_clip's BPE tokenizer (pip package open_clip_torch) or --token_ids") from e
    return np.asarray(open_clip.get_tokenizer("ViT-B-32")([text]), dtype=np.int64)


def encode_text(tokens, text_model):
    """search.py:92-97 encode_text: unit-norm (1, D) fp32 on the host"""
    return text_model.encode_text(tokens).cpu().numpy().astype("float32")


def search_gpu(q, vecs, topk, device="cuda:0"):
    """exact IndexFlatIP.search on the GPU: -> (scores (nq,k), ids (nq,k))"""
    from . import ops
    dev = torch.device(device)
    k = max(1, min(topk, vecs.shape[0]))
    dq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    db = torch.from_numpy(np.ascontiguousarray(vecs, dtype=np.float32)).to(dev)
    scores = ops.gemm(dq, db, w_const=False)
    s, i = ops.topk_rows(scores, k)
    return s.cpu().numpy(), i.cpu().numpy()


def do_search(q, vecs, paths, topk=10):
    sim, ids = search_gpu(q, vecs, topk)
    return [(paths[i], float(sim[0, j])) for j, i in enumerate(ids[0]) if i != -1]


def code_rnorm(codes, chunk=1 << 16):
    """r = float32(1 / sqrt(float64(sum (2c - 255)^2))) per row of u8 codes (n, D): the reciprocal length of the dequantised
    vector, computed here on the host (the device multiplies by it and never takes a root).  Every 2c - 255 is odd, so the sum is
    at least D and never 0."""
    codes = np.asarray(codes)
    assert codes.dtype == np.uint8 and codes.ndim == 2
    r = np.empty(codes.shape[0], dtype=np.float32)
    for i in range(0, codes.shape[0], chunk):
        v = 2 * codes[i:i + chunk].astype(np.int64) - 255
        r[i:i + chunk] = (1.0 / np.sqrt((v * v).sum(axis=1).astype(np.float64))).astype(np.float32)
    return r


def finite_threshold(threshold, what="threshold"):
    """a score threshold as a float; NaN and the infinities are refused here, before anything is loaded or launched"""
    t = float(threshold)
    if not np.isfinite(t):
        raise ValueError(f"{what} must be a finite score, got {t}")
    return t


def duplicate_groups(i, j):
    """connected components, with at least two members, of the graph whose edges are the pairs (i[e], j[e]): union-find on the
    host -> [[row, ...], ...], members in index order, groups ordered by their first member"""
    parent = {}

    def find(a):
        root = a
        while parent.setdefault(root, root) != root:
            root = parent[root]
        while parent[a] != root:       # path compression
            parent[a], a = root, parent[a]
        return root

    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)      # the root is the component's lowest row
    groups = {}
    for a in sorted(parent):
        groups.setdefault(find(a), []).append(a)
    return [g for _, g in sorted(groups.items()) if len(g) > 1]


MAX_CLUSTERS = 65536     # sgic_assign_codes_f32c's limit on K


def centroids_from_sums(sums, counts, previous):
    """the update step of the spherical k-means over the codes: sums (K, D) int64, the exact sum of the members' dequantised
    integer vectors 2c - 255 (ops.cluster_sums), counts (K,), previous (K, D) fp32 -> (K, D) fp32 unit rows,
    float32(s / sqrt(sum s^2)) with s in float64.  A cluster without members, or whose sum is all zero, keeps its previous row"""
    s = np.asarray(sums).astype(np.float64)
    out = np.array(previous, dtype=np.float32, copy=True)
    if s.shape != out.shape or np.asarray(counts).shape != (s.shape[0],):
        raise ValueError(f"sums {s.shape}, counts {np.asarray(counts).shape} and previous centroids {out.shape} do not match")
    length = np.sqrt((s * s).sum(axis=1))
    live = (np.asarray(counts) > 0) & (length > 0)
    out[live] = (s[live] / length[live, None]).astype(np.float32)
    return out


def cluster_report(assign, score):
    """the clusters of an assignment as the `clusters` command lists them: assign (n,) cluster ids, score (n,) fp32, each row's
    score against its own centroid -> [{"cluster", "size", "representative", "members"}] for the non-empty clusters.  `members`:
    the cluster's rows, score descending (the fp32 bits), equal scores -> the lower row; `representative`: the first of them.
    Clusters by size descending, equal sizes -> the lower cluster index"""
    assign, score = np.asarray(assign), np.asarray(score, dtype=np.float32)
    if assign.ndim != 1 or assign.shape != score.shape:
        raise ValueError(f"assign {assign.shape} and score {score.shape} must be two vectors of one length")
    order = np.lexsort((np.arange(assign.size), -score, assign))       # by cluster, then score descending, then row
    ids, start, size = np.unique(assign[order], return_index=True, return_counts=True)
    out = []
    for j in np.lexsort((ids, -size)):
        rows = order[start[j]:start[j] + size[j]]
        out.append({"cluster": int(ids[j]), "size": int(size[j]), "representative": int(rows[0]), "members": rows.astype(np.int64)})
    return out


def retrieval_summary(rank, score, ks=(1, 5, 10)):
    """what a set of target ranks says about retrieval, in fp64: rank (nq,) the 0-based position of each query's target in the
    full result list (CodeIndex.rank), score (nq,) the pairs' scores -> {"queries", "recall@k" for every k of ks, "mrr",
    "mean_rank", "median_rank", "mean_score"}.  recall@k: the share of rank < k; mrr: the mean of 1 / (rank + 1); the median of
    an even count is the mean of the two middle ranks.  No queries: "queries" is 0 and everything else None"""
    rank, score = np.asarray(rank).reshape(-1), np.asarray(score).reshape(-1)
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError(f"recall@k needs k >= 1, got {ks}")
    if rank.shape != score.shape:
        raise ValueError(f"{rank.size} ranks and {score.size} scores")
    if rank.size and int(rank.min()) < 0:
        raise ValueError(f"ranks are positions >= 0, got {int(rank.min())}")
    out = {"queries": int(rank.size)}
    r = rank.astype(np.float64)
    for k in ks:
        out[f"recall@{k}"] = float(np.mean(rank < k)) if rank.size else None
    out["mrr"] = float(np.mean(1.0 / (r + 1.0))) if rank.size else None
    out["mean_rank"] = float(np.mean(r)) if rank.size else None
    out["median_rank"] = float(np.median(r)) if rank.size else None
    out["mean_score"] = float(np.mean(score.astype(np.float64))) if rank.size else None
    return out


def pair_by_stem(query_ids, corpus_ids):
    """the pairing of `recall`: a query row belongs to the corpus row whose id has the same file stem (the name without
    directories and without its last extension) -> (query rows int64, target rows int64, unmatched query count).  Two corpus ids
    with one stem would make the target ambiguous: a ValueError that names them"""
    rows = {}
    for j, cid in enumerate(corpus_ids):
        stem = Path(cid).stem
        if stem in rows:
            raise ValueError(f"corpus ids {corpus_ids[rows[stem]]!r} and {cid!r} share the stem {stem!r}: the target of a query of that name is ambiguous")
        rows[stem] = j
    qrows, targets = [], []
    for i, qid in enumerate(query_ids):
        j = rows.get(Path(qid).stem)
        if j is not None:
            qrows.append(i)
            targets.append(j)
    return np.asarray(qrows, dtype=np.int64), np.asarray(targets, dtype=np.int64), len(query_ids) - len(qrows)


class CodeIndex:
    """an index of the u8 CLIP codes themselves: `codes` (n, D) u8, `ids` [n].  Searched with the fused i8 kernel
    (ops.search_codes) for u8 query codes and with its fp32-query sibling (ops.search_codes_f32q) for text / image vectors: scores
    are the cosine of the dequantised vectors, 1 byte per coordinate on the device."""
    MAX_DIM_F32Q = 2048     # three query digit planes have to fit the LDS (csrc/search.hip)
    MAX_QUERY_NORM = 1.0 + 1e-3

    def __init__(self, codes, ids, model_id=None):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        if self.codes.ndim != 2 or self.codes.shape[0] != len(ids):
            raise ValueError(f"codes {self.codes.shape} do not match {len(ids)} ids")
        self.ids = list(ids)
        self.model_id = model_id
        self.r = code_rnorm(self.codes)
        self._dev = None

    @property
    def dim(self):
        return int(self.codes.shape[1])

    def __len__(self):
        return self.codes.shape[0]

    @classmethod
    def from_c2df_dir(cls, c2df_dir, log=print):
        """every searchable *.c2df under c2df_dir (recursive, sorted); unreadable or unsearchable files are skipped with a line"""
        paths = sorted(Path(c2df_dir).glob("**/*.c2df"))
        if not paths:
            raise RuntimeError(f"no .c2df under {c2df_dir}")
        rows, keep, model_id = [], [], None
        for p in paths:
            try:
                codes, _, meta = embedded_clip_codes(p)
            except Exception as e:   # NotSearchable, or a file that is not a container at all
                log(f"[SKIP] {p.name}: {e}")
                continue
            if rows and codes.size != rows[0].size:
                raise ValueError(f"{p}: code of dim {codes.size} in an index of dim {rows[0].size}")
            rows.append(codes)
            keep.append(str(p))
            if model_id is None and meta.get("model_id"):
                model_id = meta["model_id"]
        if not rows:
            raise RuntimeError(f"no searchable .c2df under {c2df_dir}")
        return cls(np.stack(rows), keep, model_id)

    def save(self, index_dir):
        root = Path(index_dir)
        root.mkdir(parents=True, exist_ok=True)
        np.save(root / "codes.npy", self.codes)
        (root / "ids.txt").write_text("\n".join(self.ids), encoding="utf-8")

    @classmethod
    def load(cls, index_dir):
        root = Path(index_dir)
        if not (root / "codes.npy").exists() or not (root / "ids.txt").exists():
            raise FileNotFoundError(f"no code index in {root}: expected codes.npy + ids.txt (sub-command `build`)")
        ids = [ln.strip() for ln in (root / "ids.txt").read_text(encoding="utf-8").splitlines() if ln.strip()]
        return cls(np.load(root / "codes.npy"), ids)

    def to(self, device="cuda:0"):
        dev = torch.device(device)
        self._dev = (torch.from_numpy(self.codes).to(dev), torch.from_numpy(self.r).to(dev))
        return self

    def search(self, q_codes, k):
        """q_codes (nq, D) u8 -> (scores (nq,k) fp32, indices (nq,k) int32), one fused launch for all queries"""
        from . import ops
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        q = np.ascontiguousarray(np.atleast_2d(q_codes), dtype=np.uint8)
        if q.shape[1] != self.dim:
            raise ValueError(f"query codes of dim {q.shape[1]} against an index of dim {self.dim}")
        k = max(1, min(int(k), len(self)))
        s, i = ops.search_codes(torch.from_numpy(q).to(db.device), torch.from_numpy(code_rnorm(q)).to(db.device), db, r_db, k)
        return s.cpu().numpy(), i.cpu().numpy()

    def _unit_queries(self, q, what):
        """the input checks of the fp32-query searches, all before anything is loaded or launched -> (nq, D) fp32 tensor, on
        whichever side it came from"""
        if self.dim > self.MAX_DIM_F32Q:
            raise ValueError(f"fp32 queries against a code index need dim <= {self.MAX_DIM_F32Q}, this one has {self.dim}: use the fp32 "
                             "index files (faiss.index + paths.json or index.faiss + ids.txt), i.e. the query without --codes")
        t = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.atleast_2d(np.asarray(q, dtype=np.float32)))
        t = (t[None, :] if t.ndim == 1 else t).to(torch.float32)
        if t.ndim != 2 or t.shape[1] != self.dim:
            raise ValueError(f"query vectors of shape {tuple(t.shape)} against an index of dim {self.dim}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("query vectors hold non-finite values")
        longest = float(t.double().norm(dim=1).max()) if t.shape[0] else 0.0
        if longest > self.MAX_QUERY_NORM:
            raise ValueError(f"query of l2 norm {longest:.6g}: {what} takes unit vectors (norm <= {self.MAX_QUERY_NORM})")
        return t

    def search_vectors(self, q, k):
        """q (nq, D) fp32 unit vectors (text / image queries), numpy or a tensor on either side -> (scores (nq,k) fp32, indices
        (nq,k) int32), one fused launch.  Refused: non-finite values, a row longer than 1 + 1e-3 (not a unit query: the fixed-point
        range is [-1, 1]), another dim, and an index of dim > 2048, which only the fp32 files can serve"""
        from . import ops
        t = self._unit_queries(q, "search_vectors")
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        k = max(1, min(int(k), len(self)))
        s, i = ops.search_codes_f32q(t.to(db.device).contiguous(), db, r_db, k)
        return s.cpu().numpy(), i.cpu().numpy()

    def _targets(self, targets, nq):
        """one row of the index per query, checked on the host before anything is loaded or launched -> (nq,) int32"""
        t = np.asarray(targets)
        if t.ndim != 1 or t.shape[0] != nq or not (np.issubdtype(t.dtype, np.integer) or t.size == 0):
            raise ValueError(f"targets of shape {t.shape} ({t.dtype}) for {nq} queries: one integer row index per query is needed")
        if t.size and (int(t.min()) < 0 or int(t.max()) >= len(self)):
            raise ValueError(f"targets span [{int(t.min())}, {int(t.max())}], outside the {len(self)} rows of the index")
        return t.astype(np.int32)

    def rank(self, q_codes, targets):
        """where each query's target row stands in the full result list of `search`: q_codes (nq, D) u8, targets (nq,) rows of
        the index -> (rank (nq,) int32, score (nq,) fp32).  rank = the number of rows `search` orders before the target (higher
        score key, or the same key and a lower index), so rank < k exactly when the target is among the k results; score = the
        bits `search` reports for the pair.  One fused launch over all rows (ops.search_codes_rank), no top-k limit"""
        from . import ops
        q = np.ascontiguousarray(np.atleast_2d(q_codes), dtype=np.uint8)
        if q.shape[1] != self.dim:
            raise ValueError(f"query codes of dim {q.shape[1]} against an index of dim {self.dim}")
        t = self._targets(targets, q.shape[0])
        if q.shape[0] == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        r, s = ops.search_codes_rank(torch.from_numpy(q).to(db.device), torch.from_numpy(code_rnorm(q)).to(db.device), db, r_db, t)
        return r.cpu().numpy(), s.cpu().numpy()

    def rank_vectors(self, q, targets):
        """`rank` for fp32 unit queries: q as for search_vectors (and refused like there), the order and the score bits those of
        `search_vectors` -> (rank (nq,) int32, score (nq,) fp32)"""
        from . import ops
        v = self._unit_queries(q, "rank_vectors")
        t = self._targets(targets, v.shape[0])
        if v.shape[0] == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        r, s = ops.search_codes_rank_f32q(v.to(db.device).contiguous(), db, r_db, t)
        return r.cpu().numpy(), s.cpu().numpy()

    def range_search_vectors(self, q, threshold, max_pairs=None):
        """every database row whose score against an fp32 unit query is >= threshold (fp32, the bits `search_vectors` reports), the
        FAISS range_search shape: q as for search_vectors -> (lims (nq + 1,) int64, scores fp32, indices int32); query j owns
        lims[j]:lims[j + 1], database index ascending.  One fused launch (ops.search_codes_range_f32q), no top-k and no limit on
        the hits per query.  Refused, before anything is loaded or launched: what search_vectors refuses and a non-finite threshold;
        more than max_pairs hits is a ValueError naming the count"""
        from . import ops
        thr = finite_threshold(threshold)
        t = self._unit_queries(q, "range_search_vectors")
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        hq, hd, hs, _ = ops.search_codes_range_f32q(t.to(db.device).contiguous(), db, r_db, thr, max_pairs=max_pairs)
        lims = np.zeros(t.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(hq.cpu().numpy(), minlength=t.shape[0]), out=lims[1:])
        return lims, hs.cpu().numpy(), hd.cpu().numpy()

    def assign(self, centroids):
        """which of the centroids each row of the index belongs to: centroids (K, D) fp32 unit rows, numpy or a tensor on either
        side -> (cluster (n,) int32, score (n,) fp32), the centroid with the highest score per row (equal scores -> the lower
        centroid) and that score, the bits `search_vectors` reports for the pair.  One fused launch (ops.assign_codes), no score
        matrix.  Refused, before anything is loaded or launched: what search_vectors refuses, and more than 65536 centroids"""
        c, s = self._assign_device(self._centroids(centroids, "assign"))
        return c.cpu().numpy(), s.cpu().numpy()

    def _centroids(self, centroids, what):
        t = self._unit_queries(centroids, what)
        if not 1 <= t.shape[0] <= MAX_CLUSTERS:
            raise ValueError(f"{what} takes 1 .. {MAX_CLUSTERS} centroids, got {t.shape[0]}")
        return t

    def _assign_device(self, t):
        from . import ops
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        return ops.assign_codes(t.to(db.device).contiguous(), db, r_db)

    def kmeans(self, k, iters=10, seed=0, init=None):
        """spherical k-means (Lloyd) over the codes, the corpus staying on the device as u8: each iteration assigns every row to its
        best centroid (ops.assign_codes), sums each cluster's members exactly in integers (ops.cluster_sums) and normalises the sums
        on the host (centroids_from_sums).  Initial centroids: `init` (k, D) fp32 unit rows, else the dequantised codes of
        default_rng(seed).choice(n, k, replace=False), sorted.  The loop ends after `iters` iterations or at the first assignment
        pass that moves no row; otherwise one more pass assigns the rows to the last update, so `assign` and `score` always belong
        to the returned centroids.  -> {"centroids" (k, D) fp32, "assign" (n,) int32, "score" (n,) fp32, "counts" (k,) int64,
        "moved": rows that changed cluster in each pass of the loop (the first pass moves all n), "iters_run": those passes}.
        Refused before anything is loaded or launched: k < 1, k > n, k > 65536, iters < 1, and what `assign` refuses of `init`"""
        k, iters, n = int(k), int(iters), len(self)
        if not 1 <= k <= min(n, MAX_CLUSTERS):
            raise ValueError(f"kmeans needs 1 <= k <= min(rows, {MAX_CLUSTERS}), got k = {k} for {n} rows")
        if iters < 1:
            raise ValueError(f"kmeans needs iters >= 1, got {iters}")
        if init is None:
            init = codes_to_unit(self.codes[np.sort(np.random.default_rng(seed).choice(n, k, replace=False))])
        cent_t = self._centroids(init, "kmeans")
        if cent_t.shape[0] != k:
            raise ValueError(f"init holds {cent_t.shape[0]} centroids, k = {k}")
        cent = cent_t.cpu().numpy()
        from . import ops
        if self._dev is None:
            self.to()
        db = self._dev[0]
        previous, moved, settled = torch.full((n,), -1, dtype=torch.int32, device=db.device), [], False
        for _ in range(iters):
            assign, score = self._assign_device(torch.from_numpy(cent))
            moved.append(int((assign != previous).sum().item()))
            if moved[-1] == 0:
                settled = True
                break
            sums, counts = ops.cluster_sums(db, assign, k)
            cent = centroids_from_sums(sums.cpu().numpy(), counts.cpu().numpy(), cent)
            previous = assign
        if not settled:
            assign, score = self._assign_device(torch.from_numpy(cent))
        assign = assign.cpu().numpy()
        return {"centroids": cent, "assign": assign, "score": score.cpu().numpy(),
                "counts": np.bincount(assign, minlength=k).astype(np.int64), "moved": moved, "iters_run": len(moved)}

    def range_search(self, q_codes, threshold, max_pairs=None):
        """every database row whose score against a query is >= threshold (fp32, the bits `search` reports), the FAISS range_search
        shape: q_codes (nq, D) u8 -> (lims (nq + 1,) int64, scores fp32, indices int32); query j owns lims[j]:lims[j + 1], database
        index ascending.  One fused launch (ops.search_codes_range), no top-k and no limit on the hits per query"""
        from . import ops
        t = finite_threshold(threshold)
        q = np.ascontiguousarray(np.atleast_2d(q_codes), dtype=np.uint8)
        if q.shape[1] != self.dim:
            raise ValueError(f"query codes of dim {q.shape[1]} against an index of dim {self.dim}")
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        hq, hd, hs, _ = ops.search_codes_range(torch.from_numpy(q).to(db.device), torch.from_numpy(code_rnorm(q)).to(db.device), db, r_db, t,
                                               max_pairs=max_pairs)
        lims = np.zeros(q.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(hq.cpu().numpy(), minlength=q.shape[0]), out=lims[1:])
        return lims, hs.cpu().numpy(), hd.cpu().numpy()

    def duplicate_pairs(self, threshold, max_pairs=1 << 24):
        """every pair of rows i < j of the index whose score is >= threshold -> (i int32, j int32, score fp32), sorted by (i, j).
        The self-join mode of the range kernel: each pair is computed once, the half below the diagonal not at all.  More than
        max_pairs pairs is a ValueError naming the count (a threshold that low describes the corpus, not its duplicates)"""
        from . import ops
        t = finite_threshold(threshold)
        if self._dev is None:
            self.to()
        db, r_db = self._dev
        hi, hj, hs, _ = ops.search_codes_range(db, r_db, db, r_db, t, self_join=True, max_pairs=max_pairs)
        return hi.cpu().numpy(), hj.cpu().numpy(), hs.cpu().numpy()

    def duplicate_groups(self, threshold, max_pairs=1 << 24, with_pairs=False):
        """the connected components (>= 2 rows) of the graph of duplicate_pairs(threshold): [[row, ...], ...], members in index
        order, groups ordered by first member; with_pairs: -> (groups, (i, j, score))"""
        i, j, s = self.duplicate_pairs(threshold, max_pairs)
        groups = duplicate_groups(i, j)
        return (groups, (i, j, s)) if with_pairs else groups

    def neighbours(self, topk, chunk=4096):
        """k-NN graph of the index over itself, own id removed: yields (row, [(neighbour row, score)] of length <= topk), queries in
        chunks so that host and device memory stay bounded"""
        k1 = min(int(topk) + 1, len(self))
        for c0 in range(0, len(self), chunk):
            s, idx = self.search(self.codes[c0:c0 + chunk], k1)
            for j in range(idx.shape[0]):
                row = [(int(i), float(v)) for i, v in zip(idx[j], s[j]) if i != c0 + j]
                yield c0 + j, row[:max(k1 - 1, 0)]   # own id absent from the list (duplicates ranked above it): drop the last


def build_index(c2df_dir, index_dir, log=print):
    """`build`: containers -> index directory.  codes.npy (u8) for the code search; the fp32 IndexFlatIP of the dequantised unit
    vectors in both layouts load_index accepts (faiss.index + paths.json, index.faiss + ids.txt); meta.json {dim, model_id}"""
    from .faiss_io import write_index_flat_ip
    ci = CodeIndex.from_c2df_dir(c2df_dir, log)
    root = Path(index_dir)
    ci.save(root)
    unit = codes_to_unit(ci.codes)
    write_index_flat_ip(str(root / "faiss.index"), unit)
    write_index_flat_ip(str(root / "index.faiss"), unit)
    (root / "paths.json").write_text(json.dumps(ci.ids, ensure_ascii=False, indent=2), encoding="utf-8")
    (root / "meta.json").write_text(json.dumps({"dim": ci.dim, "model_id": ci.model_id}, ensure_ascii=False, indent=2), encoding="utf-8")
    log(f"[OK] index of {len(ci)} containers, dim {ci.dim}, in {root}")
    return ci


IMAGE_EXTS = ("jpg", "jpeg", "png", "webp", "bmp")     # the reference's default --exts (build.py:265)
_ONE_TOWER = "ViT-B-32"


def list_images(image_dir, exts=None):
    """every file under image_dir (recursive) with one of the extensions, case-insensitive (build.py:173-181), SORTED: the
    reference keeps rglob's order, which is the file system's"""
    want = {"." + e.strip().lower().lstrip(".") for e in (exts or IMAGE_EXTS) if e.strip()}
    return sorted(p for p in Path(image_dir).rglob("*") if p.is_file() and p.suffix.lower() in want)


def select_images(files, limit=None, desired=None, random_pick=False, seed=None):
    """build.py:218-224: target = desired if desired and desired > 0 else limit; with 0 < target <= len(files) a
    random.Random(seed).sample of that many when random_pick, else the first target files; otherwise all of them"""
    import random
    files = list(files)
    target = desired if (desired is not None and desired > 0) else limit
    if target is not None and 0 < target <= len(files):
        return random.Random(seed).sample(files, target) if random_pick else files[:target]
    return files


def build_index_from_images(image_dir, index_dir, clip_ckpt=None, small=False, batch_size=32, exts=None, limit=None, random_pick=False,
                            seed=None, desired=None, device="cuda:0", log=print):
    """`build-images`: a folder of ordinary images -> index directory, with the CLIP tower alone (no Codec is built, no codec weights are
    loaded).  Files are listed sorted and selected as the reference does (select_images); a selected file whose size header cannot be
    read is skipped with a line, one whose pixels fail to decode later ends the run with an error naming it (the reference skips
    both; compress.py here does the same as this).  Batches come from the compress driver's ingest (ShardLoader, GPU JPEG decode, one
    batch ahead); the u8 canvas goes straight to ClipCodec.u8_to_codes.  Writes what `build` writes: faiss.index + paths.json +
    meta.json, index.faiss + ids.txt, and codes.npy -- the tower's own u8 output, row for row.  -> the record that is also printed."""
    import time
    from . import ops
    from . import weights as W
    from .codec import ClipCodec
    from .compress import load_state
    from .config import CLIP_B32, CLIP_TINY
    from .faiss_io import write_index_flat_ip
    from .ingest import DeviceIngest, ShardLoader, image_size
    t_start = time.perf_counter()
    image_dir, root = Path(image_dir), Path(index_dir)
    listed = list_images(image_dir, exts)
    if not listed:
        raise RuntimeError(f"There is no image in {image_dir}")
    picked = select_images(listed, limit, desired, random_pick, seed)
    t_hdr = time.perf_counter()

    def header(p):
        try:
            image_size(p)
        except Exception as e:   # noqa: BLE001 -- not an image, truncated header, ...
            return str(e)
        return None

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, max(2, os.cpu_count() or 4))) as pool:      # the pool size of ShardLoader's own pass
        why = list(pool.map(header, picked))
    for p, e in zip(picked, why):
        if e is not None:
            log(f"[SKIP] {p.name}: {e}")
    files = [str(p) for p, e in zip(picked, why) if e is None]
    header_ms = (time.perf_counter() - t_hdr) * 1e3
    if not files:
        raise RuntimeError(f"no readable image among the {len(listed)} files of {image_dir}")
    log(f"[INFO] Using {len(files)} images to build the index")

    dev = torch.device(device)
    torch.cuda.set_device(dev)
    ccfg = CLIP_TINY if small else CLIP_B32
    csd = load_state(clip_ckpt, W.clip_spec, ccfg, 4321)
    if clip_ckpt and not any(k.startswith("clip.") for k in csd):
        csd = {f"clip.{k}": v for k, v in csd.items()}
    clipc = ClipCodec(csd, ccfg, dev)
    D, n = ccfg.embed_dim, len(files)
    unit, codes = np.zeros((n, D), dtype=np.float32), np.zeros((n, D), dtype=np.uint8)
    ingest = DeviceIngest(dev)
    host_ms, gpu_evs = {}, []
    # pinned once: pinning is a device-synchronising allocation (a batch never holds more than batch_size images, ingest.plan_batches)
    pins = [(torch.empty(max(1, batch_size), D, dtype=torch.float32).pin_memory(), torch.empty(max(1, batch_size), D, dtype=torch.uint8).pin_memory())
            for _ in range(3)]

    def collect(job):
        """host side of one batch: its rows, once the device-to-host copies have landed"""
        batch, copied, pu, pq, ev = job
        copied.synchronize()
        if batch.jpeg is not None:            # decoded on the GPU: a corrupt entropy-coded segment shows up as an error code
            err = batch.jpeg.err_host.numpy()[:len(batch.paths)]
            if err.any():
                raise RuntimeError(f"corrupt JPEG data in {[p for p, c in zip(batch.paths, err) if c]} (codes {err[err != 0].tolist()})")
        ev.synchronize()
        batch.release()
        unit[batch.indices] = pu.numpy()          # rows land at the files' positions, whatever the batch plan was
        codes[batch.indices] = pq.numpy()

    t_loop = time.perf_counter()      # the clock of compress.py's own rate: the loader's header pass and plan, every batch, the last sync
    loader = ShardLoader(files, batch_size, pad_to=256)
    try:
        pending = None
        it = iter(loader)
        batch = next(it, None)
        tok = ingest.start(batch) if batch is not None else None
        while batch is not None:
            t_a = time.perf_counter()
            nxt = next(it, None)
            t_b = time.perf_counter()
            ntok = ingest.start(nxt) if nxt is not None else None      # one batch ahead, enqueued before this batch's kernels
            d, copied = tok
            cur = torch.cuda.current_stream()
            cur.wait_event(copied)
            d.record_stream(cur)
            t_c = time.perf_counter()
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
            u, q = clipc.u8_to_codes(d, batch.hw)
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            gpu_evs.append((ev0, ev1))
            slot = pins[len(gpu_evs) % len(pins)]       # two batches are in flight at most: this one and `pending`
            pu, pq = slot[0][:u.shape[0]], slot[1][:q.shape[0]]
            pu.copy_(u, non_blocking=True)
            pq.copy_(q, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            t_d = time.perf_counter()
            if pending is not None:
                collect(pending)
            t_e = time.perf_counter()
            for k, v in (("wait_loader", t_b - t_a), ("ingest", t_c - t_b), ("submit", t_d - t_c), ("collect_incl_gpu_wait", t_e - t_d)):
                host_ms[k] = host_ms.get(k, 0.0) + v * 1e3
            pending = (batch, copied, pu, pq, ev)
            batch, tok = nxt, ntok
        if pending is not None:
            collect(pending)
    finally:
        loader.close()
    torch.cuda.synchronize()
    loop_s = time.perf_counter() - t_loop
    nb = max(1, len(gpu_evs))
    gpu_ms = sum(a.elapsed_time(b) for a, b in gpu_evs[1:]) / (len(gpu_evs) - 1) if len(gpu_evs) > 1 else None   # first batch: autotune

    ids = list(files)
    root.mkdir(parents=True, exist_ok=True)
    write_index_flat_ip(str(root / "faiss.index"), unit)
    write_index_flat_ip(str(root / "index.faiss"), unit)
    (root / "paths.json").write_text(json.dumps(ids, ensure_ascii=False, indent=2), encoding="utf-8")
    (root / "ids.txt").write_text("\n".join(ids), encoding="utf-8")
    (root / "meta.json").write_text(json.dumps({"dim": D, "model_id": clipc.model_name}, ensure_ascii=False, indent=2), encoding="utf-8")
    np.save(root / "codes.npy", codes)
    ops.save_tile_cache()
    dt = time.perf_counter() - t_start
    rec = {"cli_images_per_s": round(n / dt, 2) if dt > 0 else 0.0, "images": n, "seconds": round(dt, 3), "batch_size": batch_size,
           "loop_images_per_s": round(n / loop_s, 2) if loop_s > 0 else 0.0, "loop_seconds": round(loop_s, 3),
           "skip_header_pass_ms": round(header_ms, 2), "weights_and_tower_setup_ms": round((t_loop - t_hdr) * 1e3 - header_ms, 2),
           "batches": len(gpu_evs), "host_ms_per_batch": {k: round(v / nb, 2) for k, v in host_ms.items()},
           "gpu_ms_per_batch": None if gpu_ms is None else round(gpu_ms, 3),
           "gpu_jpeg_batches": loader.gpu_batches, "gpu_scan_jpeg_batches": loader.gpu_scan_batches, "host_decoded_batches": loader.host_batches,
           "note": "cli_images_per_s: files -> index, with listing, the skip pass over the headers, weights and the index files; "
                   "loop_images_per_s: the loader's header pass and plan, JPEG/PNG decode, H2D, CLIP preprocessing + tower, D2H (the clock of "
                   "compress.py's rate)"}
    log(f"[OK] index of {n} images, dim {D}, in {root}")
    print(json.dumps(rec), flush=True)
    return rec


def _hits_by_score(ci, lims, s, idx, j):
    """query j's share of a range_search result as the CLI prints it: score descending, ties to the lower index"""
    sj, ij = s[lims[j]:lims[j + 1]], idx[lims[j]:lims[j + 1]]
    order = np.lexsort((ij, -sj))
    return [{"path": ci.ids[i], "score": float(v)} for i, v in zip(ij[order], sj[order])]


def _query_codes(index_dir, c2df, topk, min_score=None, max_pairs=None):
    """`query-c2df --codes`: a file -> result list; a directory -> {path: result list}, all queries in one fused call.  min_score:
    every hit with score >= min_score instead of the top k, score descending, ties to the lower index; more than max_pairs of them
    is a ValueError naming the count"""
    ci = CodeIndex.load(index_dir)
    src = Path(c2df)
    files = sorted(src.glob("**/*.c2df")) if src.is_dir() else [src]
    if not files:
        raise RuntimeError(f"no .c2df under {src}")
    codes = np.stack([embedded_clip_codes(f)[0] for f in files])
    if min_score is None:
        s, idx = ci.search(codes, topk)
        res = [[{"path": ci.ids[i], "score": float(v)} for i, v in zip(idx[j], s[j])] for j in range(len(files))]
    else:
        lims, s, idx = ci.range_search(codes, min_score, max_pairs=max_pairs)
        res = [_hits_by_score(ci, lims, s, idx, j) for j in range(len(files))]
    return {str(f): r for f, r in zip(files, res)} if src.is_dir() else res[0]


def _query_vector(args):
    """the query of `query-text` / `query-image` / `query-c2df` as a (1, D) fp32 unit vector"""
    if args.cmd == "query-c2df":
        return decode_clip_from_c2df(args.c2df)[0][None, :]
    from . import weights as W
    from .compress import load_state
    from .config import CLIP_B32, CLIP_TINY
    ccfg = CLIP_TINY if getattr(args, "small", False) else CLIP_B32
    if args.cmd == "query-image":
        from .codec import ClipCodec
        from .compress import load_image
        csd = load_state(args.clip_ckpt, W.clip_spec, ccfg, 4321)
        return ClipCodec(csd, ccfg, "cuda:0").image_to_unit_vec(load_image(args.image))[None, :]
    from .clip import ClipTextHIP
    toks = tokenize(args.text, ccfg.ctx, args.token_ids)
    tsd = load_state(args.clip_ckpt, W.clip_text_spec, ccfg, 4321)
    return encode_text(toks, ClipTextHIP(tsd, ccfg, "cuda:0"))


def write_duplicates(index_dir, threshold, out=None, max_pairs=1 << 24):
    """`duplicates`: the groups of rows of the code index linked by a score >= threshold, one JSON line per group:
    {"paths": [...], "links": [{"a": path, "b": path, "score": s}, ...]}, links sorted by (row of a, row of b).  A last line on
    stderr gives the counts.  -> (rows, pairs, groups, files in groups)"""
    ci = CodeIndex.load(index_dir)
    groups, (i, j, s) = ci.duplicate_groups(threshold, max_pairs, with_pairs=True)
    group_of = {row: g for g, rows in enumerate(groups) for row in rows}
    links = [[] for _ in groups]
    for a, b, v in zip(i.tolist(), j.tolist(), s.tolist()):      # already sorted by (a, b)
        links[group_of[a]].append({"a": ci.ids[a], "b": ci.ids[b], "score": v})
    fh = open(out, "w", encoding="utf-8") if out else sys.stdout
    try:
        for rows, ln in zip(groups, links):
            fh.write(json.dumps({"paths": [ci.ids[r] for r in rows], "links": ln}, ensure_ascii=False) + "\n")
    finally:
        if out:
            fh.close()
    counts = (len(ci), len(i), len(groups), sum(len(g) for g in groups))
    print("[OK] %d rows, %d pairs with score >= %r, %d groups, %d files in groups" % (counts[0], counts[1], threshold, counts[2], counts[3]),
          file=sys.stderr)
    return counts


def write_clusters(index_dir, k, iters=10, seed=0, members=20, save_dir=None, out=None):
    """`clusters`: spherical k-means over the code index, one JSON line per non-empty cluster, largest first:
    {"cluster", "size", "representative": path, "mean_score", "members": [{"path", "score"}, ...]} -- members score descending, at
    most `members` of them (-1: all); mean_score the fp64 mean of all the cluster's fp32 scores.  A last line on stderr gives n, k,
    the passes run, the rows moved in each and the mean score over all rows.  save_dir: centroids.npy, assign.npy, clusters.json.
    -> the k-means result"""
    ci = CodeIndex.load(index_dir)
    res = ci.kmeans(k, iters=iters, seed=seed)
    fh = open(out, "w", encoding="utf-8") if out else sys.stdout
    try:
        for c in cluster_report(res["assign"], res["score"]):
            rows = c["members"]
            listed = rows if members < 0 else rows[:members]
            fh.write(json.dumps({"cluster": c["cluster"], "size": c["size"], "representative": ci.ids[c["representative"]],
                                 "mean_score": float(res["score"][rows].astype(np.float64).mean()),
                                 "members": [{"path": ci.ids[r], "score": float(res["score"][r])} for r in listed]},
                                ensure_ascii=False) + "\n")
    finally:
        if out:
            fh.close()
    if save_dir is not None:
        root = Path(save_dir)
        root.mkdir(parents=True, exist_ok=True)
        np.save(root / "centroids.npy", res["centroids"])
        np.save(root / "assign.npy", res["assign"])
        (root / "clusters.json").write_text(json.dumps({"n": len(ci), "dim": ci.dim, "k": int(k), "seed": int(seed),
                                                        "iters_run": res["iters_run"], "moved": res["moved"]}), encoding="utf-8")
    print("[OK] %d rows, k = %d, %d passes, moved %s, mean score %.6f" % (len(ci), int(k), res["iters_run"], res["moved"],
                                                                       float(res["score"].astype(np.float64).mean())), file=sys.stderr)
    return res


def _missing_index_files(index_dir, vectors):
    """what `recall` needs of an index directory and does not find -> message or None, without reading a file"""
    root = Path(index_dir)
    if vectors:
        if not any((root / a).exists() and (root / b).exists() for a, b, _ in _INDEX_LAYOUTS):
            return f"no FAISS index in {root}: expected " + " or ".join(f"{a} + {b}" for a, b, _ in _INDEX_LAYOUTS)
    elif not (root / "codes.npy").exists() or not (root / "ids.txt").exists():
        return f"no code index in {root}: expected codes.npy + ids.txt (sub-commands `build` / `build-images`)"
    return None


def write_recall(index_dir, queries_dir, vectors=False, ks=(1, 5, 10), out=None):
    """`recall`: how well the rows of one index directory (the queries) find their partners in another (the corpus).  A query row
    is paired with the corpus row whose id has the same file stem (pair_by_stem); queries without a partner are counted and left
    out.  Default: the queries' u8 codes (codes.npy) through CodeIndex.rank; vectors: their fp32 vectors (load_index) through
    CodeIndex.rank_vectors.  Prints one JSON line, retrieval_summary plus "corpus", "unmatched", "policy"; `out`: one JSON line
    per matched query {"query", "target", "rank", "score"}, in query order.  -> the summary"""
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError(f"recall@k needs k >= 1, got {ks}")
    for d, v in ((index_dir, False), (queries_dir, vectors)):      # both directories, before a file of either is read
        why = _missing_index_files(d, v)
        if why:
            raise FileNotFoundError(why)
    ci = CodeIndex.load(index_dir)
    if vectors:
        q, qids = load_index(queries_dir)
    else:
        qi = CodeIndex.load(queries_dir)
        q, qids = qi.codes, qi.ids
    if q.shape[1] != ci.dim:
        raise ValueError(f"queries of dim {q.shape[1]} ({queries_dir}) against a corpus of dim {ci.dim} ({index_dir})")
    qrows, targets, unmatched = pair_by_stem(qids, ci.ids)
    if qrows.size:
        rank, score = (ci.rank_vectors if vectors else ci.rank)(q[qrows], targets)
    else:
        rank, score = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
    if out:
        with open(out, "w", encoding="utf-8") as fh:
            for i, t, r, s in zip(qrows.tolist(), targets.tolist(), rank.tolist(), score.tolist()):
                fh.write(json.dumps({"query": qids[i], "target": ci.ids[t], "rank": r, "score": s}, ensure_ascii=False) + "\n")
    rec = retrieval_summary(rank, score, ks)
    rec.update({"corpus": len(ci), "unmatched": int(unmatched), "policy": "f32q" if vectors else "u8"})
    print(json.dumps(rec), flush=True)
    return rec


_THRESHOLD_HELP = ("score threshold (cosine of the dequantised codes, fp32).  Measured on quantised unit codes at D = 512: a row scores "
                   "1 +- 2^-23 against itself (so 1.0 can miss it), one code off by one step <= 0.99997, 64 codes off about 0.998, all 512 "
                   "off about 0.985, unrelated rows < 0.2.  About 0.99999 selects identical codes only, 0.98-0.99 re-encodes of one "
                   "picture")


_VECTOR_THRESHOLD_HELP = ("with --codes: every hit with score >= MIN_SCORE instead of the top k (--topk is ignored then), score "
                          "descending, ties to the lower index.  The score is the cosine between the query vector and the dequantised "
                          "code, fp32.  ")
_TEXT_THRESHOLD_HELP = (_VECTOR_THRESHOLD_HELP + "Which scores text queries reach against image codes has not been measured here: there "
                        "is no recommended value, look at the top-k scores of a few queries of your own first")
_IMAGE_THRESHOLD_HELP = (_VECTOR_THRESHOLD_HELP + "Measured on the u8 codes at D = 512, and valid for an image query only where its "
                         "vector is (nearly) the dequantised code of an indexed picture: identical codes score 1 +- 2^-23 (about 0.99999 "
                         "selects them), re-encodes of one picture 0.98-0.99.  Scores of merely similar pictures have not been measured "
                         "here")
_MAX_PAIRS_HELP = "with --min_score: refuse (and name the count) when more hits than this pass the threshold"


def main(argv=None):
    ap = argparse.ArgumentParser(description="query-text / query-image / query-c2df / build / build-images / neighbours / duplicates / clusters / recall")
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name, arg in (("query-text", "--text"), ("query-image", "--image"), ("query-c2df", "--c2df")):
        p = sub.add_parser(name)
        p.add_argument("--index_dir", type=Path, required=True)
        p.add_argument(arg, type=str, required=True)
        p.add_argument("--topk", type=int, default=10)
        p.add_argument("--clip_ckpt", type=str, default=None)
        if name == "query-image":
            p.add_argument("--small", action="store_true", help="TINY test tower (an index built with --small)")
        if name == "query-text":
            p.add_argument("--small", action="store_true", help="TINY test text tower (an index built with --small); needs --token_ids "
                           "within its vocabulary and context")
            p.add_argument("--token_ids", type=str, default=None, help="comma-separated BPE ids (offline tokenizer bypass)")
        if name == "query-c2df":
            p.add_argument("--codes", action="store_true", help="search the u8 code index (codes.npy) with the fused i8 kernel; "
                           "--c2df may then be a directory")
            p.add_argument("--min_score", type=float, default=None, help="with --codes: every hit with score >= MIN_SCORE instead of "
                           "the top k (--topk is ignored then), score descending, ties to the lower index.  " + _THRESHOLD_HELP)
        else:
            p.add_argument("--codes", action="store_true", help="search the u8 code index (codes.npy) with the fused fp32-query "
                           "kernel instead of the fp32 index files")
            p.add_argument("--min_score", type=float, default=None, help=_TEXT_THRESHOLD_HELP if name == "query-text" else _IMAGE_THRESHOLD_HELP)
        p.add_argument("--max_pairs", type=int, default=1 << 24, help=_MAX_PAIRS_HELP)
    p = sub.add_parser("build", help="index directory from a directory of .c2df containers")
    p.add_argument("--c2df_dir", type=Path, required=True)
    p.add_argument("--index_dir", type=Path, required=True)
    p = sub.add_parser("build-images", help="index directory from a folder of images, with the CLIP tower alone")
    p.add_argument("--image_dir", type=Path, required=True)
    p.add_argument("--index_dir", type=Path, required=True)
    p.add_argument("--model_id", type=str, default=None, help=f"only {_ONE_TOWER}[:pretrained] exists here")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--exts", type=str, default=",".join(IMAGE_EXTS))
    p.add_argument("--limit", type=int, default=None, help="use only N images (ignored if --desired is also given)")
    p.add_argument("--desired", type=int, default=None, help="target number of images")
    p.add_argument("--random", action="store_true", help="random sample instead of the first N (needs --limit or --desired)")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--clip_ckpt", type=str, default=None)
    p.add_argument("--small", action="store_true", help="TINY test tower")
    # the reference's downloader flags parse, and are refused: nothing here opens a socket
    p.add_argument("--auto_download", action="store_true", help="refused: there is no downloader")
    p.add_argument("--download_dir", type=Path, default=None, help="refused: there is no downloader")
    p.add_argument("--download_size", type=str, default=None, help="refused: there is no downloader")
    p.add_argument("--timeout", type=int, default=None, help="refused: there is no downloader")
    p = sub.add_parser("neighbours", help="k nearest neighbours of every vector of the code index, one JSON line each")
    p.add_argument("--index_dir", type=Path, required=True)
    p.add_argument("--topk", type=int, default=10)
    p.add_argument("--out", type=Path, default=None)
    p = sub.add_parser("duplicates", help="groups of near-duplicate rows of the code index, one JSON line each")
    p.add_argument("--index_dir", type=Path, required=True)
    p.add_argument("--threshold", type=float, required=True, help=_THRESHOLD_HELP + ".  There is no default")
    p.add_argument("--out", type=Path, default=None)
    p.add_argument("--max_pairs", type=int, default=1 << 24, help="refuse (and name the count) when more pairs than this pass the threshold")
    p = sub.add_parser("clusters", help="group the code index into k themes (spherical k-means), one JSON line per cluster")
    p.add_argument("--index_dir", type=Path, required=True)
    p.add_argument("--k", type=int, required=True, help="number of clusters, 1 .. min(rows, 65536)")
    p.add_argument("--iters", type=int, default=10, help="iterations at most; the loop ends early once no row changes cluster")
    p.add_argument("--seed", type=int, default=0, help="seed of the initial centroids (k rows of the index)")
    p.add_argument("--members", type=int, default=20, help="members listed per cluster, best first; -1 lists all")
    p.add_argument("--save_dir", type=Path, default=None, help="also write centroids.npy, assign.npy and clusters.json here")
    p.add_argument("--out", type=Path, default=None)
    p = sub.add_parser("recall", help="how well the rows of one index directory retrieve their partners (same file stem) in another")
    p.add_argument("--index_dir", type=Path, required=True, help="the corpus: an index directory with codes.npy + ids.txt")
    p.add_argument("--queries_dir", type=Path, required=True, help="the queries: another index directory (`build` / `build-images`)")
    p.add_argument("--vectors", action="store_true", help="take the queries' fp32 vectors (the fp32-query kernel) instead of their u8 codes")
    p.add_argument("--k", type=int, nargs="+", default=[1, 5, 10], help="the k of the recall@k figures")
    p.add_argument("--out", type=Path, default=None, help="one JSON line per matched query: query, target, rank, score")
    args = ap.parse_args(argv)
    if args.cmd == "recall":
        if any(k < 1 for k in args.k):      # refused before any file is read or kernel launched
            ap.error(f"--k {' '.join(str(k) for k in args.k)}: every k must be at least 1")
        for d, v in ((args.index_dir, False), (args.queries_dir, args.vectors)):
            why = _missing_index_files(d, v)
            if why:
                ap.error(why)
        write_recall(args.index_dir, args.queries_dir, args.vectors, args.k, args.out)
        return 0
    for flag in ("threshold", "min_score"):      # refused before any file is read or kernel launched
        if getattr(args, flag, None) is not None and not np.isfinite(getattr(args, flag)):
            ap.error(f"--{flag} {getattr(args, flag)}: a finite score is needed")
    if getattr(args, "min_score", None) is not None and not args.codes:
        ap.error("--min_score needs --codes: only the u8 code index has a threshold search")
    if args.cmd == "clusters":
        if args.k < 1 or args.k > MAX_CLUSTERS:      # refused before any file is read or kernel launched
            ap.error(f"--k {args.k}: 1 .. {MAX_CLUSTERS} clusters")
        if args.iters < 1:
            ap.error(f"--iters {args.iters}: at least one iteration")
        if args.members < -1:
            ap.error(f"--members {args.members}: a count, or -1 for all")
        write_clusters(args.index_dir, args.k, args.iters, args.seed, args.members, args.save_dir, args.out)
        return 0
    if args.cmd == "duplicates":
        write_duplicates(args.index_dir, args.threshold, args.out, args.max_pairs)
        return 0
    if args.cmd == "build":
        build_index(args.c2df_dir, args.index_dir)
        return 0
    if args.cmd == "build-images":
        used = [f for f in ("auto_download", "download_dir", "download_size", "timeout") if getattr(args, f) not in (None, False)]
        if used:
            ap.error("build-images: " + ", ".join("--" + f for f in used) + ": there is no downloader here, nothing in this tool "
                     "reaches the network; put the images into --image_dir yourself")
        if args.model_id is not None and args.model_id.split(":")[0] != _ONE_TOWER:
            ap.error(f"build-images: --model_id {args.model_id}: the one CLIP tower that exists here is {_ONE_TOWER}[:pretrained]")
        build_index_from_images(args.image_dir, args.index_dir, clip_ckpt=args.clip_ckpt, small=args.small, batch_size=args.batch_size,
                                exts=[e for e in args.exts.split(",") if e.strip()], limit=args.limit, random_pick=args.random,
                                seed=args.seed, desired=args.desired)
        return 0
    if args.cmd == "neighbours":
        ci = CodeIndex.load(args.index_dir)
        out = open(args.out, "w", encoding="utf-8") if args.out else sys.stdout
        try:
            for row, nb in ci.neighbours(args.topk):
                out.write(json.dumps({"path": ci.ids[row], "neighbours": [{"path": ci.ids[i], "score": v} for i, v in nb]},
                                     ensure_ascii=False) + "\n")
        finally:
            if args.out:
                out.close()
        return 0
    if args.cmd == "query-c2df" and args.codes:
        print(json.dumps(_query_codes(args.index_dir, args.c2df, args.topk, args.min_score, args.max_pairs), ensure_ascii=False, indent=2))
        return 0
    if args.codes:   # text / image vector against the u8 codes
        ci = CodeIndex.load(args.index_dir)
        if args.min_score is not None:      # every hit above the threshold, in the shape of `query-c2df --codes --min_score`
            lims, sim, idx = ci.range_search_vectors(_query_vector(args), args.min_score, max_pairs=args.max_pairs)
            print(json.dumps(_hits_by_score(ci, lims, sim, idx, 0), ensure_ascii=False, indent=2))
            return 0
        sim, idx = ci.search_vectors(_query_vector(args), args.topk)
        print(json.dumps([{"path": ci.ids[i], "score": float(v)} for i, v in zip(idx[0], sim[0]) if i != -1], ensure_ascii=False, indent=2))
        return 0
    vecs, paths = load_index(args.index_dir)
    q = _query_vector(args)
    print(json.dumps([{"path": p, "score": s} for p, s in do_search(q, vecs, paths, args.topk)], ensure_ascii=False, indent=2))
    return 0


if __name__ == "__main__":
    sys.exit(main())
