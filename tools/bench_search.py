#!/usr/bin/env python3
"""Time the fused searches over u8 codes (csrc/search.hip: ops.search_codes for u8 query codes, ops.search_codes_f32q for fp32
text / image vectors) against the fp32 path they stand beside (ops.gemm + ops.topk_rows on the codes_to_unit database), device time
only, uploads excluded for both.

Protocol: seeded data made on the device, both paths warmed up, then timed with device events in one process, alternating, twice
(the two repeats show the spread).  D = 512, k = 10, n in {1e4, 1e6}, nq in {1, 16, 1024}; plus the corpus self-search
(`neighbours`) at n = 1e5, where the fp32 path would need a 40 GB score matrix in one piece and is timed in query chunks instead.
fp32 queries (random unit vectors): the same n, nq in {1, 16, 256}; each database fragment feeds three MFMAs there, so the i8 share
counts 3 n nq D multiply-accumulates.

Per point: milliseconds per call; for nq <= 16 the database bytes the fused kernel has to read over its time, as a share of the
6.3 TB/s this card's HBM delivers; for nq = 1024 its i8 multiply-accumulates over time as a share of the dense i8 MFMA peak
(2.5e15 MAC/s, twice the bf16 rate), with the bound that applies named.

    python tools/bench_search.py [--quick] > profiles/search_codes.txt"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sgic_amd  # noqa: E402,F401
from sgic_amd import ops  # noqa: E402
from sgic_amd.search import code_rnorm  # noqa: E402

HBM_BYTES_PER_S = 6.3e12       # achievable (float4 copy), not the 8 TB/s of the data sheet
I8_MAC_PER_S = 2.5e15          # dense i8 MFMA peak: 5 POP/s
DEV = "cuda:0"


def unit_codes(n, dim, seed):
    """quantised random unit vectors, as the compress side stores them; made on the device in slices"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.empty(n, dim, dtype=torch.uint8, device=DEV)
    for i in range(0, n, 1 << 17):
        v = torch.randn(min(1 << 17, n - i), dim, generator=g, device=DEV)
        v = v / v.norm(dim=1, keepdim=True)
        out[i:i + v.shape[0]] = torch.round((v * 0.5 + 0.5) * 255).to(torch.uint8)
    return out


def to_unit(codes):
    """search.codes_to_unit on the device, same operation order (fp32 divide, scale, shift, normalise)"""
    v = codes.to(torch.float32) / 255.0 * 2.0 - 1.0
    return (v / v.norm(dim=1, keepdim=True).clamp_min(1e-9)).contiguous()


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def point(n, nq, dim, k, db, r_db, db32, repeats=2):
    q = unit_codes(nq, dim, 1000 + nq)
    r_q = torch.from_numpy(code_rnorm(q.cpu().numpy())).to(DEV)
    q32 = to_unit(q)
    fused = lambda: ops.search_codes(q, r_q, db, r_db, k)                     # noqa: E731
    parent = lambda: ops.topk_rows(ops.gemm(q32, db32, w_const=False), k)      # noqa: E731
    for _ in range(2):
        fused()
    for _ in range(8):              # the GEMM's launch-mode tuner samples the first occurrences of a new shape
        parent()
    ops.finalize_autotune()
    torch.cuda.synchronize()
    work = n * nq
    iters = 50 if work <= 2e7 else (10 if work <= 2e8 else 3)
    tf, tp = [], []
    for _ in range(repeats):
        tf.append(timed(fused, iters))
        tp.append(timed(parent, iters))
    s_f, i_f = fused()
    s_p, i_p = parent()
    rec = {"n": n, "nq": nq, "D": dim, "k": k, "iters": iters, "fused_ms": tf, "parent_ms": tp,
           "speedup": min(tp) / min(tf), "ids_equal_share": float((i_f == i_p).float().mean()),
           "max_score_diff": float((s_f - s_p).abs().max())}
    t = min(tf) * 1e-3
    if nq <= 16:
        rec["bound"] = "HBM"
        rec["fused_share_of_hbm"] = n * dim / t / HBM_BYTES_PER_S
    else:
        t_mac, t_mem = n * nq * dim / I8_MAC_PER_S, n * dim / HBM_BYTES_PER_S
        rec["bound"] = "i8 MFMA" if t_mac >= t_mem else "HBM"
        rec["fused_share_of_i8_peak"] = n * nq * dim / t / I8_MAC_PER_S
    return rec


def point_f32q(n, nq, dim, k, db, r_db, db32, repeats=2):
    g = torch.Generator(device=DEV).manual_seed(2000 + nq)
    q32 = torch.randn(nq, dim, generator=g, device=DEV)
    q32 = (q32 / q32.norm(dim=1, keepdim=True)).contiguous()
    fused = lambda: ops.search_codes_f32q(q32, db, r_db, k)                    # noqa: E731
    parent = lambda: ops.topk_rows(ops.gemm(q32, db32, w_const=False), k)      # noqa: E731
    for _ in range(2):
        fused()
    for _ in range(8):
        parent()
    ops.finalize_autotune()
    torch.cuda.synchronize()
    work = n * nq
    iters = 50 if work <= 2e7 else (10 if work <= 2e8 else 3)
    tf, tp = [], []
    for _ in range(repeats):
        tf.append(timed(fused, iters))
        tp.append(timed(parent, iters))
    s_f, i_f = fused()
    s_p, i_p = parent()
    rec = {"what": "fp32 queries", "n": n, "nq": nq, "D": dim, "k": k, "iters": iters, "fused_ms": tf, "parent_ms": tp,
           "speedup": min(tp) / min(tf), "ids_equal_share": float((i_f == i_p).float().mean()),
           "max_score_diff": float((s_f - s_p).abs().max())}
    t = min(tf) * 1e-3
    if nq <= 16:
        rec["bound"] = "HBM"
        rec["fused_share_of_hbm"] = n * dim / t / HBM_BYTES_PER_S
    else:
        t_mac, t_mem = 3 * n * nq * dim / I8_MAC_PER_S, n * dim / HBM_BYTES_PER_S
        rec["bound"] = "i8 MFMA" if t_mac >= t_mem else "HBM"
        rec["fused_share_of_i8_peak"] = 3 * n * nq * dim / t / I8_MAC_PER_S
    return rec


def neighbours_point(n, dim, k, chunk=4096, repeats=2):
    db = unit_codes(n, dim, 7)
    r = torch.from_numpy(code_rnorm(db.cpu().numpy())).to(DEV)
    db32 = to_unit(db)

    def fused():
        return ops.search_codes(db, r, db, r, k + 1)

    def parent():
        for c0 in range(0, n, chunk):
            ops.topk_rows(ops.gemm(db32[c0:c0 + chunk], db32, w_const=False), k + 1)

    fused()
    for _ in range(3):
        parent()
    ops.finalize_autotune()
    torch.cuda.synchronize()
    tf, tp = [], []
    for _ in range(repeats):
        tf.append(timed(fused, 1))
        tp.append(timed(parent, 1))
    t = min(tf) * 1e-3
    return {"what": "neighbours (corpus self-search, own id included: k + 1 results)", "n": n, "nq": n, "D": dim, "k": k + 1,
            "fused_ms": tf, "parent_chunked_ms": tp, "parent_chunk": chunk, "parent_one_piece_score_matrix_GB": n * n * 4 / 1e9,
            "speedup": min(tp) / min(tf), "bound": "i8 MFMA", "fused_share_of_i8_peak": n * n * dim / t / I8_MAC_PER_S}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_search needs the GPU: there is nothing to time without one")
    dim, k = 512, 10
    sizes = [10 ** 4] if args.quick else [10 ** 4, 10 ** 6]
    print(f"# {torch.cuda.get_device_name(0)}; D={dim} k={k}; ms per call, two repeats each, fused and parent alternating")
    for n in sizes:
        db = unit_codes(n, dim, 42)
        r_db = torch.from_numpy(code_rnorm(db.cpu().numpy())).to(DEV)
        db32 = to_unit(db)
        for nq in (1, 16, 1024):
            print(json.dumps(point(n, nq, dim, k, db, r_db, db32)), flush=True)
        for nq in (1, 16, 256):
            print(json.dumps(point_f32q(n, nq, dim, k, db, r_db, db32)), flush=True)
        del db, r_db, db32
    print(json.dumps(neighbours_point(10 ** 4 if args.quick else 10 ** 5, dim, k)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
