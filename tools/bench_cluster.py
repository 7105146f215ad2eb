#!/usr/bin/env python3
"""Time the clustering over u8 codes (csrc/search.hip assign_codes_kernel / cluster_sums_kernel: ops.assign_codes, ops.cluster_sums,
CodeIndex.kmeans) against what the tree could do without them, device time only, uploads excluded for both.

Protocol (that of tools/bench_search_range.py, whose seeded corpus this uses): D = 512; both paths warmed up, then timed with device
events in one process, alternating, twice (both repeats are reported, they show the spread).  Every point runs in a child process of
its own under a time limit; the first point that fails ends the run.

  assign    ops.assign_codes at n = 1e6, K in {256, 1024} random unit centroids, against the route without a resident fp32 copy: per
            chunk of 65 536 rows codes_to_unit's arithmetic on the device, fp32 torch.matmul against the centroids, argmax (the
            dequantisation is part of its price).  Required: not slower than that beyond its own repeat-to-repeat spread.  The i8
            MAC rate (3 n K D over time) is given against 2.5e15 MAC/s.
  assign16  ops.assign_codes at n = 1e6, K = 16 against search_codes_range_f32q's kernel (nq = 16, counter reset + kernel alone): the
            same bytes and the same three MFMAs per fragment.  No pass mark; the share of 6.3 TB/s is given for both.
  sums      ops.cluster_sums at n = 1e6, K = 256 (the assignment of 256 random centroids) against chunked torch.index_add_ of
            2 c - 255 as int64.  Required: not slower beyond the spread.  Bytes of codes over time are given.
  kmeans    CodeIndex.kmeans at n = 1e5, k = 64, 10 iterations, the whole call on the wall clock, and the device time of one assign
            and one sums call at that shape: what is left per iteration is the host (read-backs, centroids_from_sums, uploads).

    python tools/bench_cluster.py [--quick] [--out profiles/cluster_codes.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_search_range import DEV, DIM, HBM_BYTES_PER_S, alternate, corpus  # noqa: E402

I8_MAC_PER_S = 2.5e15
CHUNK = 1 << 16


def centroids(K, seed):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    c = torch.randn(K, DIM, generator=g, device=DEV)
    return (c / c.norm(dim=1, keepdim=True)).contiguous()


def fp32_assign(db, cent):
    """the counterpart: dequantise a chunk, fp32 GEMM, argmax; no fp32 copy of the corpus stays resident"""
    import torch
    out = torch.empty(db.shape[0], dtype=torch.int64, device=db.device)
    for i in range(0, db.shape[0], CHUNK):
        v = (db[i:i + CHUNK].float() / 255.0) * 2.0 - 1.0
        v = v / v.norm(dim=1, keepdim=True)
        out[i:i + CHUNK] = torch.matmul(v, cent.t()).argmax(dim=1)
    return out


def point_assign(n, K):
    from sgic_amd import ops
    db, r = corpus(n, 42)
    cent = centroids(K, 5)
    new = lambda: ops.assign_codes(cent, db, r)             # noqa: E731
    old = lambda: fp32_assign(db, cent)                     # noqa: E731
    agree = float((new()[0].long() == old()).float().mean())
    new()
    tn, to = alternate((new, old), 5)
    spread = max(to) - min(to)
    return {"what": "assign_codes vs chunked dequantise + fp32 matmul + argmax", "n": n, "K": K, "D": DIM, "iters": 5, "assign_ms": tn,
            "fp32_route_ms": to, "fp32_route_spread_ms": spread, "ratio": min(to) / min(tn), "same_cluster_share": agree,
            "i8_mac_per_s": 3.0 * n * K * DIM / (min(tn) * 1e-3), "share_of_i8_peak": 3.0 * n * K * DIM / (min(tn) * 1e-3) / I8_MAC_PER_S,
            "required": "not slower than the fp32 route beyond its own spread: min(assign) <= min(fp32) + spread",
            "met": bool(min(tn) <= min(to) + spread)}


def point_assign16(n):
    import torch
    from sgic_amd import ops
    db, r = corpus(n, 42)
    cent = centroids(16, 5)
    cap = 4096
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    oq, od = torch.empty(cap, dtype=torch.int32, device=DEV), torch.empty(cap, dtype=torch.int32, device=DEV)
    os_ = torch.empty(cap, dtype=torch.float32, device=DEV)

    def rng_kernel():
        count.zero_()
        ops.search_codes_range_f32q_launch(cent, db, r, 0.95, None, cap, count, oq, od, os_)

    new = lambda: ops.assign_codes(cent, db, r)             # noqa: E731
    for fn in (new, rng_kernel, new, rng_kernel):
        fn()
    tn, tr = alternate((new, rng_kernel), 10)
    share = lambda ms: n * DIM / (ms * 1e-3) / HBM_BYTES_PER_S   # noqa: E731
    return {"what": "assign_codes K = 16 vs search_codes_range_f32q nq = 16 (counter reset + kernel alone)", "n": n, "K": 16, "D": DIM,
            "iters": 10, "assign_ms": tn, "range_kernel_ms": tr, "assign_share_of_hbm": share(min(tn)),
            "range_kernel_share_of_hbm": share(min(tr)), "required": "none (a recorded data point)"}


def point_sums(n, K):
    import torch
    from sgic_amd import ops
    db, r = corpus(n, 42)
    assign = ops.assign_codes(centroids(K, 5), db, r)[0]
    idx = assign.long()

    def old():
        sums = torch.zeros(K, DIM, dtype=torch.int64, device=DEV)
        for i in range(0, n, CHUNK):
            sums.index_add_(0, idx[i:i + CHUNK], 2 * db[i:i + CHUNK].to(torch.int64) - 255)
        return sums, torch.bincount(idx, minlength=K)

    new = lambda: ops.cluster_sums(db, assign, K)           # noqa: E731
    (s1, c1), (s0, c0) = new(), old()
    equal = bool(torch.equal(s1, s0) and torch.equal(c1, c0))
    tn, to = alternate((new, old), 3)
    spread = max(to) - min(to)
    return {"what": "cluster_sums (sort included) vs chunked index_add_ of 2c - 255 as int64", "n": n, "K": K, "D": DIM, "iters": 3,
            "sums_ms": tn, "index_add_ms": to, "index_add_spread_ms": spread, "ratio": min(to) / min(tn), "equal": equal,
            "largest_cluster": int(c1.max()), "codes_GB_per_s": n * DIM / (min(tn) * 1e-3) / 1e9,
            "required": "not slower than index_add_ beyond its own spread: min(sums) <= min(index_add) + spread",
            "met": bool(equal and min(tn) <= min(to) + spread)}


def point_kmeans(n, k, iters):
    import torch
    from sgic_amd import ops
    from sgic_amd.search import CodeIndex
    db, r = corpus(n, 42)
    ci = CodeIndex(db.cpu().numpy(), [""] * n).to(DEV)
    ci.kmeans(k, iters=1)                                   # warm-up
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ci.kmeans(k, iters=iters, seed=0)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    cent = torch.from_numpy(res["centroids"]).to(DEV)
    assign = torch.from_numpy(res["assign"]).to(DEV)
    ta, ts = alternate((lambda: ops.assign_codes(cent, db, r), lambda: ops.cluster_sums(db, assign, k)), 10)
    passes = res["iters_run"] + (0 if res["moved"][-1] == 0 else 1)      # assignment passes, the final one included
    per_iter = min(walls) / res["iters_run"]
    return {"what": "CodeIndex.kmeans, whole call (wall clock)", "n": n, "k": k, "D": DIM, "iters": iters, "iters_run": res["iters_run"],
            "assign_passes": passes, "moved": res["moved"], "whole_call_ms": walls, "ms_per_iteration": per_iter,
            "assign_ms": ta, "sums_ms": ts, "host_ms_per_iteration": per_iter - min(ta) * passes / res["iters_run"] - min(ts),
            "mean_score": float(res["score"].mean()), "required": "none"}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"assign": point_assign, "assign16": point_assign16, "sums": point_sums, "kmeans": point_kmeans}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_codes.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    s = 100 if args.quick else 1
    points = [f"assign:{1000000 // s}:256", f"assign:{1000000 // s}:1024", f"assign16:{1000000 // s}", f"sums:{1000000 // s}:256",
              f"kmeans:{100000 // s}:64:10"]
    lines = [f"# tools/bench_cluster.py; D={DIM}; ms per call, two repeats each, the new call and its counterpart alternating in one "
             "process per point"]
    for p in points:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--point", p], capture_output=True, text=True,
                                  timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"# point {p}: no result within {args.limit} s; the run ends here")
            break
        if done.returncode != 0:
            lines.append(f"# point {p}: exit status {done.returncode}; the run ends here\n# " + done.stderr.strip()[-400:].replace("\n", "\n# "))
            break
        lines.append(done.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if len(lines) == len(points) + 1 else 1


if __name__ == "__main__":
    sys.exit(main())
