#!/usr/bin/env python3
"""Time the rank-of-target sink of the code search (csrc/search.hip search_rank_kernel: ops.search_codes_rank,
ops.search_codes_rank_f32q) against the top-k search of the same (nq, n): ops.search_codes / ops.search_codes_f32q at k = 10, device
time only, uploads of the corpus excluded for both.

Protocol (that of tools/bench_search_range.py, whose seeded corpus this uses): D = 512; both calls warmed up, then timed with device
events in one process, alternating, twice (both repeats are reported, they show the spread).  Every point runs in a child process of
its own under a time limit; the first point that fails ends the run.

  rank    u8 queries (rows of the corpus), targets: the queries' own rows for the first half, random rows for the second.
  vrank   fp32 queries (the dequantised unit vectors of the same rows), same targets.

`rank_ms` is the whole wrapper (targets checked on the host and uploaded, workspace and outputs allocated, pre-pass, scan);
`rank_launch_ms` the C entry point alone into preallocated arrays (pre-pass + scan); `topk_ms` the top-k wrapper (workspace and
outputs allocated, scan, merge).  All read n D bytes once: the share of 6.3 TB/s is given for each.  No pass mark was fixed before
the measurement; `ratio` = min(topk) / min(rank).

    python tools/bench_search_rank.py [--quick] [--out profiles/search_rank.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_search_range import DEV, DIM, HBM_BYTES_PER_S, alternate, corpus  # noqa: E402

K = 10


def point(n, nq, vectors):
    import numpy as np
    import torch
    from sgic_amd import _lib, ops
    from sgic_amd.search import codes_to_unit
    db, r = corpus(n, 42)
    rows = torch.arange(0, nq, device=DEV) * (n // nq)
    qc = db[rows].contiguous()
    rq = r[rows].contiguous()
    qv = torch.from_numpy(codes_to_unit(qc.cpu().numpy())).to(DEV).contiguous()
    targets = rows.cpu().numpy().astype(np.int64)
    targets[nq // 2:] = np.random.default_rng(3).integers(0, n, nq - nq // 2)
    dt = torch.from_numpy(targets.astype(np.int32)).to(DEV)
    work = torch.empty(4 * nq, dtype=torch.uint8, device=DEV)
    orank = torch.empty(nq, dtype=torch.int32, device=DEV)
    oscore = torch.empty(nq, dtype=torch.float32, device=DEV)
    size = ctypes.c_size_t(4 * nq)
    if vectors:
        whole = lambda: ops.search_codes_rank_f32q(qv, db, r, targets)                 # noqa: E731
        launch = lambda: _lib.call("sgic_search_rank_f32q", qv, db, r, dt, nq, n, DIM, 0, work, size, orank, oscore)   # noqa: E731
        topk = lambda: ops.search_codes_f32q(qv, db, r, K)                             # noqa: E731
    else:
        whole = lambda: ops.search_codes_rank(qc, rq, db, r, targets)                  # noqa: E731
        launch = lambda: _lib.call("sgic_search_rank_u8", qc, rq, db, r, dt, nq, n, DIM, 0, work, size, orank, oscore)   # noqa: E731
        topk = lambda: ops.search_codes(qc, rq, db, r, K)                              # noqa: E731
    rank, score = whole()
    launch()
    s, idx = topk()
    torch.cuda.synchronize()
    same = bool(torch.equal(rank, orank) and torch.equal(score, oscore))
    rank_h, idx_h = rank.cpu().numpy(), idx.cpu().numpy()
    agree = all((rank_h[j] < K) == (int(targets[j]) in idx_h[j].tolist()) and (rank_h[j] >= K or idx_h[j, rank_h[j]] == targets[j])
                for j in range(nq))
    iters = 20 if n <= 200000 else 10
    tw, tl, tt = alternate((whole, launch, topk), iters)
    share = lambda ms: n * DIM / (ms * 1e-3) / HBM_BYTES_PER_S   # noqa: E731
    return {"what": ("search_codes_rank_f32q vs search_codes_f32q" if vectors else "search_codes_rank vs search_codes") + f" k = {K}",
            "n": n, "nq": nq, "D": DIM, "iters": iters, "rank_ms": tw, "rank_launch_ms": tl, "topk_ms": tt,
            "topk_spread_ms": max(tt) - min(tt), "ratio": min(tt) / min(tw), "ratio_launch": min(tt) / min(tl),
            "rank_launch_share_of_hbm": share(min(tl)), "topk_share_of_hbm": share(min(tt)), "own_row_ranks_zero": bool((rank_h[:nq // 2] == 0).all()),
            "wrapper_equals_launch": same, "consistent_with_topk": bool(agree), "required": "none fixed before the measurement"}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_search_rank needs the GPU: there is nothing to time without one")
    kind, n, nq = spec.split(":")
    rec = point(int(n), int(nq), kind == "vrank")
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_rank.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=120, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    s = 100 if args.quick else 1
    big, mid = 1000000 // s, 100000 // s
    points = [f"rank:{big}:1", f"rank:{big}:16", f"rank:{big}:64", f"rank:{mid}:64", f"vrank:{big}:1", f"vrank:{big}:16", f"vrank:{big}:64",
              f"vrank:{mid}:32"]
    lines = [f"# tools/bench_search_rank.py; D={DIM} k={K}; ms per call, two repeats each, the rank call, its launch alone and the top-k "
             "search alternating in one process per point"]
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
