#!/usr/bin/env python3
"""Time the threshold (range) search over u8 codes (csrc/search.hip search_range_kernel: ops.search_codes_range) against the top-k
search it stands beside (ops.search_codes), device time only, uploads excluded for both.

Protocol: a seeded corpus made on the device, D = 512, 1 % of its rows overwritten with near-duplicates of other rows (8 codes moved
by one step), T = 0.95; both paths warmed up, then timed with device events in one process, alternating, twice (both repeats are
reported, they show the spread).  Every point runs in a child process of its own under a time limit; the first point that fails ends
the run.

  dup     duplicate_pairs (the self-join, sort and count read-back included) at n = 1e5, against the loop of `neighbours`:
          search_codes with k = 11, queries in chunks of 4096.  Required: not slower than that loop in the same run.
  range   search_codes_range at n = 1e6, nq in {1, 16} (the queries are corpus rows, so there are hits), against search_codes with
          k = 10 on the same inputs.  `range_ms` is the whole wrapper (counter zeroed, kernel, count read back, hits sorted);
          `range_kernel_ms` the counter reset and the kernel alone into preallocated arrays.  Required: within the spread the top-k
          search's own two repeats show.  Both read n D bytes once: the share of 6.3 TB/s is given for each.
  dense   T = -2, nq = 64, n = 1e5: every pair is a hit, 6.4e6 entries; output-bound, no pass mark.

--vectors runs the fp32-query points instead (search_range_kernel with F32Query: ops.search_codes_range_f32q), same protocol:

  vrange  search_codes_range_f32q at n = 1e6, nq in {1, 16}; the queries are the dequantised unit vectors of corpus rows that have
          a planted near-duplicate, so a handful of hits exist.  Counterpart: search_codes_f32q with k = 10 on the same inputs, what
          top-k-and-filter costs.  Whole wrapper and "counter reset + kernel alone", as for `range`.  Required: not slower than the
          counterpart beyond the counterpart's own repeat-to-repeat spread.
  vdense  T = -2, nq = 32, n = 1e5: 3.2e6 entries; output-bound, no pass mark.

    python tools/bench_search_range.py [--quick] [--out profiles/search_range.txt]
    python tools/bench_search_range.py --vectors [--quick] [--out profiles/search_range_f32q.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.3e12       # achievable (float4 copy), not the 8 TB/s of the data sheet
DEV = "cuda:0"
DIM, THRESHOLD = 512, 0.95


def corpus(n, seed):
    """quantised random unit codes made on the device in slices; every hundredth row a near-duplicate of the row before it
    -> (codes u8 (n, D), reciprocal norms fp32 (n,))"""
    import torch
    from sgic_amd.search import code_rnorm
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.empty(n, DIM, dtype=torch.uint8, device=DEV)
    for i in range(0, n, 1 << 17):
        v = torch.randn(min(1 << 17, n - i), DIM, generator=g, device=DEV)
        v = v / v.norm(dim=1, keepdim=True)
        out[i:i + v.shape[0]] = torch.round((v * 0.5 + 0.5) * 255).to(torch.uint8)
    dup = torch.arange(1, n, 100, device=DEV)
    out[dup] = out[dup - 1]
    cols = torch.arange(0, DIM, DIM // 8, device=DEV)
    out[dup[:, None], cols[None, :]] += 1                       # 8 codes one step up (unit codes sit near 128, far from 255)
    return out, torch.from_numpy(code_rnorm(out.cpu().numpy())).to(DEV)


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, iters, repeats=2):
    times = [[] for _ in fns]
    for _ in range(repeats):
        for t, fn in zip(times, fns):
            t.append(timed(fn, iters))
    return times


def point_dup(n, chunk=4096):
    from sgic_amd import ops
    db, r = corpus(n, 7)
    new = lambda: ops.search_codes_range(db, r, db, r, THRESHOLD, self_join=True)      # noqa: E731

    def parent():
        for c0 in range(0, n, chunk):
            ops.search_codes(db[c0:c0 + chunk], r[c0:c0 + chunk], db, r, 11)

    pairs = new()[3]
    parent()
    tn, tp = alternate((new, parent), 1)
    return {"what": "duplicate_pairs (self-join) vs the neighbours loop (search_codes k = 11, chunks of 4096)", "n": n, "D": DIM,
            "T": THRESHOLD, "pairs": pairs, "self_join_ms": tn, "neighbours_loop_ms": tp, "ratio": min(tp) / min(tn),
            "required": "self-join not slower than the loop", "met": bool(min(tn) <= min(tp))}


def point_range(n, nq):
    import torch
    from sgic_amd import ops
    db, r = corpus(n, 42)
    rows = torch.arange(nq, device=DEV) * 100                    # corpus rows that each have a planted near-duplicate
    q, rq = db[rows].contiguous(), r[rows].contiguous()
    cap = 4096
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    oq, od = torch.empty(cap, dtype=torch.int32, device=DEV), torch.empty(cap, dtype=torch.int32, device=DEV)
    os_ = torch.empty(cap, dtype=torch.float32, device=DEV)

    def kernel():
        count.zero_()
        ops.search_codes_range_launch(q, rq, db, r, THRESHOLD, False, None, cap, count, oq, od, os_)

    wrapper = lambda: ops.search_codes_range(q, rq, db, r, THRESHOLD)      # noqa: E731
    topk = lambda: ops.search_codes(q, rq, db, r, 10)                      # noqa: E731
    hits = wrapper()[3]
    for fn in (kernel, topk, wrapper, topk):
        fn()
    tw, tk, tt = alternate((wrapper, kernel, topk), 10)
    spread = max(tt) - min(tt)
    share = lambda ms: n * DIM / (ms * 1e-3) / HBM_BYTES_PER_S   # noqa: E731
    return {"what": "search_codes_range vs search_codes k = 10", "n": n, "nq": nq, "D": DIM, "T": THRESHOLD, "hits": hits, "iters": 10,
            "range_ms": tw, "range_kernel_ms": tk, "topk_ms": tt, "topk_spread_ms": spread,
            "range_share_of_hbm": share(min(tw)), "range_kernel_share_of_hbm": share(min(tk)), "topk_share_of_hbm": share(min(tt)),
            "required": "range within the top-k search's own spread: min(range) <= min(topk) + spread",
            "met_wrapper": bool(min(tw) <= min(tt) + spread), "met_kernel": bool(min(tk) <= min(tt) + spread)}


def point_dense(n, nq):
    import torch
    from sgic_amd import ops
    db, r = corpus(n, 9)
    q, rq = db[:nq].contiguous(), r[:nq].contiguous()
    cap = nq * n
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    oq, od = torch.empty(cap, dtype=torch.int32, device=DEV), torch.empty(cap, dtype=torch.int32, device=DEV)
    os_ = torch.empty(cap, dtype=torch.float32, device=DEV)

    def kernel():
        count.zero_()
        ops.search_codes_range_launch(q, rq, db, r, -2.0, False, None, cap, count, oq, od, os_)

    wrapper = lambda: ops.search_codes_range(q, rq, db, r, -2.0)           # noqa: E731
    assert wrapper()[3] == cap
    kernel()
    tw, tk = alternate((wrapper, kernel), 3)
    return {"what": "dense emission, T = -2 (output-bound, no pass mark)", "n": n, "nq": nq, "D": DIM, "entries": cap,
            "range_ms": tw, "range_kernel_ms": tk, "kernel_output_GB_per_s": cap * 12 / (min(tk) * 1e-3) / 1e9,
            "note": "range_ms: the default capacity overflows, so the wrapper launches twice, then sorts 6.4e6 keys"}


def unit_queries(db, rows):
    """the dequantised unit vectors of corpus rows (search.codes_to_unit's arithmetic, on the device) -> (len(rows), D) fp32"""
    v = (db[rows].float() / 255.0) * 2.0 - 1.0
    return (v / v.norm(dim=1, keepdim=True)).contiguous()


def point_vrange(n, nq):
    import torch
    from sgic_amd import ops
    db, r = corpus(n, 42)
    q = unit_queries(db, torch.arange(nq, device=DEV) * 100)     # corpus rows that each have a planted near-duplicate
    cap = 4096
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    oq, od = torch.empty(cap, dtype=torch.int32, device=DEV), torch.empty(cap, dtype=torch.int32, device=DEV)
    os_ = torch.empty(cap, dtype=torch.float32, device=DEV)

    def kernel():
        count.zero_()
        ops.search_codes_range_f32q_launch(q, db, r, THRESHOLD, None, cap, count, oq, od, os_)

    wrapper = lambda: ops.search_codes_range_f32q(q, db, r, THRESHOLD)     # noqa: E731
    topk = lambda: ops.search_codes_f32q(q, db, r, 10)                     # noqa: E731
    hits = wrapper()[3]
    for fn in (kernel, topk, wrapper, topk):
        fn()
    tw, tk, tt = alternate((wrapper, kernel, topk), 10)
    spread = max(tt) - min(tt)
    share = lambda ms: n * DIM / (ms * 1e-3) / HBM_BYTES_PER_S   # noqa: E731
    return {"what": "search_codes_range_f32q vs search_codes_f32q k = 10", "n": n, "nq": nq, "D": DIM, "T": THRESHOLD, "hits": hits,
            "iters": 10, "range_ms": tw, "range_kernel_ms": tk, "topk_ms": tt, "topk_spread_ms": spread,
            "range_share_of_hbm": share(min(tw)), "range_kernel_share_of_hbm": share(min(tk)), "topk_share_of_hbm": share(min(tt)),
            "required": "range not slower than the top-k search beyond its own spread: min(range) <= min(topk) + spread",
            "met_wrapper": bool(min(tw) <= min(tt) + spread), "met_kernel": bool(min(tk) <= min(tt) + spread)}


def point_vdense(n, nq):
    import torch
    from sgic_amd import ops
    db, r = corpus(n, 9)
    q = unit_queries(db, torch.arange(nq, device=DEV))
    cap = nq * n
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    oq, od = torch.empty(cap, dtype=torch.int32, device=DEV), torch.empty(cap, dtype=torch.int32, device=DEV)
    os_ = torch.empty(cap, dtype=torch.float32, device=DEV)

    def kernel():
        count.zero_()
        ops.search_codes_range_f32q_launch(q, db, r, -2.0, None, cap, count, oq, od, os_)

    wrapper = lambda: ops.search_codes_range_f32q(q, db, r, -2.0)          # noqa: E731
    assert wrapper()[3] == cap
    kernel()
    tw, tk = alternate((wrapper, kernel), 3)
    return {"what": "fp32 queries, dense emission, T = -2 (output-bound, no pass mark)", "n": n, "nq": nq, "D": DIM, "entries": cap,
            "range_ms": tw, "range_kernel_ms": tk, "kernel_output_GB_per_s": cap * 12 / (min(tk) * 1e-3) / 1e9,
            "note": "range_ms: the default capacity overflows, so the wrapper launches twice, then sorts the keys"}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_search_range needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"dup": point_dup, "range": point_range, "dense": point_dense, "vrange": point_vrange, "vdense": point_vdense}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--vectors", action="store_true", help="the fp32-query points (vrange, vdense) instead of the u8 ones")
    ap.add_argument("--out", default=None, help="default: profiles/search_range.txt, with --vectors profiles/search_range_f32q.txt")
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    s = 100 if args.quick else 1
    points = [f"dup:{100000 // s}", f"range:{1000000 // s}:1", f"range:{1000000 // s}:16", f"dense:{100000 // s}:64"]
    if args.vectors:
        points = [f"vrange:{1000000 // s}:1", f"vrange:{1000000 // s}:16", f"vdense:{100000 // s}:32"]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "search_range_f32q.txt" if args.vectors else "search_range.txt")
    lines = [f"# tools/bench_search_range.py; D={DIM} T={THRESHOLD}; ms per call, two repeats each, the new call and its counterpart "
             "alternating in one process per point"]
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
