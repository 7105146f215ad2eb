#!/usr/bin/env python3
"""Time the FID / KID path on the GPU (fid.InceptionFID.features: csrc/fid.hip's producers and pools + split GEMMs; the fp64 Gram
kernel and the host eigen-decompositions behind fid.fid and fid.kid) against a torch fp32 version of the same definition on the
device (tests/fid_ref.py: F.interpolate, F.conv2d with the folded weights, the pools), device time only.

Protocol (that of tools/bench_lpips.py): seeded u8 images made on the device, N windows of 256 x 256 (one per image); synthetic
weights; both paths warmed up (which also settles the GEMMs' launch modes), then timed with device events in one process,
alternating, twice (both repeats are reported, they show the spread).  Every point runs in a child process of its own under a time
limit; the first point that fails ends the run.

  feat      InceptionFID.features against the torch version, both in chunks of the same number of windows.  Expected: not slower than
            the torch version beyond that version's own repeat-to-repeat spread.  The largest relative L2 difference of an image's
            features between the two is reported.
  tail      n = m = 4096 feature rows: the second moments (ops.gram_f64) by device events; fid.fid and fid.kid (100 subsets of 1000)
            by the wall clock, host eigen-decompositions and read-backs included.
  decode    one Codec.decode_batch (LARGE architecture, synthetic weights) of 64 of the 256 x 256 images the windows come from.  No
            pass mark; the parent adds the share of the features (and of the tail) in the decode of as many images as windows.

    python tools/bench_fid.py [--quick] [--out profiles/fid.txt]

The per-kernel breakdown of profiles/fid_kernels.txt is a run of its own under the profiler, with no tuning launches in the trace:

    rocprofv3 --kernel-trace --stats -d DIR -o fid -- python tools/bench_fid.py --trace-pass 64:8
    python tools/bench_fid.py --trace-table DIR/fid_results.db [--out profiles/fid_kernels.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_quality import pairs, point_decode  # noqa: E402
from bench_search_range import DEV, alternate  # noqa: E402


def point_feat(N, iters):
    import torch
    import torch.nn.functional as F
    import fid_ref
    from sgic_amd import fid, ops
    a, _ = pairs(N, 256, 256, 3)
    sd = fid.synth_weights(1234)
    model = fid.InceptionFID(sd, DEV)
    ref = fid_ref.Ref(sd, torch.float32, DEV)
    chunk = max(1, model.max_operand_bytes // fid.OPERAND_BYTES_PER_IMAGE)      # the same windows per pass for both

    def old():
        out = torch.empty(N, fid.DIM, device=DEV)
        for s in range(0, N, chunk):
            x = a[s:s + chunk].permute(0, 3, 1, 2).float() / 255
            out[s:s + chunk] = ref.features_of_input(2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1)
        return out

    new = lambda: model.features(a)                              # noqa: E731
    f1, f0 = new().double(), old().double()
    diff = float(((f1 - f0).norm(dim=1) / f0.norm(dim=1)).max())
    for _ in range(2):
        new()
        old()
    ops.finalize_autotune()                                      # no launch-mode race is left open inside the timed region
    tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": "InceptionFID.features vs torch fp32 on the device", "windows": N, "H": 256, "W": 256, "iters": iters,
            "windows_per_chunk": chunk, "fid_ms": tn, "torch_ms": to, "torch_spread_ms": spread, "ratio": min(to) / min(tn),
            "largest_relative_l2_difference": diff,
            "expected": "not slower than torch beyond its own spread: min(fid) <= min(torch) + spread", "met": bool(min(tn) <= min(to) + spread)}


def point_tail(n, iters):
    import torch
    from sgic_amd import fid, ops
    g = torch.Generator(device=DEV).manual_seed(5)
    X = torch.relu(torch.randn(n, fid.DIM, generator=g, device=DEV) + 0.3)
    Y = torch.relu(X + 0.2 * torch.randn(n, fid.DIM, generator=g, device=DEV))
    xt = X.t().contiguous()
    gram = lambda: ops.gram_f64(xt)                              # noqa: E731
    gram()
    (tg,) = alternate((gram,), iters)
    out = {"what": "the statistics behind FID and KID", "n": n, "m": n, "d": fid.DIM, "second_moments_gram_ms": tg}
    for name, fn in (("fid", lambda: fid.fid(X, Y)), ("kid", lambda: fid.kid(X, Y))):
        torch.cuda.synchronize()
        t = time.perf_counter()
        val = fn()
        torch.cuda.synchronize()
        out[f"{name}_wall_ms"] = (time.perf_counter() - t) * 1e3
        out[name] = val
    out["expected"] = "none (once per evaluation)"
    return out


def trace_pass(spec):
    """N:P -> P passes of InceptionFID.features over N windows of 256 x 256 with the library's built-in launch modes (ops.AUTOTUNE =
    False: no tuning launches), nothing timed here: what a profiler around this process sees"""
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    from sgic_amd import fid, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_fid needs the GPU: there is nothing to trace without one")
    N, passes = (int(v) for v in spec.split(":"))
    ops.AUTOTUNE = False
    a, _ = pairs(N, 256, 256, 3)
    model = fid.InceptionFID(fid.synth_weights(1234), DEV)
    for _ in range(passes):
        f = model.features(a)
    torch.cuda.synchronize()
    print(json.dumps({"what": "trace pass", "windows": N, "passes": passes, "feature_sum": float(f.double().sum())}), flush=True)
    return 0


def trace_table(db, out, note):
    """the profiler's database of a --trace-pass run -> the per-kernel table (share, calls, total ms, kernel), kernels under 0.05 % left out"""
    import re
    import sqlite3
    c = sqlite3.connect(db)
    rows = c.execute("select name, total_calls, percentage from top_kernels order by total_duration desc").fetchall()
    total_ns = c.execute("select sum(duration) from kernels").fetchone()[0]

    def short(n):
        n = n.replace("void ", "").replace("(anonymous namespace)::", "")
        return re.split(r"\((?=[a-zA-Z ]*(const|\*|int|float|unsigned|S3Args))", n)[0]
    lines = [f"# rocprofv3 --kernel-trace --stats -d DIR -o fid -- python tools/bench_fid.py --trace-pass {note}; then --trace-table DIR/fid_results.db",
             "# ops.AUTOTUNE = False (the library's built-in launch modes, no tuning launches in the trace); 1 x MI355X",
             f"# total kernel time {total_ns / 1e6:.2f} ms over {sum(r[1] for r in rows)} dispatches",
             "# share %  calls  total ms  kernel"]
    lines += [f"{pct:6.2f}  {calls:5d}  {pct / 100 * total_ns / 1e6:8.3f}  {short(n)}" for n, calls, pct in rows if pct >= 0.05]
    with open(out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_fid needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"feat": point_feat, "tail": point_tail, "decode": point_decode}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=300, help="seconds each point may take")
    ap.add_argument("--trace-pass", default=None, metavar="N:P", help="P untimed passes over N windows in this process, for a profiler around it")
    ap.add_argument("--trace-table", default=None, metavar="DB", help="the profiler's database of a --trace-pass run -> the per-kernel table")
    ap.add_argument("--trace-note", default="64:8", help="the N:P the database was taken with (goes into the table's header)")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    if args.trace_pass:
        return trace_pass(args.trace_pass)
    if args.trace_table:
        out = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "fid_kernels.txt")
        return trace_table(args.trace_table, out, args.trace_note)
    points = ["feat:4:2", "tail:64:1"] if args.quick else ["feat:64:5", "feat:256:3", "tail:4096:3", "decode:256:64:3"]
    lines = ["# tools/bench_fid.py; ms per call, two repeats each, InceptionFID.features and its torch counterpart alternating in one "
             "process per point"]
    recs = []
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
        recs.append(json.loads(lines[-1]))
        print(lines[-1], flush=True)
    ok = len(recs) == len(points)
    tail = [q for q in recs if "fid_wall_ms" in q]
    for r in recs:          # features (+ the tail, once per evaluation) as a share of the decode_batch that feeds them
        d = [q for q in recs if "decode_ms" in q]
        if "fid_ms" in r and d:      # the decode of as many 256 x 256 images as there are windows, in batches of the measured size
            dec = min(d[0]["decode_ms"]) * r["windows"] / d[0]["B"]
            rec = {"what": "FID features as a share of decode_batch", "windows": r["windows"], "decode_batches_of": d[0]["B"],
                   "share": min(r["fid_ms"]) / dec}
            if tail:
                rec["fid_and_kid_at_4096_over_this_decode"] = (tail[0]["fid_wall_ms"] + tail[0]["kid_wall_ms"]) / dec
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    if not ok:
        print(lines[-1], file=sys.stderr, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
