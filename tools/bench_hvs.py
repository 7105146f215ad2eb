#!/usr/bin/env python3
"""Time the luma measures of evaluate.py --hvs (csrc/hvs.hip: ops.hvs_luma_u8, hvs_vifp, hvs_gmsd, hvs_psnr), device time only, and
set every entry point against the time its compulsory bytes would take at the HBM's rate.

Protocol (that of tools/bench_quality.py): seeded u8 pairs made on the device, B = 32 at 256^2 and at 1024^2; every entry point
warmed up, then timed with device events around `iters` back-to-back calls, the four alternating, twice (both repeats are reported,
they show the spread).  Every point runs in a child process of its own under a time limit; the first point that fails ends the run.

  entry     us per call of each entry point, the bytes it has to move (bytes_moved below: every input read once, every plane of
            VIFp's pyramid written once and read by its two consumers, the partial sums) and bound_us = bytes / 8.0 TB/s, the HBM's
            specified rate.  At these sizes the planes fit the 256 MiB Infinity Cache, so the bound is a floor for data that comes
            from HBM, not a prediction.  No pass mark: the numbers are for DESIGN.md section 20.
  kernels   the same calls, `iters` times each and nothing else: the workload to run under `rocprofv3 --kernel-trace --stats`,
            whose kernel_stats CSV `--fold` turns into us per kernel (the trace adds a few us to every dispatch's timestamps)

    python tools/bench_hvs.py [--quick] [--out profiles/hvs.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o hvs -- python tools/bench_hvs.py --point kernels:1024:32:20
    python tools/bench_hvs.py --fold DIR/.../hvs_kernel_stats.csv"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_quality import pairs  # noqa: E402
from bench_search_range import alternate  # noqa: E402

HBM_BYTES_PER_US = 8.0e6      # 8.0 TB/s, the specified peak
KERNELS = ("hvs_luma_kernel", "vif_stats_kernel", "vif_down_kernel", "hvs_sum2_kernel", "gmsd_tile_kernel", "gmsd_final_kernel",
           "psnr_hvs_kernel")


def bytes_moved(B, H, W):
    """the compulsory traffic of each entry point for B pairs of H x W, in bytes (fp64 planes; partial sums per 16 x 32 tile or
    32-block group are counted, they are small)"""
    n = B * H * W
    h, w, pyr, tiles = H, W, 0, 0
    for s, N in enumerate((17, 9, 5, 3)):
        if s:
            h, w = (h - N + 2) // 2, (w - N + 2) // 2
            pyr += 2 * 8 * B * h * w * (3 if s < 3 else 2)      # written once, read by the statistics and (but the last) the next filter
        tiles += -(-(h - N + 1) // 16) * -(-(w - N + 1) // 32)
    gt = -(-((H + 1) // 2) // 16) * -(-((W + 1) // 2) // 32)
    groups = -(-((H // 8) * (W // 8)) // 32)
    return {"luma": 11 * n, "vifp": 16 * n + pyr + 2 * 16 * B * tiles, "gmsd": 16 * n + 2 * 24 * B * gt,
            "psnr": 16 * B * (H // 8) * (W // 8) * 64 + 2 * 16 * B * groups}


def calls(size, B):
    from sgic_amd import ops
    from sgic_amd.jpeg_enc import _LUMA
    a, b = pairs(B, size, size, 3)
    ya, yb = ops.hvs_luma_u8(a), ops.hvs_luma_u8(b)
    return {"luma": lambda: ops.hvs_luma_u8(a), "vifp": lambda: ops.hvs_vifp(ya, yb), "gmsd": lambda: ops.hvs_gmsd(ya, yb),
            "psnr": lambda: ops.hvs_psnr(ya, yb, _LUMA)}


def point_entry(size, B, iters):
    fns = calls(size, B)
    for fn in fns.values():
        fn()
        fn()
    times = alternate(tuple(fns.values()), iters)
    moved = bytes_moved(B, size, size)
    rec = {"what": "entry points of csrc/hvs.hip, device events around back-to-back calls", "B": B, "H": size, "W": size, "iters": iters}
    for (k, _), t in zip(fns.items(), times):
        rec[k] = {"us": [1e3 * v for v in t], "bytes_moved": moved[k], "bound_us": moved[k] / HBM_BYTES_PER_US,
                  "share_of_bound": moved[k] / HBM_BYTES_PER_US / (1e3 * min(t))}
    rec["bound"] = "bytes_moved / 8.0 TB/s (HBM, specified); luma is one of the two planes a pair needs"
    return rec


def point_kernels(size, B, iters):
    import torch
    fns = calls(size, B)
    for fn in fns.values():
        for _ in range(iters):
            fn()
    torch.cuda.synchronize()
    return {"what": "the workload for rocprofv3 --kernel-trace --stats", "B": B, "H": size, "W": size, "calls_of_each_entry_point": iters}


def fold(path):
    """a kernel_stats CSV of rocprofv3 -> one line per kernel of csrc/hvs.hip: calls, average / min / max us"""
    out = []
    with open(path, newline="", encoding="utf-8") as fh:
        for row in csv.DictReader(fh):
            name = next((k for k in KERNELS if k in row["Name"]), None)
            if name:
                out.append({"kernel": re.search(name + r"(<\d+>)?", row["Name"]).group(0),
                            "calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                            "max_us": float(row["MaxNs"]) / 1e3})
    return sorted(out, key=lambda r: r["kernel"])


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_hvs needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"entry": point_entry, "kernels": point_kernels}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hvs.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--fold", default=None, help="print the kernels of csrc/hvs.hip from a rocprofv3 kernel_stats CSV, one JSON line each")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.fold:
        for r in fold(args.fold):
            print(json.dumps(r))
        return 0
    if args.point:
        return run_point(args.point)
    points = ["entry:64:2:3"] if args.quick else ["entry:256:32:200", "entry:1024:32:50"]
    lines = ["# tools/bench_hvs.py; us per call by device events around back-to-back calls, two repeats each, the entry points "
             "alternating in one process per point; bound_us = bytes_moved / 8.0 TB/s"]
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
