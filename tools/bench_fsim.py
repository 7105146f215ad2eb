#!/usr/bin/env python3
"""Time FSIM / FSIMc of evaluate.py --fsim (csrc/fsim.hip: ops.fsim, ops.fsim_phasecong, ops.fsim_planes_u8), device time only, and
set the transform against the time its flops would take at the fp64 rate of the chip.

Protocol (that of tools/bench_hvs.py): seeded u8 pairs made on the device, B = 32 at 256 x 256 and at 768 x 512 (F = 2: 384 x 256
after the reduction); every entry point warmed up, then timed with device events around `iters` back-to-back calls, the entry points
alternating, twice (both repeats are reported, they show the spread).  Every point runs in a child process of its own under a time
limit; the first point that fails ends the run.

  entry     ms per call of ops.fsim (the whole measure of B pairs), ops.fsim_phasecong (the PC maps of the 2 B reduced Y planes) and
            ops.fsim_planes_u8; transform_flop = 17 transforms per plane (one forward, sixteen inverse) of 8 h w (h + w) flop each,
            2 B planes; bound_ms = transform_flop / 78.6 TFLOP/s, the specified fp64 vector rate (the fp64 matrix rate is the same
            figure).  No pass mark: the numbers are for DESIGN.md section 21.
  decode    one Codec.decode_batch (LARGE architecture, synthetic weights) of as many images of the same size: what the measurement
            rides on in evaluate.py
  kernels   ops.fsim `iters` times and nothing else: the workload to run under `rocprofv3 --kernel-trace --stats`, whose
            kernel_stats CSV `--fold` turns into us per kernel (the trace adds a few us to every dispatch's timestamps)

    python tools/bench_fsim.py [--quick] [--out profiles/fsim.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fsim -- python tools/bench_fsim.py --point kernels:768:512:32:3
    python tools/bench_fsim.py --fold DIR/.../fsim_kernel_stats.csv"""
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
from bench_search_range import DEV, alternate  # noqa: E402

FP64_FLOP_PER_MS = 78.6e9      # 78.6 TFLOP/s, the specified fp64 vector peak
KERNELS = ("fsim_planes_kernel", "fsim_flat_kernel", "fsim_filter_kernel", "fsim_fstat_kernel", "fsim_dft_pass_kernel",
           "fsim_threshold_kernel", "fsim_pc_kernel", "fsim_pool_kernel", "fsim_final_kernel")
MODES = ("FWD_REAL", "FWD_CPLX", "INV_FILT", "INV_LAST")


def transform_flop(B, H, W):
    """the flop of the dense transforms of B pairs of H x W: per plane 17 two-pass transforms of 8 h w (h + w) (a complex
    multiply-add is 8 flop; the real forward pass is counted as complex)"""
    from sgic_amd.quality import fsim_reduction
    _, h, w = fsim_reduction(H, W)
    return 2 * B * 17 * 8 * h * w * (h + w)


def point_entry(H, W, B, iters):
    from sgic_amd import ops
    a, b = pairs(B, H, W, 3)
    ys = torch_cat_y(ops.fsim_planes_u8(a), ops.fsim_planes_u8(b))
    fns = {"fsim": lambda: ops.fsim(a, b), "phasecong": lambda: ops.fsim_phasecong(ys), "planes": lambda: ops.fsim_planes_u8(a)}
    for fn in fns.values():
        fn()
        fn()
    times = alternate(tuple(fns.values()), iters)
    flop = transform_flop(B, H, W)
    rec = {"what": "entry points of csrc/fsim.hip, device events around back-to-back calls", "B": B, "H": H, "W": W, "iters": iters,
           "reduced": list(ys.shape[1:]), "transform_flop": flop, "bound_ms": flop / FP64_FLOP_PER_MS}
    for (k, _), t in zip(fns.items(), times):
        rec[k] = {"ms": t}
    rec["phasecong"]["share_of_bound"] = rec["bound_ms"] / min(rec["phasecong"]["ms"])
    rec["bound"] = "transform_flop / 78.6 TFLOP/s (fp64 vector, specified)"
    return rec


def torch_cat_y(pa, pb):
    import torch
    return torch.cat([pa[:, 0], pb[:, 0]]).contiguous()


def point_decode(H, W, B, iters):
    from sgic_amd import weights as Wt
    from sgic_amd.codec import Codec
    from sgic_amd.config import LARGE
    from sgic_amd.data import synth_images
    codec = Codec(Wt.synth_weights(Wt.full_spec(LARGE), seed=1234), LARGE, DEV)
    codec.hybrid_codec.quantize_feat.force_zero_thres = 0.12
    codec.hybrid_codec.quantize_feat.update(force=True)
    enc = codec.encode_batch(synth_images(B, H, W, 7).to(DEV))
    run = lambda: codec.decode_batch(enc)                   # noqa: E731
    run()
    run()
    (t,) = alternate((run,), iters)
    return {"what": "Codec.decode_batch, LARGE architecture, synthetic weights (bitstreams -> x_hat on the device)", "B": B, "H": H,
            "W": W, "iters": iters, "decode_ms": t}


def point_kernels(H, W, B, iters):
    import torch
    from sgic_amd import ops
    a, b = pairs(B, H, W, 3)
    for _ in range(iters):
        ops.fsim(a, b)
    torch.cuda.synchronize()
    return {"what": "the workload for rocprofv3 --kernel-trace --stats", "B": B, "H": H, "W": W, "calls_of_fsim": iters,
            "transform_flop_per_call": transform_flop(B, H, W)}


def fold(path):
    """a kernel_stats CSV of rocprofv3 -> one line per kernel of csrc/fsim.hip: calls, total / average / min / max us"""
    out = []
    with open(path, newline="", encoding="utf-8") as fh:
        for row in csv.DictReader(fh):
            name = next((k for k in KERNELS if k in row["Name"]), None)
            if name:
                m = re.search(name + r"<\(?[^>]*?(\d)\)?>", row["Name"])
                label = name + (f"<{MODES[int(m.group(1))]}>" if m and name == "fsim_dft_pass_kernel" else "")
                out.append({"kernel": label, "calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3,
                            "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                            "max_us": float(row["MaxNs"]) / 1e3})
    return sorted(out, key=lambda r: r["kernel"])


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_fsim needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"entry": point_entry, "decode": point_decode, "kernels": point_kernels}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsim.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--fold", default=None, help="print the kernels of csrc/fsim.hip from a rocprofv3 kernel_stats CSV, one JSON line each")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.fold:
        for r in fold(args.fold):
            print(json.dumps(r))
        return 0
    if args.point:
        return run_point(args.point)
    points = ["entry:64:48:2:3"] if args.quick else ["entry:256:256:32:10", "entry:768:512:32:4", "decode:256:256:32:5", "decode:768:512:32:2"]
    lines = ["# tools/bench_fsim.py; ms per call by device events around back-to-back calls, two repeats each, the entry points "
             "alternating in one process per point; bound_ms = transform_flop / 78.6 TFLOP/s"]
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
