#!/usr/bin/env python3
"""Time LPIPS-Alex on the GPU (lpips_alex.LpipsAlex.measure: patch producers + split GEMMs, split 3x3 convolutions, csrc/lpips_alex.hip
and csrc/lpips.hip) against a torch fp32 version of the same definition on the device (F.conv2d, max_pool2d, the head as tensor
expressions), device time only.

Protocol (that of tools/bench_lpips.py): seeded u8 pairs made on the device, B = 32 at 256^2 and B = 8 at 1024^2; synthetic weights;
both paths warmed up (which also settles the GEMMs' and convolutions' launch modes), then timed with device events in one process,
alternating, twice (both repeats are reported, they show the spread).  Every point runs in a child process of its own under a time
limit; the first point that fails ends the run.

  alex      LpipsAlex.measure against torch_lpips_alex.  Required: not slower than the torch version beyond that version's own
            repeat-to-repeat spread.  The largest relative difference of a layer value between the two is reported.
  decode    one Codec.decode_batch (LARGE architecture, synthetic weights) of the same batch: what the measurement rides on in
            evaluate.py.  No pass mark; the parent adds LPIPS-Alex's share of it.

    python tools/bench_lpips_alex.py [--quick] [--out profiles/lpips_alex.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_quality import pairs, point_decode  # noqa: E402
from bench_search_range import DEV, alternate  # noqa: E402


def torch_lpips_alex(a, b, sd, chunk):
    """the counterpart: the definition with torch ops in fp32 on the device, both sides of `chunk` pairs per pass -> layers (B, 5)"""
    import torch
    import torch.nn.functional as F
    from sgic_amd import lpips_alex
    shift = torch.tensor([-.030, -.088, -.188], device=a.device).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], device=a.device).view(1, 3, 1, 1)
    out = torch.empty(a.shape[0], 5, dtype=torch.float32, device=a.device)
    for s in range(0, a.shape[0], chunk):
        n = min(chunk, a.shape[0] - s)
        x = torch.cat([a[s:s + n], b[s:s + n]]).permute(0, 3, 1, 2).float() / 255.0 * 2.0 - 1.0
        x = (x - shift) / scale
        for j, (i, (_, _, _, stride, pad)) in enumerate(zip(lpips_alex.CONV_IDX, lpips_alex.CONV_CFG)):
            if j in lpips_alex.POOL_BEFORE:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"], sd[f"features.{i}.bias"], stride=stride, padding=pad))
            u = x / (torch.sqrt((x * x).sum(dim=1, keepdim=True)) + 1e-10)
            w = sd[f"lin{j}.model.1.weight"].view(1, -1, 1, 1)
            out[s:s + n, j] = (w * (u[:n] - u[n:]) ** 2).sum(dim=1).mean(dim=(1, 2))
    return out


def point_alex(size, B, iters):
    import numpy as np
    from sgic_amd import lpips_alex, ops
    a, b = pairs(B, size, size, 3)
    sd = lpips_alex.synth_weights(1234)
    model = lpips_alex.LpipsAlex(sd, DEV)
    dsd = {k: v.to(DEV) for k, v in sd.items()}
    chunk = max(1, lpips_alex.MAX_PIXELS // (2 * size * size))        # the same pixel bound for both
    new = lambda: model.measure(a, b)                            # noqa: E731
    old = lambda: torch_lpips_alex(a, b, dsd, chunk).cpu()       # noqa: E731 -- one read-back, like measure
    l1, l0 = new()[1], old().double().numpy()
    diff = float((np.abs(l1 - l0) / l0).max())
    for _ in range(2):
        new()
        old()
    ops.finalize_autotune()                                      # no launch-mode race is left open inside the timed region
    tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": "LpipsAlex.measure vs torch fp32 on the device", "B": B, "H": size, "W": size, "iters": iters, "pairs_per_chunk": chunk,
            "alex_ms": tn, "torch_ms": to, "torch_spread_ms": spread, "ratio": min(to) / min(tn), "largest_relative_layer_difference": diff,
            "mean_lpips_alex": float(l1.sum(axis=1).mean()),
            "required": "not slower than torch beyond its own spread: min(alex) <= min(torch) + spread", "met": bool(min(tn) <= min(to) + spread)}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips_alex needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"alex": point_alex, "decode": point_decode}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_alex.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    points = ["alex:64:2:3"] if args.quick else ["alex:256:32:10", "alex:1024:8:5", "decode:256:32:5", "decode:1024:8:3"]
    lines = ["# tools/bench_lpips_alex.py; ms per call, two repeats each, LpipsAlex.measure and its torch counterpart alternating in one "
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
    for r in recs:          # LPIPS-Alex as a share of the decode_batch that feeds it
        d = [q for q in recs if "decode_ms" in q and (q["B"], q["H"]) == (r["B"], r["H"])]
        if "alex_ms" in r and d:
            lines.append(json.dumps({"what": "LPIPS-Alex as a share of decode_batch", "B": r["B"], "H": r["H"], "W": r["W"],
                                     "share": min(r["alex_ms"]) / min(d[0]["decode_ms"])}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    if not ok:
        print(lines[-1], file=sys.stderr, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
