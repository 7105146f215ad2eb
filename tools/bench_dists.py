#!/usr/bin/env python3
"""Time DISTS-VGG on the GPU (dists.DistsVGG.measure: split 3x3 convolutions + csrc/dists.hip) against a torch fp32 version of the
same definition on the device (F.conv2d, the L2 pool as a depthwise F.conv2d, the head as tensor expressions), device time only.

Protocol (that of tools/bench_lpips.py): seeded u8 pairs made on the device, B = 32 at 256^2 and B = 8 at 1024^2; synthetic weights;
both paths warmed up (which also settles the convolutions' launch modes), then timed with device events in one process, alternating,
twice (both repeats are reported, they show the spread).  Every point runs in a child process of its own under a time limit; the
first point that fails ends the run.

  dists     DistsVGG.measure against torch_dists.  Required: not slower than the torch version beyond that version's own
            repeat-to-repeat spread.  The largest relative difference of the score between the two is reported.
  decode    one Codec.decode_batch (LARGE architecture, synthetic weights) of the same batch: what the measurement rides on in
            evaluate.py.  No pass mark; the parent adds DISTS's share of it.

    python tools/bench_dists.py [--quick] [--out profiles/dists.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_quality import pairs, point_decode  # noqa: E402
from bench_search_range import DEV, alternate  # noqa: E402


def torch_dists(a, b, sd, chunk):
    """the counterpart: the definition with torch ops in fp32 on the device, both sides of `chunk` pairs per pass -> dists (B,)"""
    import torch
    import torch.nn.functional as F
    from sgic_amd import dists, lpips
    mean = torch.tensor([0.485, 0.456, 0.406], device=a.device).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=a.device).view(1, 3, 1, 1)
    hann = torch.tensor([1.0, 2.0, 1.0], device=a.device)
    hann = (hann[:, None] * hann[None, :] / 16.0).view(1, 1, 3, 3)
    alpha, beta = torch.split(sd["alpha"], dists.TAP_CH), torch.split(sd["beta"], dists.TAP_CH)
    W = sd["alpha"].sum() + sd["beta"].sum()
    out = torch.zeros(a.shape[0], dtype=torch.float32, device=a.device)

    def term(f, n, al, be):
        x, y = f[:n], f[n:]
        mx, my = x.mean(dim=(2, 3)), y.mean(dim=(2, 3))
        vx, vy = (x * x).mean(dim=(2, 3)) - mx * mx, (y * y).mean(dim=(2, 3)) - my * my
        cxy = (x * y).mean(dim=(2, 3)) - mx * my
        S1 = (2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6)
        S2 = (2 * cxy + 1e-6) / (vx + vy + 1e-6)
        return (al * (1 - S1)).sum(dim=1) + (be * (1 - S2)).sum(dim=1)

    for s in range(0, a.shape[0], chunk):
        n = min(chunk, a.shape[0] - s)
        x = torch.cat([a[s:s + n], b[s:s + n]]).permute(0, 3, 1, 2).float() / 255.0
        out[s:s + n] += term(x, n, alpha[0], beta[0])
        x = (x - mean) / std
        tap = 1
        for j, i in enumerate(lpips.CONV_IDX):
            x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"], sd[f"features.{i}.bias"], padding=1))
            if j in lpips.TAP_AFTER:
                out[s:s + n] += term(x, n, alpha[tap], beta[tap])
                tap += 1
            if j in lpips.POOL_AFTER:
                x = torch.sqrt(F.conv2d(x * x, hann.expand(x.shape[1], 1, 3, 3), stride=2, padding=1, groups=x.shape[1]) + 1e-12)
    return out / W


def point_dists(size, B, iters):
    import numpy as np
    from sgic_amd import dists, lpips
    a, b = pairs(B, size, size, 3)
    sd = dists.synth_weights(1234)
    model = dists.DistsVGG(sd, DEV)
    dsd = {k: v.to(DEV) for k, v in sd.items()}
    chunk = max(1, lpips.MAX_PIXELS // (2 * size * size))        # the same pixel bound for both
    new = lambda: model.measure(a, b)                       # noqa: E731
    old = lambda: torch_dists(a, b, dsd, chunk).cpu()       # noqa: E731 -- one read-back, like measure
    d1, d0 = new()[0], old().double().numpy()
    diff = float((np.abs(d1 - d0) / d0).max())
    for _ in range(2):
        new()
        old()
    tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": "DistsVGG.measure vs torch fp32 on the device", "B": B, "H": size, "W": size, "iters": iters, "pairs_per_chunk": chunk,
            "dists_ms": tn, "torch_ms": to, "torch_spread_ms": spread, "ratio": min(to) / min(tn), "largest_relative_difference": diff,
            "mean_dists": float(d1.mean()),
            "required": "not slower than torch beyond its own spread: min(dists) <= min(torch) + spread", "met": bool(min(tn) <= min(to) + spread)}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_dists needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"dists": point_dists, "decode": point_decode}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dists.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    points = ["dists:64:2:3"] if args.quick else ["dists:256:32:10", "dists:1024:8:5", "decode:256:32:5", "decode:1024:8:3"]
    lines = ["# tools/bench_dists.py; ms per call, two repeats each, DistsVGG.measure and its torch counterpart alternating in one "
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
    for r in recs:          # DISTS as a share of the decode_batch that feeds it
        d = [q for q in recs if "decode_ms" in q and (q["B"], q["H"]) == (r["B"], r["H"])]
        if "dists_ms" in r and d:
            lines.append(json.dumps({"what": "DISTS as a share of decode_batch", "B": r["B"], "H": r["H"], "W": r["W"],
                                     "share": min(r["dists_ms"]) / min(d[0]["decode_ms"])}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
