#!/usr/bin/env python3
"""Time the fused quality measurement (csrc/quality.hip: ops.quality_u8) against a torch fp64 version of the same definition on the
device (squared error, five levels of avg_pool2d, depthwise 11-tap filters, ssim / cs maps and their means), device time only.

Protocol (that of tools/bench_cluster.py): seeded u8 pairs made on the device, B = 32 at 256^2 and B = 8 at 1024^2; both paths warmed
up, then timed with device events in one process, alternating, twice (both repeats are reported, they show the spread).  Every point
runs in a child process of its own under a time limit; the first point that fails ends the run.

  quality   ops.quality_u8 against torch_quality.  Required: not slower than the torch version beyond that version's own
            repeat-to-repeat spread.  The largest difference of a level value between the two is reported.
  decode    one Codec.decode_batch (LARGE architecture, synthetic weights) of the same batch: what the measurement rides on in
            evaluate.py.  No pass mark.

    python tools/bench_quality.py [--quick] [--out profiles/quality.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_search_range import DEV, alternate  # noqa: E402


def pairs(B, H, W, seed):
    """a smooth random field and the same with noise of +-12: (B, H, W, 3) u8 on the device, twice"""
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    low = torch.rand(B, 3, H // 16 + 2, W // 16 + 2, generator=g, device=DEV)
    a = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    a = (a * 255).round().permute(0, 2, 3, 1).contiguous()
    b = (a + torch.randint(-12, 13, a.shape, generator=g, device=DEV)).clamp(0, 255)
    return a.to(torch.uint8), b.to(torch.uint8)


FILTER = {"how": "conv2d"}


def torch_quality(a, b):
    """the counterpart: the same definition with torch ops in fp64 -> (sse (B, 3) int64, levels (B, 3, 5, 2) float64)"""
    import torch
    import torch.nn.functional as F
    d = a.to(torch.int64) - b.to(torch.int64)
    sse = (d * d).sum(dim=(1, 2))
    X = a.permute(0, 3, 1, 2).to(torch.float64) / 255.0
    Y = b.permute(0, 3, 1, 2).to(torch.float64) / 255.0
    g = torch.exp(-(torch.arange(11, dtype=torch.float64, device=a.device) - 5.0) ** 2 / 4.5)
    g = g / g.sum()
    wh, wv = g.view(1, 1, 1, 11).repeat(3, 1, 1, 1), g.view(1, 1, 11, 1).repeat(3, 1, 1, 1)

    def filt(v):
        if FILTER["how"] == "conv2d":
            try:
                return F.conv2d(F.conv2d(v, wh, groups=3), wv, groups=3)
            except RuntimeError:       # no fp64 depthwise convolution in this build: eleven shifted slices per pass
                FILTER["how"] = "slices"
        n = v.shape[3] - 10
        h = sum(g[i] * v[:, :, :, i:i + n] for i in range(11))
        m = v.shape[2] - 10
        return sum(g[i] * h[:, :, i:i + m, :] for i in range(11))

    out = torch.empty(a.shape[0], 3, 5, 2, dtype=torch.float64, device=a.device)
    for s in range(5):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
        cs = (2.0 * s12 + 9e-4) / (s1 + s2 + 9e-4)
        ssim = (2.0 * mu1 * mu2 + 1e-4) / (mu1 * mu1 + mu2 * mu2 + 1e-4) * cs
        out[:, :, s, 0] = ssim.flatten(2).mean(-1)
        out[:, :, s, 1] = cs.flatten(2).mean(-1)
        if s < 4:
            pad = [X.shape[2] % 2, X.shape[3] % 2]
            X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    return sse, out


def point_quality(size, B, iters):
    import torch
    from sgic_amd import ops
    a, b = pairs(B, size, size, 3)
    new = lambda: ops.quality_u8(a, b)                      # noqa: E731
    old = lambda: torch_quality(a, b)                       # noqa: E731
    (s1, l1), (s0, l0) = new(), old()
    equal, diff = bool(torch.equal(s1, s0)), float((l1 - l0).abs().max())
    new()
    old()
    tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": "quality_u8 vs torch fp64 on the device", "B": B, "H": size, "W": size, "iters": iters, "quality_ms": tn,
            "torch_ms": to, "torch_spread_ms": spread, "ratio": min(to) / min(tn), "torch_filter": FILTER["how"], "sse_equal": equal,
            "largest_level_difference": diff, "required": "not slower than torch beyond its own spread: min(quality) <= min(torch) + spread",
            "met": bool(equal and min(tn) <= min(to) + spread)}


def point_decode(size, B, iters):
    from sgic_amd import weights as W
    from sgic_amd.codec import Codec
    from sgic_amd.config import LARGE
    from sgic_amd.data import synth_images
    codec = Codec(W.synth_weights(W.full_spec(LARGE), seed=1234), LARGE, DEV)
    codec.hybrid_codec.quantize_feat.force_zero_thres = 0.12
    codec.hybrid_codec.quantize_feat.update(force=True)
    enc = codec.encode_batch(synth_images(B, size, size, 7).to(DEV))
    run = lambda: codec.decode_batch(enc)                   # noqa: E731
    run()
    run()
    (t,) = alternate((run,), iters)
    return {"what": "Codec.decode_batch, LARGE architecture, synthetic weights (bitstreams -> x_hat on the device)", "B": B, "H": size,
            "W": size, "iters": iters, "decode_ms": t, "required": "none (what the measurement rides on)"}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_quality needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"quality": point_quality, "decode": point_decode}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    points = ["quality:192:2:3"] if args.quick else ["quality:256:32:50", "quality:1024:8:20", "decode:256:32:5", "decode:1024:8:3"]
    lines = ["# tools/bench_quality.py; ms per call, two repeats each, the fused call and its torch counterpart alternating in one "
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
