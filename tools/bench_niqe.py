#!/usr/bin/env python3
"""Time the fused NIQE block sums (csrc/niqe.hip: ops.niqe_blocks_u8) against a torch fp64 version of the same definition on the
device (integer luma, the eight-tap half-size plane, the ten class sums from 49 shifted slices, MSCN, the five maps of every block
and their masked sums), device time only.

Protocol (that of tools/bench_quality.py): seeded u8 images made on the device, B = 32 at 256^2 and B = 8 at 1024^2; both paths
warmed up, then timed with device events in one process, alternating, twice (both repeats are reported, they show the spread).  Every
point runs in a child process of its own under a time limit; the first point that fails ends the run.

  niqe      ops.niqe_blocks_u8 against torch_niqe.  Required: not slower than the torch version beyond that version's own
            repeat-to-repeat spread.  Whether the counts are equal and the largest relative difference of a sum are reported.
  decode    one Codec.decode_batch (LARGE architecture, synthetic weights) of the same batch: what the measurement rides on in
            evaluate.py.  No pass mark.

    python tools/bench_niqe.py [--quick] [--out profiles/niqe.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_quality import point_decode  # noqa: E402
from bench_search_range import DEV, alternate  # noqa: E402


def images(B, H, W, seed):
    """a smooth random field plus noise of +-4: (B, H, W, 3) u8 on the device"""
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    low = torch.rand(B, 3, H // 16 + 2, W // 16 + 2, generator=g, device=DEV)
    a = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    a = (a * 255).round().permute(0, 2, 3, 1).contiguous()
    return (a + torch.randint(-4, 5, a.shape, generator=g, device=DEV)).clamp(0, 255).to(torch.uint8)


def torch_niqe(x, weights):
    """the counterpart: the same definition with torch ops, fp64 and int64 -> (stats (B, nbh, nbw, 2, 5, 5), sharp (B, nbh, nbw))"""
    import torch
    import torch.nn.functional as F
    B, H, W, _ = x.shape
    nbh, nbw = H // 96, W // 96
    v = x[:, :nbh * 96, :nbw * 96].to(torch.int64)
    n = 65481 * v[..., 0] + 128553 * v[..., 1] + 24966 * v[..., 2]
    q, r = n // 255000, n % 255000
    y = 16 + q + ((2 * r > 255000) | ((2 * r == 255000) & (q % 2 == 1))).to(torch.int64)
    taps = torch.tensor([-3, -9, 29, 111, 111, 29, -9, -3], dtype=torch.int64, device=x.device)

    def half_axis(p):      # along the last axis, symmetric extension
        m = p.shape[-1]
        idx = torch.arange(-3, m + 3, device=x.device)
        idx = torch.where(idx < 0, -idx - 1, torch.where(idx >= m, 2 * m - 1 - idx, idx))
        e = p[..., idx]
        return sum(taps[k] * e[..., k:k + m:2][..., :m // 2] for k in range(8))

    h = half_axis(half_axis(y).transpose(1, 2)).transpose(1, 2)
    stats = torch.empty(B, nbh, nbw, 2, 5, 5, dtype=torch.float64, device=x.device)
    sharp = None
    order = [(a, b) for a in range(4) for b in range(a, 4)]
    for s, (plane, unit) in enumerate(((y, 1.0), (h, 2.0 ** -16))):
        Hs, Ws = plane.shape[1:]
        pad = F.pad(plane.to(torch.float64).unsqueeze(1), (3, 3, 3, 3), mode="replicate").squeeze(1)      # integers below 2^53: exact
        c = pad[:, 3:3 + Hs, 3:3 + Ws]
        ssum = [torch.zeros_like(c) for _ in range(10)]
        qsum = [torch.zeros_like(c) for _ in range(10)]
        for di in range(-3, 4):
            for dj in range(-3, 4):
                k = order.index(tuple(sorted((abs(di), abs(dj)))))
                d = pad[:, 3 + di:3 + di + Hs, 3 + dj:3 + dj + Ws] - c
                ssum[k] = ssum[k] + d
                qsum[k] = qsum[k] + d * d
        m = torch.zeros_like(c)
        var = torch.zeros_like(c)
        for k in range(10):
            m = m + weights[k] * (ssum[k] * unit)
            var = var + weights[k] * (qsum[k] * (unit * unit))
        sigma = torch.sqrt(torch.abs(var - m * m))
        S = 96 >> s
        blk = ((0.0 - m) / (sigma + 1.0)).view(B, nbh, S, nbw, S).permute(0, 1, 3, 2, 4)
        maps = [blk] + [blk * torch.roll(blk, sh, dims=(3, 4)) for sh in ((0, 1), (1, 0), (1, 1), (1, -1))]
        for k, mp in enumerate(maps):
            neg, pos, sq = mp < 0, mp > 0, mp * mp
            stats[:, :, :, s, k, 0] = neg.sum(dim=(3, 4))
            stats[:, :, :, s, k, 1] = pos.sum(dim=(3, 4))
            stats[:, :, :, s, k, 2] = (sq * neg).sum(dim=(3, 4))
            stats[:, :, :, s, k, 3] = (sq * pos).sum(dim=(3, 4))
            stats[:, :, :, s, k, 4] = mp.abs().sum(dim=(3, 4))
        if s == 0:
            sharp = sigma.view(B, nbh, S, nbw, S).permute(0, 1, 3, 2, 4).sum(dim=(3, 4)) / (S * S)
    return stats, sharp


def point_niqe(size, B, iters):
    import torch
    from sgic_amd import niqe, ops
    x = images(B, size, size, 3)
    w = niqe.window_weights()
    new = lambda: ops.niqe_blocks_u8(x)                     # noqa: E731
    old = lambda: torch_niqe(x, w)                          # noqa: E731
    (s1, h1), (s0, h0) = new(), old()
    equal = bool(torch.equal(s1[..., :2], s0[..., :2]))
    rel = float(((s1[..., 2:] - s0[..., 2:]).abs() / s0[..., 2:].abs().clamp_min(1e-300)).max())
    rel_sharp = float(((h1 - h0).abs() / h0.abs().clamp_min(1e-300)).max())
    new()
    old()
    tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": "niqe_blocks_u8 vs torch fp64 on the device", "B": B, "H": size, "W": size, "iters": iters, "niqe_ms": tn,
            "torch_ms": to, "torch_spread_ms": spread, "ratio": min(to) / min(tn), "counts_equal": equal,
            "largest_relative_difference_of_a_sum": rel, "largest_relative_difference_of_sharpness": rel_sharp,
            "required": "not slower than torch beyond its own spread: min(niqe) <= min(torch) + spread",
            "met": bool(equal and min(tn) <= min(to) + spread)}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_niqe needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"niqe": point_niqe, "decode": point_decode}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "niqe.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    points = ["niqe:192:2:3"] if args.quick else ["niqe:256:32:50", "niqe:1024:8:20", "decode:256:32:5", "decode:1024:8:3"]
    lines = ["# tools/bench_niqe.py; ms per call, two repeats each, the fused call and its torch counterpart alternating in one "
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
