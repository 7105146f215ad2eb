"""CLIP preprocessing from the u8 canvas (ClipHIP.preprocess_u8) against the route through the fp32 image
(ops.u8canvas_to_f32chw_pad + ClipHIP.preprocess(hw=)), on the same canvas, both routes alternating in one process; and, third in
the rotation, the call compress makes for a batch of one size (ClipHIP.preprocess(x) on the unpadded fp32 batch).
Device events around `iters` back-to-back calls, after a warm-up; two repeats, both reported.  The algorithmic bytes of the new
route -- the canvas bytes of the row window it reads, the u8 intermediate written and read, the fp32 output -- over its time give
its share of the 6.3 TB/s HBM peak (they say nothing of the table reads, which stay in cache).
The event times are HOST-INCLUSIVE: each call runs its Python side (geometry, two ctypes calls, allocations, three to five launches)
between the events, and at these sizes that can be longer than the kernels.  The device-only times come from a run of its own under
the profiler, one case at a time, summed per route from the kernel statistics:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/bench_clip_u8.py 50 32 256
usage: python tools/bench_clip_u8.py [iters=200] [B size]      (no B size: B = 32 at 256, B = 8 at 1024 and B = 1 at 256)"""
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sgic_amd  # noqa
from sgic_amd import ops
from sgic_amd import weights as W
from sgic_amd.clip import ClipHIP, pil_coeffs, resize_geometry
from sgic_amd.config import CLIP_B32

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
HBM_PEAK = 6.3e12
if not torch.cuda.is_available():
    sys.exit("bench_clip_u8 needs the GPU: there is no CPU path to time")
dev = torch.device("cuda:0")
# the preprocessing does not touch the tower's weights; a two-layer tower keeps the set-up short
cfg = dataclasses.replace(CLIP_B32, layers=2)
clip = ClipHIP(W.synth_weights(W.clip_spec(cfg), seed=5), cfg, dev)
S = cfg.image_size


def algorithmic_bytes(hw):
    total = 0
    for h, w in hw:
        OH, OW, top, left = resize_geometry(h, w, S)
        bh, _, _ = pil_coeffs(w, OW)
        bv, _, _ = pil_coeffs(h, OH)
        rows = int(bv[top + S - 1].sum() - bv[top, 0])
        cols = int(bh[left + S - 1].sum() - bh[left, 0])
        total += 3 * rows * cols + 2 * 3 * rows * S + 12 * S * S
    return total


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e3     # microseconds per call


CASES = [(int(sys.argv[2]), int(sys.argv[3]))] if len(sys.argv) > 3 else [(32, 256), (8, 1024), (1, 256)]
for B, side in CASES:
    rng = np.random.default_rng(side)
    canvas = torch.from_numpy(rng.integers(0, 256, (B, side, side, 3), dtype=np.uint8)).to(dev)
    hw = [(side, side)] * B
    new = lambda: clip.preprocess_u8(canvas, hw)
    old = lambda: clip.preprocess(ops.u8canvas_to_f32chw_pad(canvas, hw, side, side), hw=hw)
    x = ops.u8canvas_to_f32chw_pad(canvas, hw, side, side)
    uniform = lambda: clip.preprocess(x)
    for _ in range(10):
        new(), old(), uniform()
    torch.cuda.synchronize()
    nbytes = algorithmic_bytes(hw)
    for rep in range(2):
        t_new, t_old, t_uni = timed(new), timed(old), timed(uniform)
        print(json.dumps({"B": B, "size": side, "repeat": rep, "iters": ITERS, "preprocess_u8_us": round(t_new, 2),
                          "via_fp32_image_us": round(t_old, 2), "uniform_fp32_us": round(t_uni, 2), "times": "host-inclusive (device events around Python calls)", "ratio_old_over_new": round(t_old / t_new, 2),
                          "algorithmic_bytes": nbytes, "share_of_hbm_peak": round(nbytes / (t_new * 1e-6) / HBM_PEAK, 4)}), flush=True)
