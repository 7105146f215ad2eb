"""CLI-level throughput of the compress driver (files -> .c2df): N synthetic JPEG files on local disk ->
`sgic_amd.compress.main` with the production architecture -> the driver's own JSON record (images/s including the header
pass, JPEG decode, H2D, GPU work, container and .npy writes, index assembly excluded from the rate's clock).
usage: python tools/cli_throughput.py [N=960] [size=256] [batch=32] [--progressive] [--gpu_progressive_jpeg] [--mixed]
  --progressive            write the corpus as progressive JPEG (libjpeg's standard script) instead of baseline
  --gpu_progressive_jpeg   pass the driver's switch of that name (progressive batches decoded on the GPU instead of the host)
  --mixed                  three legs in one process: the uniform corpus (N files size x size) at `batch`, a mixed corpus (N files of
                           all-distinct sizes H, W in size-63 .. size, so all pad to the size x size geometry) at `batch`, and the
                           uniform corpus at --batch_size 1 (how an exact-size planner runs the mixed corpus); each leg reports its
                           record and torch.cuda.max_memory_allocated"""
import gc
import io
import json
import os
import sys
import tempfile
import time
from contextlib import redirect_stdout

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

import sgic_amd  # noqa
from sgic_amd import compress
from sgic_amd.data import synth_images

FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
POS = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(POS[0]) if len(POS) > 0 else 960
S = int(POS[1]) if len(POS) > 1 else 256
B = int(POS[2]) if len(POS) > 2 else 32
PROGRESSIVE = "--progressive" in FLAGS
MIXED = "--mixed" in FLAGS
EXTRA = ["--gpu_progressive_jpeg"] if "--gpu_progressive_jpeg" in FLAGS else []


def write_corpus(src, sizes):
    os.makedirs(src)
    base = ((synth_images(64, S, S, 3) * 0.5 + 0.5) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    t0 = time.perf_counter()
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(np.ascontiguousarray(np.roll(base[i % 64], i // 64, axis=0)[:h, :w])).save(
            os.path.join(src, f"im{i:05d}.jpg"), quality=90, progressive=PROGRESSIVE)
    print(f"wrote {len(sizes)} JPEGs ({len(set(sizes))} sizes, up to {S}x{S}) in {time.perf_counter() - t0:.1f}s", file=sys.stderr, flush=True)


def run(src, out, batch, leg, passes=2):
    for rep in range(passes):          # the second pass runs with a warm tile cache and page cache: the steady-state CLI rate
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        buf = io.StringIO()
        t0 = time.perf_counter()
        with redirect_stdout(buf):
            rc = compress.main(["--dataset_dir", src, "--save_dir", f"{out}_{leg}_{rep}", "--batch_size", str(batch)] + EXTRA)
        wall = time.perf_counter() - t0
        rec = json.loads(buf.getvalue().strip().splitlines()[-1])
        rec.update(rc=rc, pass_=rep, wall_incl_model_build_s=round(wall, 2), size=S, progressive_corpus=PROGRESSIVE, flags=EXTRA,
                   leg=leg, max_memory_allocated_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                   peak_above_leg_start_gib=round((torch.cuda.max_memory_allocated() - start) / 2 ** 30, 2))
        print(json.dumps(rec), flush=True)


with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, "out")
    write_corpus(os.path.join(tmp, "in"), [(S, S)] * N)
    if not MIXED:
        run(os.path.join(tmp, "in"), out, B, "uniform")
    else:
        side = np.arange(max(1, S - 63), S + 1)
        if N > len(side) ** 2:
            sys.exit(f"--mixed: at most {len(side) ** 2} distinct sizes in {side[0]}..{S}")
        pick = np.random.default_rng(0).choice(len(side) ** 2, N, replace=False)
        write_corpus(os.path.join(tmp, "mixed"), [(int(side[k // len(side)]), int(side[k % len(side)])) for k in pick])
        run(os.path.join(tmp, "in"), out, B, "uniform")
        run(os.path.join(tmp, "mixed"), out, B, "mixed")
        run(os.path.join(tmp, "in"), out, 1, "uniform_b1")
