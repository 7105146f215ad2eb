#!/usr/bin/env python3
"""Time the GPU u8 resize (csrc/resize.hip: ops.resize_u8) against what the host path would do: copy the pixels to the host and
`PIL.Image.resize` them on a pool of 16 threads.  Both sides start from the same u8 images on the device and end with the resized
images in host memory, so the copy of the pixels counts for Pillow and the copy of the result for the kernels.

Protocol (that of tools/bench_jpeg_enc.py): seeded images made on the device; the outputs are compared with Pillow's before any
timing; both paths warmed up, then timed with device events in one process, alternating, twice (both repeats are reported, they show
the spread).  Every point runs in a child process of its own under a time limit; the first point that fails ends the run.

  resize   ops.resize_u8 (+ .cpu()) against the Pillow pool.  Required: not slower than the pool beyond the pool's own
           repeat-to-repeat spread.
  anchor   evaluate.py --anchor jpeg --anchor_optimize on the four textures of tests/test_gpu_evaluate_anchor.py and
           tests/golden/ref_apple.jpg (SMALL architecture, compressed once), without and with --anchor_scales 1 2 3 4 6 8: host clock
           around each call, alternating, three runs each (the price of six ladders), and per image the container's bytes and the
           anchor's picked (scale, quality), bytes, PSNR and MS-SSIM in dB on both sides; the same for the apple against the size of
           the reference's own container, tests/golden/ref_apple.c2df (evaluate.jpeg_anchors with that budget).  No pass mark.

    python tools/bench_resize.py [--quick] [--out profiles/resize.txt]"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_quality import pairs  # noqa: E402
from bench_search_range import alternate  # noqa: E402

THREADS = 16
FILTERS = {1: "lanczos", 2: "bicubic"}      # the filter codes of sgic_resize_u8_batch
SCALES = ["1", "2", "3", "4", "6", "8"]
REQUIRED = "not slower than the Pillow pool beyond its own spread: min(gpu) <= min(pillow) + spread"


def point_resize(B, H, W, OH, OW, filt, iters):
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from PIL import Image
    from sgic_amd import ops
    name = FILTERS[filt]
    pil = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}[name]
    x = pairs(B, H, W, 3)[1]
    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        new = lambda: ops.resize_u8(x, OH, OW, name).cpu()                                                          # noqa: E731
        old = lambda: list(pool.map(lambda a: np.asarray(Image.fromarray(a).resize((OW, OH), pil)), x.cpu().numpy()))   # noqa: E731
        equal = bool(np.array_equal(new().numpy(), np.stack(old())))
        new()
        old()
        tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": f"ops.resize_u8 ({name}) vs Pillow Image.resize on 16 threads, device pixels -> resized images in host memory",
            "B": B, "H": H, "W": W, "OH": OH, "OW": OW, "filter": name, "iters": iters, "gpu_ms": tn, "pillow_ms": to,
            "pillow_spread_ms": spread, "ratio": min(to) / min(tn), "bytes_equal": equal, "required": REQUIRED,
            "met": bool(equal and min(tn) <= min(to) + spread)}


def point_anchor(iters):
    import tempfile
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import quality_ref
    from sgic_amd import compress, evaluate
    with tempfile.TemporaryDirectory() as root:
        src, out = os.path.join(root, "imgs"), os.path.join(root, "out")
        os.makedirs(src)
        for i, (h, w) in enumerate([(256, 256)] * 3 + [(200, 300)]):
            Image.fromarray(quality_ref.texture(np.random.default_rng(40 + i), h, w)).save(os.path.join(src, f"im{i}.png"))
        Image.open(os.path.join(ROOT, "tests", "golden", "ref_apple.jpg")).convert("RGB").save(os.path.join(src, "ref_apple.png"))
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            assert compress.main(["--dataset_dir", src, "--save_dir", out, "--small", "--batch_size", "4"]) == 0
        base = ["--originals", src, "--bitstreams", os.path.join(out, "bitstreams"), "--small", "--anchor", "jpeg", "--anchor_optimize"]
        sides = {"full": [], "scales": ["--anchor_scales"] + SCALES}

        def run(side):
            torch.cuda.synchronize()
            t = time.perf_counter()
            with contextlib.redirect_stderr(io.StringIO()):
                assert evaluate.main(base + sides[side] + ["--out", os.path.join(root, side + ".jsonl")]) == 0
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        for side in sides:
            run(side)
        ms = {side: [] for side in sides}
        for _ in range(iters):
            for side in sides:
                ms[side].append(run(side))
        reports = {}
        for side in sides:
            with open(os.path.join(root, side + ".jsonl"), encoding="utf-8") as fh:
                reports[side] = [json.loads(ln) for ln in fh.read().splitlines()]
        # the apple at the rate of the reference's own container (tests/golden/ref_apple.c2df, real weights): the budget the SMALL
        # architecture's container above does not reach
        budget = os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_apple.c2df"))
        apple = torch.from_numpy(np.array(Image.open(os.path.join(src, "ref_apple.png")).convert("RGB")))[None].cuda()
        at_rate = {"full": evaluate.jpeg_anchors(apple, [budget], 2, optimize=True)[0],
                   "scales": evaluate.jpeg_anchors(apple, [budget], 2, optimize=True, scales=[int(r) for r in SCALES])[0]}
    pick = lambda a: {k: a[k] for k in ("scale", "quality", "over_rate", "bytes", "psnr", "ms_ssim_db") if k in a}      # noqa: E731
    rows = []
    for full, sc in zip(reports["full"][:-1], reports["scales"][:-1]):
        rows.append({"name": full["name"], "height": full["height"], "width": full["width"], "container_bytes": full["bytes"],
                     "anchor": pick(full["anchor"]), "anchor_scales": pick(sc["anchor"])})
    keys = ("anchor_bpp", "anchor_psnr", "anchor_ms_ssim_db", "anchor_over_rate", "anchor_scale_counts")
    summary = {side: {k: reports[side][-1][k] for k in keys if k in reports[side][-1]} for side in sides}
    return {"what": "evaluate.py --anchor jpeg --anchor_optimize without and with --anchor_scales " + " ".join(SCALES) + ", SMALL "
                    "architecture, synthetic weights: the four textures of tests/test_gpu_evaluate_anchor.py and "
                    "tests/golden/ref_apple.jpg, compressed once; wall clock of the whole call (model build included)",
            "iters": iters, "full_ms": ms["full"], "scales_ms": ms["scales"], "added_ms": min(ms["scales"]) - min(ms["full"]),
            "images": rows, "summary": summary,
            "ref_apple_at_reference_container": {"container_bytes": budget, "anchor": pick(at_rate["full"]),
                                                 "anchor_scales": pick(at_rate["scales"])}, "required": "none"}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"resize": point_resize, "anchor": point_anchor}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    # resize:B:H:W:OH:OW:filter:iters
    points = ["resize:2:64:48:32:24:1:3"] if args.quick else \
        ["resize:32:256:256:128:128:1:50", "resize:32:64:64:256:256:2:50", "resize:4:1000:859:250:215:1:50", "resize:4:250:215:1000:859:2:50",
         "anchor:3"]
    ok = False
    lines = ["# tools/bench_resize.py; ms per call, two repeats each, the GPU resize and the Pillow pool alternating in one process per point"]
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
    else:
        ok = True          # every point gave its line
    timed = [(p, json.loads(ln)) for p, ln in zip(points, lines[1:]) if not ln.startswith("#") and "met" in json.loads(ln)]
    lines.append("# requirement (" + REQUIRED + "): met at " + (", ".join(p for p, r in timed if r["met"]) or "no point") +
                 "; missed at " + (", ".join(p for p, r in timed if not r["met"]) or "no point"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
