#!/usr/bin/env python3
"""Time the GPU baseline JPEG encoder (csrc/jpeg_enc.hip: jpeg_enc.encode_batch) against what the host path would do: copy the pixels
to the host and `PIL.Image.save(format="JPEG")` them on a pool of 16 threads.  Both sides start from the same u8 images on the device
and end with whole files in host memory, so the copy of the pixels counts for Pillow and the copy of the coded bytes for the encoder.

Protocol (that of tools/bench_quality.py): seeded images made on the device; both paths warmed up, then timed with device events in
one process, alternating, twice (both repeats are reported, they show the spread).  Every point runs in a child process of its own
under a time limit; the first point that fails ends the run.

  enc      encode_batch against the Pillow pool; the files are compared first.  Required: not slower than the pool beyond the
           pool's own repeat-to-repeat spread.
  ladder   the file sizes at qualities 1..95 (jpeg_enc.ladder_sizes, what evaluate.py --anchor jpeg searches) against the pool saving
           every image at every quality.  Same requirement.
  anchor   evaluate.py on the four images of tests/test_gpu_evaluate.py (SMALL architecture) with and without --anchor jpeg, host
           clock around each call, alternating.  No pass mark; the corpus is small, so this is mostly fixed cost.

    python tools/bench_jpeg_enc.py [--quick] [--out profiles/jpeg_enc.txt]"""
import argparse
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
REQUIRED = "not slower than the Pillow pool beyond its own spread: min(gpu) <= min(pillow) + spread"


def pillow_save(arr, quality, subsampling=2):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def point_enc(size, B, quality, iters):
    from concurrent.futures import ThreadPoolExecutor
    from sgic_amd import jpeg_enc
    x = pairs(B, size, size, 3)[1]
    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        new = lambda: jpeg_enc.encode_batch(x, quality, 2)                                           # noqa: E731
        old = lambda: list(pool.map(lambda a: pillow_save(a, quality), x.cpu().numpy()))             # noqa: E731
        got, want = new(), old()
        equal = got == want
        new()
        old()
        tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": "jpeg_enc.encode_batch vs Pillow save on 16 threads, 4:2:0, device pixels -> files in host memory", "B": B, "H": size,
            "W": size, "quality": quality, "iters": iters, "file_bytes_mean": sum(len(f) for f in got) / B, "gpu_ms": tn, "pillow_ms": to,
            "pillow_spread_ms": spread, "ratio": min(to) / min(tn), "files_equal": bool(equal), "required": REQUIRED,
            "met": bool(equal and min(tn) <= min(to) + spread)}


def point_ladder(size, B, iters):
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from sgic_amd import jpeg_enc
    x = pairs(B, size, size, 3)[1]
    jobs = [(b, q) for b in range(B) for q in jpeg_enc.LADDER]
    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        new = lambda: jpeg_enc.ladder_sizes(x, 2)                                                    # noqa: E731

        def old():
            arrs = x.cpu().numpy()
            return np.array(list(pool.map(lambda j: len(pillow_save(arrs[j[0]], j[1])), jobs)), dtype=np.int64).reshape(B, -1)

        equal = bool((new() == old()).all())
        tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    return {"what": "jpeg_enc.ladder_sizes (qualities 1..95) vs Pillow save of every image at every quality on 16 threads", "B": B,
            "H": size, "W": size, "rungs": len(jpeg_enc.LADDER), "iters": iters, "gpu_ms": tn, "pillow_ms": to, "pillow_spread_ms": spread,
            "ratio": min(to) / min(tn), "sizes_equal": equal, "required": REQUIRED, "met": bool(equal and min(tn) <= min(to) + spread)}


def point_anchor(iters):
    import contextlib
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
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            assert compress.main(["--dataset_dir", src, "--save_dir", out, "--small", "--batch_size", "4"]) == 0
        base = ["--originals", src, "--bitstreams", os.path.join(out, "bitstreams"), "--small", "--out", os.path.join(root, "r.jsonl")]

        def run(extra):
            torch.cuda.synchronize()
            t = time.perf_counter()
            with contextlib.redirect_stderr(io.StringIO()):
                assert evaluate.main(base + extra) == 0
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        run([])
        run(["--anchor", "jpeg"])
        plain, anchor = [], []
        for _ in range(iters):
            plain.append(run([]))
            anchor.append(run(["--anchor", "jpeg"]))
    return {"what": "evaluate.py --bitstreams on 4 images (3 x 256^2, 200 x 300), SMALL architecture, synthetic weights: wall clock of "
                    "the whole call (model build included) without and with --anchor jpeg; a small corpus, mostly fixed cost",
            "iters": iters, "plain_ms": plain, "anchor_ms": anchor, "added_ms": min(anchor) - min(plain), "required": "none"}


def run_point(spec):
    import torch
    sys.path.insert(0, ROOT)
    import sgic_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_enc needs the GPU: there is nothing to time without one")
    kind, args = spec.split(":")[0], [int(a) for a in spec.split(":")[1:]]
    rec = {"enc": point_enc, "ladder": point_ladder, "anchor": point_anchor}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_enc.txt"))
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    points = ["enc:192:2:75:3"] if args.quick else ["enc:256:32:75:50", "enc:256:32:95:50", "enc:512:16:75:30", "ladder:256:32:3", "anchor:3"]
    lines = ["# tools/bench_jpeg_enc.py; ms per call, two repeats each, the GPU encoder and the Pillow pool alternating in one process per "
             "point"]
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
