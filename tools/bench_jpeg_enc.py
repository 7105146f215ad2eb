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

  --optimize   the same enc and ladder points for the optimised Huffman tables (encode_batch / ladder_sizes with optimize=True against
               Pillow's save(optimize=True) on the pool; same requirement), each with the baseline-table encoder as a third side in the
               same process (for information: the cost of the histogram and table passes), and in place of anchor:
  size     evaluate.py --anchor jpeg with and without --anchor_optimize on that corpus and on tests/golden/ref_apple.jpg compressed
           once (SMALL architecture): per image the container's bytes, the picked quality, over_rate, the anchor's bytes, PSNR and
           MS-SSIM in dB.  No timing, no pass mark.

  --progressive   the enc points for progressive files (encode_batch with progressive=True against Pillow's save(progressive=True) on
                  the pool; same requirement), with the optimised sequential encoder as a third side in the same process (for
                  information: the call launches about fifteen times as many kernels), and one more point without a pass mark:
  tiled    one 2048 x 2048 image of the correction-bit tile of tests/jpeg_enc_prog_ref.py at q 100, 4:4:4: the most segments per
           run, so the most work for the doubling rounds.
  sizes    the bytes of the baseline, optimised and progressive files of tests/golden/ref_apple.jpg and of two natural-like images
           at several qualities, each file compared with Pillow's.  No timing, no pass mark.

    python tools/bench_jpeg_enc.py [--quick] [--optimize | --progressive] [--out profiles/jpeg_enc.txt]"""
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
REQUIRED = "not slower than the Pillow pool beyond its own spread: min(gpu) <= min(pillow) + spread"


def pillow_save(arr, quality, subsampling=2, optimize=False, progressive=False):
    from PIL import Image
    buf = io.BytesIO()
    if progressive:
        Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling=subsampling, progressive=True)
    elif optimize:
        Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling=subsampling, optimize=True)
    else:
        Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


@contextlib.contextmanager
def pillow_block(size):
    """Pillow sizes the buffer of an optimised save from the image and fails on a larger file: room for any file of a size x size
    image while an --optimize point runs (set once, around the pool; the threads only read it; size 0 leaves it alone), the old value
    afterwards"""
    from PIL import ImageFile
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 16 * size * size)
    try:
        yield
    finally:
        ImageFile.MAXBLOCK = keep


def _with_baseline(rec, tb, tn, progressive=False):
    """the third side of an --optimize point: the baseline-table encoder in the same process, for information; of a --progressive
    point: the optimised sequential encoder"""
    if progressive:
        rec.update({"gpu_optimize_ms": tb, "progressive_over_optimize": min(tn) / min(tb)})
    else:
        rec.update({"gpu_baseline_tables_ms": tb, "optimize_over_baseline": min(tn) / min(tb)})
    return rec


def point_enc(size, B, quality, iters, optimize=0, x=None, subsampling=2):
    """optimize: 0 the Annex K tables, 1 fitted tables, 2 progressive.  x: the images, (B, size, size, 3) u8 on the device"""
    from concurrent.futures import ThreadPoolExecutor
    from sgic_amd import jpeg_enc
    prog = optimize == 2
    if x is None:
        x = pairs(B, size, size, 3)[1]
    with pillow_block(size if optimize else 0), ThreadPoolExecutor(max_workers=THREADS) as pool:
        new = lambda: jpeg_enc.encode_batch(x, quality, subsampling, optimize=bool(optimize), progressive=prog)   # noqa: E731
        old = lambda: list(pool.map(lambda a: pillow_save(a, quality, subsampling, bool(optimize), prog), x.cpu().numpy()))      # noqa: E731
        base = lambda: jpeg_enc.encode_batch(x, quality, subsampling, optimize=prog)                              # noqa: E731
        got, want = new(), old()
        equal = got == want
        new()
        old()
        if optimize:
            base()
            tn, to, tb = alternate((new, old, base), iters)
        else:
            tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    what = "jpeg_enc.encode_batch(progressive=True) vs Pillow save(progressive=True)" if prog else \
        "jpeg_enc.encode_batch(optimize=True) vs Pillow save(optimize=True)" if optimize else "jpeg_enc.encode_batch vs Pillow save"
    layout = {0: "4:4:4", 1: "4:2:2", 2: "4:2:0"}[subsampling]
    rec = {"what": what + f" on 16 threads, {layout}, device pixels -> files in host memory", "B": B, "H": size,
           "W": size, "quality": quality, "iters": iters, "file_bytes_mean": sum(len(f) for f in got) / B, "gpu_ms": tn, "pillow_ms": to,
           "pillow_spread_ms": spread, "ratio": min(to) / min(tn), "files_equal": bool(equal), "required": REQUIRED,
           "met": bool(equal and min(tn) <= min(to) + spread)}
    return _with_baseline(rec, tb, tn, prog) if optimize else rec


def point_tiled(size, iters):
    """one image of the correction-bit tile at q 100, 4:4:4: every luma block of the last scan is all correction bits, so its one run
    is cut every 15 blocks.  No pass mark."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_enc_prog_ref
    rec = point_enc(size, 1, 100, iters, 2, torch.from_numpy(jpeg_enc_prog_ref.tiled(size, size)[None]).cuda(), 0)
    rec["what"] = "the correction-bit tile of tests/jpeg_enc_prog_ref.py, tiled: " + rec["what"]
    rec["required"] = "none"
    del rec["met"]
    return rec


def point_sizes():
    """file sizes of the three kinds of file the encoder writes (what decompress.py --format jpg [--optimize | --progressive] calls),
    each compared with Pillow's file first: tests/golden/ref_apple.jpg decoded, and natural-like images.  No timing, no pass mark."""
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_enc_ref
    from sgic_amd import jpeg_enc
    images = [("ref_apple", np.array(Image.open(os.path.join(ROOT, "tests", "golden", "ref_apple.jpg")).convert("RGB")), (50, 75, 90)),
              ("natural 512", jpeg_enc_ref.image("natural", 512, 512, 1), (50, 75, 90)),
              ("natural 256", jpeg_enc_ref.image("natural", 256, 256, 1), (50, 75, 90))]
    images.append(("ref_apple", images[0][1], (5, 10, 20)))
    rows, equal = [], True
    with pillow_block(1024):
        for name, a, qs in images:
            x = torch.from_numpy(a[None]).cuda()
            for q in qs:
                sizes = []
                for opt, prog in ((False, False), (True, False), (False, True)):
                    got = jpeg_enc.encode_batch(x, q, 2, optimize=opt, progressive=prog)[0]
                    equal = equal and got == pillow_save(a, q, 2, opt, prog)
                    sizes.append(len(got))
                rows.append({"image": name, "height": a.shape[0], "width": a.shape[1], "quality": q, "baseline": sizes[0],
                             "optimize": sizes[1], "progressive": sizes[2], "progressive_over_optimize": round(sizes[2] / sizes[1], 3)})
    return {"what": "bytes of jpeg_enc.encode_batch's files, 4:2:0: Annex K tables, optimize=True, progressive=True", "rows": rows,
            "files_equal": bool(equal), "required": "none"}


def point_ladder(size, B, iters, optimize=0):
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from sgic_amd import jpeg_enc
    x = pairs(B, size, size, 3)[1]
    jobs = [(b, q) for b in range(B) for q in jpeg_enc.LADDER]
    with pillow_block(size if optimize else 0), ThreadPoolExecutor(max_workers=THREADS) as pool:
        new = lambda: jpeg_enc.ladder_sizes(x, 2, optimize=bool(optimize))                           # noqa: E731
        base = lambda: jpeg_enc.ladder_sizes(x, 2)                                                   # noqa: E731

        def old():
            arrs = x.cpu().numpy()
            return np.array(list(pool.map(lambda j: len(pillow_save(arrs[j[0]], j[1], 2, bool(optimize))), jobs)),
                            dtype=np.int64).reshape(B, -1)

        equal = bool((new() == old()).all())
        if optimize:
            base()
            tn, to, tb = alternate((new, old, base), iters)
        else:
            tn, to = alternate((new, old), iters)
    spread = max(to) - min(to)
    what = "jpeg_enc.ladder_sizes(optimize=True) (qualities 1..95) vs Pillow save(optimize=True)" if optimize else \
        "jpeg_enc.ladder_sizes (qualities 1..95) vs Pillow save"
    rec = {"what": what + " of every image at every quality on 16 threads", "B": B,
           "H": size, "W": size, "rungs": len(jpeg_enc.LADDER), "iters": iters, "gpu_ms": tn, "pillow_ms": to, "pillow_spread_ms": spread,
           "ratio": min(to) / min(tn), "sizes_equal": equal, "required": REQUIRED, "met": bool(equal and min(tn) <= min(to) + spread)}
    return _with_baseline(rec, tb, tn) if optimize else rec


def point_size():
    """the size effect of --anchor_optimize: the picks and the numbers of the anchor with and without it, per image"""
    import tempfile
    import numpy as np
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import quality_ref
    from sgic_amd import compress, evaluate
    rows = []
    with tempfile.TemporaryDirectory() as root:
        src, out = os.path.join(root, "imgs"), os.path.join(root, "out")
        os.makedirs(src)
        for i, (h, w) in enumerate([(256, 256)] * 3 + [(200, 300)]):
            Image.fromarray(quality_ref.texture(np.random.default_rng(40 + i), h, w)).save(os.path.join(src, f"im{i}.png"))
        Image.open(os.path.join(ROOT, "tests", "golden", "ref_apple.jpg")).convert("RGB").save(os.path.join(src, "ref_apple.png"))
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            assert compress.main(["--dataset_dir", src, "--save_dir", out, "--small", "--batch_size", "4"]) == 0
        base = ["--originals", src, "--bitstreams", os.path.join(out, "bitstreams"), "--small", "--anchor", "jpeg"]
        reports = []
        for extra in ([], ["--anchor_optimize"]):
            rep = os.path.join(root, f"r{len(extra)}.jsonl")
            with contextlib.redirect_stderr(io.StringIO()):
                assert evaluate.main(base + extra + ["--out", rep]) == 0
            with open(rep, encoding="utf-8") as fh:
                reports.append([json.loads(ln) for ln in fh.read().splitlines()])
        for plain, opt in zip(reports[0][:-1], reports[1][:-1]):
            pick = lambda a: {k: a[k] for k in ("quality", "over_rate", "bytes", "psnr", "ms_ssim_db")}      # noqa: E731
            rows.append({"name": plain["name"], "height": plain["height"], "width": plain["width"], "container_bytes": plain["bytes"],
                         "anchor": pick(plain["anchor"]), "anchor_optimize": pick(opt["anchor"])})
        keys = ("anchor_bpp", "anchor_psnr", "anchor_ms_ssim_db", "anchor_over_rate")
        summary = {"anchor": {k: reports[0][-1][k] for k in keys}, "anchor_optimize": {k: reports[1][-1][k] for k in keys}}
    return {"what": "evaluate.py --anchor jpeg without and with --anchor_optimize, SMALL architecture, synthetic weights: the four "
                    "textures of tests/test_gpu_evaluate_anchor.py and tests/golden/ref_apple.jpg, compressed once", "images": rows,
            "summary": summary, "required": "none"}


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
    rec = {"enc": point_enc, "ladder": point_ladder, "anchor": point_anchor, "size": point_size, "tiled": point_tiled, "sizes": point_sizes}[kind](*args)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the protocol, not a measurement)")
    ap.add_argument("--optimize", action="store_true", help="the points of the optimised Huffman tables (default --out: profiles/jpeg_enc_opt.txt)")
    ap.add_argument("--progressive", action="store_true", help="the points of the progressive encoder (default --out: profiles/jpeg_enc_prog.txt)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help="run one point in this process (what the parent starts, under its time limit)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each point may take")
    args = ap.parse_args(argv)
    if args.point:
        return run_point(args.point)
    if args.optimize and args.progressive:
        ap.error("--optimize and --progressive are two sets of points: give one")
    points = ["enc:192:2:75:3"] if args.quick else ["enc:256:32:75:50", "enc:256:32:95:50", "enc:512:16:75:30", "ladder:256:32:3", "anchor:3"]
    if args.optimize:       # the trailing 1 is the points' optimize argument
        points = [p + ":1" for p in points if not p.startswith("anchor")] + ([] if args.quick else ["size"])
    if args.progressive:    # the trailing 2 is the points' optimize argument; the anchor keeps its sequential files, so no ladder
        points = [p + ":2" for p in points if p.startswith("enc")] + (["tiled:256:2"] if args.quick else ["tiled:2048:10", "sizes"])
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jpeg_enc_prog.txt" if args.progressive else "jpeg_enc_opt.txt" if args.optimize else "jpeg_enc.txt")
    ok = False
    lines = ["# tools/bench_jpeg_enc.py" + (" --optimize" if args.optimize else " --progressive" if args.progressive else "") +
             "; ms per call, two repeats each, the GPU encoder and the Pillow pool" +
             (" and the baseline-table encoder" if args.optimize else " and the optimised sequential encoder" if args.progressive else "") +
             " alternating in one process per point"]
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
    if args.optimize or args.progressive:      # said plainly: which of the timed points met the requirement
        timed = [(p, json.loads(ln)) for p, ln in zip(points, lines[1:]) if not ln.startswith("#") and "met" in json.loads(ln)]
        lines.append("# requirement (" + REQUIRED + "): met at " + (", ".join(p for p, r in timed if r["met"]) or "no point") +
                     "; missed at " + (", ".join(p for p, r in timed if not r["met"]) or "no point"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
