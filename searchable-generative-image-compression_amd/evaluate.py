#!/usr/bin/env python3
"""Rate and distortion of a compressed folder: bpp, PSNR, SSIM and MS-SSIM of every image against its original, measured on the GPU
(quality.measure; the measures of the reference's taming/modules/losses/quality.py that need no network weights).

  evaluate.py --originals imgs --bitstreams out/bitstreams      decodes the containers (as decompress.py does, but the u8 image stays
                                                                on the device and no PNG is written)
  evaluate.py --originals imgs --recon_dir out/results          compares two folders; no model is built (--bitstreams adds the rate)

One JSON line per image, sorted by name, to --out (default: stdout); a summary line to stderr, which is also the last line of --out.
Originals and reconstructions are matched by file stem."""
import argparse
import json
import math
import os
import sys
from glob import glob

import numpy as np
import torch

torch.set_grad_enabled(False)

FIELDS = ("psnr", "ssim", "ms_ssim", "ms_ssim_db")


def to_u8_hwc_device(x_chw_01):
    """decompress.to_u8_hwc (torchvision's save_image arithmetic) without the copy to the host: the bytes of the PNG"""
    return x_chw_01.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def load_rgb(path):
    """-> (H, W, 3) u8, or the exception that reading raised (the caller reports it: this runs on a pool thread)"""
    from PIL import Image
    try:
        return np.array(Image.open(path).convert("RGB"), dtype=np.uint8)
    except Exception as e:   # noqa: BLE001 -- any unreadable file is a [SKIP] line, not the end of the run
        return e


def by_stem(paths):
    from .compress import stem_of
    return {stem_of(p): p for p in sorted(paths)}


def _json_number(v):
    if v is None:
        return None
    v = float(v)
    return ("inf" if v > 0 else "-inf") if math.isinf(v) else v


def summarise(records):
    """the summary line: count and the fp64 means of bpp, psnr (finite values), ms_ssim; ms_ssim_db of the mean ms_ssim"""
    def mean(vals):
        return float(np.mean(np.array(vals, dtype=np.float64))) if vals else None
    ms = mean([r["ms_ssim"] for r in records if r["ms_ssim"] is not None])
    with np.errstate(divide="ignore"):
        db = None if ms is None else float(0.0 - 10.0 * np.log10(1.0 - ms))
    return {"images": len(records), "bpp": mean([r["bpp"] for r in records if r["bpp"] is not None]),
            "psnr": mean([r["psnr"] for r in records if isinstance(r["psnr"], float)]), "ms_ssim": ms, "ms_ssim_db": _json_number(db)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--originals", type=str, required=True, help="directory with the original images")
    ap.add_argument("--bitstreams", type=str, default=None, help="directory with *.c2df (decoded here unless --recon_dir is given)")
    ap.add_argument("--recon_dir", type=str, default=None, help="directory with reconstructions (decompress.py's results/)")
    ap.add_argument("--out", type=str, default=None, help="report file (JSON lines); default: stdout")
    ap.add_argument("--ckpt_path", type=str, default=None)
    ap.add_argument("--gpu_idx", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args(argv)
    if not args.bitstreams and not args.recon_dir:
        ap.error("give --bitstreams, --recon_dir or both")
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")

    from concurrent.futures import ThreadPoolExecutor
    from . import quality

    torch.cuda.set_device(args.gpu_idx)
    dev = torch.device("cuda", args.gpu_idx)
    originals = by_stem(glob(os.path.join(args.originals, "*.*")))
    containers = by_stem(glob(os.path.join(args.bitstreams, "*.c2df"))) if args.bitstreams else {}
    recons = by_stem(glob(os.path.join(args.recon_dir, "*.*"))) if args.recon_dir else None
    records = []

    def skip(name, reason):
        print(f"[SKIP] {name}: {reason}", file=sys.stderr)

    candidates = recons if recons is not None else containers
    for stem in sorted(set(originals) - set(candidates)):
        skip(stem, "no reconstruction for this original")
    for stem in sorted(set(candidates) - set(originals)):
        skip(stem, "no original for this reconstruction")
    stems = sorted(set(candidates) & set(originals))

    def measure_chunk(chunk, pending):
        """chunk: [(stem, reconstruction (H, W, 3) u8 on the device)]; pending: the loads of their originals, in the same order.
        Pairs of one size are measured as one batch."""
        groups = {}
        for (stem, rec), fut in zip(chunk, pending):
            org = fut.result()
            if isinstance(org, Exception):
                skip(stem, f"unreadable original ({org})")
            elif org.shape != tuple(rec.shape):
                skip(stem, f"original is {org.shape[0]}x{org.shape[1]}, reconstruction {rec.shape[0]}x{rec.shape[1]}")
            else:
                groups.setdefault(org.shape, []).append((stem, org, rec))
        for (H, W, _), members in groups.items():
            a = torch.from_numpy(np.stack([m[1] for m in members])).to(dev)
            m = quality.measure(a, torch.stack([m[2] for m in members]))
            for j, (stem, _, _) in enumerate(members):
                nbytes = os.path.getsize(containers[stem]) if stem in containers else None
                rec = {"name": stem, "height": H, "width": W, "bytes": nbytes, "bpp": None if nbytes is None else 8 * nbytes / (H * W)}
                for k in FIELDS:
                    rec[k] = None if m[k] is None else _json_number(m[k][j])
                records.append(rec)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        if recons is not None:
            for s in range(0, len(stems), args.batch_size):
                part = stems[s:s + args.batch_size]
                pending = [pool.submit(load_rgb, originals[st]) for st in part]
                chunk = []
                keep = []
                for st, fut, arr in zip(part, pending, pool.map(load_rgb, [recons[st] for st in part])):
                    if isinstance(arr, Exception):
                        skip(st, f"unreadable reconstruction ({arr})")
                    else:
                        chunk.append((st, torch.from_numpy(arr).to(dev)))
                        keep.append(fut)
                measure_chunk(chunk, keep)
        else:
            from . import weights as W
            from .codec import Codec
            from .compress import load_state
            from .config import LARGE, SMALL
            from .filemaker import unpack_c2df
            cfg = SMALL if args.small else LARGE
            model = Codec(load_state(args.ckpt_path, W.full_spec, cfg, 1234), cfg, dev)
            model.hybrid_codec.quantize_feat.force_zero_thres = 0.12
            model.hybrid_codec.quantize_feat.update(force=True)
            items, groups = {}, {}
            for st in stems:
                try:
                    items[st] = unpack_c2df(containers[st])
                except Exception as e:   # noqa: BLE001 -- a truncated or foreign file
                    skip(st, f"unreadable container ({e})")
                    continue
                groups.setdefault(tuple(int(v) for v in items[st][0]["img_shape"]), []).append(st)
            for shape, members in groups.items():           # containers of one padded geometry decode as one batch (decompress.py)
                for s in range(0, len(members), args.batch_size):
                    part = members[s:s + args.batch_size]
                    pending = [pool.submit(load_rgb, originals[st]) for st in part]      # read underneath the GPU decode
                    x_hat = model.decode_batch([items[st][0] for st in part])
                    chunk = []
                    for j, st in enumerate(part):
                        pl, pr, pt, pb = items[st][1].get("padding", [0, 0, 0, 0])
                        H, Wd = x_hat.shape[2] - pt - pb, x_hat.shape[3] - pl - pr
                        chunk.append((st, to_u8_hwc_device(x_hat[j, :, pt:pt + H, pl:pl + Wd].clamp(-1, 1) * 0.5 + 0.5)))
                    measure_chunk(chunk, pending)

    records.sort(key=lambda r: r["name"])
    summary = json.dumps(summarise(records))
    lines = [json.dumps(r) for r in records]
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines + [summary]))
    else:
        for ln in lines:
            print(ln)
    print(summary, file=sys.stderr)
    return 0 if records else 1


if __name__ == "__main__":
    sys.exit(main())
