#!/usr/bin/env python3
"""Counterpart of the reference driver src/decompress.py (same flags; writes save_dir/results/<stem>.png),
running the MI355X decode path.  Files with identical shapes are decoded as one batch.  --format jpg writes baseline JPEG files
encoded on the GPU instead (jpeg_enc: the bytes Pillow's save(quality, subsampling) would write for the same pixels; with --optimize
those of save(quality, subsampling, optimize=True): Huffman tables fitted to every image; with --progressive those of
save(quality, subsampling, progressive=True): ten scans, tables fitted to every scan).  --max_side N reduces results whose longer
side exceeds N on the device before they are written (ops.resize_u8, Lanczos: the pixels of Pillow's Image.resize)."""
import argparse
import os
import sys
from glob import glob

import numpy as np
import torch

torch.set_grad_enabled(False)


def to_u8_hwc(x_chw_01):
    """torchvision.utils.save_image semantics for one image: mul(255).add_(0.5).clamp_(0,255) -> u8 (decompress.py:114)"""
    return x_chw_01.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def save_png(x_chw_01, path):
    from PIL import Image
    Image.fromarray(to_u8_hwc(x_chw_01)).save(path)


def _write_bytes(path, data):
    with open(path, "wb") as f:
        f.write(data)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--base_config", type=str, default=None)
    ap.add_argument("--ckpt_path", type=str, default=None)
    ap.add_argument("--dataset_dir", type=str, required=True, help="directory with *.c2df")
    ap.add_argument("--save_dir", type=str, required=True)
    ap.add_argument("--gpu_idx", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--format", choices=("png", "jpg"), default="png", help="results as PNG (host zlib) or as JPEG encoded on the GPU")
    ap.add_argument("--quality", type=int, default=90, help="JPEG quality, 1..100 (--format jpg)")
    ap.add_argument("--subsampling", type=int, choices=(0, 1, 2), default=2, help="JPEG chroma layout: 0 4:4:4, 1 4:2:2, 2 4:2:0")
    ap.add_argument("--optimize", action="store_true", help="JPEG with Huffman tables fitted to every image, as Pillow's optimize=True (--format jpg)")
    ap.add_argument("--progressive", action="store_true",
                    help="progressive JPEG, as Pillow's progressive=True: ten scans, tables fitted to every scan (--format jpg; --optimize changes nothing then)")
    ap.add_argument("--max_side", type=int, default=None, metavar="N",
                    help="reduce results whose longer side exceeds N (1..16384) to that side, Lanczos, before they are written")
    args = ap.parse_args(argv)
    if args.max_side is not None and not 1 <= args.max_side <= 16384:
        ap.error("--max_side must be in 1..16384")
    if not 1 <= args.quality <= 100:
        ap.error("--quality must be in 1..100")
    if args.optimize and args.format != "jpg":
        ap.error("--optimize fits the Huffman tables of a JPEG file: give --format jpg")
    if args.progressive and args.format != "jpg":
        ap.error("--progressive orders the scans of a JPEG file: give --format jpg")

    from . import weights as W
    from .codec import Codec
    from .compress import load_state
    from .config import LARGE, SMALL
    from .filemaker import unpack_c2df

    torch.cuda.set_device(args.gpu_idx)
    dev = torch.device("cuda", args.gpu_idx)
    cfg = SMALL if args.small else LARGE
    sd = load_state(args.ckpt_path, W.full_spec, cfg, 1234)
    model = Codec(sd, cfg, dev)
    model.hybrid_codec.quantize_feat.force_zero_thres = 0.12
    model.hybrid_codec.quantize_feat.update(force=True)
    out_dir = os.path.join(args.save_dir, "results")
    os.makedirs(out_dir, exist_ok=True)

    files = sorted(glob(os.path.join(args.dataset_dir, "*.c2df")))
    items = []
    for fp in files:
        enc, header = unpack_c2df(fp)
        items.append((fp, enc, header))
    groups = {}
    for i, (_, enc, _) in enumerate(items):
        groups.setdefault(tuple(int(v) for v in enc["img_shape"]), []).append(i)
    # PNG encoding (zlib, releases the GIL) runs on a thread pool underneath the next batch's GPU decode
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        pending = []
        for shape, idxs in groups.items():
            for s in range(0, len(idxs), args.batch_size):
                chunk = idxs[s:s + args.batch_size]
                x_hat = model.decode_batch([items[i][1] for i in chunk])
                crops = {}      # --format jpg, --max_side: the u8 images of this batch by cropped size, still on the device
                for j, i in enumerate(chunk):
                    fp, _, header = items[i]
                    pl, pr, pt, pb = header.get("padding", [0, 0, 0, 0])
                    H, Wd = x_hat.shape[2] - pt - pb, x_hat.shape[3] - pl - pr   # negative-pad crop (decompress.py:110-112)
                    x01 = x_hat[j, :, pt:pt + H, pl:pl + Wd].clamp(-1, 1) * 0.5 + 0.5
                    stem = os.path.splitext(os.path.basename(fp))[0]
                    if args.format == "jpg" or args.max_side is not None:
                        from .evaluate import to_u8_hwc_device
                        crops.setdefault((H, Wd), []).append((os.path.join(out_dir, f"{stem}.{args.format}"), to_u8_hwc_device(x01)))
                        continue
                    a = to_u8_hwc(x01)
                    path = os.path.join(out_dir, stem + ".png")
                    pending.append(pool.submit(lambda arr, p: Image.fromarray(arr).save(p), a, path))
                for (H, Wd), members in crops.items():       # one resize and one encode per distinct cropped size
                    from . import jpeg_enc, ops
                    from .resize import max_side_size
                    images = torch.stack([m[1] for m in members])
                    if args.max_side is not None and max(H, Wd) > args.max_side:
                        images = ops.resize_u8(images, *max_side_size(H, Wd, args.max_side), "lanczos")
                    if args.format == "png":
                        for (path, _), arr in zip(members, images.cpu().numpy()):
                            pending.append(pool.submit(lambda arr, p: Image.fromarray(arr).save(p), arr, path))
                        continue
                    files = jpeg_enc.encode_batch(images, args.quality, args.subsampling, optimize=args.optimize,
                                                  progressive=args.progressive)   # only the coded bytes cross the bus
                    for (path, _), data in zip(members, files):
                        pending.append(pool.submit(_write_bytes, path, data))
        for f in pending:
            f.result()
    return 0


if __name__ == "__main__":
    sys.exit(main())
