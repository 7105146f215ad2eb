"""evaluate.py --anchor_scales restated with Pillow alone: reduce with Lanczos, save(quality, subsampling, optimize), open, enlarge with
bicubic, fp64 PSNR (quality_ref).  What the GPU tests hold jpeg_anchors(scales=...) to."""
import io
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref  # noqa: E402

LADDER = range(1, 96)


def reduced_size(H, W, r):
    return (H + r - 1) // r, (W + r - 1) // r


def save(a, q, subsampling=2, optimize=False):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=q, subsampling=subsampling, optimize=optimize)
    return buf.getvalue()


def psnr(a, b):
    """quality.combine's fp64 PSNR from the exact squared error (the SSIM fields are not needed to choose a scale)"""
    import sgic_amd  # noqa: F401
    from sgic_amd.quality import combine
    return float(combine(quality_ref.sse(a[None], b[None]), None, a.shape[0], a.shape[1])["psnr"][0])


def at_scale(a, r, budget, subsampling=2, optimize=False, fixed_quality=None):
    """one scale of one image -> dict(scale, coded (h, w), quality, over_rate, data, decoded (H, W, 3), psnr)"""
    from PIL import Image
    H, W, _ = a.shape
    h, w = reduced_size(H, W, r)
    src = a if r == 1 else np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))
    if fixed_quality is None:
        with ThreadPoolExecutor(max_workers=8) as pool:      # libjpeg runs outside the GIL
            sizes = dict(zip(LADDER, pool.map(lambda q: len(save(src, q, subsampling, optimize)), LADDER)))
        fits = [q for q, n in sizes.items() if n <= budget]
        q, over = (max(fits), False) if fits else (min(sizes), True)
    else:
        q, over = fixed_quality, None
    data = save(src, q, subsampling, optimize)
    if over is None:
        over = budget is not None and len(data) > budget
    dec = Image.open(io.BytesIO(data)).convert("RGB")
    if r != 1:
        dec = dec.resize((W, H), Image.BICUBIC)
    dec = np.asarray(dec)
    return {"scale": r, "coded": (h, w), "quality": q, "over_rate": over, "data": data, "decoded": dec, "psnr": psnr(a, dec)}


def anchor(a, scales, budget, subsampling=2, optimize=False, fixed_quality=None):
    """-> (the kept scale's dict, lead): lead is how far the kept scale's PSNR is above the next best fitting one (dB; None with
    fewer than two fitting scales)"""
    cands = [at_scale(a, r, budget, subsampling, optimize, fixed_quality) for r in sorted(scales)]
    fits = [c for c in cands if not c["over_rate"]]
    if fits:
        best = max(fits, key=lambda c: (c["psnr"], -c["scale"]))
        rest = sorted((c["psnr"] for c in fits if c is not best), reverse=True)
        return best, (best["psnr"] - rest[0] if rest else None)
    return min(cands, key=lambda c: (len(c["data"]), c["scale"])), None
