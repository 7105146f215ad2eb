"""The cases, images and references of the u8 resize tests (ops.resize_u8, csrc/resize.hip).  Pillow is the reference:
Image.fromarray(x).resize((OW, OH), filter).  Beside it a numpy restatement of Pillow's ImagingResample for 8-bit images
(precompute_coeffs, normalize_coeffs_8bpc and the two passes), which shows the accumulators before the clamp."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref  # noqa: E402

FILTERS = ("bicubic", "lanczos")
SUPPORT = {"bicubic": 2.0, "lanczos": 3.0}
KINDS = ("texture", "noise", "checker")

# (H, W, OH, OW, filter or None for both)
GEOMETRIES = [
    (1, 1, 1, 1, None), (1, 1, 7, 5, None), (8, 8, 8, 8, None),                                        # single pixel, identity
    (17, 9, 5, 3, None), (5, 3, 17, 9, None), (33, 47, 9, 12, None), (64, 48, 8, 6, None),             # small reductions, enlargements
    (37, 53, 37, 20, None),                                                                            # horizontal only
    (37, 53, 19, 53, None),                                                                            # vertical only
    (256, 256, 86, 86, None), (86, 86, 256, 256, None), (200, 300, 34, 50, None), (34, 50, 200, 300, None),   # the anchor's shapes
    (250, 215, 1000, 859, None), (1000, 859, 250, 215, None),
    (2, 16384, 2, 2, "lanczos"), (16384, 2, 2, 2, "lanczos"),            # more taps than any LDS tile, count clipped to the image
    (3, 300, 3, 299, None), (300, 3, 299, 3, None),                      # past an 8-bit axis index; a new tap window at almost every output
]
CASES = [(h, w, oh, ow, f) for h, w, oh, ow, named in GEOMETRIES for f in ((named,) if named else FILTERS)]
# a checkerboard enlargement: both filters' negative lobes overshoot at every 0/255 edge, on both sides
CLAMP_CASE = (34, 50, 200, 300)


def case_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}x{c[3]}-{c[4]}"


def image(kind, H, W, seed=0):
    """-> (H, W, 3) u8"""
    if kind == "texture":
        return quality_ref.texture(np.random.default_rng(40 + seed), H, W)
    if kind == "noise":
        return np.random.default_rng(900 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "checker":      # 0 / 255 squares of period 3
        yy, xx = np.mgrid[0:H, 0:W]
        return np.repeat(((((yy // 3) + (xx // 3)) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2).copy()
    raise ValueError(kind)


def pil_filter(name):
    from PIL import Image
    return {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]


def pillow(x, OH, OW, filt):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(x), "RGB").resize((OW, OH), pil_filter(filt)))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def coeffs(in_size, out_size, filt):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc in Python floats (IEEE doubles, libm's sin)
    -> (bounds int32 (out, 2), kk int32 (out, ksize), zero past the count)"""
    f = _bicubic if filt == "bicubic" else _lanczos
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = SUPPORT[filt] * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    bounds, kk = np.zeros((out_size, 2), dtype=np.int32), np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0)
        bounds[xx] = (xmin, count)
    return bounds, kk


def _pass(x, bounds, kk, axis):
    """one 8-bit pass along `axis` of (H, W, 3) -> (u8 result, least and largest accumulator >> 22 before the clamp)"""
    x = np.moveaxis(x, axis, 0).astype(np.int64)
    n = x.shape[0]
    out = np.empty((bounds.shape[0],) + x.shape[1:], dtype=np.int64)
    for o in range(bounds.shape[0]):      # a row of taps at a time: the 16384-tap cases stay small
        lo, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        assert 0 <= lo and lo + cnt <= n
        out[o] = (np.tensordot(kk[o, :cnt].astype(np.int64), x[lo:lo + cnt], axes=(0, 0)) + (1 << 21)) >> 22
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis), int(out.min()), int(out.max())


def restated(x, OH, OW, filt, tables=None):
    """the two passes in numpy, horizontal first with a u8 intermediate.  tables: ((bounds_h, kk_h), (bounds_v, kk_v)), default
    coeffs() -> (result, least, largest unclamped value over both passes)"""
    H, W, _ = x.shape
    th, tv = tables if tables is not None else (coeffs(W, OW, filt), coeffs(H, OH, filt))
    mid, lo_h, hi_h = _pass(x, th[0], th[1], 1)
    out, lo_v, hi_v = _pass(mid, tv[0], tv[1], 0)
    return out, min(lo_h, lo_v), max(hi_h, hi_v)


def clamp_case(filt):
    """the checkerboard case whose sums leave 0..255 on both sides -> (image, Pillow's result); asserts that they do, and that
    Pillow's bytes show both clamps"""
    H, W, OH, OW = CLAMP_CASE
    x = image("checker", H, W)
    _, lo, hi = restated(x, OH, OW, filt)
    want = pillow(x, OH, OW, filt)
    assert lo < 0 and hi > 255, (filt, lo, hi)
    assert want.min() == 0 and want.max() == 255
    return x, want
