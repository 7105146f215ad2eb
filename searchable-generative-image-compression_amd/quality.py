"""Rate-distortion measures of a reconstruction against its original: PSNR, SSIM and MS-SSIM (the arithmetic of the reference's
taming/modules/losses/quality.py: `pytorch_msssim.MS_SSIM(data_range=1.0)`, written out in DESIGN.md section 12).  The sums run on
the GPU (ops.quality_u8, csrc/quality.hip); the last step, a few numbers per image, is numpy fp64 on the host."""
import numpy as np

MS_WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float64)
MIN_SIDE = 160      # five levels need a shorter side above (11 - 1) * 2^4


def combine(sse, levels, H, W):
    """sse (B, 3) int64 and levels (B, 3, 5, 2) float64 ({mean ssim, mean cs} per channel and level; None for images too small
    for five levels) of H x W images -> {"psnr", "ssim", "ms_ssim", "ms_ssim_db"}: float64 arrays (B,), the last three None without
    levels.  psnr = 10 log10(255^2 3HW / sum sse), inf for equal images; ms_ssim = the channel mean of prod_l v_l^w_l with
    v = relu(cs_0 .. cs_3, ssim_4); ms_ssim_db = -10 log10(1 - ms_ssim), inf at 1; ssim = the channel mean of the level-0 ssim."""
    tot = np.asarray(sse, dtype=np.int64).sum(axis=1).astype(np.float64)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(65025.0 * (3 * int(H) * int(W)) / tot)
    if levels is None:
        return {"psnr": psnr, "ssim": None, "ms_ssim": None, "ms_ssim_db": None}
    levels = np.asarray(levels, dtype=np.float64)
    v = np.maximum(np.concatenate([levels[:, :, :4, 1], levels[:, :, 4:, 0]], axis=2), 0.0)
    ms = np.prod(v ** MS_WEIGHTS, axis=2).mean(axis=1)
    with np.errstate(divide="ignore"):
        db = 0.0 - 10.0 * np.log10(1.0 - ms)       # 0.0 - x: ms_ssim = 0 reads 0.0, not -0.0
    return {"psnr": psnr, "ssim": levels[:, :, 0, 0].mean(axis=1), "ms_ssim": ms, "ms_ssim_db": db}


def measure(a_u8, b_u8):
    """a_u8 (original), b_u8 (reconstruction): (B, H, W, 3) u8 CUDA tensors -> combine()'s dict.  Images whose shorter side is
    <= 160 have no five-level pyramid: PSNR from a plain integer squared error, None for the SSIM fields.  One read-back."""
    import torch
    assert a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.shape == b_u8.shape
    assert a_u8.dim() == 4 and a_u8.shape[3] == 3 and a_u8.shape[0] >= 1
    B, H, W, _ = a_u8.shape
    if min(H, W) <= MIN_SIDE:
        d = a_u8.to(torch.int64) - b_u8.to(torch.int64)
        return combine((d * d).sum(dim=(1, 2)).cpu().numpy(), None, H, W)
    from . import ops
    sse, levels = ops.quality_u8(a_u8.contiguous(), b_u8.contiguous())
    return combine(sse.cpu().numpy(), levels.cpu().numpy(), H, W)


# The hand-crafted full-reference measures on luma (evaluate.py --hvs; csrc/hvs.hip)

HVS_FIELDS = ("vifp", "gmsd", "psnr_hvs", "psnr_hvs_m")
VIFP_WINDOWS = (17, 9, 5, 3)      # N = 2^(4 - s + 1) + 1 of the scales s = 1..4
PSNR_HVS_MIN_SIDE = 8             # one whole 8 x 8 block


def _vifp_min_side():
    """the smallest side at which scale 4 has one valid sample, from the window arithmetic: scale s > 1 keeps every second sample
    of the valid filter output of scale s - 1 (n -> ceil((n - N + 1) / 2)), and every scale needs n >= N for its statistics"""
    def fits(n):
        for s, N in enumerate(VIFP_WINDOWS):
            if s and n >= N:
                n = (n - N + 2) // 2
            if n < N:
                return False
        return True
    n = 1
    while not fits(n):
        n += 1
    return n


VIFP_MIN_SIDE = _vifp_min_side()      # 41


def _luma_pair(a_u8, b_u8):
    import torch
    from . import ops
    assert a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.shape == b_u8.shape
    assert a_u8.dim() == 4 and a_u8.shape[3] == 3 and a_u8.shape[0] >= 1
    return ops.hvs_luma_u8(a_u8.contiguous()), ops.hvs_luma_u8(b_u8.contiguous())


def _vifp(ya, yb):
    from . import ops
    H, W = ya.shape[1:]
    if min(H, W) < VIFP_MIN_SIDE:
        raise ValueError(f"VIFp needs both sides >= {VIFP_MIN_SIDE} (scale 4 has no valid sample below that), got {H} x {W}")
    sums = ops.hvs_vifp(ya, yb)
    equal = (ya == yb).flatten(1).all(dim=1).cpu().numpy()
    sums = sums.cpu().numpy()
    num, den = sums[:, 0], sums[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):      # a flat original carries no information: 1 for equal images, else 0
        return np.where(den == 0.0, np.where(equal, 1.0, 0.0), num / den)


def _psnr_hvs(ya, yb):
    from . import ops
    from .jpeg_enc import _LUMA
    H, W = ya.shape[1:]
    if min(H, W) < PSNR_HVS_MIN_SIDE:
        raise ValueError(f"PSNR-HVS needs both sides >= {PSNR_HVS_MIN_SIDE} (one whole 8 x 8 block), got {H} x {W}")
    sums = ops.hvs_psnr(ya, yb, _LUMA).cpu().numpy()
    with np.errstate(divide="ignore"):      # equal images: inf, as "psnr"
        db = 10.0 * np.log10(65025.0 / (sums / (64.0 * (H // 8) * (W // 8))))
    return db[:, 0], db[:, 1]


def vifp(a_u8, b_u8):
    """pixel-domain VIF of B pairs: a_u8 (original), b_u8 (reconstruction) (B, H, W, 3) u8 CUDA tensors -> float64 (B,).
    ValueError for images with a side below VIFP_MIN_SIDE."""
    return _vifp(*_luma_pair(a_u8, b_u8))


def gmsd(a_u8, b_u8):
    """gradient magnitude similarity deviation of B pairs -> float64 (B,); 0 for equal images"""
    from . import ops
    return ops.hvs_gmsd(*_luma_pair(a_u8, b_u8)).cpu().numpy()


def psnr_hvs(a_u8, b_u8):
    """-> (psnr_hvs, psnr_hvs_m): float64 (B,) each, inf for equal images.  ValueError for images with a side below 8."""
    return _psnr_hvs(*_luma_pair(a_u8, b_u8))


def measure_hvs(a_u8, b_u8):
    """the three measures from one luma plane per image -> {"vifp", "gmsd", "psnr_hvs", "psnr_hvs_m"}: float64 (B,), or None for
    a measure the images are too small for (vifp below VIFP_MIN_SIDE, psnr_hvs and psnr_hvs_m below 8), as measure() does"""
    from . import ops
    ya, yb = _luma_pair(a_u8, b_u8)
    side = min(ya.shape[1:])
    hvs, hvs_m = _psnr_hvs(ya, yb) if side >= PSNR_HVS_MIN_SIDE else (None, None)
    return {"vifp": _vifp(ya, yb) if side >= VIFP_MIN_SIDE else None, "gmsd": ops.hvs_gmsd(ya, yb).cpu().numpy(),
            "psnr_hvs": hvs, "psnr_hvs_m": hvs_m}


# FSIM and FSIMc (evaluate.py --fsim; csrc/fsim.hip)

FSIM_FIELDS = ("fsim", "fsimc")
FSIM_MIN_SIDE = 2                 # the frequency grid of an odd axis divides by n - 1
FSIM_MAX_REDUCED_SIDE = 2048      # a resource cap: the dense transform is cubic, its twiddle table lives in LDS


def fsim_reduction(H, W):
    """-> (F, h, w): F = max(1, round(min(H, W) / 256)) with MATLAB's round (383 -> 1, 384 -> 2); every plane is averaged over
    F x F and rows and columns 0, F, 2F, .. are kept"""
    F = max(1, int(np.floor(min(H, W) / 256.0 + 0.5)))
    return F, -(-H // F), -(-W // F)


def _fsim_check(H, W, reduce=True):
    if min(H, W) < FSIM_MIN_SIDE:
        raise ValueError(f"FSIM needs both sides >= {FSIM_MIN_SIDE}, got {H} x {W}")
    h, w = fsim_reduction(H, W)[1:] if reduce else (H, W)
    if max(h, w) > FSIM_MAX_REDUCED_SIDE:
        raise ValueError(f"FSIM needs the reduced longer side <= {FSIM_MAX_REDUCED_SIDE}, got {h} x {w}")


def phase_congruency(planes):
    """planes (B, h, w) float64 CUDA tensor -> float64 (B, h, w) numpy: the phase congruency map FSIM weighs with.  ValueError for
    a side below FSIM_MIN_SIDE or above FSIM_MAX_REDUCED_SIDE."""
    from . import ops
    assert planes.dim() == 3 and planes.shape[0] >= 1
    _fsim_check(planes.shape[1], planes.shape[2], reduce=False)
    return ops.fsim_phasecong(planes.contiguous()).cpu().numpy()


def fsim(a_u8, b_u8):
    """FSIM and FSIMc of B pairs: a_u8 (original), b_u8 (reconstruction) (B, H, W, 3) u8 CUDA tensors -> (fsim, fsimc), float64 (B,)
    each; exactly 1 for equal images.  ValueError for images with a side below FSIM_MIN_SIDE or a reduced longer side above
    FSIM_MAX_REDUCED_SIDE."""
    import torch
    from . import ops
    assert a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.shape == b_u8.shape
    assert a_u8.dim() == 4 and a_u8.shape[3] == 3 and a_u8.shape[0] >= 1
    _fsim_check(a_u8.shape[1], a_u8.shape[2])
    f, fc = ops.fsim(a_u8.contiguous(), b_u8.contiguous())
    return f.cpu().numpy(), fc.cpu().numpy()


def measure_fsim(a_u8, b_u8):
    """-> {"fsim", "fsimc"}: float64 (B,), or None for both where fsim() refuses the size, as measure() does"""
    try:
        _fsim_check(a_u8.shape[1], a_u8.shape[2])
    except ValueError:
        return {"fsim": None, "fsimc": None}
    f, fc = fsim(a_u8, b_u8)
    return {"fsim": f, "fsimc": fc}
