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
