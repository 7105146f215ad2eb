"""The Pillow reference of CLIP preprocessing the GPU tests compare with, bit for bit: PIL bicubic resize (shortest side S) -> centre
crop -> / 255 -> Normalize, from the bytes as they are (the u8-canvas route) or behind ToPILImage's truncation (the fp32 route)."""
import numpy as np


def pillow_from_u8(u8_hw3, S, mean, std):
    """Image.fromarray(u8) -> resize -> crop -> / 255 -> Normalize: no float round trip.  -> (3, S, S) float32"""
    from PIL import Image
    H, W, _ = u8_hw3.shape
    oh, ow = (S, int(S * W / H)) if H <= W else (int(S * H / W), S)
    pil = Image.fromarray(np.ascontiguousarray(u8_hw3), "RGB").resize((ow, oh), Image.BICUBIC)
    top, left = int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))
    arr = np.asarray(pil)[top:top + S, left:left + S].astype(np.float32) / np.float32(255)
    return ((arr - np.float32(mean)) / np.float32(std)).transpose(2, 0, 1).astype(np.float32)


def pillow_from_f32(x_chw, S, mean, std):
    """x (3, H, W) fp32 torch tensor in [-1, 1] on the host: ToPILImage on x * 0.5 + 0.5 (which truncates), then pillow_from_u8"""
    u8 = (x_chw.clamp(-1, 1).mul(0.5).add(0.5)).mul(255).byte().permute(1, 2, 0).numpy()
    return pillow_from_u8(u8, S, mean, std)
