"""What the perceptual pair metrics (lpips.LpipsVGG, lpips_alex.LpipsAlex, dists.DistsVGG) share: the checkpoint loader, the weight
layout of the split convolutions, the VGG16 trunk (its tables, its synthetic weights, its walk) and the chunked measure loop.  The
kernels they share are csrc/producers.h."""
import math

import numpy as np
import torch

# torchvision's vgg16().features: index of every convolution, its channels, and what follows its ReLU
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CH = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
           (512, 512), (512, 512), (512, 512))
POOL_AFTER = (1, 3, 6, 9)            # positions in CONV_IDX whose ReLU is followed by a pool
TAP_AFTER = (1, 3, 6, 9, 12)         # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
MAX_PIXELS = 1 << 21                 # pixels of one chunk, both sides of its pairs counted (see LpipsMeasure.measure)


def lpips_canonical_key(key):
    """a checkpoint's key -> the canonical key of an LPIPS model, or None for a key that is not part of it (scaling_layer.*, a
    classifier)"""
    parts = key.split(".")
    if len(parts) == 3 and parts[0] == "features" and parts[2] in ("weight", "bias"):
        return key
    if len(parts) == 4 and parts[0] == "net" and parts[1].startswith("slice") and parts[3] in ("weight", "bias"):
        return f"features.{parts[2]}.{parts[3]}"
    if len(parts) == 4 and parts[0].startswith("lin") and parts[1] == "model" and parts[2] in ("0", "1") and parts[3] == "weight":
        return f"{parts[0]}.model.1.weight"
    return None


def load_state(paths, want, canonical_key, label, alt_shapes=None):
    """one or more torch.load-able state dicts (paths, or dicts already loaded) -> the canonical fp32 state dict with the keys and
    shapes of `want`.  canonical_key: a checkpoint's key -> its key in `want`, or None; alt_shapes: canonical key -> further shapes it
    may come in (reshaped to want's).  Later files win.  Every shape is checked; a missing key is named in the error."""
    if isinstance(paths, (str, bytes, dict)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    out = {}
    for p in paths:
        sd = p if isinstance(p, dict) else torch.load(p, map_location="cpu", weights_only=True)
        sd = sd.get("state_dict", sd)
        for key, v in sd.items():
            ck = canonical_key(key)
            if ck is None or ck not in want:
                continue
            ok = (want[ck],) + tuple((alt_shapes or {}).get(ck, ()))
            if tuple(v.shape) not in ok:
                raise ValueError(f"{label} weights: {key} has shape {tuple(v.shape)}, expected {' or '.join(str(s) for s in ok)}")
            out[ck] = v.detach().to(torch.float32).reshape(want[ck]).contiguous()
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError(f"{label} weights: missing {', '.join(missing)}")
    return {k: out[k] for k in want}


def conv_matrix(w, pad_cin_to=None):
    """(Cout, Cin, k, k) -> (Cout, (ky, kx, cin)) contiguous, the B operand of the split convolutions.  pad_cin_to: cin is zero-padded
    to a multiple of it first (the implicit 3x3 path reads whole 32-channel slices per tap); the columns are then zero-padded to a
    multiple of 32 (a patch matrix's whole slices)."""
    w = w.permute(0, 2, 3, 1)
    cout, k, _, cin = w.shape
    if pad_cin_to and cin % pad_cin_to:
        w = torch.cat([w, torch.zeros(cout, k, k, pad_cin_to - cin % pad_cin_to)], dim=3)
    w = w.reshape(cout, -1)
    if w.shape[1] % 32:
        w = torch.cat([w, torch.zeros(cout, 32 - w.shape[1] % 32)], dim=1)
    return w.contiguous()


def vgg_conv(sd, device):
    """the canonical state dict -> [(weight matrix, bias, padded Cin, Cout)] of the thirteen convolutions on the device (conv1_1
    zero-padded from 3 to 32 input channels)"""
    out = []
    for i, (_, cout) in zip(CONV_IDX, CONV_CH):
        w = conv_matrix(sd[f"features.{i}.weight"], pad_cin_to=32)
        out.append((w.to(device), sd[f"features.{i}.bias"].to(device), w.shape[1] // 9, cout))
    return out


def vgg_synth_trunk(g):
    """synthetic VGG16 trunk from generator g: convolutions He-normal with std = sqrt(2 / (9 Cin)), biases uniform in [0, 0.05], drawn
    in trunk order, weight before bias"""
    sd = {}
    for i, (cin, cout) in zip(CONV_IDX, CONV_CH):
        sd[f"features.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{i}.bias"] = torch.rand(cout, generator=g) * 0.05
    return sd


def run_vgg16(conv, hp, n, H, W, on_tap, pool):
    """the trunk over the n images whose input layer is in hp (HaloPlanes).  on_tap(tap, y, h, w): called with every tapped
    convolution's output (n h w, C) before its ReLU; pool(y, h, w, C, pooled) -> the next convolution's HaloPlanes from y, after the
    metric's pool when pooled.  No synchronisation."""
    from . import ops
    h, w, tap = H, W, 0
    for j, (wt, bias, cin, cout) in enumerate(conv):
        y = ops.conv3x3(hp, wt, bias, n, h, w, cin, cout, precision="split3")       # before its ReLU: the consumers apply it
        if j in TAP_AFTER:
            on_tap(tap, y, h, w)
            tap += 1
        if j + 1 < len(conv):
            hp = pool(y, h, w, cout, j in POOL_AFTER)
            h, w = hp.H, hp.W


def checked_pair(a_u8, b_u8, min_side):
    """the argument checks of every measure -> (a, b) contiguous, or None when min(H, W) < min_side"""
    assert a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.shape == b_u8.shape and a_u8.is_cuda and b_u8.is_cuda
    assert a_u8.dim() == 4 and a_u8.shape[3] == 3 and a_u8.shape[0] >= 1
    if min(a_u8.shape[1:3]) < min_side:
        return None
    return a_u8.contiguous(), b_u8.contiguous()


def chunked(measure_chunk, B, H, W, max_pixels):
    """measure_chunk(s, n) for the pairs s .. s+n-1 of every chunk of at most max_pixels pixels (2 n H W, both sides counted; at least
    one pair), in order"""
    step = max(1, int(max_pixels) // (2 * H * W))
    for s in range(0, B, step):
        measure_chunk(s, min(step, B - s))


class LpipsMeasure:
    """the measure of the two LPIPS models: a subclass sets min_side, device, max_pixels and _chunk(a, b, layers (5, Bc) float64)"""

    def measure(self, a_u8, b_u8):
        """a_u8, b_u8: (B, H, W, 3) u8 CUDA tensors -> (lpips (B,) float64, layers (B, 5) float64: the five taps' distances, lpips =
        their sum in tap order), numpy, one read-back; None when min(H, W) < min_side.  The batch runs in chunks of at most
        max_pixels = 2^21 pixels (2 Bc H W, both sides counted; at least one pair), so memory does not grow with B (the class says
        what a chunk holds), and the planes buffers of a geometry are cached (ops.halo_planes_buffer).  A pair's result depends
        neither on the chunking nor on its slot."""
        pair = checked_pair(a_u8, b_u8, self.min_side)
        if pair is None:
            return None
        B, H, W, _ = a_u8.shape
        layers = torch.empty(5, B, dtype=torch.float64, device=self.device)

        def one(s, n):
            part = layers[:, s:s + n] if n == B else torch.empty(5, n, dtype=torch.float64, device=self.device)
            self._chunk(pair[0][s:s + n], pair[1][s:s + n], part)
            if n != B:
                layers[:, s:s + n] = part
        chunked(one, B, H, W, self.max_pixels)
        lay = np.ascontiguousarray(layers.cpu().numpy().T)
        total = lay[:, 0].copy()
        for k in range(1, 5):
            total += lay[:, k]
        return total, lay
