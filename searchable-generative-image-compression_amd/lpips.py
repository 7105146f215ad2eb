"""LPIPS with the VGG16 trunk (the reference's taming/modules/losses/lpips.py, whose trunk is torchvision's vgg16().features), on the
GPU: the definition is written out in DESIGN.md section 14.  The thirteen 3x3 convolutions run through ops.conv3x3 as implicit
bf16x3 split GEMMs (always, also under SGIC_GEMM=f32: the path needs the planes layout); the input layer, ReLU / max-pool into the
next convolution's operand planes and the head are csrc/lpips.hip.  Weights are a checkpoint the user has (load_weights) or
synthetic (synth_weights: the tests)."""
import math

import numpy as np
import torch

# torchvision's vgg16().features: index of every convolution, its channels, and what follows its ReLU
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CH = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
           (512, 512), (512, 512), (512, 512))
POOL_AFTER = (1, 3, 6, 9)            # positions in CONV_IDX whose ReLU is followed by max-pool 2x2
TAP_AFTER = (1, 3, 6, 9, 12)         # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
TAP_CH = (64, 128, 256, 512, 512)
MIN_SIDE = 16                        # four pools must leave a pixel
_SLICE_OF = {i: 1 + sum(i >= s for s in (4, 9, 16, 23)) for i in CONV_IDX}      # the reference's net.slice{s}.{i}
MAX_PIXELS = 1 << 21                 # pixels of one chunk, both sides of its pairs counted (see LpipsVGG.measure)


def expected_shapes():
    """canonical key -> shape: features.{i}.{weight,bias} and lin{k}.model.1.weight"""
    out = {}
    for i, (cin, cout) in zip(CONV_IDX, CONV_CH):
        out[f"features.{i}.weight"] = (cout, cin, 3, 3)
        out[f"features.{i}.bias"] = (cout,)
    for k, c in enumerate(TAP_CH):
        out[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return out


def _canonical_key(key):
    """a checkpoint's key -> the canonical key, or None for a key that is not part of LPIPS-VGG (scaling_layer.*, a classifier)"""
    parts = key.split(".")
    if len(parts) == 3 and parts[0] == "features" and parts[2] in ("weight", "bias"):
        return key
    if len(parts) == 4 and parts[0] == "net" and parts[1].startswith("slice") and parts[3] in ("weight", "bias"):
        return f"features.{parts[2]}.{parts[3]}"
    if len(parts) == 4 and parts[0].startswith("lin") and parts[1] == "model" and parts[2] in ("0", "1") and parts[3] == "weight":
        return f"{parts[0]}.model.1.weight"
    return None


def load_weights(paths):
    """one or more torch.load-able state dicts (paths, or dicts already loaded) -> the canonical fp32 state dict of
    expected_shapes().  Accepted keys: features.{i}.{weight,bias} (torchvision), net.slice{s}.{i}.{weight,bias} and
    lin{k}.model.{0,1}.weight (the reference's LPIPS.state_dict(), with or without the dropout slot).  Later files win.  Every shape
    is checked; a missing key is named in the error."""
    if isinstance(paths, (str, bytes, dict)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    want = expected_shapes()
    out = {}
    for p in paths:
        sd = p if isinstance(p, dict) else torch.load(p, map_location="cpu", weights_only=True)
        sd = sd.get("state_dict", sd)
        for key, v in sd.items():
            ck = _canonical_key(key)
            if ck is None or ck not in want:
                continue
            if tuple(v.shape) != want[ck]:
                raise ValueError(f"LPIPS weights: {key} has shape {tuple(v.shape)}, expected {want[ck]}")
            out[ck] = v.detach().to(torch.float32).contiguous()
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError(f"LPIPS weights: missing {', '.join(missing)}")
    return {k: out[k] for k in want}


def synth_weights(seed, path=None, style="torchvision"):
    """synthetic weights of the production architecture (the tests): convolutions He-normal with std = sqrt(2 / (9 Cin)), biases
    uniform in [0, 0.05], lin weights uniform in [0, 2 / C].  -> the canonical state dict; `path` also writes it as a state dict
    file, style "torchvision" (features.* keys) or "reference" (net.slice*.* keys and the dropout slot)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for i, (cin, cout) in zip(CONV_IDX, CONV_CH):
        sd[f"features.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{i}.bias"] = torch.rand(cout, generator=g) * 0.05
    for k, c in enumerate(TAP_CH):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) * (2.0 / c)
    if path is not None:
        assert style in ("torchvision", "reference"), style
        torch.save(sd if style == "torchvision" else to_reference_keys(sd), path)
    return sd


def to_reference_keys(sd):
    """the canonical state dict under the keys of the reference's LPIPS.state_dict()"""
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        out[f"net.slice{_SLICE_OF[int(parts[1])]}.{parts[1]}.{parts[2]}" if parts[0] == "features" else k] = v
    return out


class LpipsVGG:
    """weights: load_weights' / synth_weights' dict, or path(s) for load_weights.  The convolution weights are reordered to
    (Cout, (ky, kx, cin)) once (conv1_1 zero-padded from 3 to 32 input channels) and split into planes on first use."""

    def __init__(self, weights, device):
        sd = load_weights(weights)
        self.device = torch.device(device)
        self.conv = []
        for i, (cin, cout) in zip(CONV_IDX, CONV_CH):
            w = sd[f"features.{i}.weight"].permute(0, 2, 3, 1)                    # (Cout, ky, kx, cin)
            if cin % 32:
                w = torch.cat([w, torch.zeros(cout, 3, 3, 32 - cin % 32)], dim=3)
            cin_p = w.shape[3]
            self.conv.append((w.reshape(cout, 9 * cin_p).contiguous().to(self.device), sd[f"features.{i}.bias"].to(self.device), cin_p, cout))
        self.lin = [sd[f"lin{k}.model.1.weight"].reshape(-1).contiguous().to(self.device) for k in range(5)]
        self.max_pixels = MAX_PIXELS

    def _chunk(self, a, b, layers):
        """layers (5, Bc) float64 on the device <- the five tap distances of the pairs (a[j], b[j]); no synchronisation"""
        from . import ops
        Bc, H, W, _ = a.shape
        hp = ops.halo_planes_buffer(self.device, 2 * Bc, H, W, 32)
        ops.lpips_input(a, hp, 0)
        ops.lpips_input(b, hp, Bc)
        h, w, tap = H, W, 0
        for j, (wt, bias, cin, cout) in enumerate(self.conv):
            y = ops.conv3x3(hp, wt, bias, 2 * Bc, h, w, cin, cout, precision="split3")       # before its ReLU: the consumers apply it
            if j in TAP_AFTER:
                ops.lpips_head(y, self.lin[tap], Bc, h, w, out=layers[tap])
                tap += 1
            if j + 1 < len(self.conv):
                pool = j in POOL_AFTER
                hp = ops.relu_pool_halo(y, 2 * Bc, h, w, cout, pool=pool)
                if pool:
                    h, w = h // 2, w // 2

    def measure(self, a_u8, b_u8):
        """a_u8, b_u8: (B, H, W, 3) u8 CUDA tensors -> (lpips (B,) float64, layers (B, 5) float64: the five taps' distances, lpips =
        their sum in tap order), numpy, one read-back; None when min(H, W) < 16.  The batch runs in chunks of at most
        max_pixels = 2^21 pixels (2 Bc H W, both sides counted; at least one pair), so memory does not grow with B: a chunk holds one
        convolution output of at most 256 B per pixel and operand planes of at most 384 B per pixel, and the planes buffers of a
        geometry are cached (ops.halo_planes_buffer).  A pair's result depends neither on the chunking nor on its slot."""
        assert a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.shape == b_u8.shape and a_u8.is_cuda and b_u8.is_cuda
        assert a_u8.dim() == 4 and a_u8.shape[3] == 3 and a_u8.shape[0] >= 1
        B, H, W, _ = a_u8.shape
        if min(H, W) < MIN_SIDE:
            return None
        a_u8, b_u8 = a_u8.contiguous(), b_u8.contiguous()
        step = max(1, int(self.max_pixels) // (2 * H * W))
        layers = torch.empty(5, B, dtype=torch.float64, device=self.device)
        for s in range(0, B, step):
            n = min(step, B - s)
            part = layers[:, s:s + n] if n == B else torch.empty(5, n, dtype=torch.float64, device=self.device)
            self._chunk(a_u8[s:s + n], b_u8[s:s + n], part)
            if n != B:
                layers[:, s:s + n] = part
        lay = np.ascontiguousarray(layers.cpu().numpy().T)
        total = lay[:, 0].copy()
        for k in range(1, 5):
            total += lay[:, k]
        return total, lay
