"""LPIPS with the AlexNet trunk, lpips.LPIPS(net="alex", version="0.1")(a, b, normalize=True): the `lpips` that the reference's
Quality_Model (taming/modules/losses/quality.py) evaluates with, on the GPU.  The definition is written out in DESIGN.md section 16;
its trunk is torchvision's alexnet().features.  The first two convolutions (11x11 stride 4, 5x5) run as bf16x3 split GEMMs over patch
matrices that csrc/lpips_alex.hip writes directly as operand planes; the last three run through ops.conv3x3 as implicit split GEMMs;
the ReLU / 3x3 max-pool producers are csrc/lpips_alex.hip, the stride-1 ReLU producer and the head are csrc/lpips.hip.  Always the
split kernels, also under SGIC_GEMM=f32: the path needs the planes layout.  Weights are a checkpoint the user has (load_weights) or
synthetic (synth_weights: the tests)."""
import math

import numpy as np
import torch

# torchvision's alexnet().features: index of every convolution, (Cin, Cout, kernel, stride, pad); a max-pool 3x3 / 2 sits in front of
# the convolutions at positions POOL_BEFORE; every convolution's ReLU is a tap
CONV_IDX = (0, 3, 6, 8, 10)
CONV_CFG = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_BEFORE = (1, 2)
TAP_CH = (64, 192, 384, 256, 256)
MIN_SIDE = 31                        # the stride-4 convolution and two pools must leave a pixel
K1_PAD = 384                         # 11 * 11 * 3 = 363 columns of the first patch matrix, padded to whole 32-column slices
MAX_PIXELS = 1 << 21                 # pixels of one chunk, both sides of its pairs counted (see LpipsAlex.measure)


def extents(n):
    """an input extent -> the extents after the first convolution, the first pool and the second pool"""
    n1 = (n - 7) // 4 + 1
    n2 = (n1 - 3) // 2 + 1
    return n1, n2, (n2 - 3) // 2 + 1


def expected_shapes():
    """canonical key -> shape: features.{i}.{weight,bias} and lin{k}.model.1.weight"""
    out = {}
    for i, (cin, cout, k, _, _) in zip(CONV_IDX, CONV_CFG):
        out[f"features.{i}.weight"] = (cout, cin, k, k)
        out[f"features.{i}.bias"] = (cout,)
    for k, c in enumerate(TAP_CH):
        out[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return out


def _canonical_key(key):
    """a checkpoint's key -> the canonical key, or None for a key that is not part of LPIPS-Alex (scaling_layer.*, a classifier)"""
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
    expected_shapes().  Accepted keys: features.{0,3,6,8,10}.{weight,bias} (torchvision), net.slice{1..5}.{i}.{weight,bias} and
    lin{k}.model.{0,1}.weight (the package's LPIPS.state_dict(), with or without the dropout slot).  Later files win.  Every shape is
    checked; a missing key is named in the error; keys of anything else are ignored."""
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
                raise ValueError(f"LPIPS-Alex weights: {key} has shape {tuple(v.shape)}, expected {want[ck]}")
            out[ck] = v.detach().to(torch.float32).contiguous()
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError(f"LPIPS-Alex weights: missing {', '.join(missing)}")
    return {k: out[k] for k in want}


def synth_weights(seed, path=None, style="torchvision"):
    """synthetic weights of the production architecture (the tests): convolutions He-normal with std = sqrt(2 / (k k Cin)), biases
    uniform in [0, 0.05], lin weights uniform in [0, 2 / C].  -> the canonical state dict; `path` also writes it as a state dict
    file, style "torchvision" (features.* keys) or "reference" (net.slice*.* keys and the dropout slot)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for i, (cin, cout, k, _, _) in zip(CONV_IDX, CONV_CFG):
        sd[f"features.{i}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (k * k * cin))
        sd[f"features.{i}.bias"] = torch.rand(cout, generator=g) * 0.05
    for k, c in enumerate(TAP_CH):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) * (2.0 / c)
    if path is not None:
        assert style in ("torchvision", "reference"), style
        torch.save(sd if style == "torchvision" else to_reference_keys(sd), path)
    return sd


def to_reference_keys(sd):
    """the canonical state dict under the keys of the package's LPIPS.state_dict(): net.slice{j+1}.{i} for the j-th convolution"""
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        out[f"net.slice{CONV_IDX.index(int(parts[1])) + 1}.{parts[1]}.{parts[2]}" if parts[0] == "features" else k] = v
    return out


class LpipsAlex:
    """weights: load_weights' / synth_weights' dict, or path(s) for load_weights.  The convolution weights are reordered to
    (Cout, (ky, kx, cin)) once (the first zero-padded from 363 to 384 columns) and split into planes on first use."""

    def __init__(self, weights, device):
        sd = load_weights(weights)
        self.device = torch.device(device)
        self.conv = []
        for i, (cin, cout, k, _, _) in zip(CONV_IDX, CONV_CFG):
            w = sd[f"features.{i}.weight"].permute(0, 2, 3, 1).reshape(cout, k * k * cin)           # (Cout, (ky, kx, cin))
            if w.shape[1] % 32:
                w = torch.cat([w, torch.zeros(cout, 32 - w.shape[1] % 32)], dim=1)
            self.conv.append((w.contiguous().to(self.device), sd[f"features.{i}.bias"].to(self.device), cin, cout))
        assert self.conv[0][0].shape[1] == K1_PAD
        self.lin = [sd[f"lin{k}.model.1.weight"].reshape(-1).contiguous().to(self.device) for k in range(5)]
        self.max_pixels = MAX_PIXELS

    def _chunk(self, a, b, layers):
        """layers (5, Bc) float64 on the device <- the five tap distances of the pairs (a[j], b[j]); no synchronisation"""
        from . import ops
        Bc, H, W, _ = a.shape
        n = 2 * Bc
        (h1, h2, h3), (w1, w2, w3) = extents(H), extents(W)
        # 11x11 / 4: patches of both sides in one operand -> GEMM
        pl = ops.Planes(n * h1 * w1, K1_PAD, self.device)
        ops.lpips_alex_conv1_patches(a, pl, 0)
        ops.lpips_alex_conv1_patches(b, pl, Bc)
        wt, bias, _, c1 = self.conv[0]
        y = ops.gemm(pl, wt, bias, precision="split3")                     # before its ReLU: the consumers apply it
        ops.lpips_head(y, self.lin[0], Bc, h1, w1, out=layers[0])
        # pool, 5x5: patches of the pooled map -> GEMM
        wt, bias, _, c2 = self.conv[1]
        y = ops.gemm(ops.relu_maxpool3_patches5(y, n, h1, w1, c1), wt, bias, precision="split3")
        ops.lpips_head(y, self.lin[1], Bc, h2, w2, out=layers[1])
        # pool, then the three 3x3 convolutions on the implicit path
        hp = ops.relu_maxpool3_halo(y, n, h2, w2, c2)
        for j in (2, 3, 4):
            wt, bias, cin, cout = self.conv[j]
            y = ops.conv3x3(hp, wt, bias, n, h3, w3, cin, cout, precision="split3")
            ops.lpips_head(y, self.lin[j], Bc, h3, w3, out=layers[j])
            if j < 4:
                hp = ops.relu_pool_halo(y, n, h3, w3, cout, pool=False)

    def measure(self, a_u8, b_u8):
        """a_u8, b_u8: (B, H, W, 3) u8 CUDA tensors -> (lpips (B,) float64, layers (B, 5) float64: the five taps' distances, lpips =
        their sum in tap order), numpy, one read-back; None when min(H, W) < 31.  The batch runs in chunks of at most
        max_pixels = 2^21 pixels (2 Bc H W, both sides counted; at least one pair), so memory does not grow with B.  Per input
        pixel a chunk holds: the first patch operand, 384 * 6 B per 16 pixels = 144 B; the second, 1600 * 6 B per pooled pixel, of
        which there is one per roughly 64 input pixels = 150 B; the first convolution's output, 16 B; everything behind it is smaller.
        All are below the 384 B per pixel of lpips.LpipsVGG.  The halo planes of a geometry are cached (ops.halo_planes_buffer).  A
        pair's result depends neither on the chunking nor on its slot."""
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
