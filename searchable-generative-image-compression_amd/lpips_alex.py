"""LPIPS with the AlexNet trunk, lpips.LPIPS(net="alex", version="0.1")(a, b, normalize=True): the `lpips` that the reference's
Quality_Model (taming/modules/losses/quality.py) evaluates with, on the GPU.  The definition is written out in DESIGN.md section 16;
its trunk is torchvision's alexnet().features.  The first two convolutions (11x11 stride 4, 5x5) run as bf16x3 split GEMMs over patch
matrices that csrc/lpips_alex.hip writes directly as operand planes; the last three run through ops.conv3x3 as implicit split GEMMs;
the ReLU / 3x3 max-pool producers are csrc/lpips_alex.hip, the stride-1 ReLU producer and the head are csrc/lpips.hip.  Always the
split kernels, also under SGIC_GEMM=f32: the path needs the planes layout.  Weights are a checkpoint the user has (load_weights) or
synthetic (synth_weights: the tests)."""
import math

import torch

from .perceptual import MAX_PIXELS, LpipsMeasure, conv_matrix, load_state, lpips_canonical_key

# torchvision's alexnet().features: index of every convolution, (Cin, Cout, kernel, stride, pad); a max-pool 3x3 / 2 sits in front of
# the convolutions at positions POOL_BEFORE; every convolution's ReLU is a tap
CONV_IDX = (0, 3, 6, 8, 10)
CONV_CFG = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_BEFORE = (1, 2)
TAP_CH = (64, 192, 384, 256, 256)
MIN_SIDE = 31                        # the stride-4 convolution and two pools must leave a pixel
K1_PAD = 384                         # 11 * 11 * 3 = 363 columns of the first patch matrix, padded to whole 32-column slices


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


def load_weights(paths):
    """one or more torch.load-able state dicts (paths, or dicts already loaded) -> the canonical fp32 state dict of
    expected_shapes().  Accepted keys: features.{0,3,6,8,10}.{weight,bias} (torchvision), net.slice{1..5}.{i}.{weight,bias} and
    lin{k}.model.{0,1}.weight (the package's LPIPS.state_dict(), with or without the dropout slot).  Later files win.  Every shape is
    checked; a missing key is named in the error; keys of anything else are ignored."""
    return load_state(paths, expected_shapes(), lpips_canonical_key, "LPIPS-Alex")


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


class LpipsAlex(LpipsMeasure):
    """weights: load_weights' / synth_weights' dict, or path(s) for load_weights.  The convolution weights are reordered to
    (Cout, (ky, kx, cin)) once (the first zero-padded from 363 to 384 columns) and split into planes on first use.  Per input pixel a
    chunk of measure holds: the first patch operand, 384 * 6 B per 16 pixels = 144 B; the second, 1600 * 6 B per pooled pixel, of
    which there is one per roughly 64 input pixels = 150 B; the first convolution's output, 16 B; everything behind it is smaller.
    All are below the 384 B per pixel of lpips.LpipsVGG."""
    min_side = MIN_SIDE

    def __init__(self, weights, device):
        sd = load_weights(weights)
        self.device = torch.device(device)
        self.conv = [(conv_matrix(sd[f"features.{i}.weight"]).to(self.device), sd[f"features.{i}.bias"].to(self.device), cin, cout)
                     for i, (cin, cout, _, _, _) in zip(CONV_IDX, CONV_CFG)]
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
