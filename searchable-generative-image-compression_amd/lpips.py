"""LPIPS with the VGG16 trunk (the reference's taming/modules/losses/lpips.py, whose trunk is torchvision's vgg16().features), on the
GPU: the definition is written out in DESIGN.md section 14.  The thirteen 3x3 convolutions run through ops.conv3x3 as implicit
bf16x3 split GEMMs (always, also under SGIC_GEMM=f32: the path needs the planes layout); the input layer, ReLU / max-pool into the
next convolution's operand planes and the head are csrc/lpips.hip.  Weights are a checkpoint the user has (load_weights) or
synthetic (synth_weights: the tests)."""
import torch

from .perceptual import CONV_CH, CONV_IDX, MAX_PIXELS, POOL_AFTER, TAP_AFTER  # noqa: F401 -- also this module's names
from .perceptual import LpipsMeasure, load_state, lpips_canonical_key, run_vgg16, vgg_conv, vgg_synth_trunk

TAP_CH = (64, 128, 256, 512, 512)
MIN_SIDE = 16                        # four pools must leave a pixel
_SLICE_OF = {i: 1 + sum(i >= s for s in (4, 9, 16, 23)) for i in CONV_IDX}      # the reference's net.slice{s}.{i}


def expected_shapes():
    """canonical key -> shape: features.{i}.{weight,bias} and lin{k}.model.1.weight"""
    out = {}
    for i, (cin, cout) in zip(CONV_IDX, CONV_CH):
        out[f"features.{i}.weight"] = (cout, cin, 3, 3)
        out[f"features.{i}.bias"] = (cout,)
    for k, c in enumerate(TAP_CH):
        out[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return out


def load_weights(paths):
    """one or more torch.load-able state dicts (paths, or dicts already loaded) -> the canonical fp32 state dict of
    expected_shapes().  Accepted keys: features.{i}.{weight,bias} (torchvision), net.slice{s}.{i}.{weight,bias} and
    lin{k}.model.{0,1}.weight (the reference's LPIPS.state_dict(), with or without the dropout slot).  Later files win.  Every shape
    is checked; a missing key is named in the error."""
    return load_state(paths, expected_shapes(), lpips_canonical_key, "LPIPS")


def synth_weights(seed, path=None, style="torchvision"):
    """synthetic weights of the production architecture (the tests): convolutions He-normal with std = sqrt(2 / (9 Cin)), biases
    uniform in [0, 0.05], lin weights uniform in [0, 2 / C].  -> the canonical state dict; `path` also writes it as a state dict
    file, style "torchvision" (features.* keys) or "reference" (net.slice*.* keys and the dropout slot)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = vgg_synth_trunk(g)
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


class LpipsVGG(LpipsMeasure):
    """weights: load_weights' / synth_weights' dict, or path(s) for load_weights.  The convolution weights are reordered to
    (Cout, (ky, kx, cin)) once (conv1_1 zero-padded from 3 to 32 input channels) and split into planes on first use.  A chunk of
    measure holds one convolution output of at most 256 B per pixel and operand planes of at most 384 B per pixel."""
    min_side = MIN_SIDE

    def __init__(self, weights, device):
        sd = load_weights(weights)
        self.device = torch.device(device)
        self.conv = vgg_conv(sd, self.device)
        self.lin = [sd[f"lin{k}.model.1.weight"].reshape(-1).contiguous().to(self.device) for k in range(5)]
        self.max_pixels = MAX_PIXELS

    def _chunk(self, a, b, layers):
        """layers (5, Bc) float64 on the device <- the five tap distances of the pairs (a[j], b[j]); no synchronisation"""
        from . import ops
        Bc, H, W, _ = a.shape
        hp = ops.halo_planes_buffer(self.device, 2 * Bc, H, W, 32)
        ops.lpips_input(a, hp, 0)
        ops.lpips_input(b, hp, Bc)
        run_vgg16(self.conv, hp, 2 * Bc, H, W,
                  lambda tap, y, h, w: ops.lpips_head(y, self.lin[tap], Bc, h, w, out=layers[tap]),
                  lambda y, h, w, c, pooled: ops.relu_pool_halo(y, 2 * Bc, h, w, c, pool=pooled))
