"""DISTS with the VGG16 trunk (DISTS_pytorch / piq.DISTS, what the reference's Quality_Model reports next to LPIPS), on the GPU: the
definition is written out in DESIGN.md section 15.  The trunk is the thirteen 3x3 convolutions of lpips.LpipsVGG through ops.conv3x3 as
implicit bf16x3 split GEMMs; the input layer, the exact u8 moments of tap 0, ReLU + L2 pool into the next convolution's operand planes
and the moments and head of taps 1..5 are csrc/dists.hip.  Weights are a checkpoint the user has (load_weights) or synthetic
(synth_weights: the tests)."""
import numpy as np
import torch

from .lpips import MIN_SIDE
from .perceptual import CONV_CH, CONV_IDX, MAX_PIXELS, POOL_AFTER, TAP_AFTER  # noqa: F401 -- also this module's names
from .perceptual import checked_pair, chunked, load_state, run_vgg16, vgg_conv, vgg_synth_trunk

TAP_CH = (3, 64, 128, 256, 512, 512)      # tap 0 is the image itself
N_CH = sum(TAP_CH)                        # 1475
C1 = C2 = 1e-6
STYLES = ("torchvision", "dists_pytorch", "piq")
_STAGE_OF = {i: 1 + sum(i >= s for s in (4, 9, 16, 23)) for i in CONV_IDX}      # DISTS_pytorch's stage{s}.{i}


def expected_shapes():
    """canonical key -> shape: features.{i}.{weight,bias}, alpha and beta"""
    out = {}
    for i, (cin, cout) in zip(CONV_IDX, CONV_CH):
        out[f"features.{i}.weight"] = (cout, cin, 3, 3)
        out[f"features.{i}.bias"] = (cout,)
    out["alpha"] = (N_CH,)
    out["beta"] = (N_CH,)
    return out


def _canonical_key(key):
    """a checkpoint's key -> the canonical key, or None for a key that is not part of DISTS-VGG (a pool's filter, mean / std, a
    classifier)"""
    if key in ("alpha", "beta"):
        return key
    parts = key.split(".")
    if len(parts) == 3 and parts[2] in ("weight", "bias") and parts[1].isdigit() and \
            (parts[0] in ("features", "model") or (parts[0].startswith("stage") and parts[0][5:].isdigit())):
        return f"features.{parts[1]}.{parts[2]}"
    return None


def load_weights(paths):
    """one or more torch.load-able state dicts (paths, or dicts already loaded) -> the canonical fp32 state dict of
    expected_shapes().  Accepted keys: the trunk as features.{i}.{weight,bias} (torchvision), stage{s}.{i}.{weight,bias}
    (DISTS_pytorch) or model.{i}.{weight,bias} (piq); alpha and beta of shape (1, 1475, 1, 1) or (1475,).  Later files win.  Every
    shape is checked; a missing key is named in the error."""
    return load_state(paths, expected_shapes(), _canonical_key, "DISTS", {k: ((1, N_CH, 1, 1),) for k in ("alpha", "beta")})


def synth_weights(seed, path=None, style="torchvision"):
    """synthetic weights of the production architecture (the tests): the trunk by lpips.synth_weights' recipe (He-normal convolutions,
    std = sqrt(2 / (9 Cin)), biases uniform in [0, 0.05]), then alpha and beta uniform in (0, 0.2].  -> the canonical state dict; `path`
    also writes it as a state dict file in one of STYLES: "torchvision" (features.* and flat alpha, beta), "dists_pytorch" (stage*.*,
    alpha and beta as (1, 1475, 1, 1)) or "piq" (model.*, alpha and beta as (1, 1475, 1, 1))."""
    g = torch.Generator().manual_seed(int(seed))
    sd = vgg_synth_trunk(g)
    sd["alpha"] = (1.0 - torch.rand(N_CH, generator=g)) * 0.2
    sd["beta"] = (1.0 - torch.rand(N_CH, generator=g)) * 0.2
    if path is not None:
        torch.save(to_style(sd, style), path)
    return sd


def to_style(sd, style):
    """the canonical state dict under the keys and shapes of one of STYLES"""
    assert style in STYLES, style
    if style == "torchvision":
        return dict(sd)
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        if parts[0] == "features":
            head = f"stage{_STAGE_OF[int(parts[1])]}" if style == "dists_pytorch" else "model"
            out[f"{head}.{parts[1]}.{parts[2]}"] = v
        else:
            out[k] = v.reshape(1, N_CH, 1, 1)
    return out


def tap0_terms(m, n, alpha, beta):
    """tap 0 from the exact integer sums: m (B, 3, 5) int64 (sum a, sum b, sum a^2, sum b^2, sum a b of the u8 values over n pixels),
    alpha, beta: three floats each -> (B, 2) float64, the structure and texture sums of x = u / 255, not yet divided by W.  The
    variances come from the integers n sum a^2 - (sum a)^2, which are exact, so a flat image has variance exactly 0."""
    out = np.zeros((m.shape[0], 2), dtype=np.float64)
    den = 65025 * n * n
    for b in range(m.shape[0]):
        s = t = 0.0
        for c in range(3):
            sa, sb, saa, sbb, sab = (int(v) for v in m[b, c])
            mx, my = sa / (255 * n), sb / (255 * n)
            vx, vy, cxy = (n * saa - sa * sa) / den, (n * sbb - sb * sb) / den, (n * sab - sa * sb) / den
            S1 = (2.0 * (mx * my) + C1) / ((mx * mx + my * my) + C1)
            S2 = (2.0 * cxy + C2) / ((vx + vy) + C2)
            s += float(alpha[c]) * (1.0 - S1)
            t += float(beta[c]) * (1.0 - S2)
        out[b] = (s, t)
    return out


class DistsVGG:
    """weights: load_weights' / synth_weights' dict, or path(s) for load_weights.  The convolution weights are reordered to
    (Cout, (ky, kx, cin)) once (conv1_1 zero-padded from 3 to 32 input channels) and split into planes on first use."""

    def __init__(self, weights, device):
        sd = load_weights(weights)
        self.device = torch.device(device)
        self.conv = vgg_conv(sd, self.device)
        alpha, beta = torch.split(sd["alpha"], TAP_CH), torch.split(sd["beta"], TAP_CH)
        self.alpha0, self.beta0 = alpha[0].tolist(), beta[0].tolist()
        self.alpha = [v.contiguous().to(self.device) for v in alpha[1:]]
        self.beta = [v.contiguous().to(self.device) for v in beta[1:]]
        self.W = float(sd["alpha"].double().sum() + sd["beta"].double().sum())
        assert self.W > 0.0, "DISTS weights: alpha and beta sum to nothing"
        self.max_pixels = MAX_PIXELS

    def _chunk(self, a, b, terms, m0):
        """terms (5, Bc, 2) float64 and m0 (Bc, 3, 5) int64 on the device <- the unnormalised terms of taps 1..5 and the u8 sums of
        tap 0 of the pairs (a[j], b[j]); no synchronisation"""
        from . import ops
        Bc, H, W, _ = a.shape
        ops.dists_moments_u8(a, b, out=m0)
        hp = ops.halo_planes_buffer(self.device, 2 * Bc, H, W, 32)
        ops.dists_input(a, hp, 0)
        ops.dists_input(b, hp, Bc)
        run_vgg16(self.conv, hp, 2 * Bc, H, W,
                  lambda tap, y, h, w: ops.dists_head(ops.dists_moments(y, Bc, h, w), self.alpha[tap], self.beta[tap], h, w, out=terms[tap]),
                  lambda y, h, w, c, pooled: ops.relu_l2pool_halo(y, 2 * Bc, h, w, c) if pooled
                  else ops.relu_pool_halo(y, 2 * Bc, h, w, c, pool=False))

    def measure(self, a_u8, b_u8):
        """a_u8, b_u8: (B, H, W, 3) u8 CUDA tensors -> (dists (B,) float64, terms (B, 6, 2) float64: every tap's structure and texture
        term, already divided by W = sum alpha + sum beta; dists = the terms added in tap order, structure before texture), numpy, one
        read-back; None when min(H, W) < 16.  The batch runs in chunks of at most max_pixels = 2^21 pixels, as LpipsVGG.measure does.
        A pair's result depends neither on the chunking nor on its slot."""
        pair = checked_pair(a_u8, b_u8, MIN_SIDE)
        if pair is None:
            return None
        B, H, W, _ = a_u8.shape
        res = torch.empty(B, 25, dtype=torch.int64, device=self.device)       # per pair: 5 x 2 fp64 bit patterns, then 3 x 5 integers

        def one(s, n):
            terms = torch.empty(5, n, 2, dtype=torch.float64, device=self.device)
            m0 = torch.empty(n, 3, 5, dtype=torch.int64, device=self.device)
            self._chunk(pair[0][s:s + n], pair[1][s:s + n], terms, m0)
            res[s:s + n, :10] = terms.view(torch.int64).permute(1, 0, 2).reshape(n, 10)
            res[s:s + n, 10:] = m0.view(n, 15)
        chunked(one, B, H, W, self.max_pixels)
        raw = res.cpu().numpy()
        out = np.empty((B, 6, 2), dtype=np.float64)
        out[:, 0] = tap0_terms(raw[:, 10:].reshape(B, 3, 5), H * W, self.alpha0, self.beta0)
        out[:, 1:] = np.ascontiguousarray(raw[:, :10]).view(np.float64).reshape(B, 5, 2)
        out /= self.W
        total = np.zeros(B, dtype=np.float64)
        for k in range(6):
            for t in range(2):
                total += out[:, k, t]
        return total, out
