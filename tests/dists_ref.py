"""A torch restatement of DISTS with the VGG16 trunk in a chosen dtype, on the CPU: the checker of
sgic_amd.dists, never the thing measured.  It imports nothing from the package; weights come in as the canonical state dict
(features.{i}.{weight,bias}, alpha, beta of 1475 values).  The case list is that of tests/lpips_ref.py."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpips_ref import CONV_IDX, KINDS, POOL_BEFORE, SEED, SIZES, TAP_AFTER, case_list  # noqa: E402,F401

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
TAP_CH = (3, 64, 128, 256, 512, 512)
N_CH = 1475
C1 = C2 = 1e-6


def input_layer(u8, dtype=torch.float32):
    """(B, H, W, 3) u8 -> (x (B, 3, H, W) = u / 255: tap 0; h = (x - mean) / std: the trunk's input); every step one operation"""
    u8 = u8 if isinstance(u8, torch.Tensor) else torch.from_numpy(np.array(u8))      # a copy: the shared cases are read-only
    x = u8.to(dtype) / 255.0
    h = (x - torch.tensor(MEAN, dtype=dtype)) / torch.tensor(STD, dtype=dtype)
    return x.permute(0, 3, 1, 2).contiguous(), h.permute(0, 3, 1, 2).contiguous()


def l2pool(f):
    """(B, C, H, W), nonnegative -> sqrt(conv(f^2, g, stride 2, zero padding 1, depthwise) + 1e-12), g the 3x3 Hanning window
    normalised to sum 1: outer(a, a) / sum with a = (0.5, 1, 0.5), which is outer((1, 2, 1), (1, 2, 1)) / 16"""
    a = torch.tensor([1.0, 2.0, 1.0], dtype=f.dtype)
    g = (a[:, None] * a[None, :] / 16.0).reshape(1, 1, 3, 3).repeat(f.shape[1], 1, 1, 1)
    return torch.sqrt(F.conv2d(f * f, g, stride=2, padding=1, groups=f.shape[1]) + 1e-12)


def taps(u8, sd, dtype):
    """the six tap feature maps, each (B, C, h, w): the image in [0, 1], then relu1_2 .. relu5_3"""
    x0, x = input_layer(u8, dtype)
    out = [x0]
    for i in CONV_IDX:
        if i in POOL_BEFORE:
            x = l2pool(x)
        x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"].to(dtype), sd[f"features.{i}.bias"].to(dtype), stride=1, padding=1))
        if i in TAP_AFTER:
            out.append(x)
    return out


def head(fx, fy, alpha, beta):
    """one tap: (B, C, h, w) features of both sides, alpha, beta (C,) -> (B, 2): sum_c alpha_c (1 - S1_c), sum_c beta_c (1 - S2_c)
    in the features' dtype.  Variances and covariance are one expression, E[uv] - E[u] E[v]: x == y gives exactly 0."""
    mx, my = fx.mean(dim=(2, 3)), fy.mean(dim=(2, 3))
    vx = (fx * fx).mean(dim=(2, 3)) - mx * mx
    vy = (fy * fy).mean(dim=(2, 3)) - my * my
    cxy = (fx * fy).mean(dim=(2, 3)) - mx * my
    S1 = (2.0 * (mx * my) + C1) / ((mx * mx + my * my) + C1)
    S2 = (2.0 * cxy + C2) / ((vx + vy) + C2)
    return torch.stack([(alpha.to(fx.dtype) * (1.0 - S1)).sum(dim=1), (beta.to(fx.dtype) * (1.0 - S2)).sum(dim=1)], dim=1)


def dists(a_u8, b_u8, sd, dtype=torch.float64):
    """-> (dists (B,), terms (B, 6, 2)) as float64 numpy arrays, computed in `dtype`: terms are the taps' structure and texture sums
    divided by W = sum alpha + sum beta; dists = the terms added in tap order, structure before texture"""
    with torch.no_grad():
        ta, tb = taps(a_u8, sd, dtype), taps(b_u8, sd, dtype)
        alpha, beta = torch.split(sd["alpha"].reshape(-1), TAP_CH), torch.split(sd["beta"].reshape(-1), TAP_CH)
        W = (sd["alpha"].double().sum() + sd["beta"].double().sum()).to(dtype)
        terms = torch.stack([head(x, y, al, be) for x, y, al, be in zip(ta, tb, alpha, beta)], dim=1) / W
        total = torch.zeros(terms.shape[0], dtype=dtype)
        for k in range(6):
            for t in range(2):
                total = total + terms[:, k, t]
    return total.double().numpy(), terms.double().numpy()


def synth_state(seed=SEED):
    """the tests' synthetic weights with the package's recipe restated: the LPIPS trunk recipe (He-normal convolutions, biases uniform
    in [0, 0.05]), then alpha and beta uniform in (0, 0.2]"""
    g = torch.Generator().manual_seed(int(seed))
    ch = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512),
          (512, 512), (512, 512))
    sd = {}
    for i, (cin, cout) in zip(CONV_IDX, ch):
        sd[f"features.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"features.{i}.bias"] = torch.rand(cout, generator=g) * 0.05
    sd["alpha"] = (1.0 - torch.rand(N_CH, generator=g)) * 0.2
    sd["beta"] = (1.0 - torch.rand(N_CH, generator=g)) * 0.2
    return sd


@functools.lru_cache(maxsize=None)
def reference(seed=SEED):
    """the fp64 restatement over case_list(seed) with synth_state(seed): a tuple of (dists (5 B,), terms (5 B, 6, 2)) per size.
    Computed once per process and shared; read-only."""
    sd = synth_state(seed)
    out = []
    for case in case_list(seed):
        tot, terms = dists(case["a"], case["b"], sd, torch.float64)
        tot.setflags(write=False)
        terms.setflags(write=False)
        out.append((tot, terms))
    return tuple(out)
