"""A torch restatement of LPIPS with the AlexNet trunk (lpips.LPIPS(net="alex", version="0.1") called with
normalize=True) in a chosen dtype, on the CPU: the checker of sgic_amd.lpips_alex, never the thing measured.  It imports nothing
from the package; weights come in as the canonical state dict (features.{0,3,6,8,10}.{weight,bias}, lin{k}.model.1.weight).  Also the
case list that the CPU and the GPU tests share."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpips_ref import natural  # noqa: E402

CONV = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
POOL_BEFORE = (3, 6)                      # max-pool 3x3 / stride 2 (no padding, floor) sits in front of these convolutions
TAP_CH = (64, 192, 384, 256, 256)         # every convolution's ReLU is a tap
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

SIZES = ((1, 31, 31), (2, 35, 67), (3, 64, 48), (1, 95, 130))
KINDS = ("identical", "noise5", "noise40", "independent", "flat")
SEED = 1234


def extents(n):
    n1 = (n - 7) // 4 + 1
    n2 = (n1 - 3) // 2 + 1
    return n1, n2, (n2 - 3) // 2 + 1


def input_layer(u8, dtype=torch.float32):
    """(B, H, W, 3) u8 -> (B, 3, H, W): every step one operation of `dtype`"""
    u8 = u8 if isinstance(u8, torch.Tensor) else torch.from_numpy(np.array(u8))      # a copy: the shared cases are read-only
    x = u8.to(dtype) / 255.0 * 2.0 - 1.0
    y = (x - torch.tensor(SHIFT, dtype=dtype)) / torch.tensor(SCALE, dtype=dtype)
    return y.permute(0, 3, 1, 2).contiguous()


def taps(u8, sd, dtype):
    """the five tap feature maps (after their ReLU), each (B, C, h, w)"""
    x = input_layer(u8, dtype)
    out = []
    for i, _, _, _, stride, pad in CONV:
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"].to(dtype), sd[f"features.{i}.bias"].to(dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def head(fa, fb, w):
    """one tap: (B, C, h, w) features of both sides, w (C,) -> (B,) in the features' dtype"""
    ua = fa / (torch.sqrt((fa * fa).sum(dim=1, keepdim=True)) + 1e-10)
    ub = fb / (torch.sqrt((fb * fb).sum(dim=1, keepdim=True)) + 1e-10)
    return (w.to(fa.dtype).reshape(1, -1, 1, 1) * (ua - ub) ** 2).sum(dim=1).mean(dim=(1, 2))


def lpips(a_u8, b_u8, sd, dtype=torch.float64):
    """-> (lpips (B,), layers (B, 5)) as float64 numpy arrays, computed in `dtype`; lpips = the layers summed in tap order"""
    with torch.no_grad():
        ta, tb = taps(a_u8, sd, dtype), taps(b_u8, sd, dtype)
        layers = torch.stack([head(x, y, sd[f"lin{k}.model.1.weight"].reshape(-1)) for k, (x, y) in enumerate(zip(ta, tb))], dim=1)
        total = layers[:, 0].clone()
        for k in range(1, 5):
            total = total + layers[:, k]
    return total.double().numpy(), layers.double().numpy()


@functools.lru_cache(maxsize=None)
def case_list(seed=SEED):
    """one entry per size of SIZES: {"size": (B, H, W), "a", "b": (5 B, H, W, 3) u8} with the pair kinds of KINDS in blocks of B
    rows: identical, noise of +-5 and of +-40 levels, an independent image, flat 17 against flat 200.  Read-only."""
    rng = np.random.default_rng(seed)
    out = []
    for B, H, W in SIZES:
        base = natural(rng, B, H, W)

        def noisy(amp):
            return np.clip(base.astype(np.int64) + rng.integers(-amp, amp + 1, base.shape), 0, 255).astype(np.uint8)
        a = np.concatenate([base, base, base, base, np.full_like(base, 17)])
        b = np.concatenate([base, noisy(5), noisy(40), natural(rng, B, H, W), np.full_like(base, 200)])
        a.setflags(write=False)
        b.setflags(write=False)
        out.append({"size": (B, H, W), "a": a, "b": b})
    return tuple(out)


def synth_state(seed=SEED):
    """the tests' synthetic weights with the package's recipe restated: He-normal convolutions (std = sqrt(2 / (k k Cin))), biases
    uniform in [0, 0.05], lin weights uniform in [0, 2 / C]"""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for i, cin, cout, k, _, _ in CONV:
        sd[f"features.{i}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5
        sd[f"features.{i}.bias"] = torch.rand(cout, generator=g) * 0.05
    for k, c in enumerate(TAP_CH):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) * (2.0 / c)
    return sd


@functools.lru_cache(maxsize=None)
def reference(seed=SEED):
    """the fp64 restatement over case_list(seed) with synth_state(seed): a tuple of (lpips (5 B,), layers (5 B, 5)) per size.
    Computed once per process and shared; read-only."""
    sd = synth_state(seed)
    out = []
    for case in case_list(seed):
        tot, lay = lpips(case["a"], case["b"], sd, torch.float64)
        tot.setflags(write=False)
        lay.setflags(write=False)
        out.append((tot, lay))
    return tuple(out)
