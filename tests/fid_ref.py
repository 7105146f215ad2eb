"""The FID Inception-v3 (pytorch-fid's InceptionV3 at pool3) restated with torch.nn.functional in a chosen dtype:
the reference of the FID tests.  No torchvision.  Weights: the canonical state dict of sgic_amd.fid (synth_weights / load_weights);
the BatchNorms are folded as the product folds them (fp64, rounded to fp32), then cast to the dtype."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def fold(sd, name, dtype):
    w = sd[f"{name}.conv.weight"].double()
    scale = sd[f"{name}.bn.weight"].double() / torch.sqrt(sd[f"{name}.bn.running_var"].double() + EPS)
    b = sd[f"{name}.bn.bias"].double() - sd[f"{name}.bn.running_mean"].double() * scale
    return (w * scale[:, None, None, None]).float().to(dtype), b.float().to(dtype)


class Ref:
    def __init__(self, sd, dtype=torch.float64, device="cpu"):
        self.sd, self.dtype, self.device = sd, dtype, torch.device(device)
        self.cache = {}
        self.trace = None          # a list: every convolution's (name, output before the ReLU) is appended

    def conv(self, x, name, stride=1, padding=0):
        if name not in self.cache:
            w, b = fold(self.sd, name, self.dtype)
            self.cache[name] = (w.to(self.device), b.to(self.device))
        w, b = self.cache[name]
        y = F.conv2d(x, w, b, stride=stride, padding=padding)
        if self.trace is not None:
            self.trace.append((name, y))
        return F.relu(y)

    def a(self, x, n):
        b1 = self.conv(x, f"{n}.branch1x1")
        b5 = self.conv(self.conv(x, f"{n}.branch5x5_1"), f"{n}.branch5x5_2", padding=2)
        b3 = self.conv(self.conv(self.conv(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1), f"{n}.branch3x3dbl_3", padding=1)
        bp = self.conv(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), f"{n}.branch_pool")
        return torch.cat([b1, b5, b3, bp], 1)

    def b(self, x, n):
        b3 = self.conv(x, f"{n}.branch3x3", stride=2)
        bd = self.conv(self.conv(self.conv(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1), f"{n}.branch3x3dbl_3", stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def c(self, x, n):
        b1 = self.conv(x, f"{n}.branch1x1")
        b7 = self.conv(x, f"{n}.branch7x7_1")
        b7 = self.conv(b7, f"{n}.branch7x7_2", padding=(0, 3))
        b7 = self.conv(b7, f"{n}.branch7x7_3", padding=(3, 0))
        bd = self.conv(x, f"{n}.branch7x7dbl_1")
        bd = self.conv(bd, f"{n}.branch7x7dbl_2", padding=(3, 0))
        bd = self.conv(bd, f"{n}.branch7x7dbl_3", padding=(0, 3))
        bd = self.conv(bd, f"{n}.branch7x7dbl_4", padding=(3, 0))
        bd = self.conv(bd, f"{n}.branch7x7dbl_5", padding=(0, 3))
        bp = self.conv(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), f"{n}.branch_pool")
        return torch.cat([b1, b7, bd, bp], 1)

    def d(self, x, n):
        b3 = self.conv(self.conv(x, f"{n}.branch3x3_1"), f"{n}.branch3x3_2", stride=2)
        b7 = self.conv(x, f"{n}.branch7x7x3_1")
        b7 = self.conv(b7, f"{n}.branch7x7x3_2", padding=(0, 3))
        b7 = self.conv(b7, f"{n}.branch7x7x3_3", padding=(3, 0))
        b7 = self.conv(b7, f"{n}.branch7x7x3_4", stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def e(self, x, n, pool):
        b1 = self.conv(x, f"{n}.branch1x1")
        b3 = self.conv(x, f"{n}.branch3x3_1")
        b3 = torch.cat([self.conv(b3, f"{n}.branch3x3_2a", padding=(0, 1)), self.conv(b3, f"{n}.branch3x3_2b", padding=(1, 0))], 1)
        bd = self.conv(self.conv(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1)
        bd = torch.cat([self.conv(bd, f"{n}.branch3x3dbl_3a", padding=(0, 1)), self.conv(bd, f"{n}.branch3x3dbl_3b", padding=(1, 0))], 1)
        p = F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) if pool == "avg" else F.max_pool2d(x, 3, 1, 1)
        return torch.cat([b1, b3, bd, self.conv(p, f"{n}.branch_pool")], 1)

    def input(self, u8_hwc):
        """(h, w, 3) u8 -> (1, 3, 299, 299): u / 255, bilinear (align_corners=False, no antialias), 2 x - 1"""
        x = torch.as_tensor(np.asarray(u8_hwc)).to(self.device).to(self.dtype).permute(2, 0, 1)[None] / 255
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
        return 2 * x - 1

    def features(self, u8_hwc, shapes=None):
        """(h, w, 3) u8 -> (2048,) in the dtype; shapes: a list that receives (H, C) after every stage"""
        return self.features_of_input(self.input(u8_hwc), shapes)[0]

    def features_of_input(self, x, shapes=None):
        """(B, 3, 299, 299) in [-1, 1] -> (B, 2048)"""
        note = (lambda t: shapes.append((t.shape[2], t.shape[1]))) if shapes is not None else (lambda t: None)
        x = self.conv(x, "Conv2d_1a_3x3", stride=2); note(x)
        x = self.conv(x, "Conv2d_2a_3x3"); note(x)
        x = self.conv(x, "Conv2d_2b_3x3", padding=1); note(x)
        x = F.max_pool2d(x, 3, 2); note(x)
        x = self.conv(x, "Conv2d_3b_1x1"); note(x)
        x = self.conv(x, "Conv2d_4a_3x3"); note(x)
        x = F.max_pool2d(x, 3, 2); note(x)
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = self.a(x, n); note(x)
        x = self.b(x, "Mixed_6a"); note(x)
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.c(x, n); note(x)
        x = self.d(x, "Mixed_7a"); note(x)
        x = self.e(x, "Mixed_7b", "avg"); note(x)
        x = self.e(x, "Mixed_7c", "max"); note(x)
        return x.mean(dim=(2, 3))


def resize_f64(u):
    """(h, w, 3) u8 -> (299, 299, 3) float64 by the written rule"""
    h, w, _ = u.shape
    x = u.astype(np.float64) / 255

    def axis(n):
        src = np.maximum((np.arange(299) + 0.5) * (n / 299) - 0.5, 0)
        i0 = np.floor(src).astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1), src - i0
    y0, y1, ly = axis(h)
    x0, x1, lx = axis(w)
    lx = lx[None, :, None]
    top = (1 - lx) * x[y0][:, x0] + lx * x[y0][:, x1]
    bot = (1 - lx) * x[y1][:, x0] + lx * x[y1][:, x1]
    ly = ly[:, None, None]
    return 2 * ((1 - ly) * top + ly * bot) - 1


def kid_numpy(X, Y, idx):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    d = X.shape[1]
    est = []
    for ix, iy in idx:
        a, b = X[ix], Y[iy]
        s = len(ix)
        kxx, kyy, kxy = (a @ a.T / d + 1) ** 3, (b @ b.T / d + 1) ** 3, (a @ b.T / d + 1) ** 3
        est.append((kxx.sum() - np.trace(kxx)) / (s * (s - 1)) + (kyy.sum() - np.trace(kyy)) / (s * (s - 1)) - 2 * kxy.sum() / (s * s))
    return float(np.mean(est)), float(np.std(est))


def ref_images():
    """the three inputs of the feature tests: (h, w, 3) u8 arrays: one 299 x 299 image and two windows of a 64 x 80 canvas; ->
    (big (1, 299, 299, 3), canvas (1, 64, 80, 3), descriptors of the two windows, the three images)"""
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:299, 0:299]
    big = np.stack([127 + 90 * np.sin(xx / 23.0 + c) * np.cos(yy / (17.0 + 3 * c)) for c in range(3)], -1) + rng.normal(0, 12, (299, 299, 3))
    big = np.clip(big, 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:64, 0:80]
    small = np.stack([120 + 100 * np.sin(xx / 5.0 + 2 * c) * np.sin(yy / (4.0 + c)) for c in range(3)], -1) + rng.normal(0, 20, (64, 80, 3))
    small = np.clip(small, 0, 255).astype(np.uint8)
    desc = np.array([(0, 0, 0, 64, 64), (0, 11, 27, 40, 53)], dtype=np.int32)
    imgs = [big, small[0:64, 0:64], small[11:51, 27:80]]
    return big[None], small[None], desc, imgs
