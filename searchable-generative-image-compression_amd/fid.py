"""FID and KID between two sets of images, on the GPU: pytorch-fid's InceptionV3 at output block 3 ("pool3", 2048 values per image),
the Frechet distance of the two feature sets and the kernel inception distance with the cubic polynomial kernel.  The definition is
written out in DESIGN.md section 17.  Every convolution runs as a bf16x3 split GEMM (ops.gemm) over the patch planes that
csrc/fid.hip's one generic producer writes (ops.patches_split3), straight into its column slice of the block's concat buffer; the
resize, the pools, the final mean and the fp64 Gram matrices of the statistics are csrc/fid.hip too.  The two symmetric
eigen-decompositions of FID run once per evaluation in numpy fp64 on the host.  Always the split kernels, also under SGIC_GEMM=f32:
the path needs the planes layout.  Weights are a checkpoint the user has (load_weights) or synthetic (synth_weights: the tests)."""
import math

import numpy as np
import torch

SIDE = 299
DIM = 2048
BN_EPS = 1e-3
MAX_OPERAND_BYTES = 1 << 30                  # the largest patch operand of one chunk (see InceptionFID.features)
OPERAND_BYTES_PER_IMAGE = 147 * 147 * 288 * 6   # Conv2d_2b_3x3: 147 x 147 rows of 9 * 32 columns in three bf16 planes

# the trunk in front of the Mixed blocks: name, or a pool
TRUNK = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxs2", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxs2")
# Mixed blocks: name, kind, input channels, the kind's parameter (A: pool features, C: the 7x7 width, E: the pool)
BLOCKS = (("Mixed_5b", "A", 192, 32), ("Mixed_5c", "A", 256, 64), ("Mixed_5d", "A", 288, 64), ("Mixed_6a", "B", 288, None),
          ("Mixed_6b", "C", 768, 128), ("Mixed_6c", "C", 768, 160), ("Mixed_6d", "C", 768, 160), ("Mixed_6e", "C", 768, 192),
          ("Mixed_7a", "D", 768, None), ("Mixed_7b", "E", 1280, "avg"), ("Mixed_7c", "E", 2048, "max"))
# the branches of every kind, concatenated in this order: a string is a convolution (suffix of the block's name) or a pool ("avg",
# "max": 3x3 / 1 / 1; "maxs2": 3x3 / 2 / 0; "pool": the block's own, E only); a tuple forks: its convolutions read the same input and
# their outputs are concatenated
BRANCHES = {
    "A": (("branch1x1",), ("branch5x5_1", "branch5x5_2"), ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), ("avg", "branch_pool")),
    "B": (("branch3x3",), ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), ("maxs2",)),
    "C": (("branch1x1",), ("branch7x7_1", "branch7x7_2", "branch7x7_3"),
          ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"), ("avg", "branch_pool")),
    "D": (("branch3x3_1", "branch3x3_2"), ("branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"), ("maxs2",)),
    "E": (("branch1x1",), ("branch3x3_1", ("branch3x3_2a", "branch3x3_2b")),
          ("branch3x3dbl_1", "branch3x3dbl_2", ("branch3x3dbl_3a", "branch3x3dbl_3b")), ("pool", "branch_pool")),
}


def _block_convs(kind, cin, p):
    """suffix -> (Cin, Cout, kh, kw, stride, ph, pw) of one Mixed block"""
    if kind == "A":
        return {"branch1x1": (cin, 64, 1, 1, 1, 0, 0), "branch5x5_1": (cin, 48, 1, 1, 1, 0, 0), "branch5x5_2": (48, 64, 5, 5, 1, 2, 2),
                "branch3x3dbl_1": (cin, 64, 1, 1, 1, 0, 0), "branch3x3dbl_2": (64, 96, 3, 3, 1, 1, 1),
                "branch3x3dbl_3": (96, 96, 3, 3, 1, 1, 1), "branch_pool": (cin, p, 1, 1, 1, 0, 0)}
    if kind == "B":
        return {"branch3x3": (cin, 384, 3, 3, 2, 0, 0), "branch3x3dbl_1": (cin, 64, 1, 1, 1, 0, 0),
                "branch3x3dbl_2": (64, 96, 3, 3, 1, 1, 1), "branch3x3dbl_3": (96, 96, 3, 3, 2, 0, 0)}
    if kind == "C":
        return {"branch1x1": (cin, 192, 1, 1, 1, 0, 0), "branch7x7_1": (cin, p, 1, 1, 1, 0, 0), "branch7x7_2": (p, p, 1, 7, 1, 0, 3),
                "branch7x7_3": (p, 192, 7, 1, 1, 3, 0), "branch7x7dbl_1": (cin, p, 1, 1, 1, 0, 0),
                "branch7x7dbl_2": (p, p, 7, 1, 1, 3, 0), "branch7x7dbl_3": (p, p, 1, 7, 1, 0, 3),
                "branch7x7dbl_4": (p, p, 7, 1, 1, 3, 0), "branch7x7dbl_5": (p, 192, 1, 7, 1, 0, 3),
                "branch_pool": (cin, 192, 1, 1, 1, 0, 0)}
    if kind == "D":
        return {"branch3x3_1": (cin, 192, 1, 1, 1, 0, 0), "branch3x3_2": (192, 320, 3, 3, 2, 0, 0),
                "branch7x7x3_1": (cin, 192, 1, 1, 1, 0, 0), "branch7x7x3_2": (192, 192, 1, 7, 1, 0, 3),
                "branch7x7x3_3": (192, 192, 7, 1, 1, 3, 0), "branch7x7x3_4": (192, 192, 3, 3, 2, 0, 0)}
    assert kind == "E", kind
    return {"branch1x1": (cin, 320, 1, 1, 1, 0, 0), "branch3x3_1": (cin, 384, 1, 1, 1, 0, 0), "branch3x3_2a": (384, 384, 1, 3, 1, 0, 1),
            "branch3x3_2b": (384, 384, 3, 1, 1, 1, 0), "branch3x3dbl_1": (cin, 448, 1, 1, 1, 0, 0),
            "branch3x3dbl_2": (448, 384, 3, 3, 1, 1, 1), "branch3x3dbl_3a": (384, 384, 1, 3, 1, 0, 1),
            "branch3x3dbl_3b": (384, 384, 3, 1, 1, 1, 0), "branch_pool": (cin, 192, 1, 1, 1, 0, 0)}


def conv_specs():
    """every convolution of the graph, in state-dict order: name -> (Cin, Cout, kh, kw, stride, ph, pw)"""
    out = {"Conv2d_1a_3x3": (3, 32, 3, 3, 2, 0, 0), "Conv2d_2a_3x3": (32, 32, 3, 3, 1, 0, 0), "Conv2d_2b_3x3": (32, 64, 3, 3, 1, 1, 1),
           "Conv2d_3b_1x1": (64, 80, 1, 1, 1, 0, 0), "Conv2d_4a_3x3": (80, 192, 3, 3, 1, 0, 0)}
    for name, kind, cin, p in BLOCKS:
        for suffix, spec in _block_convs(kind, cin, p).items():
            out[f"{name}.{suffix}"] = spec
    return out


def block_out_channels(kind, cin, p):
    """channels of a Mixed block's concatenation"""
    convs = _block_convs(kind, cin, p)
    total = 0
    for branch in BRANCHES[kind]:
        last = branch[-1]
        total += cin if last == "maxs2" else sum(convs[s][1] for s in (last if isinstance(last, tuple) else (last,)))
    return total


def expected_shapes():
    """canonical key -> shape: <name>.conv.weight and <name>.bn.{weight,bias,running_mean,running_var}"""
    out = {}
    for name, (cin, cout, kh, kw, _, _, _) in conv_specs().items():
        out[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{name}.bn.{k}"] = (cout,)
    return out


def load_weights(paths):
    """one or more torch.load-able state dicts (paths, or dicts already loaded) -> the canonical fp32 state dict of expected_shapes().
    The keys are those of torchvision's inception_v3 and of pytorch-fid's pt_inception file (the same spelling); a "state_dict"
    nesting is unwrapped; fc.*, AuxLogits.*, num_batches_tracked and keys of anything else are ignored.  Later files win.  Every shape
    is checked; a missing key is named in the error."""
    if isinstance(paths, (str, bytes, dict)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    want = expected_shapes()
    out = {}
    for p in paths:
        sd = p if isinstance(p, dict) else torch.load(p, map_location="cpu", weights_only=True)
        sd = sd.get("state_dict", sd)
        for key, v in sd.items():
            if key not in want:
                continue
            if tuple(v.shape) != want[key]:
                raise ValueError(f"FID Inception weights: {key} has shape {tuple(v.shape)}, expected {want[key]}")
            out[key] = v.detach().to(torch.float32).contiguous()
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError(f"FID Inception weights: missing {', '.join(missing)}")
    return {k: out[k] for k in want}


def synth_weights(seed, path=None):
    """synthetic weights of the production architecture (the tests): convolutions He-normal with std = sqrt(2 / (kh kw Cin)), bn.weight
    uniform in [0.8, 1.2], bn.bias uniform in [0, 0.1], running_mean normal with standard deviation 0.1, running_var uniform in
    [0.5, 1.5].  -> the canonical state dict; `path` also writes it as a state dict file."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, (cin, cout, kh, kw, _, _, _) in conv_specs().items():
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (kh * kw * cin))
        sd[f"{name}.bn.weight"] = 0.8 + 0.4 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.1 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(cout, generator=g)
    if path is not None:
        torch.save(sd, path)
    return sd


def fold_bn(sd, name):
    """the inference BatchNorm (eps = 1e-3) of convolution `name` folded into it, in fp64, rounded to fp32 -> (weight (Cout, Cin, kh,
    kw), bias (Cout,))"""
    w = sd[f"{name}.conv.weight"].to(torch.float64)
    scale = sd[f"{name}.bn.weight"].to(torch.float64) / torch.sqrt(sd[f"{name}.bn.running_var"].to(torch.float64) + BN_EPS)
    bias = sd[f"{name}.bn.bias"].to(torch.float64) - sd[f"{name}.bn.running_mean"].to(torch.float64) * scale
    return (w * scale[:, None, None, None]).to(torch.float32), bias.to(torch.float32)


def patch_grid(H, W, P):
    """the windows (y0, x0, h, w) of an H x W image under the HiFiC protocol: the P x P windows at (i P, j P) that fit, then those at
    (P / 2 + i P, P / 2 + j P) that fit; P = 0: the whole image as one window; an image smaller than P in either dimension: none"""
    if P == 0:
        return [(0, 0, H, W)]
    out = [(y, x, P, P) for y in range(0, H - P + 1, P) for x in range(0, W - P + 1, P)]
    out += [(y, x, P, P) for y in range(P // 2, H - P + 1, P) for x in range(P // 2, W - P + 1, P)]
    return out


def descriptors(n_images, H, W, P):
    """(n_images * windows, 5) int32 rows (image, y0, x0, h, w): patch_grid(H, W, P) of every image, image-major"""
    g = patch_grid(H, W, P)
    return np.array([(b,) + w for b in range(n_images) for w in g], dtype=np.int32).reshape(-1, 5)


class InceptionFID:
    """weights: load_weights' / synth_weights' dict, or path(s) for load_weights.  Every BatchNorm is folded once (fold_bn); the
    weights are reordered to (Cout, (ky, kx, cin)), zero-padded to whole 32-column slices, and split into planes on first use."""

    def __init__(self, weights, device):
        sd = load_weights(weights)
        self.device = torch.device(device)
        self.conv = {}
        for name, (cin, cout, kh, kw, st, ph, pw) in conv_specs().items():
            w, b = fold_bn(sd, name)
            w = w.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin)
            if w.shape[1] % 32:
                w = torch.cat([w, torch.zeros(cout, 32 - w.shape[1] % 32)], dim=1)
            self.conv[name] = (w.contiguous().to(self.device), b.contiguous().to(self.device), (cin, cout, kh, kw, st, ph, pw))
        self.max_operand_bytes = MAX_OPERAND_BYTES
        self.trace = None          # a list (tests / debugging): every convolution appends (name, y (rows, Cout) before the ReLU, OH, OW)

    def _conv(self, name, x, cols, n, H, W, out=None, planes=None):
        """convolution `name` on columns `cols` of x (n*H*W, ld) (before its ReLU; `planes`: its operand when already written) ->
        (y (n*OH*OW, Cout) before its ReLU, written into `out` when given, OH, OW)"""
        from . import ops
        wt, bias, (cin, cout, kh, kw, st, ph, pw) = self.conv[name]
        assert cols[1] == cin, (name, cols)
        if planes is None:
            planes = ops.patches_split3(x, n, H, W, kh, kw, st, st, ph, pw, relu=name != "Conv2d_1a_3x3", cols=cols)
        y = ops.gemm(planes, wt, bias, out=out, precision="split3")
        OH, OW = ops.conv_out(H, kh, st, ph), ops.conv_out(W, kw, st, pw)
        if self.trace is not None:
            self.trace.append((name, y, OH, OW))
        return y, OH, OW

    def _block(self, name, kind, cin, p, x, n, H, W):
        """one Mixed block on x (n*H*W, cin) -> (its concatenation (n*OH*OW, Cout) before the ReLUs, OH, OW)"""
        from . import ops
        stride2 = kind in ("B", "D")
        OH, OW = (ops.conv_out(H, 3, 2, 0), ops.conv_out(W, 3, 2, 0)) if stride2 else (H, W)
        out = torch.empty(n * OH * OW, block_out_channels(kind, cin, p), dtype=torch.float32, device=self.device)
        first = None                     # relu + pack of the block's input: the operand of every 1x1 convolution that reads it
        col = 0
        for branch in BRANCHES[kind]:
            cur, cols, h, w = x, (0, cin), H, W
            for i, op in enumerate(branch):
                last = i == len(branch) - 1
                if op == "maxs2":
                    ops.relu_maxpool3s2(cur, n, h, w, out=out, col0=col)
                    col += cin
                elif op in ("avg", "max", "pool"):
                    pool = p if op == "pool" else op
                    cur = (ops.relu_avgpool3s1p1 if pool == "avg" else ops.relu_maxpool3s1p1)(cur, n, h, w)
                else:
                    for s in (op if isinstance(op, tuple) else (op,)):
                        cname = f"{name}.{s}"
                        cout = self.conv[cname][2][1]
                        planes = None
                        if cur is x and self.conv[cname][2][2:] == (1, 1, 1, 0, 0):
                            if first is None:
                                first = ops.patches_split3(x, n, H, W, 1, 1)
                            planes = first
                        y, h2, w2 = self._conv(cname, cur, cols, n, h, w, out=out[:, col:col + cout] if last else None, planes=planes)
                        if last:
                            col += cout
                    if not last:
                        cur, cols, h, w = y, (0, cout), h2, w2
        assert col == out.shape[1], (name, col, out.shape)
        return out, OH, OW

    def _chunk(self, canvas, desc):
        from . import ops
        n = desc.shape[0]
        x = ops.fid_resize299(canvas, desc).view(n * SIDE * SIDE, 3)
        H = W = SIDE
        c = 3
        for op in TRUNK:
            if op == "maxs2":
                x, H, W = ops.relu_maxpool3s2(x, n, H, W), ops.conv_out(H, 3, 2, 0), ops.conv_out(W, 3, 2, 0)
            else:
                x, H, W = self._conv(op, x, (0, c), n, H, W)
                c = x.shape[1]
        for name, kind, cin, p in BLOCKS:
            x, H, W = self._block(name, kind, cin, p, x, n, H, W)
        return ops.relu_mean_rows(x, n, H * W)

    def features(self, canvas_u8, descriptors=None):
        """canvas_u8 (B, H, W, 3) u8 on the device; descriptors (n, 5) int32 rows (image, y0, x0, h, w), default: every image whole ->
        (n, 2048) fp32 on the device: pool3 of every window.  The windows run in chunks whose largest patch operand (Conv2d_2b_3x3's,
        37 MB per window) stays under max_operand_bytes = 2^30 (at least one window), so memory does not grow with n.  A window's
        result depends neither on the chunking nor on its slot.  No synchronisation."""
        assert canvas_u8.dtype == torch.uint8 and canvas_u8.is_cuda and canvas_u8.dim() == 4 and canvas_u8.shape[3] == 3
        canvas_u8 = canvas_u8.contiguous()
        B, H, W, _ = canvas_u8.shape
        if descriptors is None:
            descriptors = np.array([(b, 0, 0, H, W) for b in range(B)], dtype=np.int32)
        desc = np.ascontiguousarray(descriptors, dtype=np.int32).reshape(-1, 5)
        n = desc.shape[0]
        out = torch.empty(n, DIM, dtype=torch.float32, device=self.device)
        step = max(1, int(self.max_operand_bytes) // OPERAND_BYTES_PER_IMAGE)
        for s in range(0, n, step):
            out[s:s + step] = self._chunk(canvas_u8, desc[s:s + step])
        return out


# ---- statistics.  Host arrays (numpy) take numpy's fp64 products: the statement of the definition, used by the CPU tests and for
# sets that are already on the host.  Device tensors take ops.gram_f64; there is no other path for them.

def _gram(a, b, ia=None, ib=None):
    """sum_k a[ia[i]][k] b[ib[j]][k] in fp64 -> numpy for numpy inputs, a device tensor for device tensors"""
    if isinstance(a, np.ndarray):
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        return (a64 if ia is None else a64[ia]) @ (b64 if ib is None else b64[ib]).T
    from . import ops
    dev = a.device
    to = lambda ix: None if ix is None else torch.from_numpy(np.ascontiguousarray(ix, dtype=np.int32)).to(dev)
    return ops.gram_f64(a, b, to(ia), to(ib))


def moments(X):
    """X (n, d) fp32, a device tensor or a numpy array -> (n, mu (d,), cov (d, d)) in numpy fp64, ddof = 1: from the fp64 column sums
    s and second moments S = X^T X (on the device: ops.gram_f64 on the transposed matrix, the sums against a row of ones) as
    (S - s s^T / n) / (n - 1)"""
    n, d = X.shape
    if n < 2:
        raise ValueError("mean and covariance need at least two samples")
    if isinstance(X, np.ndarray):
        xt = np.ascontiguousarray(X.T, dtype=np.float32)
        ones = np.ones((1, n), dtype=np.float32)
        S, s = _gram(xt, xt), _gram(ones, xt)[0]
    else:
        xt = X.to(torch.float32).t().contiguous()
        ones = torch.ones(1, n, dtype=torch.float32, device=X.device)
        S, s = _gram(xt, xt).cpu().numpy(), _gram(ones, xt)[0].cpu().numpy()
    mu = s / n
    return n, mu, (S - np.outer(s, s) / n) / (n - 1)


class FeatureStats:
    """the features of one set of images, accumulated block by block on the device"""

    def __init__(self):
        self.blocks = []

    def add(self, feats):
        assert feats.dim() == 2 and feats.dtype == torch.float32
        self.blocks.append(feats)

    @property
    def n(self):
        return sum(b.shape[0] for b in self.blocks)

    def features(self):
        """(n, d) fp32 on the device, in the order added"""
        return self.blocks[0] if len(self.blocks) == 1 else torch.cat(self.blocks, dim=0)

    def moments(self):
        return moments(self.features())


def fid_from_stats(mu_x, cov_x, mu_y, cov_y):
    """|mu_x - mu_y|^2 + tr cov_x + tr cov_y - 2 sum_i sqrt(max(lambda_i, 0)), lambda the eigenvalues of cov_x^1/2 cov_y cov_x^1/2: two
    symmetric eigen-decompositions in numpy fp64 (lambda_i <= d eps lambda_max counts as 0).  Equal to tr sqrtm(cov_x cov_y) where that
    is defined; needs no eps offset for rank-deficient covariances."""
    mu_x, mu_y = np.asarray(mu_x, dtype=np.float64), np.asarray(mu_y, dtype=np.float64)
    cov_x, cov_y = np.asarray(cov_x, dtype=np.float64), np.asarray(cov_y, dtype=np.float64)
    lam, V = np.linalg.eigh((cov_x + cov_x.T) * 0.5)
    root = (V * np.sqrt(np.maximum(lam, 0.0))) @ V.T
    M = root @ ((cov_y + cov_y.T) * 0.5) @ root
    ev = np.linalg.eigvalsh((M + M.T) * 0.5)
    # an eigenvalue below the solver's own resolution d eps lambda_max is a zero of a rank-deficient product that came out as noise of
    # either sign; its square root would be sqrt(eps) large, so it counts as the 0 it stands for (the cut of numpy's matrix_rank)
    ev = np.where(ev > ev.max() * len(ev) * np.finfo(np.float64).eps, ev, 0.0) if len(ev) and ev.max() > 0 else np.zeros_like(ev)
    diff = mu_x - mu_y
    return float(diff @ diff + np.trace(cov_x) + np.trace(cov_y) - 2.0 * np.sqrt(ev).sum())


def fid(X, Y):
    """X (n, d), Y (m, d) fp32 feature sets (device tensors or numpy arrays) -> the Frechet distance of their Gaussians (float).  With
    fewer samples than dimensions the covariances are rank-deficient and the number is biased (it is still defined)."""
    _, mx, cx = moments(X)
    _, my, cy = moments(Y)
    return fid_from_stats(mx, cx, my, cy)


def kid_indices(n, m, subsets=100, subset_size=1000, seed=0):
    """the subsets of KID: for every subset s = min(subset_size, n, m) rows of X, then s rows of Y, each drawn without replacement from
    numpy.random.default_rng(seed) -> list of (ix, iy) int64 arrays"""
    s = min(int(subset_size), n, m)
    rng = np.random.default_rng(seed)
    return [(rng.choice(n, s, replace=False), rng.choice(m, s, replace=False)) for _ in range(int(subsets))]


def kid(X, Y, subsets=100, subset_size=1000, seed=0):
    """kernel inception distance with k(a, b) = (a.b / d + 1)^3: the mean and the standard deviation (ddof = 0) over kid_indices'
    subsets of the unbiased estimate (sum K_XX - tr K_XX) / (s (s-1)) + (sum K_YY - tr K_YY) / (s (s-1)) - 2 sum K_XY / s^2 ->
    (kid, kid_std), (None, None) when s < 2.  Device tensors: the Gram matrices are ops.gram_f64 over the gathered rows, the cubes
    and sums fp64 on the device, one read-back."""
    n, m, d = X.shape[0], Y.shape[0], X.shape[1]
    s = min(int(subset_size), n, m)
    if s < 2:
        return None, None
    host = isinstance(X, np.ndarray)
    terms = []
    for ix, iy in kid_indices(n, m, subsets, subset_size, seed):
        t = []
        for a, b, ia, ib in ((X, X, ix, ix), (Y, Y, iy, iy), (X, Y, ix, iy)):
            K = (_gram(a, b, ia, ib) / d + 1.0) ** 3
            t += [K.sum(), np.trace(K) if host else torch.trace(K)]
        terms.append(np.array(t, dtype=np.float64) if host else torch.stack(t))
    T = np.stack(terms) if host else torch.stack(terms).cpu().numpy()
    est = (T[:, 0] - T[:, 1]) / (s * (s - 1)) + (T[:, 2] - T[:, 3]) / (s * (s - 1)) - 2.0 * T[:, 4] / (s * s)
    return float(est.mean()), float(est.std())
