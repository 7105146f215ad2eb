"""An fp64 numpy restatement of the three luma measures of evaluate.py --hvs, written from their definitions,
not from the kernels: VIFp with whole N x N windows, GMSD with explicit zero padding and a two-pass standard deviation, PSNR-HVS
and PSNR-HVS-M with matrix DCTs block by block.  Plain loops over window taps and blocks; no optional package."""
import numpy as np

Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                   72, 92, 95, 98, 112, 100, 103, 99], dtype=np.float64).reshape(8, 8)       # T.81 Annex K.1, luminance
MASKCOF = (10.0 / Q_LUMA) ** 2
CSFCOF = 2.5735088 * (10.0 / Q_LUMA)
VIFP_MIN_SIDE = 41
EPS = 1e-10


def luma(img_u8):
    """(..., 3) u8 -> fp64 Y on the 0..255 scale, unrounded"""
    x = np.asarray(img_u8).astype(np.float64)
    return 0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]


# ------------------------------------------------------------------------------------------------------------------ VIFp

def gauss_window(N):
    """the N x N Gaussian of sigma N / 5, normalised to sum 1"""
    d = np.arange(N, dtype=np.float64) - (N // 2)
    w = np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * (N / 5.0) ** 2))
    return w / w.sum()


def filter_valid(x, w):
    """the correlation of x with the window over its 'valid' support (the window is symmetric: a convolution alike)"""
    N = w.shape[0]
    h, wd = x.shape[0] - N + 1, x.shape[1] - N + 1
    out = np.zeros((h, wd))
    for u in range(N):
        for v in range(N):
            out += w[u, v] * x[u:u + h, v:v + wd]
    return out


def vifp_sums(ya, yb):
    """-> (num, den) over the four scales; ValueError below the smallest size"""
    if min(ya.shape) < VIFP_MIN_SIDE:
        raise ValueError(f"VIFp needs both sides >= {VIFP_MIN_SIDE}")
    x, y = ya, yb
    num = den = 0.0
    for s in range(1, 5):
        w = gauss_window(2 ** (4 - s + 1) + 1)
        if s > 1:
            x, y = filter_valid(x, w)[::2, ::2], filter_valid(y, w)[::2, ::2]
        mu1, mu2 = filter_valid(x, w), filter_valid(y, w)
        s1 = filter_valid(x * x, w) - mu1 * mu1
        s2 = filter_valid(y * y, w) - mu2 * mu2
        s12 = filter_valid(x * y, w) - mu1 * mu2
        s1[s1 < 0] = 0.0
        s2[s2 < 0] = 0.0
        g = s12 / (s1 + EPS)
        sv = s2 - g * s12
        k = s1 < EPS
        g[k] = 0.0
        sv[k] = s2[k]
        s1[k] = 0.0
        k = s2 < EPS
        g[k] = 0.0
        sv[k] = 0.0
        k = g < 0
        sv[k] = s2[k]
        g[k] = 0.0
        sv[sv <= EPS] = EPS
        num += float(np.log10(1.0 + g * g * s1 / (sv + 2.0)).sum())
        den += float(np.log10(1.0 + s1 / 2.0).sum())
    return num, den


def vifp(ya, yb):
    num, den = vifp_sums(ya, yb)
    if den == 0.0:      # a flat original
        return 1.0 if np.array_equal(ya, yb) else 0.0
    return num / den


# ------------------------------------------------------------------------------------------------------------------ GMSD

def conv_same_zero(x, k):
    """MATLAB's conv2(x, k, 'same'): the true convolution with zeros outside x, the central part of the full result"""
    kh, kw = k.shape
    H, W = x.shape
    full = np.zeros((H + kh - 1, W + kw - 1))
    for p in range(kh):
        for q in range(kw):
            full[p:p + H, q:q + W] += k[p, q] * x
    r0, c0 = (kh - 1 + 1) // 2, (kw - 1 + 1) // 2       # ceil((k - 1) / 2)
    return full[r0:r0 + H, c0:c0 + W]


def gms_map(ya, yb):
    ave = np.full((2, 2), 0.25)
    hx = np.array([[1.0, 0.0, -1.0]] * 3) / 3.0
    hy = hx.T
    a, b = conv_same_zero(ya, ave)[::2, ::2], conv_same_zero(yb, ave)[::2, ::2]
    m1 = np.sqrt(conv_same_zero(a, hx) ** 2 + conv_same_zero(a, hy) ** 2)
    m2 = np.sqrt(conv_same_zero(b, hx) ** 2 + conv_same_zero(b, hy) ** 2)
    return (2.0 * m1 * m2 + 170.0) / (m1 * m1 + m2 * m2 + 170.0)


def gmsd(ya, yb):
    g = gms_map(ya, yb)
    return float(np.sqrt(np.mean((g - g.mean()) ** 2)))       # two passes


# ------------------------------------------------------------------------------------------------------------------ PSNR-HVS

def dct_matrix():
    k = np.arange(8, dtype=np.float64)
    C = np.cos((2.0 * k[None, :] + 1.0) * k[:, None] * np.pi / 16.0) * 0.5
    C[0] = np.sqrt(0.125)
    return C


def vari(X):
    return float(np.var(X, ddof=1) * X.size)


def block_mask(B, D):
    ac = D * D * MASKCOF
    m = float(ac.sum() - ac[0, 0])
    pop = vari(B)
    if pop != 0.0:
        pop = (vari(B[:4, :4]) + vari(B[:4, 4:]) + vari(B[4:, :4]) + vari(B[4:, 4:])) / pop
    return np.sqrt(m * pop) / 32.0


def block_errors(Ba, Bb):
    """one 8 x 8 block pair -> (the error without masking, with masking)"""
    C = dct_matrix()
    Da, Db = C @ Ba @ C.T, C @ Bb @ C.T
    mask = max(block_mask(Ba, Da), block_mask(Bb, Db))
    u = np.abs(Da - Db)
    thr = mask / MASKCOF
    um = np.where(u < thr, 0.0, u - thr)
    um[0, 0] = u[0, 0]
    return float(((u * CSFCOF) ** 2).sum()), float(((um * CSFCOF) ** 2).sum())


def psnr_hvs(ya, yb):
    """-> (PSNR-HVS, PSNR-HVS-M); inf for MSE = 0; ValueError below 8 x 8"""
    H, W = ya.shape
    if min(H, W) < 8:
        raise ValueError("PSNR-HVS needs both sides >= 8")
    tot = np.zeros(2)
    for i in range(0, H - 7, 8):
        for j in range(0, W - 7, 8):
            tot += block_errors(ya[i:i + 8, j:j + 8], yb[i:i + 8, j:j + 8])
    mse = tot / ((H // 8) * (W // 8) * 64.0)
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(65025.0 / mse)
    return float(db[0]), float(db[1])


def measure(a_u8, b_u8):
    """one (H, W, 3) u8 pair -> the four values; None where the image is too small"""
    ya, yb = luma(a_u8), luma(b_u8)
    side = min(ya.shape)
    hvs, hvs_m = psnr_hvs(ya, yb) if side >= 8 else (None, None)
    return {"vifp": vifp(ya, yb) if side >= VIFP_MIN_SIDE else None, "gmsd": gmsd(ya, yb), "psnr_hvs": hvs, "psnr_hvs_m": hvs_m}


# ------------------------------------------------------------------------------------------------------------------ cases

def smooth(H, W, seed):
    """a smooth colour gradient with a slow wave, (H, W, 3) u8"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.stack([40.0 + 170.0 * (rng.uniform(0.2, 1.0) * x / W + rng.uniform(0.2, 1.0) * y / H) / 2.0
                    + 20.0 * np.sin(rng.uniform(0.05, 0.3) * x + rng.uniform(0.05, 0.3) * y + c) for c in range(3)], axis=-1)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def blur(a):
    """the 3 x 3 mean (edges replicated), rounded"""
    p = np.pad(a.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = a.shape[:2]
    return ((sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) + 4) // 9).astype(np.uint8)


def make_pair(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":           # seeded random u8, the original plus noise
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    elif kind == "blur":          # a smooth gradient and its blur
        a = smooth(H, W, seed)
        b = blur(a)
    elif kind == "identical":
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        b = a.copy()
    elif kind == "flat":          # two different constant images
        a, b = np.full((H, W, 3), 90, np.uint8), np.full((H, W, 3), 140, np.uint8)
    elif kind == "flat_equal":
        a = np.full((H, W, 3), 90, np.uint8)
        b = a.copy()
    elif kind == "offset":        # the original plus 3 in every channel, nowhere clipped
        a = rng.integers(0, 253, (H, W, 3), dtype=np.uint8)
        b = a + np.uint8(3)
    else:
        raise ValueError(kind)
    return a, b


_CASES = {}


def case(kind, H, W):
    """-> (a, b, measure(a, b)) of one pair, computed once and shared.  Read-only."""
    key = (kind, H, W)
    if key not in _CASES:
        a, b = make_pair(kind, H, W, 7 * H + W)
        a.setflags(write=False)
        b.setflags(write=False)
        _CASES[key] = (a, b, measure(a, b))
    return _CASES[key]
