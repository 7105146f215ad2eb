"""An fp64 numpy restatement of FSIM and FSIMc as DESIGN.md section 21 defines them (Zhang et al.'s FeatureSIM.m with its embedded
phasecong2), written from that text and not from the kernels: np.fft for the transforms, plain loops over the taps of the 'same'
filters, np.median for the noise threshold, the sums S2 and Sij from the spatial filters.  No optional package."""
import numpy as np

MIN_SIDE = 2
MAX_REDUCED_SIDE = 2048
NSCALE, NORIENT = 4, 4
MIN_WAVELENGTH, MULT, SIGMA_ONF = 6.0, 2.0, 0.55
SIGMA_THETA = np.pi / NORIENT / 1.2
K_NOISE, EPSILON = 2.0, 1e-4
T1, T2, T3, T4, LAMBDA = 0.85, 160.0, 200.0, 200.0, 0.03


# ------------------------------------------------------------------------------------------------------------------ planes

def yiq(img_u8):
    """(..., 3) u8 -> (Y, I, Q), fp64, unrounded, one multiply or add per written operation"""
    x = np.asarray(img_u8).astype(np.float64)
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    return (0.299 * R + 0.587 * G) + 0.114 * B, (0.596 * R - 0.274 * G) - 0.322 * B, (0.211 * R - 0.523 * G) + 0.312 * B


def reduction(H, W):
    """-> (F, h, w): F = max(1, round(min(H, W) / 256)) with MATLAB's round; the reduced plane keeps rows and columns 0, F, 2F, .."""
    F = max(1, int(np.floor(min(H, W) / 256.0 + 0.5)))
    return F, -(-H // F), -(-W // F)


def mean_same(x, F):
    """the F x F mean over 'same' support with zero padding, anchored as conv2(x, ones(F) / F^2, 'same'): output sample i along an
    axis covers the inputs i + F // 2 - F + 1 .. i + F // 2.  The taps are added row by row from the lowest offset, then divided."""
    H, W = x.shape
    lo = F // 2 - F + 1
    p = np.zeros((H + 2 * F, W + 2 * F))
    p[F:F + H, F:F + W] = x
    acc = np.zeros((H, W))
    for u in range(lo, lo + F):
        for v in range(lo, lo + F):
            acc = acc + p[F + u:F + u + H, F + v:F + v + W]
    return acc / float(F * F)


def reduce_plane(x, F):
    return np.ascontiguousarray(mean_same(x, F)[::F, ::F])


def reduced_planes(img_u8):
    """(H, W, 3) u8 -> the reduced (Y, I, Q) planes"""
    F = reduction(*np.asarray(img_u8).shape[:2])[0]
    return tuple(reduce_plane(p, F) for p in yiq(img_u8))


# ------------------------------------------------------------------------------------------------------------------ filters

def axis_coords(n):
    k = np.arange(n, dtype=np.float64)
    return (k - n / 2.0) / n if n % 2 == 0 else (k - (n - 1) / 2.0) / (n - 1)


def filter_bank(h, w):
    """-> (logGabor (4, h, w), spread (4, h, w)), both already ifftshifted; filter_{s,o} = logGabor[s] * spread[o]"""
    x, y = np.meshgrid(axis_coords(w), axis_coords(h))
    radius = np.fft.ifftshift(np.sqrt(x * x + y * y))
    theta = np.fft.ifftshift(np.arctan2(-y, x))
    lp = 1.0 / (1.0 + (radius / 0.45) ** 30)
    radius[0, 0] = 1.0
    lg = np.zeros((NSCALE, h, w))
    for s in range(NSCALE):
        fo = 1.0 / (MIN_WAVELENGTH * MULT ** s)
        lg[s] = np.exp(-(np.log(radius / fo)) ** 2 / (2.0 * np.log(SIGMA_ONF) ** 2)) * lp
        lg[s][0, 0] = 0.0
    sintheta, costheta = np.sin(theta), np.cos(theta)
    spread = np.zeros((NORIENT, h, w))
    for o in range(NORIENT):
        angl = o * np.pi / NORIENT
        ds = sintheta * np.cos(angl) - costheta * np.sin(angl)
        dc = costheta * np.cos(angl) + sintheta * np.sin(angl)
        spread[o] = np.exp(-np.arctan2(ds, dc) ** 2 / (2.0 * SIGMA_THETA ** 2))
    return lg, spread


def spatial_sums(lg, spread_o):
    """-> (S2, Sij) of one orientation from g_s = Re(ifft2(filter_{s,o})) sqrt(h w)"""
    h, w = spread_o.shape
    g = [np.real(np.fft.ifft2(lg[s] * spread_o)) * np.sqrt(float(h * w)) for s in range(NSCALE)]
    S2 = sum(float(np.sum(g[s] ** 2)) for s in range(NSCALE))
    Sij = sum(float(np.sum(g[s] * g[t])) for s in range(NSCALE) for t in range(s + 1, NSCALE))
    return S2, Sij


def parseval_sums(lg, spread_o):
    """the same two sums in the frequency domain, from the Hermitian-symmetrised filters Fh[k] = (F[k] + F[-k]) / 2"""
    Fh = []
    for s in range(NSCALE):
        F = lg[s] * spread_o
        Fh.append(0.5 * (F + np.roll(F[::-1, ::-1], (1, 1), axis=(0, 1))))
    S2 = sum(float(np.sum(Fh[s] ** 2)) for s in range(NSCALE))
    Sij = sum(float(np.sum(Fh[s] * Fh[t])) for s in range(NSCALE) for t in range(s + 1, NSCALE))
    return S2, Sij


# ------------------------------------------------------------------------------------------------------------------ phase congruency

def phase_congruency(P):
    """(h, w) fp64 -> the PC map; a flat plane gives 0 everywhere without a transform"""
    P = np.asarray(P, dtype=np.float64)
    h, w = P.shape
    if min(h, w) < MIN_SIDE:
        raise ValueError(f"FSIM needs both sides >= {MIN_SIDE}")
    if P.max() == P.min():
        return np.zeros((h, w))
    lg, spread = filter_bank(h, w)
    X = np.fft.fft2(P)
    energy_all, an_all = np.zeros((h, w)), np.zeros((h, w))
    for o in range(NORIENT):
        EO = [np.fft.ifft2(X * (lg[s] * spread[o])) for s in range(NSCALE)]
        sumE = sum(np.real(e) for e in EO)
        sumO = sum(np.imag(e) for e in EO)
        sumA = sum(np.abs(e) for e in EO)
        XE = np.sqrt(sumE ** 2 + sumO ** 2) + EPSILON
        mE, mO = sumE / XE, sumO / XE
        energy = np.zeros((h, w))
        for e in EO:
            energy = energy + (np.real(e) * mE + np.imag(e) * mO - np.abs(np.real(e) * mO - np.imag(e) * mE))
        med = float(np.median(np.abs(EO[0]) ** 2))
        noise_power = (-med / np.log(0.5)) / float(np.sum((lg[0] * spread[o]) ** 2))
        S2, Sij = spatial_sums(lg, spread[o])
        tau = np.sqrt((2.0 * noise_power * S2 + 4.0 * noise_power * Sij) / 2.0)
        T = (tau * np.sqrt(np.pi / 2.0) + K_NOISE * np.sqrt((2.0 - np.pi / 2.0) * tau ** 2)) / 1.7
        energy_all += np.maximum(energy - T, 0.0)
        an_all += sumA
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(an_all == 0.0, 0.0, energy_all / an_all)


# ------------------------------------------------------------------------------------------------------------------ pooling

def corr_same_zero(x, k):
    """sum_{p,q} k[p, q] x[i + p - 1, j + q - 1] for a 3 x 3 k, zeros outside x.  (conv2's 'same' is this with k flipped; for the
    antisymmetric Scharr kernels that only changes the sign, which the magnitude drops.)"""
    H, W = x.shape
    p = np.zeros((H + 2, W + 2))
    p[1:H + 1, 1:W + 1] = x
    out = np.zeros((H, W))
    for u in range(3):
        for v in range(3):
            if k[u, v] != 0.0:
                out = out + k[u, v] * p[u:u + H, v:v + W]
    return out


SCHARR_X = np.array([[3.0, 0.0, -3.0], [10.0, 0.0, -10.0], [3.0, 0.0, -3.0]]) / 16.0


def gradient_magnitude(Y):
    return np.sqrt(corr_same_zero(Y, SCHARR_X) ** 2 + corr_same_zero(Y, SCHARR_X.T) ** 2)


def chroma_term(I1, I2, Q1, Q2):
    """C = real((Si Sq)^0.03): |c|^0.03, times cos(0.03 pi) where c < 0"""
    Si = (2.0 * I1 * I2 + T3) / (I1 * I1 + I2 * I2 + T3)
    Sq = (2.0 * Q1 * Q2 + T4) / (Q1 * Q1 + Q2 * Q2 + T4)
    c = Si * Sq
    return np.where(c < 0.0, np.abs(c) ** LAMBDA * np.cos(LAMBDA * np.pi), np.abs(c) ** LAMBDA)


def pool(planes1, planes2, PC1, PC2):
    """the reduced (Y, I, Q) planes of both images and their PC maps -> (FSIM, FSIMc)"""
    Y1, I1, Q1 = planes1
    Y2, I2, Q2 = planes2
    G1, G2 = gradient_magnitude(Y1), gradient_magnitude(Y2)
    Spc = (2.0 * PC1 * PC2 + T1) / (PC1 * PC1 + PC2 * PC2 + T1)
    Sg = (2.0 * G1 * G2 + T2) / (G1 * G1 + G2 * G2 + T2)
    PCm = np.maximum(PC1, PC2)
    den = float(np.sum(PCm))
    if den == 0.0:
        same = all(np.array_equal(a, b) for a, b in zip(planes1, planes2))
        return (1.0, 1.0) if same else (0.0, 0.0)
    sl = Spc * Sg * PCm
    return float(np.sum(sl)) / den, float(np.sum(sl * chroma_term(I1, I2, Q1, Q2))) / den


def fsim(a_u8, b_u8):
    """one (H, W, 3) u8 pair -> (FSIM, FSIMc); ValueError outside the limits"""
    a_u8, b_u8 = np.asarray(a_u8), np.asarray(b_u8)
    H, W = a_u8.shape[:2]
    if min(H, W) < MIN_SIDE:
        raise ValueError(f"FSIM needs both sides >= {MIN_SIDE}, got {H} x {W}")
    _, h, w = reduction(H, W)
    if max(h, w) > MAX_REDUCED_SIDE:
        raise ValueError(f"FSIM needs the reduced longer side <= {MAX_REDUCED_SIDE}, got {h} x {w}")
    p1, p2 = reduced_planes(a_u8), reduced_planes(b_u8)
    return pool(p1, p2, phase_congruency(p1[0]), phase_congruency(p2[0]))


# ------------------------------------------------------------------------------------------------------------------ cases

def blur(a):
    """the 3 x 3 mean (edges replicated), rounded"""
    p = np.pad(a.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = a.shape[:2]
    return ((sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) + 4) // 9).astype(np.uint8)


def make_pair(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":           # seeded random u8 and the same plus noise
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    elif kind == "step":          # a smooth colour field with a vertical step, and the same plus Gaussian noise of sigma 6
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        f = np.stack([60.0 + 50.0 * x / W + 40.0 * y / H + 15.0 * np.sin(0.21 * x + 0.13 * y + c) + 70.0 * (x >= W // 2) * (1 - 0.3 * c)
                      for c in range(3)], axis=-1)
        a = np.clip(np.rint(f), 0, 255).astype(np.uint8)
        b = np.clip(np.rint(f + rng.normal(0.0, 6.0, f.shape)), 0, 255).astype(np.uint8)
    elif kind == "blur":          # seeded smooth-ish texture and its 3 x 3 blur
        base = rng.integers(0, 256, ((H + 3) // 4, (W + 3) // 4, 3), dtype=np.uint8)
        a = np.repeat(np.repeat(base, 4, axis=0), 4, axis=1)[:H, :W]
        a = blur(np.ascontiguousarray(a))
        b = blur(a)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


_CASES = {}


def case(kind, H, W):
    """-> (a, b, {"planes_a", "planes_b", "pc_a", "pc_b", "fsim", "fsimc"}) of one pair, computed once and shared.  Read-only."""
    key = (kind, H, W)
    if key not in _CASES:
        a, b = make_pair(kind, H, W, 11 * H + W)
        pa, pb = reduced_planes(a), reduced_planes(b)
        pca, pcb = phase_congruency(pa[0]), phase_congruency(pb[0])
        f, fc = pool(pa, pb, pca, pcb)
        for arr in (a, b, pca, pcb) + pa + pb:
            arr.setflags(write=False)
        _CASES[key] = (a, b, {"planes_a": pa, "planes_b": pb, "pc_a": pca, "pc_b": pcb, "fsim": f, "fsimc": fc})
    return _CASES[key]
