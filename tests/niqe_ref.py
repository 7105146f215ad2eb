"""CPU restatement of sgic_niqe_u8 / niqe.Niqe in numpy fp64: the integer luma, the integer half-size plane, the
MSCN map from integer class sums, the block sums of the five maps, and the score.  From the product it takes only the ten window
weights (niqe.window_weights) and the AGGD fit (niqe.features), as quality_ref takes quality.combine.  Also the images, the synthetic
pristine model and the tolerances the tests share."""
import math

import numpy as np

BLOCK = 96
TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.int64)      # imresize(., 0.5): bicubic, antialiased, over 256
SHIFTS = [(0, 1), (1, 0), (1, 1), (1, -1)]
REL = 2e-12          # what the device's block sums may differ by (relative): sums of <= 9216 non-negative fp64 terms


def luma(img):
    """(..., 3) u8 -> int64: 16 + round_half_even((65481 R + 128553 G + 24966 B) / 255000), in integers"""
    v = img.astype(np.int64)
    n = 65481 * v[..., 0] + 128553 * v[..., 1] + 24966 * v[..., 2]
    q, r = n // 255000, n % 255000
    up = (2 * r > 255000) | ((2 * r == 255000) & (q % 2 == 1))
    return 16 + q + up.astype(np.int64)


def crop(y):
    H, W = y.shape[-2:]
    return y[..., :H // BLOCK * BLOCK, :W // BLOCK * BLOCK]


def half_axis(x, axis):
    x = np.moveaxis(x, axis, -1)
    n = x.shape[-1]
    idx = np.arange(-3, n + 3)
    idx = np.where(idx < 0, -idx - 1, np.where(idx >= n, 2 * n - 1 - idx, idx))      # symmetric: -1 -> 0, n -> n - 1
    p = x[..., idx]
    out = np.zeros(x.shape[:-1] + (n // 2,), dtype=np.int64)
    for k in range(8):
        out += TAPS[k] * p[..., k:k + n:2][..., :n // 2]
    return np.moveaxis(out, -1, axis)


def half(y):
    """(..., H, W) int64 (even sizes) -> the numerators over 65536 of MATLAB's imresize(y, 0.5), (..., H / 2, W / 2) int64"""
    return half_axis(half_axis(y, -1), -2)


def class_of(di, dj):
    a, b = sorted((abs(di), abs(dj)))
    return [(p, q) for p in range(4) for q in range(p, 4)].index((a, b))


def mscn(x, p):
    """x (H, W) int64, values x 2^-p -> (mscn, sigma), both (H, W) float64"""
    import sgic_amd  # noqa: F401
    from sgic_amd.niqe import window_weights
    w = window_weights()
    H, W = x.shape
    pad = np.pad(x, 3, mode="edge")
    s = np.zeros((10, H, W), dtype=np.int64)
    q = np.zeros((10, H, W), dtype=np.int64)
    for di in range(-3, 4):
        for dj in range(-3, 4):
            d = pad[3 + di:3 + di + H, 3 + dj:3 + dj + W] - x
            k = class_of(di, dj)
            s[k] += d
            q[k] += d * d
    m = np.zeros((H, W), dtype=np.float64)
    v = np.zeros((H, W), dtype=np.float64)
    for k in range(10):
        m = m + w[k] * (s[k].astype(np.float64) * 2.0 ** -p)
        v = v + w[k] * (q[k].astype(np.float64) * 2.0 ** (-2 * p))
    sigma = np.sqrt(np.abs(v - m * m))
    return (0.0 - m) / (sigma + 1.0), sigma


def map_stats(n):
    neg, pos = n < 0, n > 0
    return [float(neg.sum()), float(pos.sum()), float((n[neg] ** 2).sum()), float((n[pos] ** 2).sum()), float(np.abs(n).sum())]


def planes(img):
    """(H, W, 3) u8 -> [(plane int64, p)] of the two scales"""
    y = crop(luma(img))
    return [(y, 0), (half(y), 16)]


def blocks(img):
    """(B, H, W, 3) u8 -> (stats (B, nbh, nbw, 2, 5, 5), sharp (B, nbh, nbw)) float64: the layout of ops.niqe_blocks_u8"""
    B, H, W, _ = img.shape
    nbh, nbw = H // BLOCK, W // BLOCK
    stats = np.zeros((B, nbh, nbw, 2, 5, 5), dtype=np.float64)
    sharp = np.zeros((B, nbh, nbw), dtype=np.float64)
    for b in range(B):
        for s, (x, p) in enumerate(planes(img[b])):
            n, sigma = mscn(x, p)
            S = BLOCK >> s
            for ih in range(nbh):
                for iw in range(nbw):
                    blk = n[ih * S:(ih + 1) * S, iw * S:(iw + 1) * S]
                    stats[b, ih, iw, s, 0] = map_stats(blk)
                    for k, sh in enumerate(SHIFTS):
                        stats[b, ih, iw, s, k + 1] = map_stats(blk * np.roll(blk, sh, axis=(0, 1)))
                    if s == 0:
                        sharp[b, ih, iw] = sigma[ih * S:(ih + 1) * S, iw * S:(iw + 1) * S].sum() / (S * S)
    return stats, sharp


def score_of_features(feat, mu_p, cov_p):
    """(nblocks, 36) -> the score, None with fewer than two NaN-free blocks"""
    good = feat[~np.isnan(feat).any(axis=1)]
    if good.shape[0] < 2:
        return None
    d = mu_p - np.nanmean(feat, axis=0)
    return float(math.sqrt(d @ np.linalg.pinv((cov_p + np.cov(good, rowvar=False)) / 2.0) @ d))


def scores(stats, mu_p, cov_p):
    """stats of blocks() -> list of B scores (None: no score)"""
    import sgic_amd  # noqa: F401
    from sgic_amd.niqe import features
    feat = features(stats)
    return [score_of_features(feat[b].reshape(-1, 36), mu_p, cov_p) for b in range(feat.shape[0])]


def fit(images):
    """MATLAB's estimatemodelparam over a list of (H, W, 3) u8 images: the rows of the blocks sharper than 0.75 x the image's
    sharpest -> (mu, cov)"""
    import sgic_amd  # noqa: F401
    from sgic_amd.niqe import features
    rows = []
    for img in images:
        stats, sharp = blocks(img[None])
        keep = sharp.reshape(-1) > 0.75 * sharp.max()
        rows.append(features(stats).reshape(-1, 36)[keep])
    rows = np.concatenate(rows, axis=0)
    good = rows[~np.isnan(rows).any(axis=1)]
    return np.nanmean(rows, axis=0), np.cov(good, rowvar=False)


# ---- the images, the pristine model and the tolerances of the tests -------------------------------------------------------

def natural(H, W, seed):
    """a smoothed random field plus noise of +-4: (H, W, 3) u8"""
    rng = np.random.default_rng(seed)
    h, w = H // 12 + 2, W // 12 + 2
    low = rng.random((h, w, 3))

    def up(n_out, n_in):
        t = (np.arange(n_out) + 0.5) * (n_in - 1) / n_out
        i0 = np.minimum(t.astype(np.int64), n_in - 2)
        f = t - i0
        m = np.zeros((n_out, n_in))
        m[np.arange(n_out), i0] = 1.0 - f
        m[np.arange(n_out), i0 + 1] = f
        return m

    field = np.einsum("ih,hwc,jw->ijc", up(H, h), low, up(W, w))
    field = 20.0 + 215.0 * (field - field.min()) / (field.max() - field.min())
    return np.clip(np.rint(field) + rng.integers(-4, 5, (H, W, 3)), 0, 255).astype(np.uint8)


def make_case(name):
    if name == "batch3":
        return np.stack([natural(256, 256, 300 + j) for j in range(3)])
    if name == "noise":
        return np.random.default_rng(5).integers(0, 256, (1, 192, 192, 3), dtype=np.uint8)
    if name == "flat":
        return np.full((1, 192, 192, 3), 77, dtype=np.uint8)
    if name == "halfflat":
        a = natural(192, 192, 21)
        a[:, 96:] = 255
        return a[None]
    if name == "ramp":
        return np.ascontiguousarray(np.broadcast_to(np.arange(192, dtype=np.uint8)[None, :, None], (192, 192, 3)))[None]
    if name == "checker":
        i, j = np.mgrid[0:192, 0:192]
        c = np.where(((i // 8) + (j // 8)) % 2 == 0, 60, 190).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(c[:, :, None], (192, 192, 3)))[None]
    H, W = (int(v) for v in name.split("x"))
    return natural(H, W, 7 * H + W)[None]


CASES = ["96x192", "192x96", "200x300", "batch3", "noise", "flat", "halfflat", "ramp", "checker", "96x100"]
NO_SCORE = ("flat", "96x100")        # the restatement must give None for these and for nothing else
NO_LAUNCH = "95x300"

_CACHE = {}


def pristine():
    """the synthetic pristine model of the tests: cov = A A^T / 36 + 0.1 I, seeded"""
    rng = np.random.default_rng(19)
    A = rng.normal(size=(36, 36))
    base = np.array(([2.5, 0.8] + [0.8, 0.05, 0.3, 0.4] * 4) * 2)
    return base + 0.05 * rng.normal(size=36), A @ A.T / 36.0 + 0.1 * np.eye(36)


def case(name):
    """-> (img, stats, sharp, scores) of one case, computed once and shared.  Read-only."""
    if name not in _CACHE:
        img = make_case(name)
        stats, sharp = blocks(img)
        for v in (img, stats, sharp):
            v.setflags(write=False)
        _CACHE[name] = (img, stats, sharp, scores(stats, *pristine()))
    return _CACHE[name]


def perturbed(stats, seed):
    """every sum (not the counts) moved by +-REL relative, seeded signs"""
    rng = np.random.default_rng(seed)
    out = np.array(stats, dtype=np.float64)
    out[..., 2:] *= 1.0 + REL * rng.choice([-1.0, 1.0], size=out[..., 2:].shape)
    return out


def score_change():
    """the largest change of a score over the case list when every block sum moves by +-REL"""
    if "score_change" not in _CACHE:
        worst = 0.0
        for k, name in enumerate(CASES):
            _, stats, _, ref = case(name)
            for seed in (2 * k, 2 * k + 1):
                for a, b in zip(ref, scores(perturbed(stats, seed), *pristine())):
                    assert (a is None) == (b is None)
                    if a is not None:
                        worst = max(worst, abs(a - b))
        _CACHE["score_change"] = worst
    return _CACHE["score_change"]


def score_tolerance():
    """what the GPU tests hold a score to: ten times the measured effect of the sums' own bound"""
    return 10.0 * score_change()


FIT_SIZES = [(192, 192), (192, 192), (192, 288), (200, 300), (192, 192), (192, 288)]


def fit_images():
    if "fit_images" not in _CACHE:
        _CACHE["fit_images"] = [natural(H, W, 900 + k) for k, (H, W) in enumerate(FIT_SIZES)]
    return _CACHE["fit_images"]


def fit_case():
    """-> (mu, cov, tol_mu, tol_cov): the restatement's fit of fit_images() and ten times the largest change of an entry when
    every block sum and sharpness moves by +-REL"""
    import sgic_amd  # noqa: F401
    from sgic_amd.niqe import features
    if "fit" not in _CACHE:
        per = [blocks(img[None]) for img in fit_images()]

        def model(move):
            rows = []
            for k, (stats, sharp) in enumerate(per):
                if move:
                    rng = np.random.default_rng(50 + k)
                    stats = perturbed(stats, 70 + k)
                    sharp = sharp * (1.0 + REL * rng.choice([-1.0, 1.0], size=sharp.shape))
                rows.append(features(stats).reshape(-1, 36)[sharp.reshape(-1) > 0.75 * sharp.max()])
            rows = np.concatenate(rows, axis=0)
            return np.nanmean(rows, axis=0), np.cov(rows[~np.isnan(rows).any(axis=1)], rowvar=False)

        (mu, cov), (mu2, cov2) = model(False), model(True)
        _CACHE["fit"] = (mu, cov, 10.0 * float(np.abs(mu - mu2).max()), 10.0 * float(np.abs(cov - cov2).max()))
    return _CACHE["fit"]
