"""CPU: the numpy restatement tests/fsim_ref.py of FSIM / FSIMc against closed forms and hand-computed values,
the size arithmetic of quality.fsim_reduction, and what evaluate.py does with the two keys.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsim_ref as ref  # noqa: E402


def _field(H, W, seed=0):
    """a smooth colour field with a vertical step at W // 2, fp64 (H, W, 3)"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([90.0 + 40.0 * np.sin(0.2 * x + c + seed) + 30.0 * np.cos(0.15 * y) + 50.0 * (x >= W // 2) for c in range(3)], axis=-1)


def _u8(f):
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def test_reduction_factor_is_matlabs_round():
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    for side, F in ((383, 1), (384, 2), (639, 2), (640, 3), (2, 1), (255, 1)):
        assert ref.reduction(side, side + 7)[0] == F and ref.reduction(side + 7, side)[0] == F
        assert quality.fsim_reduction(side, side + 7) == ref.reduction(side, side + 7)
    assert ref.reduction(385, 401) == (2, 193, 201) and ref.reduction(641, 643) == (3, 214, 215)       # ceil sizes at odd H
    assert quality.FSIM_MIN_SIDE == ref.MIN_SIDE == 2 and quality.FSIM_MAX_REDUCED_SIDE == ref.MAX_REDUCED_SIDE == 2048


@pytest.mark.parametrize("F", [2, 3, 4])
def test_same_anchor_against_a_full_convolution(F):
    """conv2(x, ones(F) / F^2, 'same') is rows and columns floor(F / 2) .. of the full convolution"""
    x = np.random.default_rng(F).uniform(-50, 255, (13, 11))
    H, W = x.shape
    full = np.zeros((H + F - 1, W + F - 1))
    for p in range(F):
        for q in range(F):
            full[p:p + H, q:q + W] += x / (F * F)
    r0 = F // 2             # ceil((F - 1) / 2)
    want = full[r0:r0 + H, r0:r0 + W]
    got = ref.mean_same(x, F)
    assert np.abs(got - want).max() < 1e-12
    # the span the text names: i + F // 2 - F + 1 .. i + F // 2, samples outside counting 0
    span = {2: (0, 1), 3: (-1, 1), 4: (-1, 2)}[F]
    i, j = 5, 6
    assert abs(got[i, j] - x[i + span[0]:i + span[1] + 1, j + span[0]:j + span[1] + 1].sum() / (F * F)) < 1e-12
    assert abs(got[H - 1, W - 1] - x[H - 1 + span[0]:, W - 1 + span[0]:].sum() / (F * F)) < 1e-12
    red = ref.reduce_plane(x, F)
    assert red.shape == (-(-H // F), -(-W // F)) and np.array_equal(red, got[::F, ::F])


def test_planes_are_single_operations():
    px = np.array([[[200, 30, 90]]], dtype=np.uint8)
    Y, I, Q = ref.yiq(px)
    assert Y[0, 0] == (0.299 * 200.0 + 0.587 * 30.0) + 0.114 * 90.0
    assert I[0, 0] == (0.596 * 200.0 - 0.274 * 30.0) - 0.322 * 90.0
    assert Q[0, 0] == (0.211 * 200.0 - 0.523 * 30.0) + 0.312 * 90.0


@pytest.mark.parametrize("h,w", [(31, 44), (47, 47), (64, 64)])
def test_filter_bank(h, w):
    lg, spread = ref.filter_bank(h, w)
    assert lg.shape == (4, h, w) and spread.shape == (4, h, w)
    assert all(lg[s][0, 0] == 0.0 for s in range(4)) and all((lg[s] * spread[o])[0, 0] == 0.0 for s in range(4) for o in range(4))
    assert lg.min() >= 0.0 and lg.max() <= 1.0 and spread.min() >= 0.0 and spread.max() <= 1.0
    # the centre frequencies: scale s peaks at radius 1 / (6 2^s), so the radius of the largest sample halves (coarsely, on a grid)
    assert ref.axis_coords(6).tolist() == [-0.5, -1 / 3, -1 / 6, 0.0, 1 / 6, 1 / 3] and ref.axis_coords(5).tolist() == [-0.5, -0.25, 0.0, 0.25, 0.5]
    if h == w and h % 2 == 0:
        # on an even square grid a quarter turn of the frequency plane maps the grid onto itself (but the Nyquist row and column):
        # spread_2 (angle pi / 2) is spread_0 turned; theta = atan2(-y, x), so (x, y) -> (y, -x) adds pi / 2 to theta
        # (rows grow downwards: c2[i, j] = c0[j, N - 1 - i], which is np.rot90(c0, 1))
        c = np.fft.fftshift(spread, axes=(1, 2))[:, 1:, 1:]          # centred, odd side, the origin in the middle
        c[:, h // 2 - 1, w // 2 - 1] = 0.0                           # the origin has no angle; logGabor is 0 there
        assert np.abs(c[2] - np.rot90(c[0], 1)).max() < 1e-12 and np.abs(c[3] - np.rot90(c[1], 1)).max() < 1e-12
    # spread_o is one-sided: 1 along its own direction, exp(-pi^2 / (2 sigma^2)) against it
    assert abs(spread[0][0, 1] - 1.0) < 1e-15 and abs(spread[0][0, w - 1] - np.exp(-np.pi ** 2 / (2 * ref.SIGMA_THETA ** 2))) < 1e-15


@pytest.mark.parametrize("h,w", [(31, 44), (47, 47), (64, 64)])
def test_parseval_gives_the_spatial_sums(h, w):
    lg, spread = ref.filter_bank(h, w)
    for o in range(4):
        S2, Sij = ref.spatial_sums(lg, spread[o])
        P2, Pij = ref.parseval_sums(lg, spread[o])
        assert abs(P2 - S2) <= 1e-13 * S2 and abs(Pij - Sij) <= 1e-13 * abs(Sij)


def test_phase_congruency_range_step_and_flat():
    H, W = 48, 64
    P = 100.0 + 60.0 * (np.arange(W)[None, :] >= W // 2) + np.zeros((H, 1))
    P = P + np.random.default_rng(1).normal(0.0, 0.5, P.shape)
    pc = ref.phase_congruency(P)
    assert pc.shape == (H, W) and pc.min() >= 0.0 and pc.max() <= 1.0
    cols = pc[8:-8].mean(axis=0)
    # the step edge carries the peak (the transform is periodic: the borders are the same step, and the middle of either plateau
    # is a point of symmetry with a smaller peak of its own)
    assert abs(int(np.argmax(cols[8:-8])) + 8 - W // 2) <= 1
    assert cols[W // 2 - 1:W // 2 + 1].max() > 2.0 * np.median(cols)
    assert np.array_equal(ref.phase_congruency(np.full((9, 12), 77.25)), np.zeros((9, 12)))
    with pytest.raises(ValueError):
        ref.phase_congruency(np.zeros((1, 12)))


def test_equal_images_give_exactly_one():
    for H, W in ((31, 44), (47, 47), (2, 2), (2, 9)):
        a = np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert ref.fsim(a, a.copy()) == (1.0, 1.0)


def test_flat_planes():
    a = np.full((20, 24, 3), 90, np.uint8)
    assert ref.fsim(a, a.copy()) == (1.0, 1.0)
    assert ref.fsim(a, np.full((20, 24, 3), 140, np.uint8)) == (0.0, 0.0)
    b = a.copy()          # another colour of (nearly) the same luma: the I and Q planes differ, so still 0
    b[..., 0], b[..., 2] = 52, 187
    assert abs(ref.yiq(b)[0][0, 0] - 90.0) < 0.5 and ref.fsim(a, b) == (0.0, 0.0)
    assert ref.fsim(np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)) == (1.0, 1.0)


def test_chroma_term_with_a_negative_product():
    """I1 = 40, I2 = -40: Si = (200 - 3200) / (3200 + 200) = -15 / 17; Q equal: Sq = 1; c < 0, so C = (15 / 17)^0.03 cos(0.03 pi)"""
    one = np.ones((1, 1))
    C = ref.chroma_term(40.0 * one, -40.0 * one, 10.0 * one, 10.0 * one)
    assert abs(C[0, 0] - (15.0 / 17.0) ** 0.03 * np.cos(0.03 * np.pi)) < 1e-15
    assert abs(C[0, 0] - np.real(complex(-15.0 / 17.0) ** 0.03)) < 1e-15          # MATLAB's real(c .^ 0.03)
    assert ref.chroma_term(40.0 * one, 40.0 * one, 10.0 * one, 10.0 * one)[0, 0] == 1.0
    pos = ref.chroma_term(40.0 * one, 20.0 * one, 10.0 * one, 10.0 * one)[0, 0]
    assert abs(pos - ((1600.0 + 200.0) / (2000.0 + 200.0)) ** 0.03) < 1e-15


def test_fsim_falls_as_noise_rises():
    f = _field(47, 47)
    a = _u8(f)
    rng = np.random.default_rng(3)
    vals = [ref.fsim(a, a)] + [ref.fsim(a, _u8(f + rng.normal(0.0, s, f.shape))) for s in (6.0, 25.0)]
    print(vals)
    assert vals[0] == (1.0, 1.0)
    assert 1.0 > vals[1][0] > vals[2][0] > 0.5 and 1.0 > vals[1][1] > vals[2][1] > 0.5
    assert vals[1][1] < vals[1][0] and vals[2][1] < vals[2][0]          # the chroma term only takes away
    assert 0.95 < vals[1][0] < 0.995 and 0.7 < vals[2][0] < 0.92


def test_limits_are_refused():
    with pytest.raises(ValueError, match="sides >= 2"):
        ref.fsim(np.zeros((1, 50, 3), np.uint8), np.zeros((1, 50, 3), np.uint8))
    with pytest.raises(ValueError, match="<= 2048"):
        ref.fsim(np.zeros((300, 2100, 3), np.uint8), np.zeros((300, 2100, 3), np.uint8))
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    with pytest.raises(ValueError, match="sides >= 2"):
        quality._fsim_check(1, 50)
    with pytest.raises(ValueError, match="<= 2048"):
        quality._fsim_check(300, 2100)
    quality._fsim_check(4100, 4100)          # F = 16: 257 x 257
    quality._fsim_check(2, 2048)


def test_summary_and_command_line(capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    assert evaluate.FSIM_FIELDS == ("fsim", "fsimc")
    base = {"bpp": 0.5, "psnr": 30.0, "ms_ssim": 0.9}
    hvs = dict(vifp=0.5, gmsd=0.1, psnr_hvs=30.0, psnr_hvs_m=34.0)
    recs = [dict(base, fsim=0.9, fsimc=0.8, lpips=0.2), dict(base, fsim=None, fsimc=None, lpips=0.4), dict(base, fsim=0.7, fsimc=0.6, lpips=0.6)]
    s = evaluate.summarise(recs)
    assert list(s) == ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db", "fsim", "fsimc", "fsim_skipped", "lpips"]
    assert abs(s["fsim"] - 0.8) < 1e-15 and abs(s["fsimc"] - 0.7) < 1e-15 and s["fsim_skipped"] == 1
    s = evaluate.summarise([dict(r, **hvs) for r in recs])
    assert list(s) == ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db", "vifp", "gmsd", "psnr_hvs", "psnr_hvs_m", "hvs_skipped",
                       "fsim", "fsimc", "fsim_skipped", "lpips"]
    anchor = dict(base, bpp=0.4, over_rate=False)
    s = evaluate.summarise([dict(r, **hvs, anchor=dict(anchor, **hvs, fsim=0.5, fsimc=0.25)) for r in recs])
    assert list(s)[-7:] == ["anchor_over_rate", "anchor_vifp", "anchor_gmsd", "anchor_psnr_hvs", "anchor_psnr_hvs_m", "anchor_fsim",
                            "anchor_fsimc"]
    assert s["anchor_fsim"] == 0.5 and s["anchor_fsimc"] == 0.25
    plain = evaluate.summarise([base])
    assert list(plain) == ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]       # without the keys nothing is added
    with pytest.raises(SystemExit):          # the flag is known: the complaint is about the folders, before any device call
        evaluate.main(["--originals", "nowhere", "--fsim"])
    err = capsys.readouterr().err
    assert "--bitstreams" in err and "unrecognized" not in err
    with pytest.raises(SystemExit):          # it takes no value
        evaluate.main(["--originals", "nowhere", "--recon_dir", "nowhere", "--fsim", "1"])
    assert "unrecognized arguments: 1" in capsys.readouterr().err
