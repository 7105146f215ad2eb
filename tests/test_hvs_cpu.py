"""CPU: the restatement tests/hvs_ref.py of VIFp, GMSD and PSNR-HVS / PSNR-HVS-M against cases with a closed
form, the two tables against published spot values, and evaluate.py's handling of --hvs in the summary and on the command line."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hvs_ref as ref  # noqa: E402


def test_tables_match_the_published_spot_values():
    """the published six-decimal tables round the closed forms.  Three of the four spot values are the closed form rounded to six
    places; CSFCof[0][1] = 25.735088 / 11 = 2.33955345..., which the published table prints as 2.339554: it agrees to less than one
    unit of the sixth place (5.5e-7) but rounds to 2.339553, so all four are held to that distance and three to the rounding too."""
    for got, published in ((ref.CSFCOF[0, 0], 1.608443), (ref.CSFCOF[0, 1], 2.339554), (ref.MASKCOF[0, 0], 0.390625),
                           (ref.MASKCOF[0, 1], 0.826446)):
        assert abs(got - published) < 1e-6
    assert round(ref.CSFCOF[0, 0], 6) == 1.608443
    assert round(ref.MASKCOF[0, 0], 6) == 0.390625 and round(ref.MASKCOF[0, 1], 6) == 0.826446
    assert abs(ref.CSFCOF[0, 0] - 25.735088 / 16) < 1e-15
    C = ref.dct_matrix()
    assert np.abs(C @ C.T - np.eye(8)).max() < 1e-15      # orthonormal


def test_window_and_smallest_vifp_size():
    """the window arithmetic: 17, 9, 5, 3; a side of 41 leaves scale 4 one valid sample, 40 none"""
    from sgic_amd import quality
    for N in (17, 9, 5, 3):
        w = ref.gauss_window(N)
        assert w.shape == (N, N) and abs(w.sum() - 1.0) < 1e-15 and w[N // 2, N // 2] == w.max()
    n = 41
    for s, N in enumerate((17, 9, 5, 3)):
        if s:
            n = len(range(0, n - N + 1, 2))
        assert n >= N
    assert n - 3 + 1 == 1
    assert quality.VIFP_MIN_SIDE == ref.VIFP_MIN_SIDE == 41 and quality.VIFP_WINDOWS == (17, 9, 5, 3)
    rng = np.random.default_rng(0)
    y = rng.uniform(0, 255, (41, 41))
    assert 0.0 < ref.vifp(y, y + rng.normal(0, 5, y.shape)) < 1.0
    for shape in ((40, 41), (41, 40)):
        with pytest.raises(ValueError, match="41"):
            ref.vifp(np.zeros(shape), np.zeros(shape))


def test_identical_images():
    a, b, m = ref.case("identical", 49, 57)
    # sv = s2 - g s12 with g = s1 / (s1 + eps) leaves sv of the order of eps, not 0: 1 - VIFp is of the order eps / sigma_n^2
    assert m["vifp"] <= 1.0 and 1.0 - m["vifp"] < 1e-9
    assert m["gmsd"] == 0.0
    assert math.isinf(m["psnr_hvs"]) and math.isinf(m["psnr_hvs_m"]) and m["psnr_hvs"] > 0


def test_constant_images_take_the_flat_rule():
    a, b, m = ref.case("flat_equal", 49, 57)
    assert ref.vifp_sums(ref.luma(a), ref.luma(b)) == (0.0, 0.0)
    assert m["vifp"] == 1.0 and m["gmsd"] == 0.0 and math.isinf(m["psnr_hvs"])
    a, b, m = ref.case("flat", 49, 57)
    assert ref.vifp_sums(ref.luma(a), ref.luma(b))[1] == 0.0 and m["vifp"] == 0.0


def test_constant_offset_of_three():
    """b = a + 3 in every channel: Yb - Ya = 3 up to rounding, so only the DC coefficient differs, by 8 * 3, and neither image's
    mask touches it.  The gradients of a and b agree wherever the 3 x 3 and 2 x 2 supports see no zero padding, so GMS = 1 on the
    interior of the map; the zero-padded border rows and columns (and the last row / column of an odd side, whose 2 x 2 mean
    includes padding) see the offset as an edge, which is what keeps the GMSD of the whole map from 0."""
    a, b, m = ref.case("offset", 49, 57)
    want = 10.0 * np.log10(255.0 ** 2 / ((3.0 * 8.0 * ref.CSFCOF[0, 0]) ** 2 / 64.0))
    assert abs(m["psnr_hvs"] - want) < 1e-11 * want and abs(m["psnr_hvs_m"] - want) < 1e-11 * want
    g = ref.gms_map(ref.luma(a), ref.luma(b))
    assert g.shape == (25, 29)
    inner = g[1:-2, 1:-2]       # 49 and 57 are odd: the last row and column of the half-size map are half padding
    assert np.abs(inner - 1.0).max() < 1e-12 and float(np.std(inner)) < 1e-12
    assert 0.0 < m["gmsd"] < 1e-3
    a, b, m = ref.case("offset", 48, 56)      # even sides: only the outermost ring sees padding
    g = ref.gms_map(ref.luma(a), ref.luma(b))
    assert np.abs(g[1:-1, 1:-1] - 1.0).max() < 1e-12 and np.abs(g[0] - 1.0).min() > 1e-9


def test_gmsd_of_constant_images_with_an_offset_in_closed_form():
    """constants c1 and c2 on an even-sided image: the half-size map is constant, its Prewitt magnitude is 0 inside, c on the four
    edges (three samples of c against a zero column or row, over 3) and c sqrt(8) / 3 in the corners (two samples each way)"""
    H, W, c1, c2 = 20, 28, 100.0, 103.0
    h, w = H // 2, W // 2
    def gms(k):
        return (2.0 * c1 * c2 * k + 170.0) / ((c1 * c1 + c2 * c2) * k + 170.0)
    vals = np.concatenate([np.full((h - 2) * (w - 2), gms(0.0)), np.full(2 * (h - 2) + 2 * (w - 2), gms(1.0)), np.full(4, gms(8.0 / 9.0))])
    want = float(np.sqrt(np.mean((vals - vals.mean()) ** 2)))
    got = ref.gmsd(np.full((H, W), c1), np.full((H, W), c2))
    assert abs(got - want) < 1e-15


def test_single_dct_basis_error_below_and_above_the_mask():
    """one textured block plus amp times the DCT basis function (2, 3): |Da - Db| is amp at that coefficient alone.  Below
    mask / MaskCof it vanishes with masking and counts (amp CSFCof)^2 without; above, masking leaves (amp - mask / MaskCof)."""
    rng = np.random.default_rng(3)
    Ba = rng.uniform(60.0, 200.0, (8, 8))
    C = ref.dct_matrix()
    basis = np.outer(C[2], C[3])
    Da = C @ Ba @ C.T
    for amp, below in ((0.5, True), (60.0, False)):
        Bb = Ba + amp * basis
        mask = max(ref.block_mask(Ba, Da), ref.block_mask(Bb, C @ Bb @ C.T))
        thr = mask / ref.MASKCOF[2, 3]
        assert (amp < thr) == below
        e, e_m = ref.block_errors(Ba, Bb)
        assert abs(e - (amp * ref.CSFCOF[2, 3]) ** 2) < 1e-9 * e
        if below:
            assert e_m < 1e-20 and e > 0.1        # the 63 other differences are rounding noise far below their thresholds
        else:
            assert abs(e_m - ((amp - thr) * ref.CSFCOF[2, 3]) ** 2) < 1e-9 * e_m
        hvs, hvs_m = ref.psnr_hvs(Ba, Bb)
        assert abs(hvs - 10.0 * np.log10(65025.0 / (e / 64.0))) < 1e-12
        assert hvs_m > hvs and (not below or hvs_m > 250.0)
    # a flat block carries no masking: pop = 0, so the same small error counts in full
    flat = np.full((8, 8), 100.0)
    e, e_m = ref.block_errors(flat, flat + 0.5 * basis)
    assert ref.block_mask(flat, C @ flat @ C.T) == 0.0 and abs(e - (0.5 * ref.CSFCOF[2, 3]) ** 2) < 1e-12


def test_partial_blocks_are_ignored_and_small_images_refused():
    rng = np.random.default_rng(4)
    ya = rng.uniform(0, 255, (15, 23))
    yb = ya + rng.normal(0, 4, ya.shape)
    whole = np.concatenate([ref.block_errors(ya[:8, j:j + 8], yb[:8, j:j + 8]) for j in (0, 8)]).reshape(2, 2).sum(axis=0)
    want = 10.0 * np.log10(65025.0 / (whole / 128.0))
    assert np.allclose(ref.psnr_hvs(ya, yb), want, rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        ref.psnr_hvs(ya[:7], yb[:7])


def test_conv_same_is_matlabs():
    """conv2([1 2 3 4], [1 1], 'same') = [3 5 7 4]: an even kernel is anchored one sample further than numpy's 'same'"""
    assert ref.conv_same_zero(np.array([[1.0, 2.0, 3.0, 4.0]]), np.array([[1.0, 1.0]])).tolist() == [[3.0, 5.0, 7.0, 4.0]]
    x = np.random.default_rng(5).uniform(0, 255, (9, 9))
    ave = ref.conv_same_zero(x, np.full((2, 2), 0.25))[::2, ::2]
    assert ave.shape == (5, 5) and abs(ave[4, 4] - x[8, 8] / 4.0) < 1e-13 and abs(ave[0, 0] - x[:2, :2].mean()) < 1e-13
    signal = pytest.importorskip("scipy.signal")      # an extra: odd kernels agree with scipy's 'same'
    hx = np.array([[1.0, 0.0, -1.0]] * 3) / 3.0
    assert np.abs(ref.conv_same_zero(x, hx) - signal.convolve2d(x, hx, mode="same")).max() < 1e-12
    assert np.abs(ref.filter_valid(x, ref.gauss_window(5)) - signal.correlate2d(x, ref.gauss_window(5), mode="valid")).max() < 1e-12


def test_q_table_is_the_encoders():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    assert tuple(int(v) for v in ref.Q_LUMA.ravel()) == tuple(jpeg_enc._LUMA)


def test_summary_and_command_line(capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    assert evaluate.HVS_FIELDS == ("vifp", "gmsd", "psnr_hvs", "psnr_hvs_m")
    base = {"bpp": 0.5, "psnr": 30.0, "ms_ssim": 0.9}
    recs = [dict(base, vifp=0.5, gmsd=0.1, psnr_hvs=30.0, psnr_hvs_m=34.0, lpips=0.2),
            dict(base, vifp=None, gmsd=0.3, psnr_hvs="inf", psnr_hvs_m="inf", lpips=0.4),
            dict(base, vifp=None, gmsd=0.2, psnr_hvs=None, psnr_hvs_m=None, lpips=0.6)]
    s = evaluate.summarise(recs)
    assert list(s) == ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db", "vifp", "gmsd", "psnr_hvs", "psnr_hvs_m", "hvs_skipped", "lpips"]
    assert s["vifp"] == 0.5 and abs(s["gmsd"] - 0.2) < 1e-15 and s["psnr_hvs"] == 30.0 and s["psnr_hvs_m"] == 34.0
    assert s["hvs_skipped"] == 2
    plain = evaluate.summarise([base])
    assert list(plain) == ["images", "bpp", "psnr", "ms_ssim", "ms_ssim_db"]       # without the keys nothing is added
    with pytest.raises(SystemExit):          # the flag is known: the complaint is about the folders, before any device call
        evaluate.main(["--originals", "nowhere", "--hvs"])
    err = capsys.readouterr().err
    assert "--bitstreams" in err and "unrecognized" not in err
    with pytest.raises(SystemExit):          # it takes no value
        evaluate.main(["--originals", "nowhere", "--recon_dir", "nowhere", "--hvs", "1"])
    assert "unrecognized arguments: 1" in capsys.readouterr().err
