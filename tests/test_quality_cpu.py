"""CPU: the fp64 restatement of the quality measures (tests/quality_ref.py) against independent statements of its parts, and the
yardstick of the GPU test's tolerance: what a change of summation order does to a level value in fp64."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as ref  # noqa: E402


@pytest.mark.parametrize("H,W", [(161, 175), (162, 161)])
def test_pyramid_is_avg_pool_times_scale(H, W):
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    pyr = ref.pyramid(img)
    x = torch.from_numpy(img).permute(0, 3, 1, 2).to(torch.float64) / 255.0
    for s in range(ref.LEVELS):
        assert pyr[s].shape[-2:] == x.shape[-2:] and int(pyr[s].max()) <= 255 * 4 ** s < 2 ** 16
        # the numerators are integers below 2^16 and the pooled values multiples of 1 / (4^s 255): the product rounds back exactly
        assert np.array_equal(pyr[s], np.rint(x.numpy() * (255 * 4 ** s)).astype(np.int64))
        assert np.abs(x.numpy() * (255 * 4 ** s) - pyr[s]).max() < 1e-9
        x = torch.nn.functional.avg_pool2d(x, kernel_size=2, padding=[d % 2 for d in x.shape[-2:]])
    assert pyr[4].shape[-2:] == (11, 11)


def test_filter_is_correlate1d_cropped():
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(3)
    x = rng.random((2, 3, 37, 45))
    g = ref.window()
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    want = correlate1d(correlate1d(x, g, axis=-1, mode="constant"), g, axis=-2, mode="constant")[..., 5:-5, 5:-5]
    for rows_first in (True, False):
        got = ref.filt(x, g, rows_first)
        assert got.shape == (2, 3, 27, 35)
        assert np.abs(got - want).max() < 1e-14


def test_identical_and_inverted():
    a, b = ref.make_pair("identical", 170, 190, 1)
    m = ref.measure(a[None], b[None])
    assert m["ms_ssim"][0] == 1.0 and m["ssim"][0] == 1.0 and math.isinf(m["psnr"][0]) and math.isinf(m["ms_ssim_db"][0])
    a, b = ref.make_pair("inverted", 170, 190, 1)
    m = ref.measure(a[None], b[None])
    assert m["ms_ssim"][0] == 0.0 and m["ms_ssim_db"][0] == 0.0
    assert m["psnr"][0] == 10.0 * np.log10(65025.0 * 3 * 170 * 190 / float(ref.sse(a[None], b[None]).sum()))


def test_combine_small_images_and_psnr():
    import sgic_amd  # noqa: F401
    from sgic_amd.quality import combine
    out = combine(np.array([[1, 2, 3], [0, 0, 0]], dtype=np.int64), None, 10, 20)
    assert out["ssim"] is None and out["ms_ssim"] is None and out["ms_ssim_db"] is None
    assert out["psnr"][0] == 10.0 * np.log10(65025.0 * 600 / 6.0) and math.isinf(out["psnr"][1])
    lv = np.ones((1, 3, 5, 2))
    lv[0, :, 2, 1] = -0.25                                   # a negative cs mean: relu -> the product is 0
    out = combine(np.array([[5, 5, 5]]), lv, 200, 200)
    assert out["ms_ssim"][0] == 0.0 and out["ssim"][0] == 1.0
    lv = np.full((1, 3, 5, 2), 0.5)
    out = combine(np.array([[5, 5, 5]]), lv, 200, 200)       # the weights sum to 1.0001
    assert abs(out["ms_ssim"][0] - 0.5 ** 1.0001) < 1e-15


def test_report_summary_and_argument_errors(capsys):
    import sgic_amd  # noqa: F401
    from sgic_amd import evaluate
    recs = [{"bpp": 0.5, "psnr": 30.0, "ms_ssim": 0.9}, {"bpp": None, "psnr": "inf", "ms_ssim": 1.0},
            {"bpp": 0.25, "psnr": 20.0, "ms_ssim": None}]
    s = evaluate.summarise(recs)
    assert s == {"images": 3, "bpp": 0.375, "psnr": 25.0, "ms_ssim": 0.95, "ms_ssim_db": float(-10.0 * np.log10(1.0 - 0.95))}
    assert evaluate.summarise([{"bpp": None, "psnr": "inf", "ms_ssim": 1.0}]) == \
        {"images": 1, "bpp": None, "psnr": None, "ms_ssim": 1.0, "ms_ssim_db": "inf"}
    assert evaluate._json_number(np.float64("inf")) == "inf" and evaluate._json_number(None) is None
    with pytest.raises(SystemExit):                           # neither --bitstreams nor --recon_dir: refused before any device call
        evaluate.main(["--originals", "nowhere"])
    assert "--bitstreams" in capsys.readouterr().err


def test_summation_order_yardstick():
    """rows-first against columns-first over the GPU test's cases: the GPU test allows 1e-11, about 300 times this"""
    worst = 0.0
    for H, W, B in ref.SIZES:
        for kind in ref.PAIRS:
            a, b, _, lv = ref.case(H, W, B, kind)
            worst = max(worst, float(np.abs(ref.levels(a, b, rows_first=False) - lv).max()))
    print(f"largest difference of a level value between the two filter orders: {worst:.3e}")
    assert worst < 1e-12
