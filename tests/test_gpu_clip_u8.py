"""GPU: CLIP preprocessing straight from the u8 canvas of the ingest (ClipHIP.preprocess_u8, sgic_clip_preprocess_u8canvas).  Against
Pillow on the bytes as they are, bit for bit; against the existing fp32 route on inputs that truncate back to the same bytes; and
the paths only large geometries take (a window of more than one LDS fill, several tiles of output columns per row)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_pillow_ref import pillow_from_u8 as _pillow  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_EXT = [(20, 33), (64, 96), (3, 96), (64, 5), (61, 61), (17, 90), (50, 7)]
LARGE_EXT = [(301, 517), (517, 301), (224, 224)]


@pytest.fixture(scope="module")
def clip():
    import sgic_amd  # noqa: F401
    from sgic_amd import weights as W
    from sgic_amd.clip import ClipHIP
    from sgic_amd.config import CLIP_TINY
    assert CLIP_TINY.image_size == 224
    return ClipHIP(W.synth_weights(W.clip_spec(CLIP_TINY), seed=5), CLIP_TINY, torch.device("cuda:0"))


def _canvas(shape, ext, rng, outside):
    c = np.full(shape, outside, dtype=np.uint8)
    for j, (h, w) in enumerate(ext):
        c[j, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return c


@pytest.mark.parametrize("shape,ext", [((7, 64, 96, 3), SMALL_EXT), ((3, 517, 640, 3), LARGE_EXT)], ids=["64x96", "517x640"])
def test_preprocess_u8_bit_exact_vs_pillow(clip, shape, ext):
    cfg = clip.cfg
    canvas = _canvas(shape, ext, np.random.default_rng(51), 0xAA)
    got = clip.preprocess_u8(torch.from_numpy(canvas).cuda(), ext).cpu().numpy()
    assert got.shape == (len(ext), 3, 224, 224)
    for j, (h, w) in enumerate(ext):
        assert np.array_equal(got[j], _pillow(canvas[j, :h, :w], 224, cfg.mean, cfg.std)), (h, w)


def test_nothing_outside_an_extent_is_read(clip):
    a = _canvas((7, 64, 96, 3), SMALL_EXT, np.random.default_rng(51), 0xAA)
    b = _canvas((7, 64, 96, 3), SMALL_EXT, np.random.default_rng(51), 0x00)
    assert not np.array_equal(a, b)
    ga = clip.preprocess_u8(torch.from_numpy(a).cuda(), SMALL_EXT)
    gb = clip.preprocess_u8(torch.from_numpy(b).cuda(), SMALL_EXT)
    assert torch.equal(ga, gb)


def test_preprocess_u8_equals_the_fp32_route_on_the_same_bytes(clip):
    """34 images in one call (two launches): the fp32 route, fed values that truncate back to the canvas bytes (x = (u + 0.5) / 255 * 2 - 1,
    all 256 checked in tests/test_build_images_cpu.py), gives the same bits"""
    rng = np.random.default_rng(52)
    ext = [tuple(int(v) for v in rng.integers(8, 65, 2)) for _ in range(34)]
    canvas = torch.from_numpy(_canvas((34, 64, 64, 3), ext, rng, 0xAA)).cuda()
    x = ((canvas.float() + 0.5) / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(clip.preprocess_u8(canvas, ext), clip.preprocess(x, hw=ext))


def test_windows_larger_than_one_lds_fill_and_several_tiles_per_row():
    """the two paths no small image takes, reached with a small S through the ops wrapper: at S = 1 an 1100 x 5000 image (5000 -> 4
    columns) has an output column of more taps than the 4096 pixels of an LDS fill, so two fills; at S = 3 a 2100 x 5000 image
    (5000 -> 7 columns) has windows of some 2860 taps every 714 pixels, so a fill holds two output columns and a row takes two
    tiles, the second one partial"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    from sgic_amd.clip import resize_geometry
    rng = np.random.default_rng(53)
    canvas = rng.integers(0, 256, (1, 2100, 5000, 3), dtype=np.uint8)
    d = torch.from_numpy(canvas).cuda()
    mean, std = np.float32([0.48, 0.45, 0.40]), np.float32([0.26, 0.27, 0.28])
    for S, (h, w) in ((1, (1100, 5000)), (3, (2100, 5000))):
        geo = np.array([(h, w) + resize_geometry(h, w, S)], dtype=np.int32)
        got = ops.clip_preprocess_u8canvas(d, geo, S, mean, std).cpu().numpy()
        assert np.array_equal(got[0], _pillow(canvas[0, :h, :w], S, mean, std)), (S, h, w)


def test_an_output_side_above_65535_on_both_routes():
    """a 1 x 30000 image at S = 3 resizes to 3 x 90000: an output side the entry points used to refuse.  Both routes against Pillow,
    the fp32 one fed values that truncate back to the canvas bytes"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    from sgic_amd.clip import resize_geometry
    h, w, S = 1, 30000, 3
    geo = np.array([(h, w) + resize_geometry(h, w, S)], dtype=np.int32)
    assert tuple(geo[0, 2:4]) == (3, 90000)
    canvas = np.random.default_rng(54).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    mean, std = np.float32([0.48, 0.45, 0.40]), np.float32([0.26, 0.27, 0.28])
    ref = _pillow(canvas[0], S, mean, std)
    d = torch.from_numpy(canvas).cuda()
    assert np.array_equal(ops.clip_preprocess_u8canvas(d, geo, S, mean, std)[0].cpu().numpy(), ref)
    x = ((d.float() + 0.5) / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(ops.clip_preprocess_ragged(x, geo, S, mean, std)[0].cpu().numpy(), ref)


def test_extents_outside_the_canvas_are_refused(clip):
    canvas = torch.zeros(2, 32, 48, 3, dtype=torch.uint8, device="cuda:0")
    for hw in ([(33, 48), (8, 8)], [(8, 8), (32, 49)], [(0, 8), (8, 8)]):
        with pytest.raises(ValueError):
            clip.preprocess_u8(canvas, hw)
