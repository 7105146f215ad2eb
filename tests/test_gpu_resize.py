"""GPU: ops.resize_u8 (csrc/resize.hip) equals Pillow's Image.resize byte for byte, for bicubic and Lanczos, over the case list of
tests/resize_cases.py; batches, repeatability, the refusals and the workspace helper."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


def _resize(x_np, OH, OW, filt):
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(x_np)).cuda()
    return ops.resize_u8(x if x.dim() == 4 else x[None], OH, OW, filt).cpu().numpy()


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_equals_pillow(case):
    H, W, OH, OW, filt = case
    images = [rc.image(kind, H, W) for kind in rc.KINDS]
    got = _resize(np.stack(images), OH, OW, filt)      # the three kinds as one batch; test_batch_equals_single holds it to singles
    assert got.shape == (3, OH, OW, 3) and got.dtype == np.uint8
    for kind, x, g in zip(rc.KINDS, images, got):
        want = rc.pillow(x, OH, OW, filt)
        assert np.array_equal(g, want), (kind, int((g != want).sum()))


@pytest.mark.parametrize("filt", rc.FILTERS)
def test_both_clamps_act(filt):
    x, want = rc.clamp_case(filt)
    H, W, OH, OW = rc.CLAMP_CASE
    assert np.array_equal(_resize(x, OH, OW, filt)[0], want)


@pytest.mark.parametrize("case", [(33, 47, 9, 12, "lanczos"), (34, 50, 200, 300, "bicubic"), (37, 53, 19, 53, "lanczos")], ids=rc.case_id)
def test_batch_equals_single(case):
    H, W, OH, OW, filt = case
    images = [rc.image(kind, H, W, seed=3) for kind in rc.KINDS]
    batch = _resize(np.stack(images), OH, OW, filt)
    for x, g in zip(images, batch):
        assert np.array_equal(_resize(x, OH, OW, filt)[0], g)


def test_two_runs_are_equal():
    x = np.stack([rc.image("noise", 200, 300, seed=s) for s in range(2)])
    for filt in rc.FILTERS:
        assert np.array_equal(_resize(x, 67, 100, filt), _resize(x, 67, 100, filt))


def _raw_call(x, out, OH, OW, filt, work, nbytes, B=None, H=None, W=None):
    from sgic_amd._lib import call
    b, h, w, _ = x.shape
    call("sgic_resize_u8_batch", x, b if B is None else B, h if H is None else H, w if W is None else W, out, OH, OW, filt, work,
         ctypes.c_size_t(nbytes))


def test_refusals_leave_the_output_untouched():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd._lib import SgicError, lib
    x = torch.from_numpy(rc.image("noise", 17, 9)[None]).cuda()
    OH, OW = 5, 3
    nbytes = lib.sgic_resize_u8_work_bytes(1, 17, 9, OH, OW, 1)
    assert nbytes > 0 and nbytes % 16 == 0
    out = torch.full((1, OH, OW, 3), 0xA5, dtype=torch.uint8, device="cuda")
    work = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 16 == 0
    good = dict(x=x, out=out, OH=OH, OW=OW, filt=1, work=work, nbytes=nbytes)
    bad = {
        "B < 1": dict(good, B=0),
        "H < 1": dict(good, H=0),
        "H > 16384": dict(good, H=16385),
        "W < 1": dict(good, W=0),
        "W > 16384": dict(good, W=16385),
        "OH < 1": dict(good, OH=0),
        "OH > 16384": dict(good, OH=16385),
        "OW < 1": dict(good, OW=0),
        "OW > 16384": dict(good, OW=16385),
        "filter 0": dict(good, filt=0),
        "filter 3": dict(good, filt=3),
        "null input": dict(good, x=None, B=1, H=17, W=9),
        "null output": dict(good, out=None),
        "null workspace": dict(good, work=None),
        "misaligned workspace": dict(good, work=work[1:]),
        "workspace one byte short": dict(good, nbytes=nbytes - 1),
    }
    for name, kw in bad.items():
        src = kw.pop("x")
        with pytest.raises(SgicError):
            if src is None:
                from sgic_amd._lib import call
                call("sgic_resize_u8_batch", None, kw["B"], kw["H"], kw["W"], kw["out"], kw["OH"], kw["OW"], kw["filt"], kw["work"],
                     ctypes.c_size_t(kw["nbytes"]))
            else:
                _raw_call(src, **kw)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()), name
    _raw_call(**good)      # the same call with nothing wrong: Pillow's bytes
    assert np.array_equal(out.cpu().numpy()[0], rc.pillow(x.cpu().numpy()[0], OH, OW, "lanczos"))


def test_python_wrapper_refuses():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    from sgic_amd._lib import SgicError
    x = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.resize_u8(x, 2, 2, "bilinear")
    with pytest.raises(SgicError):
        ops.resize_u8(x, 0, 2)
    with pytest.raises(SgicError):
        ops.resize_u8(x, 2, 16385)


def test_geometry_helpers():
    import sgic_amd  # noqa: F401
    from sgic_amd.resize import max_side_size, reduced_size
    assert max_side_size(1, 16384, 100) == (1, 100)
    assert max_side_size(200, 300, 100) == (67, 100)
    assert max_side_size(90, 100, 100) == (90, 100)
    assert reduced_size(1000, 859, 4) == (250, 215)
    assert reduced_size(200, 300, 8) == (25, 38)
    x = rc.image("texture", 200, 300)      # the helpers feed the kernel: --max_side 100 of a 200 x 300 image
    oh, ow = max_side_size(200, 300, 100)
    assert np.array_equal(_resize(x, oh, ow, "lanczos")[0], rc.pillow(x, oh, ow, "lanczos"))
