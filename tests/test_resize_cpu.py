"""CPU: the host side of the u8 resize: the two geometry rules, the tables the library makes on the host against a numpy restatement
of Pillow's precompute_coeffs (and, through the restated passes, against Pillow's bytes), and the clamp coverage of the case list."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as rc  # noqa: E402


def test_reduced_size():
    import sgic_amd  # noqa: F401
    from sgic_amd.resize import reduced_size
    assert reduced_size(1000, 859, 1) == (1000, 859)
    assert reduced_size(1000, 859, 4) == (250, 215)
    assert reduced_size(1000, 859, 3) == (334, 287)
    assert reduced_size(256, 256, 3) == (86, 86)
    assert reduced_size(200, 300, 6) == (34, 50)
    assert reduced_size(200, 300, 8) == (25, 38)
    assert reduced_size(5, 3, 16) == (1, 1)
    with pytest.raises(ValueError):
        reduced_size(5, 3, 0)


def test_max_side_size():
    import sgic_amd  # noqa: F401
    from sgic_amd.resize import max_side_size
    assert max_side_size(200, 300, 300) == (200, 300)
    assert max_side_size(200, 300, 1000) == (200, 300)
    assert max_side_size(200, 300, 100) == (67, 100)          # 66.67 rounds up
    assert max_side_size(300, 200, 100) == (100, 67)
    assert max_side_size(256, 256, 100) == (100, 100)
    assert max_side_size(1000, 859, 500) == (500, 430)        # 429.5 rounds half up
    assert max_side_size(1, 16384, 100) == (1, 100)           # 0.006 would round to 0: at least 1
    assert max_side_size(16384, 1, 100) == (100, 1)
    assert max_side_size(3, 5, 1) == (1, 1)
    with pytest.raises(ValueError):
        max_side_size(3, 5, 0)


@pytest.mark.parametrize("filt", rc.FILTERS)
def test_checkerboard_covers_both_clamps(filt):
    rc.clamp_case(filt)


def _axes():
    seen = []
    for h, w, oh, ow, f in rc.CASES:
        for a in ((w, ow, f), (h, oh, f)):
            if a not in seen:
                seen.append(a)
    return seen


@pytest.mark.parametrize("axis", _axes(), ids=lambda a: f"{a[0]}-{a[1]}-{a[2]}")
def test_host_tables_equal_the_restatement(axis):
    """every axis of the case list: the tables the resize call makes on the host are the restatement's, entry for entry"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    n_in, n_out, filt = axis
    bounds, kk = ops.resize_u8_coeffs(n_in, n_out, filt)
    want_b, want_k = rc.coeffs(n_in, n_out, filt)
    assert np.array_equal(bounds, want_b)
    assert kk.shape == want_k.shape and np.array_equal(kk, want_k)


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[0] * c[1] <= 300 * 300], ids=rc.case_id)
def test_host_tables_give_pillows_bytes(case):
    """the library's tables through the restated passes equal Pillow's resize: the definition the GPU kernels are held to"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    H, W, OH, OW, filt = case
    tables = (ops.resize_u8_coeffs(W, OW, filt), ops.resize_u8_coeffs(H, OH, filt))
    for kind in rc.KINDS:
        x = rc.image(kind, H, W)
        got, _, _ = rc.restated(x, OH, OW, filt, tables)
        assert np.array_equal(got, rc.pillow(x, OH, OW, filt)), kind


def test_table_refusals():
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    from sgic_amd._lib import SgicError, lib
    with pytest.raises(SgicError):
        ops.resize_u8_coeffs(16385, 4, "lanczos")
    assert lib.sgic_resize_u8_work_bytes(1, 8, 8, 4, 4, 1) > 0
    for bad in ((0, 8, 8, 4, 4, 1), (1, 0, 8, 4, 4, 1), (1, 8, 16385, 4, 4, 2), (1, 8, 8, 0, 4, 2), (1, 8, 8, 4, 16385, 1),
                (1, 8, 8, 4, 4, 0), (1, 8, 8, 4, 4, 3)):
        assert lib.sgic_resize_u8_work_bytes(*bad) == 0, bad
