"""CPU: sgic_gemm_split3_plan -- the host-only function the split GEMM's dispatcher itself runs to turn (M, N, convolution?, launch
mode) into launches: the first launch's tile, the row at which a second launch starts (0: none) and that launch's mode.
Mode 26 takes ONE launch of 160x256 tiles when the product is not a convolution, 128x256 tiles need more than one round of the
256 CUs and 160x256 tiles fit in one; everything else keeps the plan it had: whole rounds of 128x256 tiles + a ring-kernel tail."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "searchable-generative-image-compression_amd", "libsgic.so"))
    fn = lib.sgic_gemm_split3_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)] * 4

    def run(M, N, mode, conv=0):
        out = [ctypes.c_int(-1) for _ in range(4)]
        rc = fn(M, N, conv, mode, *[ctypes.byref(o) for o in out])
        assert rc == 0, rc
        return tuple(o.value for o in out)      # tile_m, tile_n, split_row, tail_mode
    return run


def _workgroups(M, N, tm, tn):
    return -(-M // tm), -(-N // tn)


def test_mode26_takes_one_round_of_160x256_tiles(plan):
    tm, tn, split, tail = plan(9248, 1024, 26)
    assert (tm, tn, split, tail) == (160, 256, 0, 0)
    assert _workgroups(9248, 1024, tm, tn) == (58, 4)              # 232 workgroups: one round
    tm, tn, split, tail = plan(12000, 768, 26)
    assert (tm, tn, split, tail) == (160, 256, 0, 0)
    assert _workgroups(12000, 768, tm, tn) == (75, 3)              # 225 workgroups


def test_mode26_keeps_the_two_launch_plan_where_160_rows_do_not_fit_one_round(plan):
    # 116 x 4 = 464 tiles of 160x256: more than a round -> 128 row tiles x 4 = two whole rounds of 128x256, then the ring kernel's 80x64 tiles
    assert plan(18496, 1024, 26) == (128, 256, 16384, 23)
    # 63 x 12 = 756 tiles of 128x256: two whole rounds are 42 row tiles (504 tiles), split at row 42 x 128
    assert plan(8000, 3072, 26) == (128, 256, 5376, 23)
    # 64 x 12 = 768 tiles are three rounds exactly: there is no remainder, one launch of 128x256 (and 52 x 12 tiles of 160x256 are no single round)
    assert plan(8192, 3072, 26) == (128, 256, 0, 0)


def test_a_convolution_is_unchanged(plan):
    # 9248 output pixels x 1024 channels as a convolution: never split into two launches, and never the 160-row tile by policy
    assert plan(9248, 1024, 26, conv=1) == (128, 256, 0, 0)
    assert plan(9248, 1024, 27, conv=1) == (128, 256, 0, 0)


def test_mode27_keeps_the_two_launch_plan(plan):
    assert plan(9248, 1024, 27) == (128, 256, 8192, 23)           # 64 row tiles x 4 = one whole round, 1 056 rows to the ring tail
    assert plan(12000, 768, 27) == (128, 256, 10880, 23)


def test_other_modes(plan):
    assert plan(9248, 1024, 32) == (160, 256, 0, 0)
    assert plan(9248, 1024, 1) == (128, 256, 0, 0)
    assert plan(8192, 768, 28) == (128, 192, 0, 0)
    assert plan(12000, 768, 6) == (128, 256, 10880, 5)            # modes 6 / 8: the same split, 64x128 / 32x32 tiles for the rest
    assert plan(12000, 768, 8) == (128, 256, 10880, 4)
    assert plan(18496, 1024, 31) == (256, 256, 16384, 1)          # 73 x 4 tiles of 256x256: one whole round is 64 row tiles
    assert plan(9248, 1024, 31) == (256, 256, 0, 0)               # 37 x 4 tiles: not one whole round, a single launch
    assert plan(64, 64, 0)[:2] == (32, 32) and plan(16384, 4096, 0)[:2] == (128, 256)
