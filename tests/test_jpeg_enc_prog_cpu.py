"""CPU: the numpy restatement of progressive JPEG encoding (tests/jpeg_enc_prog_ref.py) writes Pillow's progressive=True files byte
for byte, and the package's framing (sgic_amd.jpeg_enc.progressive_file) is Pillow's.  The GPU encoder is compared with both in
test_gpu_jpeg_enc_prog.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_prog_ref as pref  # noqa: E402
import jpeg_enc_ref as ref  # noqa: E402


def test_case_list_equals_pillow():
    cases = ref.case_images()
    assert len(cases) == 52
    for name, img, q, sub in cases:
        assert pref.encode(img, q, sub)[0] == pref.pillow_bytes(img, q, sub), name


def test_optimize_changes_nothing():
    img = ref.image("natural", 33, 47, 3)
    assert pref.pillow_bytes(img, 85, 2, optimize=True) == pref.pillow_bytes(img, 85, 2)


@pytest.mark.parametrize("h,w,q,sub,flushes", [(128, 128, 100, 0, 17), (128, 128, 95, 2, None), (40, 128, 100, 0, None)])
def test_correction_bit_flush(h, w, q, sub, flushes):
    """the tiled image fills libjpeg's correction-bit buffer: in the last luma scan a run is cut before it ends"""
    img = pref.tiled(h, w)
    got, info = pref.encode(img, q, sub)
    assert got == pref.pillow_bytes(img, q, sub)
    forced = [pref.forced_flushes(info["events"][scan]) for scan in (5, 9)]      # the two luma refinement scans
    assert sum(forced) > 0
    if flushes is not None:           # no block of the last scan codes a symbol: one run of 256 blocks, cut 17 times
        assert forced[1] == flushes and pref.eobrun_counts(info["events"][9])[::2] == (flushes + 1, 0)


@pytest.mark.parametrize("column", [None, 8, 320])
def test_eobrun_limit(column):
    """32 942 blocks per component.  Flat: one run per AC scan, split at 0x7FFF.  A textured block at raster index 32 761: the run
    in front of it stays whole.  At 32 800: the run is split and its rest of 33 blocks ends at the textured block."""
    img = pref.flat_large(column)
    got, info = pref.encode(img, 75, 0)
    assert got == pref.pillow_bytes(img, 75, 0)
    for scan in (1, 2, 3, 4, 5, 7, 8, 9):
        ev = info["events"][scan]
        runs, largest, coded = pref.eobrun_counts(ev)
        if column is None:
            assert (runs, largest, coded) == (2, 0x7FFF, 0), scan
        elif column == 8:
            assert (runs, largest) == (2, 32761) and coded > 0, scan
        else:
            assert pref.eobrun_values(ev)[:2] == [0x7FFF, 33] and runs == 3 and coded > 0, scan


def test_package_framing_is_pillows():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    assert [tuple(s) for s in jpeg_enc.PROGRESSION] == [tuple(s) for s in pref.SCRIPT]
    for sub, (h, w, q) in enumerate([(37, 53, 90), (40, 72, 60), (48, 64, 75)]):
        img = ref.image("natural", h, w, 20 + sub)
        want = pref.pillow_bytes(img, q, sub)
        tables = ref.quant_tables(q)
        assert (jpeg_enc.quant_tables(q) == tables).all()
        head = jpeg_enc._header_front(h, w, tables, sub, sof=0xC2)
        assert head == pref.front(h, w, tables, sub) and want[:len(head)] == head
        _, info = pref.encode(img, q, sub)
        huffman = [(pl[1:17], pl[17:]) for scan in info["dht"] for pl in scan]
        assert jpeg_enc.progressive_file(h, w, tables, sub, huffman, info["segments"]) == want
        with pytest.raises(ValueError):
            jpeg_enc.progressive_file(h, w, tables, sub, huffman[:9], info["segments"])


def test_limits_blocks_and_slot_bytes():
    """two limits: 2 675 992 coded blocks (32-bit bit offsets in the largest scan) and a slot of at most 2^31 - 1 bytes (d_len and
    cap are 31-bit).  The first binds at 4:4:4, the second at 4:2:2 and 4:2:0; every accepted shape has a cap the batch call takes"""
    import ctypes
    import sgic_amd  # noqa: F401
    from sgic_amd._lib import lib
    out = ctypes.c_size_t(0)

    def cap(h, w, sub):
        out.value = 0
        return lib.sgic_jpeg_encode_prog_cap(h, w, sub, ctypes.byref(out)), out.value

    def work(h, w, sub):
        return lib.sgic_jpeg_encode_prog_work_bytes(1, h, w, sub, ctypes.byref(out))

    # (subsampling, the largest accepted width at this height, MCU width in pixels, coded blocks there)
    for sub, h, w, step, blocks in [(0, 7552, 7552, 8, 944 * 944 * 3), (1, 10240, 8032, 16, 1280 * 502 * 4), (2, 10240, 10144, 16, 640 * 634 * 6)]:
        rc, c = cap(h, w, sub)
        assert rc == 0 and c <= 0x7FFFFFFF and blocks <= 2675992 and work(h, w, sub) == 0, (sub, c)
        assert cap(h, w + step, sub)[0] == -1 and work(h, w + step, sub) == -1, sub
    assert (944 * 945 * 3 > 2675992)                                   # 4:4:4: the next MCU column passes the block limit
    assert 640 * 635 * 6 <= 2675992 and 1280 * 503 * 4 <= 2675992        # 4:2:0, 4:2:2: it passes only the slot limit
    assert cap(10240, 10240, 2)[0] == -1                               # 2 457 600 blocks, but a slot of 2 166 374 720 bytes
