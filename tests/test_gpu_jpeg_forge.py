"""GPU JPEG decode (csrc/jpeg.hip) on forged files Pillow does not write (tests/jpeg_forge.py): unusual layouts through both
kernels' paths, one batch of differing layouts, and the short scans the kernels must report (error code 3).  The expected pixels are
the installed Pillow's; the bar is equality of every u8 sample.  Files the parsers refuse never reach a kernel
(tests/test_jpeg_forge_cpu.py ends those at the parser)."""
import io
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_forge  # noqa: E402

pytestmark = pytest.mark.gpu


def _pillow(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


_ids = lambda v: v if isinstance(v, str) and len(v) < 60 else ""
BOTH = [(n, d) for n, d, e in jpeg_forge.unusual_cases() if e == "both"]
SCANS = [(n, d) for n, d, e in jpeg_forge.unusual_cases() if e in ("both", "scans_only")]


def _same(got, ref, what):
    assert got.shape == ref.shape, what
    bad = int((got != ref).sum())
    assert bad == 0, f"{what}: {bad} of {ref.size} samples differ (max {np.abs(got.astype(int) - ref.astype(int)).max()})"


@pytest.mark.parametrize("name,data", BOTH, ids=_ids)
def test_unusual_files_through_the_baseline_kernel(name, data):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    b = J.JpegBatch([data])
    _same(b.decode("cuda:0").cpu().numpy()[0], _pillow(data), name)
    assert b.last_err.cpu().tolist() == [0]


@pytest.mark.parametrize("name,data", SCANS, ids=_ids)
def test_unusual_files_through_the_scan_kernel(name, data):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    b = J.ScanJpegBatch([data])
    _same(b.decode("cuda:0").cpu().numpy()[0], _pillow(data), name)
    assert b.last_err.cpu().tolist() == [0]


def test_one_batch_of_differing_layouts():
    """eight 40x56 files -- 4:4:0, 4:2:0, 4:4:4 with 16-bit tables, table ids 2 and 3, grey declared 2x2, restart interval 1, odd
    component ids, Adobe transform 1 -- in ONE launch: image b is Pillow's image b (per-image tables, offsets and layouts)"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    cases = jpeg_forge.layout_batch()
    assert len(cases) == 8
    datas = [d for _, d in cases]
    for batch in (J.JpegBatch(datas), J.ScanJpegBatch(datas)):
        got = batch.decode("cuda:0").cpu().numpy()
        for i, (name, d) in enumerate(cases):
            _same(got[i], _pillow(d), f"{type(batch).__name__} image {i} ({name})")


@pytest.mark.parametrize("name,data", [(n, d) for n, d, e in jpeg_forge.malformed_cases() if e == "decode_error"], ids=_ids)
def test_short_scan_is_reported_with_code_3(name, data):
    """a scan that ends before its last MCU (inside the batch's zero-padded blob: every read is in bounds) sets error code 3 for its
    image only; the good image of the batch is Pillow's; the default check=True raises"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    good = jpeg_forge.forged(40, 56, jpeg_forge.S444)
    for cls in (J.JpegBatch, J.ScanJpegBatch):
        b = cls([good, data])
        out = b.decode("cuda:0", check=False)
        assert b.last_err.cpu().tolist() == [0, 3], cls.__name__
        _same(out[0].cpu().numpy(), _pillow(good), cls.__name__)
        with pytest.raises(RuntimeError):
            b.decode("cuda:0")
