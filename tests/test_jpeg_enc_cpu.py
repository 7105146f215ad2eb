"""CPU: the numpy restatement of baseline JPEG encoding (jpeg_enc_ref) writes Pillow's files byte for byte, and the host half of the
encoder (jpeg_enc.quant_tables / header / pick_quality) agrees with Pillow's files.  No GPU, no kernel."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_ref as ref  # noqa: E402


def test_restatement_equals_pillow_on_the_case_list():
    zrl = stuffed = 0
    for name, img, q, sub in ref.case_images():
        mine, stats = ref.encode(img, q, sub)
        assert mine == ref.pillow_bytes(img, q, sub), name
        zrl += stats["zrl"]
        stuffed += stats["stuffed"]
    # the list reaches the two rare paths of the entropy coder: runs of 16 zeros and byte stuffing
    assert zrl >= 1 and stuffed >= 1, (zrl, stuffed)


def test_restatement_dummy_rows_and_chroma_row_rule():
    # 8 x 8 at 4:2:0: chroma row 4 repeats row 3 (the mean of image rows 6 and 7), and three of the four luma blocks are dummies
    img = ref.image("noise", 8, 8, 5)
    _, cb, _ = ref.planes(img, 2)
    assert cb.shape == (8, 8) and (cb[4:] == cb[3]).all()
    assert ref.encode(img, 90, 2)[0] == ref.pillow_bytes(img, 90, 2)


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("q", [1, 5, 49, 50, 75, 95, 100])
def test_header_and_tables_equal_pillow(q, sub):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    img = ref.image("natural", 33, 47, 3)
    data = ref.pillow_bytes(img, q, sub)
    tables = jpeg_enc.quant_tables(q)
    assert tables.shape == (2, 64) and tables.dtype == np.uint16
    qt = Image.open(io.BytesIO(data)).quantization          # Pillow hands them out in natural order
    for i in range(2):
        assert [int(v) for v in tables[i]] == list(qt[i])
    assert (tables == ref.quant_tables(q)).all()
    head = jpeg_enc.header(33, 47, tables, sub)
    assert head == ref.header(33, 47, tables, sub)
    assert data[:len(head)] == head
    assert head[-14:-12] == b"\xff\xda"                   # the header ends with the SOS segment


def test_quant_tables_refuses_bad_quality():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    for q in (0, 101, -3):
        with pytest.raises(ValueError):
            jpeg_enc.quant_tables(q)


def test_pick_quality():
    import sgic_amd  # noqa: F401
    from sgic_amd.jpeg_enc import pick_quality
    # not monotone: q = 4 is smaller than q = 3 and fits; the rule looks at every entry
    assert pick_quality({1: 100, 2: 120, 3: 160, 4: 150, 5: 170}, 155) == (4, False)
    assert pick_quality({1: 100, 2: 120, 3: 90, 4: 150}, 95) == (3, False)
    assert pick_quality({1: 100, 2: 120, 3: 130}, 99) == (1, True)            # nothing fits
    assert pick_quality({1: 100, 2: 120, 3: 130}, 130) == (3, False)          # "not larger than": equality fits
    assert pick_quality({q: 10 * q for q in range(1, 96)}, 10 ** 6) == (95, False)   # everything fits
    assert pick_quality({3: 50, 7: 80}, 10) == (3, True)
    with pytest.raises(ValueError):
        pick_quality({}, 10)
