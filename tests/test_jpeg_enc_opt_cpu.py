"""CPU: the numpy restatement of JPEG encoding with optimised Huffman tables (jpeg_enc_opt_ref) writes the files of Pillow's
save(optimize=True) byte for byte, the length limiter included, and jpeg_enc.header takes the image's own tables.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_opt_ref as oref  # noqa: E402
import jpeg_enc_ref as ref  # noqa: E402


def test_restatement_equals_pillow_on_the_case_list():
    longest = 0
    for name, img, q, sub in ref.case_images():
        mine, info = oref.encode(img, q, sub)
        assert mine == oref.pillow_bytes(img, q, sub), name
        assert len(mine) <= len(ref.pillow_bytes(img, q, sub)), name
        longest = max(longest, info["longest"])
    assert longest <= 16          # the list never reaches the limiter; the next test does


def test_restatement_equals_pillow_on_the_limiter_case():
    img = ref.image("natural", 256, 256, 5)
    mine, info = oref.encode(img, 100, 2)
    assert info["longest"] > 16, "the case no longer reaches the length limiter"
    assert mine == oref.pillow_bytes(img, 100, 2)


def test_optimal_table_ties_limiter_and_single_symbol():
    # one symbol: it shares size 1 with the pseudo-symbol, which then leaves
    bits, vals, longest = oref.optimal_table([0] * 7 + [5] + [0] * 248)
    assert bits == [1] + [0] * 15 and vals == [7] and longest == 1
    # equal counts: the pseudo-symbol and the larger symbols merge first; four leaves of size 2, and the pseudo-symbol leaves
    bits, vals, _ = oref.optimal_table([1, 1, 1] + [0] * 253)
    assert bits == [0, 3] + [0] * 14 and vals == [0, 1, 2]
    # Fibonacci counts make a chain deeper than 16; the limited counts still satisfy Kraft with the pseudo-symbol's slot
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    bits, vals, longest = oref.optimal_table(fib[::-1] + [0] * (256 - len(fib)))
    assert longest > 16 and sum(bits) == len(vals) == 24
    assert sum(n << (16 - ln) for ln, n in enumerate(bits, 1)) < 1 << 16
    assert vals[0] == 0 and sorted(vals) == list(range(24))


@pytest.mark.parametrize("q,sub", [(1, 2), (30, 1), (75, 0), (100, 2)])
def test_header_takes_the_images_tables(q, sub):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    img = ref.image("natural", 33, 47, 3)
    data = oref.pillow_bytes(img, q, sub)
    _, info = oref.encode(img, q, sub)
    tables = jpeg_enc.quant_tables(q)
    head = jpeg_enc.header(33, 47, tables, sub, huffman=info["huffman"])
    assert head == oref.header(33, 47, tables, sub, info["huffman"])
    assert data[:len(head)] == head and head[-14:-12] == b"\xff\xda"
    assert len(head) == len(jpeg_enc.header(33, 47, tables, sub)) - 432 + 4 * 21 + sum(len(v) for _, v in info["huffman"])
    # without huffman: today's bytes
    assert jpeg_enc.header(33, 47, tables, sub) == ref.header(33, 47, tables, sub) == jpeg_enc.header(33, 47, tables, sub, None)
    with pytest.raises(ValueError):
        jpeg_enc.header(33, 47, tables, sub, huffman=info["huffman"][:3])
