"""CPU: the C oracle alone satisfies every premise that tests/test_gpu_coder_tables.py rests on, so a red GPU test there can only be
the kernel: every table and message of tests/coder_cases.py round-trips through orc.rans_encode / orc.Decoder, the long stream is
longer than the decoder's LDS window, and the made tables have the bins, rows and symbols that the kernels' branches need."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coder_cases as cc  # noqa: E402
from oracle import orc  # noqa: E402


@pytest.mark.parametrize("name", cc.TABLES)
def test_tables_are_well_formed(name):
    cdf, sizes, offsets = cc.table(name)
    rows, cols = cdf.shape
    assert sizes.shape == offsets.shape == (rows,)
    assert sizes.min() >= 3 and sizes.max() == cols
    for r in range(rows):
        row = cdf[r, :sizes[r]]
        assert row[0] == 0 and row[-1] == 65536 and (np.diff(row) > 0).all(), r
    if name in cc.SHAPES:
        assert (rows, cols) == cc.SHAPES[name] and sizes[0] == cols
        assert np.array_equal(offsets, -((sizes - 1) // 2))


@pytest.mark.parametrize("name", cc.TABLES)
def test_oracle_round_trip_every_table_and_length(name):
    for n, skips in cc.MESSAGE_CASES:
        sym, idx = cc.message_batch(name, n, skips)
        for b in range(len(sym)):
            data = cc.stream(name, sym[b], idx[b])
            assert len(data) >= 5 and data[0] == 1
            got = cc.oracle_decode(name, data, idx[b], cuts=(cc.odd_cut(n),))
            assert np.array_equal(got, cc.expected(sym[b], idx[b])), (n, skips, b)
            assert np.array_equal(got, cc.oracle_decode(name, data, idx[b])), (n, skips, b)


def test_messages_hold_the_extremes_and_the_skips():
    tab = cc.table("golden")
    sym, idx = cc.messages(tab, 5000, 3)
    assert idx.min() == -1 and idx.max() == 255 and sym.dtype == idx.dtype == np.int16
    for v in cc.EXTREMES:
        assert ((sym == v) & (idx >= 0)).any(), v          # coded, not skipped
    assert np.abs(np.delete(sym, np.arange(96, 5000, 97))).max() == 40
    assert cc.chunk_end_positions(1024) == [0, 1023] and cc.chunk_end_positions(1025) == [0, 1023, 1024]
    assert cc.chunk_end_positions(2049) == [0, 1023, 1024, 2048]
    for n in cc.SKIP_AT_CHUNK_ENDS:
        _, idx = cc.message_batch("golden", n, True)
        assert (idx[:, cc.chunk_end_positions(n)] == -1).all()
        # without the variant those entries are (mostly) coded: the variant changes something
        assert (cc.message_batch("golden", n, False)[1][:, cc.chunk_end_positions(n)] >= 0).any()
    for n in cc.LENGTHS:
        assert 1 <= cc.odd_cut(n) <= n and (cc.odd_cut(n) % 2 == 1)
        assert n < 64 or cc.odd_cut(n) % 64 != 0


def test_long_stream_leaves_the_lds_window():
    sym, idx, data = cc.long_case()
    assert len(sym) == cc.LONG_N == 20000
    assert len(data) > 4 * cc.DEC_WIN
    assert np.array_equal(cc.oracle_decode("golden", data, idx), sym)
    assert np.array_equal(cc.oracle_decode("golden", data, idx, cuts=(6667, 13331)), sym)


def test_slot_and_cursor_cases():
    sym, idx, data = cc.slot_case()
    need = len(data)
    assert len(sym) == 600 and max(64, need - 8) == need - 8          # the band need - 8 .. need + 64 is all above the least slot
    assert np.array_equal(cc.oracle_decode("golden", data, idx), cc.expected(sym, idx))
    sym0, idx0, long0 = cc.bypass_heavy_case()
    assert (idx0 >= 0).all() and len(long0) > need + 48 + 600         # it cannot fit the slot that the other just fits
    sym, idx, data, cut = cc.cursor_case()
    assert (idx >= 0).all() and len(cut) == 2 * len(data) // 3 and cut.tobytes() == data[:len(cut)]
    k = cc.odd_cut(len(sym))
    d = orc.Decoder(cut.tobytes(), cc.orc_table("golden"))
    assert np.array_equal(d.decode(idx[:k]), sym[:k])                 # a third of the symbols is within two thirds of the bytes
    with pytest.raises(ValueError):
        d.decode(idx[k:])                                             # the rest is not: the oracle flags the over-read
    assert idx[77] >= 0 and sym[77:].any()
    for short in range(5):                                            # no room for the flag byte and the 4 bytes of state
        with pytest.raises(ValueError):
            orc.Decoder(data[:short], cc.orc_table("golden"))
    with pytest.raises(ValueError):
        orc.Decoder(bytes([0x11, 0, 0, 0x80, 0]), cc.orc_table("golden"))


@pytest.mark.parametrize("name", cc.MADE)
def test_made_tables_have_frequency_one_and_a_row_of_three(name):
    cdf, sizes, _ = cc.table(name)
    assert (sizes == 3).any()
    freq1 = [r for r in range(len(sizes)) if (np.diff(cdf[r, :sizes[r]]) == 1).any()]
    assert freq1
    # and the messages code such bins, so the freq < 2 branch of the encoder runs
    sym, idx = cc.message_batch(name, 5000, False)
    hit = False
    for b in range(len(sym)):
        v, rows = cc.coded_values(cc.table(name), sym[b], idx[b])
        hit = hit or bool((cdf[rows, v + 1] - cdf[rows, v] == 1).any())
    assert hit


def test_decodable_tables_fit_the_documented_lds_bound():
    for name in cc.DECODABLE:
        rows, cols = cc.table(name)[0].shape
        assert cols <= cc.MAX_DEC_COLS and cc.dec_lds_bytes(rows, cols) <= cc.LDS_BYTES, name
    assert (300 * 128 + 2 * 300) * 4 + 4096 <= 160 * 1024
    rows, cols = cc.TOO_BIG_FOR_LDS
    assert cols <= cc.MAX_DEC_COLS and cc.dec_lds_bytes(rows, cols) > cc.LDS_BYTES
    for name in cc.ENCODE_ONLY:
        assert cc.table(name)[0].shape[1] > cc.MAX_DEC_COLS
    # the tables differ in LDS size, the golden one being the largest but one: what the alternation test needs
    assert cc.dec_lds_bytes(1, 3) < cc.dec_lds_bytes(7, 64) < cc.dec_lds_bytes(256, 103)


@pytest.mark.parametrize("n", cc.LENGTHS[1:])
def test_7x65_messages_use_the_one_entry_of_the_second_register(n):
    """a row of 65 entries: the decoder's probe holds row[64] alone in v1, read as `end` of bin 63 (the bypass bin of that row)"""
    tab = cc.table("7x65")
    sym, idx = cc.message_batch("7x65", n, False)
    full = np.flatnonzero(tab[1] == 65)
    assert 0 in full
    hit = 0
    for b in range(len(sym)):
        v, rows = cc.coded_values(tab, sym[b], idx[b])
        hit += int(((v == 63) & np.isin(rows, full)).sum())
    assert hit > 0


def test_7x64_rows_stay_in_the_first_register():
    assert cc.table("7x64")[1].max() == 64 and cc.table("300x128")[1].max() == 128 and cc.table("1x3")[1].tolist() == [3]
