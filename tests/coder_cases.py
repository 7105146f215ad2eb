"""The tables, messages and references of the rANS coder tests (csrc/entropy.hip: rans_encode_kernel, rans_decode_init_kernel,
rans_decode_kernel, sgic_cdf_table_create).  The C restatement of the reference coder (oracle/sgic_oracle.c through oracle.orc) is
the reference, for any table; tests/test_coder_cases_cpu.py holds it to every premise the GPU tests rest on.  No GPU, no torch."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import orc  # noqa: E402

DEC_WIN = 4096                # stream bytes rans_decode_kernel stages in LDS; later bytes come from global memory
ENC_CHUNK = 1024              # symbols per pass of rans_encode_kernel, walked from the end of the message
MAX_DEC_COLS = 128            # the decoder's lane-parallel probe: row[lane] and row[lane + 64]
LDS_BYTES = 160 * 1024


def dec_lds_bytes(rows, cols):
    """dynamic LDS of one decode launch: the table, the row sizes and offsets, the stream window"""
    return (rows * cols + 2 * rows) * 4 + DEC_WIN


def make_table(rows, cols, seed):
    """-> (cdf int32 [rows, cols], sizes int32 [rows], offsets int32 [rows]).  Row 0 has `cols` entries, the other rows 3..cols, the
    last row 3 (the least the table builder takes) so that every table of more than one row has such a row.  A row of `size` entries
    codes nb = size - 1 bins, the last of them the bypass sentinel.  The pmf kinds cycle by row: flat, spiky (many bins of frequency 1:
    the coder's freq < 2 branch), narrow Gaussian (frequency 1 in both tails).  Entries past a row's size are 0."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(3, cols + 1, rows).astype(np.int32)
    sizes[rows - 1] = 3
    sizes[0] = cols
    cdf = np.zeros((rows, cols), dtype=np.int32)
    for r in range(rows):
        nb = int(sizes[r]) - 1
        kind = r % 3
        if kind == 0:
            pmf = np.full(nb, 1.0 / nb)
        elif kind == 1:
            pmf = rng.random(nb) ** 8
        else:
            pmf = np.exp(-0.5 * ((np.arange(nb) - 0.5 * (nb - 1)) / max(0.5, nb / 24.0)) ** 2)
        cdf[r, :nb + 1] = orc.pmf_to_quantized_cdf((pmf / pmf.sum()).astype(np.float32), 16).astype(np.int32)
    offsets = (-((sizes - 1) // 2)).astype(np.int32)
    return cdf, sizes, offsets


def golden_table():
    t = np.load(os.path.join(ROOT, "tests", "golden", "cdf_table.npz"))
    return t["cdf"].astype(np.int32), t["cdf_length"].astype(np.int32).reshape(-1), t["offset"].astype(np.int32).reshape(-1)


SHAPES = {"1x3": (1, 3), "7x64": (7, 64), "7x65": (7, 65), "300x128": (300, 128), "5x129": (5, 129)}
TABLES = tuple(SHAPES) + ("golden",)
ENCODE_ONLY = ("5x129",)                                   # decode refuses cols > 128
DECODABLE = tuple(t for t in TABLES if t not in ENCODE_ONLY)
MADE = tuple(t for t in SHAPES if SHAPES[t][0] > 1)        # the made tables of more than one row
TOO_BIG_FOR_LDS = (320, 128)                               # the table builder takes it, decode refuses it


@functools.lru_cache(maxsize=None)
def table(name):
    """-> (cdf, sizes, offsets) of a name in TABLES; made once, read-only"""
    if name == "golden":
        t = golden_table()
    else:
        rows, cols = SHAPES[name]
        t = make_table(rows, cols, 1000 * rows + cols)
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def orc_table(name):
    return orc.Table(*table(name))


LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
SKIP_AT_CHUNK_ENDS = (1024, 1025, 2049)
EXTREMES = (-32768, 32767, -3000, 3000)
# (n, whether the entries at the encoder's chunk ends are skipped)
MESSAGE_CASES = tuple((n, False) for n in LENGTHS) + tuple((n, True) for n in SKIP_AT_CHUNK_ENDS)


def chunk_end_positions(n):
    return sorted(p for p in {0, 1023, 1024, n - 1} if 0 <= p < n)


def messages(tab, n, seed, skip_chunk_ends=False):
    """-> (sym int16 [n], idx int16 [n]) for tab = (cdf, sizes, offsets): idx from -1 (skipped) .. rows - 1, sym from +-40, every
    97th entry one of EXTREMES in turn (the bypass path at its longest)"""
    rows = tab[0].shape[0]
    rng = np.random.default_rng(seed)
    idx = rng.integers(-1, rows, n).astype(np.int16)
    sym = rng.integers(-40, 41, n).astype(np.int16)
    at = np.arange(96, n, 97)
    sym[at] = np.array(EXTREMES, dtype=np.int16)[np.arange(len(at)) % 4]
    if skip_chunk_ends:
        idx[chunk_end_positions(n)] = -1
    return sym, idx


def message_batch(name, n, skip_chunk_ends, B=3):
    """B messages of different seeds -> (sym [B, n], idx [B, n])"""
    pairs = [messages(table(name), n, 7919 * n + 31 * b + int(skip_chunk_ends), skip_chunk_ends) for b in range(B)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def odd_cut(n):
    """an odd symbol count inside 1..n, no multiple of the decoder's 64-symbol groups"""
    return min(n, (n // 3) | 1)


def coded_values(tab, sym, idx):
    """the bin each coded symbol lands in (sym - offset, folded onto the bypass bin outside 0..size-3) -> (values, rows) of the entries
    with idx >= 0"""
    _, sizes, offsets = tab
    keep = idx >= 0
    rows = idx[keep].astype(np.int64)
    v = sym[keep].astype(np.int64) - offsets[rows]
    mx = sizes[rows].astype(np.int64) - 2
    return np.where((v < 0) | (v >= mx), mx, v), rows


def expected(sym, idx):
    return np.where(idx < 0, 0, sym).astype(np.int16)


def stream(name, sym, idx):
    return orc.rans_encode(sym, idx, orc_table(name))


def oracle_decode(name, data, idx, cuts=()):
    """orc.Decoder over idx cut at `cuts` -> int16 [n]"""
    d = orc.Decoder(data, orc_table(name))
    edges = [0] + list(cuts) + [len(idx)]
    return np.concatenate([d.decode(idx[a:b]) for a, b in zip(edges[:-1], edges[1:])])


LONG_N = 20000


@functools.lru_cache(maxsize=None)
def long_case():
    """one golden-table message whose stream is several decoder windows long -> (sym, idx, stream bytes)"""
    rng = np.random.default_rng(0)
    sym = np.rint(rng.standard_normal(LONG_N) * 60).astype(np.int16)
    idx = np.full(LONG_N, 255, dtype=np.int16)
    sym.setflags(write=False)
    idx.setflags(write=False)
    return sym, idx, stream("golden", sym, idx)


SLOT_N = 600


@functools.lru_cache(maxsize=None)
def slot_case():
    """the message of the slot-size band -> (sym, idx, stream bytes), golden table"""
    sym, idx = messages(table("golden"), SLOT_N, 23)
    return sym, idx, stream("golden", sym, idx)


@functools.lru_cache(maxsize=None)
def bypass_heavy_case():
    """as long as slot_case(), every symbol coded and on the bypass path at its longest -> (sym, idx, stream bytes)"""
    sym = np.random.default_rng(4).choice(np.array([-30000, 30000], dtype=np.int16), SLOT_N)
    idx = np.abs(slot_case()[1])
    return sym, idx, stream("golden", sym, idx)


@functools.lru_cache(maxsize=None)
def cursor_case():
    """a golden-table message with every symbol coded, and its stream cut at two thirds -> (sym, idx, stream bytes, cut stream u8)"""
    sym, idx = messages(table("golden"), SLOT_N, 29)
    idx = np.abs(idx)
    data = stream("golden", sym, idx)
    return sym, idx, data, np.frombuffer(data, dtype=np.uint8)[: 2 * len(data) // 3].copy()
