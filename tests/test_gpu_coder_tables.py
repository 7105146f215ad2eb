"""GPU: the rANS kernels of csrc/entropy.hip against the C oracle over the tables and messages of tests/coder_cases.py: other table
shapes than the codec's 256 x 103, every encoder chunk edge, streams longer than the decoder's LDS window, tables of different size in
turn, the band of slot sizes around the exact stream size, and the cursor's error state.  Every comparison is equality of bytes or
integers with oracle.orc; tests/test_coder_cases_cpu.py holds the oracle to the premises."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coder_cases as cc  # noqa: E402
from oracle import orc  # noqa: E402

pytestmark = pytest.mark.gpu

SGIC_EINVAL, SGIC_ENOSPC = -1, -3
PAD = 7                       # idx_stride = out_stride = n + PAD
BAD_IDX = 300                 # fills the padding of the index rows: past every table here, so reading it would set err = 3
FILL = 0x5A5A                 # fills the decode output before a call


def _torch():
    import torch
    import sgic_amd  # noqa: F401
    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a)).cuda()         # a copy: the case list's arrays are read-only


def _rc(name, *args):
    """the C ABI's return code itself (sgic_amd._lib.call raises on any non-zero one); args: tensors, None, ints, table handles"""
    torch = _torch()
    from sgic_amd import _lib
    conv = [_lib.ptr(a) if a is None or isinstance(a, torch.Tensor) else _lib.c_int(a) if isinstance(a, int) else a for a in args]
    return getattr(_lib.lib, name)(*conv, _lib.stream())


@pytest.fixture(scope="module")
def tables():
    """name -> handle of every table of the case list, and of the one that is too big for the decoder's LDS"""
    _torch()
    from sgic_amd.entropy.MLCodec_rans import _Tables
    T = _Tables()
    h = {name: T.handles[T.add(*cc.table(name))] for name in cc.TABLES}
    rows, cols = cc.TOO_BIG_FOR_LDS
    h["too big"] = T.handles[T.add(*cc.make_table(rows, cols, 5))]     # sgic_cdf_table_create takes it
    yield h
    T.clear()


class Encoded:
    """sgic_rans_encode_batch of sym, idx [B, n] into B slots of `cap` bytes that start `guard` bytes into a buffer filled with
    0xA5, with `guard` more bytes behind the last slot"""

    def __init__(self, handle, sym, idx, cap, guard=0):
        torch = _torch()
        from sgic_amd._lib import call
        self.B, self.n = sym.shape
        self.cap, self.guard = cap, guard
        self.buf = torch.full((guard + self.B * cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out = self.buf[guard:]
        self.meta = torch.full((3, self.B), -77, dtype=torch.int32, device="cuda")
        self.d_off, self.d_len = self.meta[0], self.meta[1]
        call("sgic_rans_encode_batch", handle, _dev(sym), _dev(idx), self.B, self.n, self.out, cap, self.meta[0], self.meta[1], self.meta[2])
        self.off, self.len, self.err = self.meta.cpu().numpy()
        self.bytes = self.buf.cpu().numpy()

    def slot(self, b):
        return self.bytes[self.guard + b * self.cap: self.guard + (b + 1) * self.cap]

    def stream(self, b):
        return self.slot(b)[self.off[b]: self.off[b] + self.len[b]].tobytes()

    def guards_intact(self):
        g = self.guard
        return bool((self.bytes[:g] == 0xA5).all() and (self.bytes[len(self.bytes) - g:] == 0xA5).all())


class Decoding:
    """a decode cursor over B streams in (B, cap) device memory; idx and out rows are n + PAD apart, the padding of idx holds BAD_IDX
    and the whole of out FILL"""

    def __init__(self, streams, cap, d_off, d_len, idx):
        torch = _torch()
        from sgic_amd._lib import call
        self.streams, self.cap, self.d_off, self.d_len = streams, cap, d_off, d_len
        self.B, self.n = idx.shape
        self.stride = self.n + PAD
        padded = np.full((self.B, self.stride), BAD_IDX, dtype=np.int16)
        padded[:, :self.n] = idx
        self.d_idx = _dev(padded)
        self.d_out = torch.full((self.B, self.stride), FILL, dtype=torch.int16, device="cuda")
        self.d_state = torch.full((self.B, 4), -1, dtype=torch.int32, device="cuda")
        call("sgic_rans_decode_init_batch", streams, cap, d_off, d_len, self.B, self.d_state)
        self.done = 0

    def rc(self, handle, count):
        """one sgic_rans_decode_batch of the next `count` symbols of every image -> its return code"""
        a = self.done
        assert a + count <= self.n
        rc = _rc("sgic_rans_decode_batch", handle, self.streams, self.cap, self.d_off, self.d_len, self.B, self.d_state,
                 self.d_idx.view(-1)[a:], count, self.stride, self.d_out.view(-1)[a:], self.stride)
        if rc == 0:
            self.done += count
        return rc

    def run(self, handle, cuts=()):
        edges = [0] + list(cuts) + [self.n]
        for a, b in zip(edges[:-1], edges[1:]):
            assert self.rc(handle, b - a) == 0
        return self

    @property
    def state(self):
        return self.d_state.cpu().numpy()

    @property
    def out(self):
        return self.d_out.cpu().numpy()


@pytest.mark.parametrize("name", cc.TABLES)
def test_encode_decode_every_table_and_length(name, tables):
    h = tables[name]
    for n, skips in cc.MESSAGE_CASES:
        sym, idx = cc.message_batch(name, n, skips)
        enc = Encoded(h, sym, idx, 16 * n + 64)
        assert enc.err.tolist() == [0, 0, 0], (n, skips)
        want = [cc.stream(name, sym[b], idx[b]) for b in range(3)]
        for b in range(3):
            assert enc.stream(b) == want[b], (n, skips, b)
            assert enc.off[b] + enc.len[b] == enc.cap
        dec = Decoding(enc.out, enc.cap, enc.d_off, enc.d_len, idx)
        if name in cc.ENCODE_ONLY:
            before = dec.state
            assert dec.rc(h, n) == SGIC_EINVAL
            assert (dec.out == FILL).all() and np.array_equal(dec.state, before)
            continue
        k = cc.odd_cut(n)
        dec.run(h, cuts=(k,))
        out, state = dec.out, dec.state
        for b in range(3):
            assert np.array_equal(out[b, :n], cc.oracle_decode(name, want[b], idx[b], cuts=(k,))), (n, skips, b)
            assert np.array_equal(out[b, :n], cc.expected(sym[b], idx[b]))
        assert (out[:, n:] == FILL).all()
        assert (state[:, 2] == 0).all(), (n, skips, state)


def test_table_too_big_for_the_lds_is_refused_by_decode_alone(tables):
    name = "golden"                                        # any valid streams: the refusal comes before a launch
    sym, idx = cc.message_batch(name, 64, False)
    enc = Encoded(tables[name], sym, idx, 16 * 64 + 64)
    dec = Decoding(enc.out, enc.cap, enc.d_off, enc.d_len, idx)
    before = dec.state
    assert dec.rc(tables["too big"], 64) == SGIC_EINVAL
    assert (dec.out == FILL).all() and np.array_equal(dec.state, before)
    dec.run(tables[name])                                  # the same cursor with the right table: untouched by the refusal
    assert np.array_equal(dec.out[:, :64], cc.expected(sym, idx))


def test_decode_past_the_lds_window(tables):
    sym, idx, want = cc.long_case()
    h = tables["golden"]
    enc = Encoded(h, sym[None], idx[None], 2 * cc.LONG_N + 64)
    assert enc.err.tolist() == [0] and enc.stream(0) == want
    assert len(want) > 4 * cc.DEC_WIN
    for cuts in ((), (6667, 13331)):                       # 6667 = 104 * 64 + 11, 13331 - 6667 = 104 * 64 + 8
        assert all(c % 64 for c in np.diff((0,) + cuts))
        dec = Decoding(enc.out, enc.cap, enc.d_off, enc.d_len, idx[None]).run(h, cuts)
        assert np.array_equal(dec.out[0, :cc.LONG_N], cc.oracle_decode("golden", want, idx, cuts)), cuts
        assert np.array_equal(dec.out[0, :cc.LONG_N], sym)
        assert dec.state[0, 2] == 0 and dec.state[0, 1] == len(want), (cuts, dec.state)


ALTERNATION = ("golden", "1x3", "golden", "7x64", "golden")


def test_tables_of_different_size_alternate():
    """the decoder's dynamic LDS depends on the table; one process decodes with a large table, a small one and the large one again.
    Tables of its own, so that what other tests did with theirs does not decide this one"""
    _torch()
    from sgic_amd.entropy.MLCodec_rans import RansDecoder, _Tables
    n = 1000
    msgs = {}
    for name in set(ALTERNATION):
        sym, idx = cc.messages(cc.table(name), n, 17)
        msgs[name] = (sym, idx, cc.stream(name, sym, idx))
    # the facade: one decoder, one cdf group per table
    dec = RansDecoder(1)
    group = {name: dec.add_cdf(*cc.table(name)) for name in sorted(set(ALTERNATION))}
    for step, name in enumerate(ALTERNATION):
        sym, idx, data = msgs[name]
        dec.set_stream(np.frombuffer(data, dtype=np.uint8))
        got = np.concatenate([dec.decode_stream(idx[:333], group[name]), dec.decode_stream(idx[333:], group[name])])
        assert np.array_equal(got, cc.oracle_decode(name, data, idx, cuts=(333,))), (step, name)
    # the C ABI: fresh handles
    T = _Tables()
    handle = {name: T.handles[T.add(*cc.table(name))] for name in sorted(set(ALTERNATION))}
    for step, name in enumerate(ALTERNATION):
        sym, idx, data = msgs[name]
        streams = _dev(np.frombuffer(data, dtype=np.uint8))
        d_len = _dev(np.array([len(data)], dtype=np.int32))
        d = Decoding(streams, len(data), None, d_len, idx[None])
        assert d.rc(handle[name], n) == 0, (step, name)
        assert np.array_equal(d.out[0, :n], cc.expected(sym, idx)), (step, name)
        assert d.state[0, 2] == 0 and d.state[0, 1] == len(data)
    T.clear()


def test_slot_bound_band(tables):
    """the encoder gives up (SGIC_ENOSPC) when fewer than 48 bytes of the slot are left before a symbol, and a stream ends with 5
    bytes of flush and flag: a slot below the stream's size must fail, one of need + 48 or more must succeed, in between either;
    nothing outside the slots is written either way"""
    h = tables["golden"]
    sym, idx, want = cc.slot_case()
    need = len(want)
    sym2, idx2 = np.stack([sym, sym]), np.stack([idx, idx])
    seen = set()
    for cap in range(max(64, need - 8), need + 64 + 1):
        enc = Encoded(h, sym2, idx2, cap, guard=64)
        assert enc.guards_intact(), cap
        for b in range(2):
            err = int(enc.err[b])
            assert err in (0, SGIC_ENOSPC), (cap, b, err)
            if err == 0:
                assert enc.off[b] + enc.len[b] == cap and enc.stream(b) == want, (cap, b)
                assert (enc.slot(b)[:enc.off[b]] == 0xA5).all(), (cap, b)
            else:
                assert enc.len[b] == 0 and enc.off[b] == cap, (cap, b)
            if cap < need:
                assert err == SGIC_ENOSPC, (cap, b)
            if cap >= need + 48:
                assert err == 0, (cap, b)
            seen.add(err)
        assert enc.err[0] == enc.err[1]
    assert seen == {0, SGIC_ENOSPC}


def test_failing_image_leaves_its_neighbour_alone(tables):
    h = tables["golden"]
    sym1, idx1, want = cc.slot_case()
    sym0, idx0, too_long = cc.bypass_heavy_case()
    cap = len(want) + 48                                   # the least slot that must take image 1
    assert len(too_long) > cap
    enc = Encoded(h, np.stack([sym0, sym1]), np.stack([idx0, idx1]), cap, guard=64)
    assert enc.err.tolist() == [SGIC_ENOSPC, 0]
    assert enc.len[0] == 0 and enc.off[0] == cap
    assert enc.stream(1) == want and enc.off[1] + enc.len[1] == cap
    assert (enc.slot(1)[:enc.off[1]] == 0xA5).all()        # image 1 wrote nothing in front of its stream, image 0 nothing behind its slot
    assert enc.guards_intact()


def _init_state(rows, lens, cap):
    """sgic_rans_decode_init_batch over front-aligned streams (rows of `cap` bytes, the first lens[b] of them the stream) -> state"""
    torch = _torch()
    from sgic_amd._lib import call
    B = len(lens)
    state = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")
    call("sgic_rans_decode_init_batch", _dev(np.asarray(rows, dtype=np.uint8).reshape(B, cap)), cap, None,
         _dev(np.asarray(lens, dtype=np.int32)), B, state)
    return state.cpu().numpy()


def test_cursor_and_error_state(tables):
    torch = _torch()
    from sgic_amd.entropy.MLCodec_rans import RansDecoder
    name, n = "golden", cc.SLOT_N
    h = tables[name]
    sym, idx, data, cut = cc.cursor_case()                 # every entry coded
    head = np.frombuffer(data, dtype=np.uint8)[:8]

    # streams shorter than the flag byte and the 4 bytes of state
    st = _init_state(np.tile(head, (5, 1)), [0, 1, 2, 3, 4], 8)
    assert (st[:, 2] == 1).all() and st[:, 1].tolist() == [0, 1, 2, 3, 4] and (st[:, 3] == 0).all()
    assert _init_state(head[:1], [0], 1)[0, 2] == 1        # no stream at all, in a buffer of one byte
    assert _init_state(head, [8], 8)[0].tolist() == [int.from_bytes(data[1:5], "little", signed=True), 5, 0, 0]
    # a flag byte that announces a multi-stream container
    assert _init_state(np.array([0x11, 0, 0, 0x80, 0], dtype=np.uint8), [5], 5)[0, 2] == 2
    # a coder state below the coder's lower bound 2^23, which no encoder leaves: refused at init (only init runs here), the bound
    # itself is the state of an empty message
    low = _init_state(np.array([[1, 0, 0, 0, 0], [1, 0xFF, 0xFF, 0x7F, 0], [1, 0, 0, 0x80, 0]], dtype=np.uint8), [5, 5, 5], 5)
    assert low[:, 2].tolist() == [2, 2, 0] and low[:, 1].tolist() == [5, 5, 5]

    fac = RansDecoder(1)
    g = fac.add_cdf(*cc.table(name))
    fac.set_stream(np.zeros(0, dtype=np.uint8))
    with pytest.raises(RuntimeError) as e:
        fac.decode_stream(idx[:8], g)
    assert type(e.value) is RuntimeError                   # the decoder's own verdict, not a refused library call

    # a stream cut at two thirds, decoded with the whole index list
    with pytest.raises(ValueError):
        cc.oracle_decode(name, cut.tobytes(), idx)         # the oracle runs off its end too
    k = cc.odd_cut(n)
    assert np.array_equal(orc.Decoder(cut.tobytes(), cc.orc_table(name)).decode(idx[:k]), sym[:k])      # the first third is all there
    d = Decoding(_dev(cut), len(cut), None, _dev(np.array([len(cut)], dtype=np.int32)), idx[None])
    assert d.rc(h, k) == 0
    assert d.state[0, 2] == 0 and np.array_equal(d.out[0, :k], sym[:k])
    assert d.rc(h, n - k) == 0
    assert d.state[0, 2] == 1 and d.state[0, 1] == len(cut)
    # right up to the symbol that ran off the end (whose own value is made of the zeros read there), zeros behind it
    good = int(np.flatnonzero(d.out[0, :n] != sym)[0])
    assert good > k and not d.out[0, good + 1:n].any()
    again = Decoding(_dev(cut), len(cut), None, d.d_len, idx[None])
    again.d_state.copy_(d.d_state)                         # a third call on the failed cursor
    assert again.rc(h, n) == 0
    assert again.state[0].tolist() == d.state[0].tolist() and not again.out[0, :n].any()
    assert (again.out[0, n:] == FILL).all()
    fac.set_stream(cut)
    with pytest.raises(RuntimeError) as e:
        fac.decode_stream(idx, g)
    assert type(e.value) is RuntimeError
    with pytest.raises(RuntimeError):                      # and it stays failed
        fac.decode_stream(idx[:8], g)

    # an index past the table's rows
    bad = idx.copy()
    bad[77] = 300
    full = _dev(np.frombuffer(data, dtype=np.uint8))
    d = Decoding(full, len(data), None, _dev(np.array([len(data)], dtype=np.int32)), bad[None])
    assert d.rc(h, n) == 0
    assert d.state[0, 2] == 3
    assert np.array_equal(d.out[0, :77], sym[:77]) and not d.out[0, 77:n].any()
    torch.cuda.synchronize()


def test_facade_two_groups():
    _torch()
    from sgic_amd.entropy.MLCodec_rans import RansDecoder, RansEncoder
    names = ("golden", "7x65")
    enc, dec = RansEncoder(False, 1), RansDecoder(1)
    for g, name in enumerate(names):
        assert enc.add_cdf(*cc.table(name)) == g and dec.add_cdf(*cc.table(name)) == g
    msg = [cc.messages(cc.table(name), 1500, 41 + g) for g, name in enumerate(names)]
    enc.reset()
    enc.encode_with_indexes(msg[1][0][:700], msg[1][1][:700], 1)
    with pytest.raises(ValueError):
        enc.encode_with_indexes(msg[0][0][:10], msg[0][1][:10], 0)       # one cdf group per stream
    enc.encode_with_indexes(msg[1][0][700:], msg[1][1][700:], 1)
    enc.flush()
    for g in (1, 0):
        if g == 0:
            enc.reset()
            enc.encode_with_indexes(msg[0][0], msg[0][1], 0)
            enc.flush()
        got = enc.get_encoded_stream()
        assert got.tobytes() == cc.stream(names[g], *msg[g]), names[g]
        dec.set_stream(got)
        out = np.concatenate([dec.decode_stream(msg[g][1][:701], g), dec.decode_stream(msg[g][1][701:], g)])
        assert np.array_equal(out, cc.expected(*msg[g])), names[g]
