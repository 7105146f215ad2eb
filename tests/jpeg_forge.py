"""Test helper: forged JPEG files that Pillow itself never writes -- unusual but well-formed ones, and malformed ones -- for the
contract of the GPU JPEG ingest (sgic_amd.jpeg, csrc/jpeg.hip): a file's pixels are Pillow's, or the file is refused (Unsupported ->
host decoder), or the decode fails loudly.

  write()            a baseline / extended-sequential writer over given quantised coefficients, sampling factors and tables: one
                     interleaved scan, optimal Huffman tables and the bit packing of jpeg_scans (tables_for / pack_events)
  unusual_cases()    well-formed files: 4:4:0, tiny 4:2:0 / 4:2:2, table ids 2 and 3, 16-bit tables, odd component ids, marker noise ...
  malformed_cases()  byte edits of forged files: truncations, bad table ids, bad Huffman tables, restart-marker damage, short scans

CPU only; the coefficients come from Pillow files (oracle.jpeg_ref.huffman_decode) or from jpeg_enc_ref's forward DCT.  Pillow decoding
a forged copy of its own file to the same pixels (tests/test_jpeg_forge_cpu.py) checks the writer itself."""
import functools
import struct

import numpy as np

import jpeg_enc_ref
from jpeg_cases import natural_like
from jpeg_scans import _events, _save, _segment, pack_events, tables_for
from oracle import jpeg_ref

ZIGZAG = jpeg_enc_ref.ZIGZAG
S444, S422, S420, S440 = [(1, 1)] * 3, [(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)]


def grid(H, W, comps):
    """-> per component (block rows, block columns) of the MCU-padded grid (a single component is not interleaved: its own blocks)"""
    if len(comps) == 1:
        return [(-(-H // 8), -(-W // 8))]
    hmax, vmax = max(h for h, _ in comps), max(v for _, v in comps)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return [(my * v, mx * h) for h, v in comps]


def write(H, W, comps, coefs, quants, *, tq_ids=None, pq16=False, sof=0xC0, cids=None, th=(0, 1), restart=0, adobe=None,
          extra_segments=()):
    """-> the bytes of a sequential Huffman JPEG with one interleaved scan.
    comps: [(h, v)] sampling factors as the SOF declares them; coefs: per component (block rows, block columns, 64) quantised
    coefficients in natural order over grid(H, W, comps); quants: per component its (64,) table in natural order; tq_ids: per
    component the table id (components sharing an id must share the table); pq16: 16-bit DQT entries; sof: the frame marker (0xC0
    baseline, 0xC1 extended); cids: component ids; th: Huffman table slot of (component 0, the other components); restart: MCUs per
    restart interval (0: none, no DRI); adobe: the transform byte of an Adobe APP14 segment (None: no segment); extra_segments: whole
    marker segments (bytes) put right after SOI"""
    nc = len(comps)
    tq_ids = list(tq_ids) if tq_ids is not None else [0, 1, 1][:nc]
    cids = list(cids) if cids is not None else [1, 2, 3][:nc]
    slot = {c: th[0] if c == 0 else th[1] for c in range(nc)}
    shape = grid(H, W, comps)
    assert all(tuple(coefs[c].shape) == (*shape[c], 64) for c in range(nc)), ([c.shape for c in coefs], shape)
    if nc == 1:
        gh, gw = shape[0]
        blocks_of = lambda u: [(0, u // gw, u % gw)]
    else:
        gh, gw = shape[0][0] // comps[0][1], shape[0][1] // comps[0][0]
        blocks_of = lambda u: [(c, (u // gw) * v + by, (u % gw) * h + bx) for c, (h, v) in enumerate(comps) for by in range(v)
                               for bx in range(h)]
    ev = _events(coefs, list(range(nc)), blocks_of, gw * gh, 0, 63, 0, 0, restart, (slot, True))
    codes, dht = tables_for(ev)
    out = bytearray(b"\xff\xd8")
    for s in extra_segments:
        out += s
    if adobe is not None:
        out += _segment(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe))
    done = {}
    for c in range(nc):
        t = np.asarray(quants[c])[ZIGZAG]
        if tq_ids[c] in done:
            assert np.array_equal(done[tq_ids[c]], t)
            continue
        done[tq_ids[c]] = t
        out += _segment(0xDB, bytes([(16 if pq16 else 0) | tq_ids[c]]) + (t.astype(">u2").tobytes() if pq16 else bytes(t.astype(np.uint8))))
    out += _segment(sof, struct.pack(">BHHB", 8, H, W, nc) + b"".join(bytes([cids[c], (h << 4) | v, tq_ids[c]]) for c, (h, v) in enumerate(comps)))
    out += _segment(0xC4, dht)
    if restart:
        out += _segment(0xDD, struct.pack(">H", restart))
    out += _segment(0xDA, bytes([nc]) + b"".join(bytes([cids[c], slot[c] << 4 | slot[c]]) for c in range(nc)) + bytes([0, 63, 0]))
    out += pack_events(ev, codes)
    return bytes(out + b"\xff\xd9")


# ---- walking a file by its markers -----------------------------------------------------------------------------------------------------
def segments(data):
    """-> [(marker, offset of its 0xFF, offset past the segment)] of the header segments up to and including the first SOS"""
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        ln = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((m, pos, pos + 2 + ln))
        pos += 2 + ln
        if m == 0xDA:
            return out


def find(data, marker, nth=0):
    """-> (offset, end) of the nth header segment with this marker"""
    return [(a, b) for m, a, b in segments(data) if m == marker][nth]


def scan_markers(data):
    """-> ([offsets of the RSTn markers in the entropy-coded segment of the first scan], offset of the marker that ends it)"""
    pos = segments(data)[-1][2]
    rst = []
    while True:
        if data[pos] == 0xFF and data[pos + 1] not in (0x00, 0xFF):
            if 0xD0 <= data[pos + 1] <= 0xD7:
                rst.append(pos)
            else:
                return rst, pos
            pos += 1
        pos += 1


# ---- coefficient sources ---------------------------------------------------------------------------------------------------------------
def pillow_coefs(data):
    """a Pillow-written baseline file -> (Parsed, per-component coefficient planes in natural order)"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    p = J.parse(data)
    return p, jpeg_ref.huffman_decode(p)


def fit(plane, bh, bw):
    """crop or zero-pad a (rows, columns, 64) coefficient plane to (bh, bw, 64)"""
    out = np.zeros((bh, bw, 64), dtype=plane.dtype)
    r, c = min(bh, plane.shape[0]), min(bw, plane.shape[1])
    out[:r, :c] = plane[:r, :c]
    return out


def reforge(data, **kw):
    """a Pillow-written baseline file -> the forged file of the same geometry, coefficients and tables"""
    p, coefs = pillow_coefs(data)
    comps = [(d["h"], d["v"]) for d in p.comps]
    shape = grid(p.H, p.W, comps)
    return write(p.H, p.W, comps, [fit(coefs[c], *shape[c]) for c in range(p.ncomp)], [p.quant[d["tq"]] for d in p.comps],
                 tq_ids=[d["tq"] for d in p.comps], **kw)


@functools.lru_cache(maxsize=None)
def _sources():
    """the two Pillow files whose coefficients the forged files are cut from: colour 4:4:4 and grey, 64x200 (8 x 25 blocks a plane)"""
    rng = np.random.default_rng(21)
    colour = _save(natural_like(64, 200, rng), quality=85, subsampling=0)
    grey = _save(natural_like(64, 200, rng, grey=True), quality=80)
    return pillow_coefs(colour), pillow_coefs(grey)


def forged(H, W, comps, **kw):
    """a forged H x W file of this sampling, its blocks cut from the top left of the source planes (a block is a block: any
    block content is a valid image, so a 4:4:4 file's planes serve every layout)"""
    (pc, cc), (pg, cg) = _sources()
    p, coefs = (pc, cc) if len(comps) == 3 else (pg, cg)
    shape = grid(H, W, comps)
    return write(H, W, comps, [fit(coefs[c], *shape[c]) for c in range(len(comps))], [p.quant[d["tq"]] for d in p.comps], **kw)


def wide_tables(quality):
    """jpeg_set_quality WITHOUT force_baseline -> (2, 64) u16 natural order: entries above 255 at low quality (16-bit DQT)"""
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([jpeg_enc_ref.BASE_LUMA, jpeg_enc_ref.BASE_CHROMA], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 32767).astype(np.uint16)


def forged_16bit(H, W, quality, subsampling, sof, seed):
    """a real image quantised with 16-bit tables (jpeg_enc_ref's colour conversion, downsampling and forward DCT)"""
    rgb = natural_like(H, W, np.random.default_rng(seed))
    tabs = wide_tables(quality)
    comps = [jpeg_enc_ref.SAMPLING[subsampling], (1, 1), (1, 1)]
    coefs = []
    for c, pl in enumerate(jpeg_enc_ref.planes(rgb, subsampling)):
        zz = jpeg_enc_ref.fdct_quant(pl, tabs[min(c, 1)])
        nat = np.zeros(zz.shape, dtype=np.int32)
        nat[..., ZIGZAG] = zz
        coefs.append(nat)
    return write(H, W, comps, coefs, [tabs[0], tabs[1], tabs[1]], pq16=True, sof=sof)


def _extreme():
    """DC +1023 / -1024 and AC +-1023 under an all-ones table: the widest Huffman categories (11 and 10 bits), sparse enough that the
    samples stay inside what an encoder of real images produces"""
    shape = grid(16, 32, S444)
    coefs = [np.zeros((*s, 64), dtype=np.int32) for s in shape]
    for c in range(3):
        coefs[c][0, 0, 0], coefs[c][0, 1, 0], coefs[c][0, 2, 0], coefs[c][0, 3, 0] = 1023, -1024, 1023, 0
        coefs[c][1, 0, 1], coefs[c][1, 1, 8], coefs[c][1, 2, 63], coefs[c][1, 3, 9] = 1023, -1023, 1023, -1023
    ones = np.ones(64, dtype=np.uint16)
    return write(16, 32, S444, coefs, [ones] * 3)


def _insert(data, at, blob):
    return data[:at] + blob + data[at:]


# ---- the two corpora -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unusual_cases():
    """-> [(name, bytes, expect)]: well-formed files Pillow does not write.  expect: "both" (parse and parse_scans take it),
    "scans_only" (parse refuses, parse_scans takes it) or "refused" (both refuse: a chroma plane too narrow for the upsampler)"""
    out = []
    for h, w in [(45, 59), (1, 9), (2, 9), (3, 3), (16, 8), (17, 23), (40, 3)]:
        out.append((f"440_{h}x{w}", forged(h, w, S440), "both"))
    out.append(("440_45x59_rst2", forged(45, 59, S440, restart=2), "both"))
    for h, w in [(33, 1), (31, 2)]:
        out.append((f"440_{h}x{w}_narrow", forged(h, w, S440), "refused"))
    for h, w in [(1, 17), (2, 17), (3, 6), (5, 5), (17, 7)]:
        out.append((f"420_{h}x{w}", forged(h, w, S420), "both"))
    for h, w in [(1, 5), (9, 6), (9, 7)]:
        out.append((f"422_{h}x{w}", forged(h, w, S422), "both"))
    out.append(("tq_ids_2_3", forged(40, 56, S420, tq_ids=[2, 3, 3]), "both"))
    for q, sub, sof in [(1, 0, 0xC1), (3, 2, 0xC0), (8, 2, 0xC1), (20, 0, 0xC0)]:
        out.append((f"pq16_q{q}_s{sub}_sof{sof & 15}", forged_16bit(37, 53, q, sub, sof, 30 + q), "both"))
    out.append(("cids_0_1_2", forged(40, 56, S420, cids=[0, 1, 2]), "both"))
    out.append(("cids_7_40_200", forged(40, 56, S422, cids=[7, 40, 200]), "both"))
    out.append(("adobe_transform1", forged(40, 56, S444, adobe=1), "both"))
    out.append(("grey_declared_2x2", forged(40, 56, [(2, 2)]), "both"))
    noise = [_segment(0xFE, b"a comment \xff\xd9 \xff\xda\x00\x08 \xff\xd8\xff\xc0 with markers in it \xff"),
             _segment(0xE1, b"Exif\x00\x00" + b"\xff\xc4\x00\x05\xff\xdb\xff\xd0\xff\x00" * 9)]
    d = forged(40, 56, S420, extra_segments=noise)
    out.append(("marker_noise_com_app1", d, "both"))
    d = forged(40, 56, S420, restart=3)
    rst, end = scan_markers(d)
    d = _insert(_insert(d, end, b"\xff\xff\xff"), rst[1], b"\xff\xff\xff")     # fill bytes before EOI, before an RSTn ...
    d = _insert(d, find(d, 0xC4)[0], b"\xff\xff\xff")                          # ... and before a header marker
    out.append(("fill_bytes_before_markers", d, "both"))
    d = forged(40, 56, S420)
    a, b = find(d, 0xDB, 0)
    wrong = d[a:a + 5] + bytes(255 - x if x < 255 else 1 for x in d[a + 5:b])
    sos = find(d, 0xDA)[0]
    out.append(("dqt_redefined_before_sos", d[:a] + wrong + d[b:sos] + d[a:b] + d[sos:], "both"))     # the last definition holds
    d = forged(40, 56, S420)
    out.append(("dri_5_then_dri_0", _insert(d, find(d, 0xDA)[0], _segment(0xDD, b"\x00\x05") + _segment(0xDD, b"\x00\x00")), "both"))
    out.append(("restart1_64x200_rst_wraps", forged(64, 200, S444, restart=1), "both"))
    out.append(("restart_above_mcu_count", forged(40, 56, S420, restart=1000), "both"))
    out.append(("extreme_coefficients", _extreme(), "both"))
    d = forged(40, 56, S420)
    out.append(("garbage_after_eoi", d + bytes(np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8)), "both"))
    out.append(("second_jpeg_after_eoi", d + forged(24, 24, S444), "both"))
    out.append(("huffman_slots_2_3_baseline", forged(40, 56, S420, th=(2, 3)), "scans_only"))
    out.append(("huffman_slots_2_3_sof1", forged(40, 56, S422, th=(3, 2), sof=0xC1), "scans_only"))
    return out


# what the installed Pillow does with each malformed file: it raises, or it decodes something (with libjpeg warnings)
MALFORMED_PILLOW = {}


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """-> [(name, bytes, expect)]: byte edits of forged files.  expect: "unsupported" (parse and parse_scans both raise Unsupported) or
    "decode_error" (both accept the file; the decode reports that the scan ended early: ValueError in the oracle, code 3 on the GPU)"""
    out = []

    def add(name, data, expect, pillow):
        out.append((name, bytes(data), expect))
        MALFORMED_PILLOW[name] = pillow

    good = forged(40, 56, S420)
    sos_a, sos_b = find(good, 0xDA)
    add("cut_in_half", good[:(sos_b + len(good)) // 2], "unsupported", "raises")
    add("cut_eoi", good[:-2], "unsupported", "raises")
    add("cut_last_3", good[:-3], "unsupported", "raises")
    add("cut_after_sos_header", good[:sos_b], "unsupported", "raises")
    add("cut_inside_sos_header", good[:sos_a + 7], "unsupported", "raises")
    add("tq_5", forged(40, 56, S420, tq_ids=[0, 5, 5]), "unsupported", "raises")
    a, b = find(good, 0xC4)
    a += 4
    while good[a] != 0x00:                                       # walk the tables of the DHT segment to the DC table of slot 0
        a += 17 + sum(good[a + 1:a + 17])
    assert a < b
    a -= 4
    for sym in (16, 200):
        add(f"dc_symbol_{sym}", good[:a + 21] + bytes([sym]) + good[a + 22:], "unsupported", "raises")
    add("dht_counts_above_256", good[:a + 5 + 14] + b"\xff\xff" + good[a + 5 + 16:], "unsupported", "raises")
    a, b = find(good, 0xC0)
    add("sof_height_0", good[:a + 5] + b"\x00\x00" + good[a + 7:], "unsupported", "raises")
    add("sof_width_0", good[:a + 7] + b"\x00\x00" + good[a + 9:], "unsupported", "raises")
    rst = forged(40, 56, S420, restart=2)                        # 3 x 4 MCUs: five markers
    a, b = find(rst, 0xDD)
    add("rst_but_dri_0", rst[:a + 4] + b"\x00\x00" + rst[b:], "unsupported", "decodes")
    add("rst_but_no_dri", rst[:a] + rst[b:], "unsupported", "decodes")
    marks, _ = scan_markers(rst)
    assert len(marks) == 5 and rst[marks[1] + 1] == 0xD1
    add("rst1_renumbered_rst3", rst[:marks[1] + 1] + b"\xd3" + rst[marks[1] + 2:], "unsupported", "decodes")
    add("one_rst_removed", rst[:marks[2]] + rst[marks[2] + 2:], "unsupported", "decodes")
    add("sos_unknown_component", good[:sos_a + 7] + b"\x09" + good[sos_a + 8:], "unsupported", "raises")
    add("eoi_after_sos_header", good[:sos_b] + b"\xff\xd9", "decode_error", "decodes")
    add("three_scan_bytes_then_eoi", good[:sos_b] + b"\x12\x34\x56\xff\xd9", "decode_error", "decodes")
    return out


@functools.lru_cache(maxsize=None)
def layout_batch():
    """-> [(name, bytes)]: eight 40x56 files of differing layouts, tables and markers for ONE batch"""
    return [("440", forged(40, 56, S440)), ("420", forged(40, 56, S420)), ("444_pq16", forged_16bit(40, 56, 3, 0, 0xC1, 77)),
            ("tq_ids_2_3", forged(40, 56, S422, tq_ids=[2, 3, 3])), ("grey_declared_2x2", forged(40, 56, [(2, 2)])),
            ("restart1", forged(40, 56, S420, restart=1)), ("cids_7_40_200", forged(40, 56, S444, cids=[7, 40, 200])),
            ("adobe_transform1", forged(40, 56, S440, adobe=1))]
