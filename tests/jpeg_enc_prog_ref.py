"""A numpy restatement of progressive JPEG encoding as libjpeg does it: the whole file that `PIL.Image.save(format="JPEG", quality=q,
subsampling=s, progressive=True)` writes.  The coefficients are jpeg_enc_ref's (planes, fdct_quant), the ten scans those of
jpeg_scans (STANDARD_COLOUR through _events, tables_for and pack_events: jcphuff.c with tables fitted to every scan), the framing is
Pillow's: SOF2, one DHT segment per table in front of the scan that uses it, SOS selectors that name only the table class in use,
no DRI.  It imports nothing from the package; the GPU encoder and the package's framing are compared with it and with Pillow."""
import io

import numpy as np

import jpeg_enc_ref as ref
import jpeg_scans

SCRIPT = jpeg_scans.STANDARD_COLOUR
CORRECTION_TILE_ROW = [233, 233, 233, 4, 4, 4, 4, 4]


def pillow_bytes(rgb, quality, subsampling, **kw):
    """Pillow sizes its output buffer from the image and fails on files past it ("broken data stream": noise at q 100), so the
    block size is raised for the call and put back"""
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 1 << 16, 16 * rgb.shape[0] * rgb.shape[1])
    try:
        Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality), subsampling=int(subsampling), progressive=True, **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


def correction_tile():
    """an 8 x 8 tile whose luma block at q 100 is all correction bits in the last scan: tiled, 15 blocks fill libjpeg's buffer"""
    rng = np.random.default_rng(0)
    tile = np.clip(rng.integers(0, 2, (8, 8)) * rng.integers(40, 256) + rng.integers(0, 30), 0, 255)
    assert tile[0].tolist() == CORRECTION_TILE_ROW
    return tile.astype(np.uint8)


def tiled(h, w):
    """-> (h, w, 3) u8: the correction tile repeated, equal in the three channels"""
    t = np.tile(correction_tile(), (-(-h // 8), -(-w // 8)))[:h, :w]
    return np.stack([t, t, t], axis=-1)


def flat_large(column=None):
    """1448 x 1456 of value 97: 32 942 blocks per component at 4:4:4, so an end-of-band run passes 0x7FFF in every AC scan.
    column: the 8 x 8 block at row 1440 and this column has texture.  Column 8 is block 32 761 of the raster, so the run in front of
    it ends six blocks short of 0x7FFF; column 320 is block 32 800, so the run is split and its rest of 33 blocks ends at a coded
    block and not at the end of the scan"""
    a = np.full((1448, 1456, 3), 97, np.uint8)
    if column is not None:
        a[1440:1448, column:column + 8] = np.random.default_rng(3).integers(0, 256, (8, 8, 3))
    return a


def coefficients(rgb, tables, subsampling):
    """-> three (block rows, block columns, 64) int64 arrays in natural order.  Luma covers whole MCUs: a dummy block is zeros with
    the DC of the block before it in its MCU, as libjpeg's coefficient buffer holds it"""
    H, W, _ = rgb.shape
    h, v = ref.SAMPLING[subsampling]
    comp = ref.planes(rgb, subsampling)
    out = []
    for c in range(3):
        zz = ref.fdct_quant(comp[c], tables[0 if c == 0 else 1])
        nat = np.zeros_like(zz)
        nat[..., ref.ZIGZAG] = zz
        out.append(nat)
    wb, hb = -(-W // 8), -(-H // 8)
    y = out[0]
    for by in range(y.shape[0]):
        for bx in range(y.shape[1]):
            if by < hb and bx < wb:
                continue
            dy, dx = by % v, bx % h
            py, px = (by, bx - 1) if dx else (by - 1, bx - dx + h - 1)       # the block before it in the MCU (dy, dx are not both 0)
            y[by, bx] = 0
            y[by, bx, 0] = y[py, px, 0]
    return out


def scan_events(rgb, tables, subsampling):
    """-> the event lists of the ten scans (jpeg_scans._events)"""
    H, W, _ = rgb.shape
    h, v = ref.SAMPLING[subsampling]
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    wb, hb = -(-W // 8), -(-H // 8)
    coefs = coefficients(rgb, tables, subsampling)
    slot = {0: 0, 1: 1, 2: 1}
    hv = [(0, h, v), (1, 1, 1), (2, 1, 1)]
    out = []
    for comps, ss, se, ah, al in SCRIPT:
        if len(comps) == 1:
            gw, gh = (wb, hb) if comps[0] == 0 else (mx, my)
            blocks_of = lambda u, c=comps[0], gw=gw: [(c, u // gw, u % gw)]
        else:
            gw, gh = mx, my
            blocks_of = lambda u: [(c, (u // mx) * cv + by, (u % mx) * ch + bx) for c, ch, cv in hv for by in range(cv) for bx in range(ch)]
        out.append(jpeg_scans._events(coefs, list(comps), blocks_of, gw * gh, ss, se, ah, al, 0, (slot, False)))
    return out


def eobrun_values(events):
    """one AC scan's events -> the EOBRUN values in stream order"""
    return [(1 << (e[2] >> 4)) + (events[j + 1][1] if e[2] >> 4 else 0) for j, e in enumerate(events)
            if e[0] == "s" and e[2] & 15 == 0 and e[2] != 0xF0]


def eobrun_counts(events):
    """one AC scan's events -> (EOBRUN symbols, the largest EOBRUN value, other symbols)"""
    values = eobrun_values(events)
    return len(values), max(values, default=0), sum(e[0] == "s" for e in events) - len(values)


def forced_flushes(events):
    """one refinement scan's events -> the EOBRUN symbols that libjpeg sent because its correction-bit buffer was full: more than 937
    correction bits follow them"""
    forced = 0
    for j, e in enumerate(events):
        if e[0] == "s" and e[2] & 15 == 0 and e[2] != 0xF0:
            k = j + 1 + (1 if e[2] >> 4 else 0)
            n = 0
            while k + n < len(events) and events[k + n][0] == "b" and events[k + n][2] == 1:
                n += 1
            forced += n > 937
    return forced


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def front(H, W, tables, subsampling):
    """SOI, APP0, the two DQT, SOF2"""
    h, v = ref.SAMPLING[subsampling]
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += _seg(0xDB, bytes([i]) + bytes(int(tables[i][z]) for z in ref.ZIGZAG))
    return out + _seg(0xC2, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, h << 4 | v, 0, 2, 0x11, 1, 3, 0x11, 1]))


def encode(rgb, quality, subsampling):
    """-> (the whole file, {"segments": the ten entropy-coded segments, "dht": per scan its DHT payloads, "events": the ten event
    lists})"""
    tables = ref.quant_tables(quality)
    events = scan_events(rgb, tables, subsampling)
    out = front(rgb.shape[0], rgb.shape[1], tables, subsampling)
    segments, dhts = [], []
    for (comps, ss, se, ah, al), ev in zip(SCRIPT, events):
        codes, dht = jpeg_scans.tables_for(ev)
        payloads = [dht[o:o + 17 + sum(dht[o + 1:o + 17])] for o in _table_starts(dht)]
        for pl in payloads:
            out += _seg(0xC4, pl)
        if ss == 0:
            sel = b"".join(bytes([c + 1, 0 if ah or c == 0 else 0x10]) for c in comps)
        else:
            sel = bytes([comps[0] + 1, 0 if comps[0] == 0 else 1])
        seg = bytes(jpeg_scans.pack_events(ev, codes))
        out += _seg(0xDA, bytes([len(comps)]) + sel + bytes([ss, se, ah << 4 | al])) + seg
        segments.append(seg)
        dhts.append(payloads)
    return out + b"\xff\xd9", {"segments": segments, "dht": dhts, "events": events}


def _table_starts(dht):
    o = 0
    while o < len(dht):
        yield o
        o += 17 + sum(dht[o + 1:o + 17])
