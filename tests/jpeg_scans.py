"""Test helper for the multi-scan JPEG path (sgic_amd.jpeg.parse_scans / ScanJpegBatch, csrc/jpeg.hip jpeg_scan_kernel):

  (a) decode(): a plain numpy / Python restatement of the coefficient decode of every scan type (T.81 G.1.2 as libjpeg-turbo's jdphuff.c
      runs it), reading the ParsedScans the product builds, then the IDCT / upsampling of oracle.jpeg_ref;
  (b) transcode(): a LOSSLESS transcoder -- the coefficients of a Pillow-written baseline file (oracle.jpeg_ref.huffman_decode)
      re-encoded progressively (or as non-interleaved sequential scans) under an arbitrary scan script, with optimal Huffman tables built
      from each scan's symbol statistics (jchuff.c jpeg_gen_optimal_table) and optional restart intervals -- for the scripts Pillow
      cannot write.  Pillow decoding a transcoded file to exactly the original's pixels checks the transcoder itself."""
import struct

import numpy as np

from oracle import jpeg_ref
from oracle.jpeg_ref import NATURAL, _Bits, _decode_sym, _receive

# libjpeg's jpeg_simple_progression for a colour / a greyscale image: (components, Ss, Se, Ah, Al)
STANDARD_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                   ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
STANDARD_GREY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


# ---- (a) the restatement ---------------------------------------------------------------------------------------------------------------
def _blocks(p, s, u):
    """-> [(component, block row, block column)] of unit u of scan s, in scan order"""
    uy, ux = divmod(u, s.gw)
    out = []
    for c in s.comps:
        d = p.comps[c]
        hs, vs = (1, 1) if len(s.comps) == 1 else (d["h"], d["v"])
        out += [(c, uy * vs + by, ux * hs + bx) for by in range(vs) for bx in range(hs)]
    return out


def _bits(br, n):
    v = br.peek(n)
    br.skip(n)
    return v


def decode_coefs(p):
    """ParsedScans -> per component (bh, bw, 64) int32 coefficients, natural order"""
    from sgic_amd import jpeg as J
    coefs = [np.zeros((d["bh"], d["bw"], 64), dtype=np.int32) for d in p.comps]
    for s in p.scans:
        br = _Bits(s.data)
        pred, eobrun, nseg = {c: 0 for c in s.comps}, 0, 1
        p1 = 1 << s.al
        for u in range(s.gw * s.gh):
            if s.restart and u and u % s.restart == 0:
                br.seek(int(s.segs[nseg]))
                nseg += 1
                pred, eobrun = {c: 0 for c in s.comps}, 0
            for (c, by, bx) in _blocks(p, s, u):
                blk = coefs[c][by, bx]
                i = s.comps.index(c)
                if s.mode in (J.M_SEQ, J.M_DC_FIRST):
                    t = _decode_sym(br, p.tabs[s.dc[i]])
                    if t:
                        pred[c] += _receive(br, t)
                    blk[0] = pred[c] << s.al
                    if s.mode == J.M_DC_FIRST:
                        continue
                if s.mode == J.M_DC_REFINE:
                    if _bits(br, 1):
                        blk[0] |= p1
                elif s.mode in (J.M_SEQ, J.M_AC_FIRST):
                    if eobrun > 0:
                        eobrun -= 1
                        continue
                    k, se = (1, 63) if s.mode == J.M_SEQ else (s.ss, s.se)
                    while k <= se:
                        rs = _decode_sym(br, p.tabs[s.ac[i]])
                        r, t = rs >> 4, rs & 15
                        if t:
                            k += r
                            blk[NATURAL[k]] = _receive(br, t) << s.al
                        elif r == 15:
                            k += 15
                        else:
                            if s.mode == J.M_AC_FIRST:
                                eobrun = (1 << r) + (_bits(br, r) if r else 0) - 1
                            break
                        k += 1
                else:                                        # AC refine: jdphuff.c decode_mcu_AC_refine
                    k = s.ss
                    if eobrun == 0:
                        while k <= s.se:
                            rs = _decode_sym(br, p.tabs[s.ac[i]])
                            r, t = rs >> 4, rs & 15
                            if t:
                                t = p1 if _bits(br, 1) else -p1
                            elif r != 15:
                                eobrun = (1 << r) + (_bits(br, r) if r else 0)
                                break
                            while k <= s.se:
                                z = NATURAL[k]
                                if blk[z] != 0:
                                    if _bits(br, 1) and (blk[z] & p1) == 0:
                                        blk[z] += p1 if blk[z] >= 0 else -p1
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            if t:
                                blk[NATURAL[k]] = t
                            k += 1
                    if eobrun > 0:
                        while k <= s.se:
                            z = NATURAL[k]
                            if blk[z] != 0 and _bits(br, 1) and (blk[z] & p1) == 0:
                                blk[z] += p1 if blk[z] >= 0 else -p1
                            k += 1
                        eobrun -= 1
        br.check_end()
    return coefs


def to_rgb(p, coefs):
    """coefficients -> (H, W, 3) u8: oracle.jpeg_ref's IDCT, fancy upsampling and colour conversion"""
    planes = [jpeg_ref.idct_blocks(coefs[c].astype(np.int16), p.quant[d["tq"]]) for c, d in enumerate(p.comps)]
    H, W = p.H, p.W
    y = planes[0][:H, :W].astype(np.int32)
    if p.ncomp == 1:
        return np.stack([y, y, y], axis=-1).astype(np.uint8)
    d1 = p.comps[1]
    hs, vs = p.hmax // d1["h"], p.vmax // d1["v"]
    cb = jpeg_ref.upsample(planes[1], d1["cw"], d1["ch"], hs, vs, W, H) - 128
    cr = jpeg_ref.upsample(planes[2], d1["cw"], d1["ch"], hs, vs, W, H) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """bytes -> (H, W, 3) u8, as `np.asarray(Image.open(...).convert("RGB"))`"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    p = J.parse_scans(data)
    return to_rgb(p, decode_coefs(p))


# ---- (b) the transcoder ----------------------------------------------------------------------------------------------------------------
def _nbits(v):
    return int(v).bit_length()


def _optimal_table(freq):
    """jchuff.c jpeg_gen_optimal_table: symbol counts (256) -> (bits[16], values) of a length-limited optimal code"""
    freq = list(freq) + [1]                  # the reserved code point: no code of all ones
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        v = v2 = 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        for i in range(257):
            if freq[i] and freq[i] <= v2 and i != c1:
                v2, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                             # drop the reserved code point
    vals = [s for size in range(1, 33) for s in range(256) if codesize[s] == size]
    return bits[1:17], vals


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def _events(coefs, comps, blocks_of, nunits, ss, se, ah, al, restart, slots):
    """one scan -> list of events: ("s", table key, symbol) | ("b", value, nbits) | ("rst",) (jcphuff.c / jchuff.c encoders)"""
    ev = []
    seq = (ss, se, ah, al) == (0, 63, 0, 0) and slots[1]
    st = {"eobrun": 0, "be": []}

    def emit_eobrun(key):
        if st["eobrun"] > 0:
            nb = _nbits(st["eobrun"]) - 1
            ev.append(("s", key, nb << 4))
            if nb:
                ev.append(("b", st["eobrun"] & ((1 << nb) - 1), nb))
            st["eobrun"] = 0
            ev.extend(("b", b, 1) for b in st["be"])
            st["be"] = []

    pred = {}
    last_key = None
    for u in range(nunits):
        if restart and u and u % restart == 0:
            if last_key is not None:
                emit_eobrun(last_key)
            ev.append(("rst",))
            pred = {}
        for (c, by, bx) in blocks_of(u):
            blk = coefs[c][by, bx]
            dkey, akey = ("dc", slots[0][c]), ("ac", slots[0][c])
            if ss == 0 and ah == 0:                                  # DC first / sequential DC
                v = int(blk[0]) >> al
                diff = v - pred.get(c, 0)
                pred[c] = v
                nb = _nbits(abs(diff))
                ev.append(("s", dkey, nb))
                if nb:
                    ev.append(("b", (diff if diff >= 0 else diff - 1) & ((1 << nb) - 1), nb))
                if not seq:
                    continue
            elif ss == 0:                                            # DC refine
                ev.append(("b", (int(blk[0]) >> al) & 1, 1))
                continue
            last_key = akey
            lo = 1 if seq else ss
            if ah == 0:                                              # AC first (or the sequential AC loop: EOB per block)
                r = 0
                for k in range(lo, se + 1):
                    t = int(blk[NATURAL[k]])
                    a = (abs(t) >> al)
                    if a == 0:
                        r += 1
                        continue
                    emit_eobrun(akey)
                    while r > 15:
                        ev.append(("s", akey, 0xF0))
                        r -= 16
                    nb = _nbits(a)
                    ev.append(("s", akey, (r << 4) + nb))
                    ev.append(("b", a if t >= 0 else (~a) & ((1 << nb) - 1), nb))
                    r = 0
                if r > 0:
                    if seq:
                        ev.append(("s", akey, 0))
                    else:
                        st["eobrun"] += 1
                        if st["eobrun"] == 0x7FFF:
                            emit_eobrun(akey)
                continue
            absv = [abs(int(blk[NATURAL[k]])) >> al for k in range(ss, se + 1)]   # AC refine
            eob = max([k for k in range(ss, se + 1) if absv[k - ss] == 1], default=0)
            r, br = 0, []
            for k in range(ss, se + 1):
                a = absv[k - ss]
                if a == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    emit_eobrun(akey)
                    ev.append(("s", akey, 0xF0))
                    r -= 16
                    ev.extend(("b", b, 1) for b in br)
                    br = []
                if a > 1:
                    br.append(a & 1)
                    continue
                emit_eobrun(akey)
                ev.append(("s", akey, (r << 4) + 1))
                ev.append(("b", 0 if blk[NATURAL[k]] < 0 else 1, 1))
                ev.extend(("b", b, 1) for b in br)
                br, r = [], 0
            if r > 0 or br:
                st["eobrun"] += 1
                st["be"] += br
                if st["eobrun"] == 0x7FFF or len(st["be"]) > 1000 - 64 + 1:
                    emit_eobrun(akey)
    if last_key is not None:
        emit_eobrun(last_key)
    return ev


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def transcode(data, script, restart=0, sequential=False):
    """Pillow-written baseline JPEG bytes -> the same coefficients as a progressive (SOF2) file -- or, with sequential=True, a
    multi-scan sequential (SOF1) file -- under `script`: [(component indices, Ss, Se, Ah, Al), ...].  restart: units (MCUs of
    interleaved scans, blocks of single-component scans) per restart interval in every scan, 0 = none"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    p = J.parse(data)
    coefs = jpeg_ref.huffman_decode(p)
    out = bytearray(b"\xff\xd8")
    for t in sorted({d["tq"] for d in p.comps}):
        out += _segment(0xDB, bytes([t]) + bytes(p.quant[t][J.ZIGZAG].astype(np.uint8)))
    sof = struct.pack(">BHHB", 8, p.H, p.W, p.ncomp) + b"".join(bytes([c + 1, (d["h"] << 4) | d["v"], d["tq"]]) for c, d in enumerate(p.comps))
    out += _segment(0xC1 if sequential else 0xC2, sof)
    slot = {c: 0 if c == 0 else 1 for c in range(p.ncomp)}
    for comps, ss, se, ah, al in script:
        comps = list(comps)
        if len(comps) == 1:
            d = p.comps[comps[0]]
            gw, gh = -(-d["cw"] // 8), -(-d["ch"] // 8)
            blocks_of = lambda u, c=comps[0], gw=gw: [(c, u // gw, u % gw)]
        else:
            gw, gh = p.mcus_x, p.mcus_y
            hv = [(c, p.comps[c]["h"], p.comps[c]["v"]) for c in comps]
            blocks_of = lambda u, hv=hv, gw=gw: [(c, (u // gw) * v + by, (u % gw) * h + bx) for c, h, v in hv for by in range(v) for bx in range(h)]
        ev = _events(coefs, comps, blocks_of, gw * gh, ss, se, ah, al, restart, (slot, sequential))
        codes, dht = tables_for(ev)
        if dht:
            out += _segment(0xC4, dht)
        out += _segment(0xDD, struct.pack(">H", restart))
        out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c + 1, slot[c] << 4 | slot[c]]) for c in comps) + bytes([ss, se, ah << 4 | al]))
        out += pack_events(ev, codes)
    out += b"\xff\xd9"
    return bytes(out)


def tables_for(ev):
    """events of one scan -> ({table key: {symbol: (code, length)}}, the DHT payload of optimal tables for their symbol statistics);
    a key is ("dc" | "ac", slot)"""
    freq = {}
    for e in ev:
        if e[0] == "s":
            freq.setdefault(e[1], np.zeros(256, dtype=np.int64))[e[2]] += 1
    codes, dht = {}, b""
    for key in sorted(freq):
        bits, vals = _optimal_table(freq[key])
        codes[key] = _codes(bits, vals)
        dht += bytes([(0 if key[0] == "dc" else 1) << 4 | key[1]]) + bytes(bits) + bytes(vals)
    return codes, dht


def pack_events(ev, codes):
    """events of one scan -> its entropy-coded segment: Huffman codes and raw bits MSB first, a zero byte stuffed after every 0xFF,
    the last byte before an RSTn marker and at the end padded with ones, RSTn numbered mod 8"""
    acc, n, nrst = 0, 0, 0
    body = bytearray()

    def flush_bytes(acc, n):
        while n >= 8:
            b = (acc >> (n - 8)) & 255
            body.append(b)
            if b == 0xFF:
                body.append(0)
            n -= 8
        return acc & ((1 << n) - 1), n
    for e in ev:
        if e[0] == "rst":
            if n:
                acc, n = (acc << (8 - n)) | ((1 << (8 - n)) - 1), 8
                acc, n = flush_bytes(acc, n)
            body += bytes([0xFF, 0xD0 + (nrst & 7)])
            nrst += 1
            continue
        code, l = codes[e[1]][e[2]] if e[0] == "s" else (e[1], e[2])
        acc, n = (acc << l) | code, n + l
        acc, n = flush_bytes(acc, n)
    if n:
        acc, n = flush_bytes((acc << (8 - n)) | ((1 << (8 - n)) - 1), 8)
    return body


# ---- the test corpus ---------------------------------------------------------------------------------------------------------------------
GOLDEN_APPLE = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "ref_apple.jpg")

# scripts Pillow cannot write, for a colour image (components 0 = Y, 1 = Cb, 2 = Cr)
SCRIPTS = {
    "spectral_only": [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)],
    "dc_per_component": [((0,), 0, 0, 0, 0), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0), ((2,), 1, 63, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0)],
    "al3_to_0": [((0, 1, 2), 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in range(3)] + [((0, 1, 2), 0, 0, 3, 2), ((0, 1, 2), 0, 0, 2, 1)] +
                [((c,), 1, 63, a + 1, a) for a in (2, 1, 0) for c in range(3)] + [((0, 1, 2), 0, 0, 1, 0)],
    "split_bands_refined": [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 2, 0, 1), ((0,), 3, 9, 0, 2), ((0,), 10, 63, 0, 1), ((1,), 1, 63, 0, 1),
                            ((2,), 1, 63, 0, 1), ((0, 1, 2), 0, 0, 1, 0), ((0,), 1, 2, 1, 0), ((0,), 3, 9, 2, 1), ((0,), 3, 9, 1, 0),
                            ((0,), 10, 63, 1, 0), ((1,), 1, 63, 1, 0), ((2,), 1, 63, 1, 0)],
    "unusual_order": [((2,), 0, 0, 0, 1), ((2,), 1, 63, 0, 0), ((0, 1), 0, 0, 0, 0), ((0,), 10, 63, 0, 0), ((2,), 0, 0, 1, 0), ((1,), 1, 63, 0, 0),
                      ((0,), 1, 9, 0, 0)],
}


def grey_script(script):
    """the component-0 part of a colour script"""
    return [((0,), ss, se, ah, al) for comps, ss, se, ah, al in script if 0 in comps]


def _save(img, **kw):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_cases(big=False):
    """-> [(name, bytes)]: Pillow `progressive=True` files over samplings, odd sizes, optimize, restart markers, quality 10..100,
    and the reference's sample image"""
    from jpeg_cases import natural_like
    rng = np.random.default_rng(11)
    spec = [(48, 64, dict(quality=75)), (37, 53, dict(quality=90, subsampling=0)), (40, 72, dict(quality=60, subsampling=1)),
            (33, 47, dict(quality=85, subsampling=2)), (64, 64, dict(quality=30, optimize=True)), (50, 50, dict(quality=95, restart_marker_blocks=3)),
            (41, 29, dict(quality=10)), (16, 16, dict(quality=100, subsampling=0)), (57, 71, dict(quality=50, subsampling=2, optimize=True,
                                                                                                 restart_marker_rows=1))]
    if big:
        spec += [(256, 256, dict(quality=90)), (511, 257, dict(quality=80, subsampling=1, restart_marker_blocks=7)),
                 (1024, 1024, dict(quality=92, optimize=True))]
    out = [(f"prog_{h}x{w}_" + "_".join(f"{k}{v}" for k, v in kw.items()), _save(natural_like(h, w, rng), progressive=True, **kw))
           for h, w, kw in spec]
    out.append(("prog_grey_45x61", _save(natural_like(45, 61, rng, grey=True), progressive=True, quality=70)))
    out.append(("prog_grey_33x17_rst", _save(natural_like(33, 17, rng, grey=True), progressive=True, quality=95, restart_marker_blocks=2)))
    out.append(("ref_apple", open(GOLDEN_APPLE, "rb").read()))
    return out


def transcoded_cases():
    """-> [(name, transcoded bytes, baseline original bytes)]: every script of SCRIPTS on colour 4:2:0 / 4:2:2 / 4:4:4 and grey files,
    restart intervals in every scan, and multi-scan sequential files"""
    from jpeg_cases import natural_like
    rng = np.random.default_rng(12)
    bases = [("420", _save(natural_like(45, 59, rng), quality=88)), ("422", _save(natural_like(40, 37, rng), quality=70, subsampling=1)),
             ("444", _save(natural_like(27, 33, rng), quality=95, subsampling=0)), ("grey", _save(natural_like(35, 42, rng, grey=True), quality=80))]
    out = []
    for bname, base in bases:
        grey = bname == "grey"
        for sname, script in SCRIPTS.items():
            out.append((f"{bname}_{sname}", transcode(base, grey_script(script) if grey else script), base))
        std = STANDARD_GREY if grey else STANDARD_COLOUR
        out.append((f"{bname}_standard_rst2", transcode(base, std, restart=2), base))
        out.append((f"{bname}_al3_rst1", transcode(base, grey_script(SCRIPTS["al3_to_0"]) if grey else SCRIPTS["al3_to_0"], restart=1), base))
        seq = [((c,), 0, 63, 0, 0) for c in ((0,) if grey else (2, 0, 1))]
        out.append((f"{bname}_sequential_multiscan_rst3", transcode(base, seq, restart=3, sequential=True), base))
    return out
