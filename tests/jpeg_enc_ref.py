"""A numpy restatement of baseline JPEG encoding as libjpeg does it with its integer arithmetic (jccolor, jcsample without smoothing,
jfdctint, the Annex K Huffman tables): the whole file that `PIL.Image.save(format="JPEG", quality=q, subsampling=s)` writes.  It
imports nothing from the package; the GPU encoder and the package's header builder are compared with it and with Pillow."""
import io

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
             62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
             112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
               99] + [99] * 32
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
            0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
            0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
            0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
            0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
            0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
            0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
              0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
              0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
              0xf9, 0xfa])
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}       # Pillow's subsampling -> luma (h, v)

# (H, W, quality, subsampling); each runs as a natural-like image, as noise and as a flat image
CASES = [(1, 1, 75, 2), (8, 8, 75, 0), (8, 8, 50, 2), (16, 16, 75, 2), (8, 24, 70, 2), (24, 8, 70, 2), (10, 10, 80, 2), (17, 9, 60, 2),
         (9, 17, 90, 2), (12, 20, 30, 1), (37, 53, 90, 0), (40, 72, 60, 1), (33, 47, 85, 2), (41, 29, 1, 2), (24, 40, 100, 0),
         (31, 33, 5, 1), (64, 48, 95, 2)]
KINDS = ("natural", "noise", "flat")


def image(kind, h, w, seed):
    """-> (h, w, 3) u8"""
    rng = np.random.default_rng(seed)
    if kind == "natural":
        import jpeg_cases
        return jpeg_cases.natural_like(h, w, rng)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3).astype(np.uint8), (h, w, 3)).copy()
    if kind == "sparse":       # a mid-grey field with one sharp corner: long zero runs between the few high coefficients
        a = np.full((h, w, 3), 128, np.uint8)
        a[::8, ::8] = 255
        return a
    raise ValueError(kind)


def case_images():
    """-> [(id, (h, w, 3) u8, quality, subsampling)]: the case list in its three kinds, and one sparse image for runs past 15"""
    out = []
    for i, (h, w, q, s) in enumerate(CASES):
        for k, kind in enumerate(KINDS):
            out.append((f"{h}x{w}_q{q}_s{s}_{kind}", image(kind, h, w, 1000 + 10 * i + k), q, s))
    out.append(("32x32_q100_s0_sparse", image("sparse", 32, 32, 0), 100, 0))
    return out


def pillow_bytes(rgb, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality), subsampling=int(subsampling))
    return buf.getvalue()


def quant_tables(quality):
    """jpeg_set_quality(force_baseline) -> (2, 64) u16 in natural order"""
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([BASE_LUMA, BASE_CHROMA], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


def huff_codes(bits, vals):
    """-> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(H, W, tables, subsampling):
    h, v = SAMPLING[subsampling]
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += _seg(0xDB, bytes([i]) + bytes(int(tables[i][z]) for z in ZIGZAG))
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, h << 4 | v, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def planes(rgb, subsampling):
    """-> the three component planes over whole MCUs, edges replicated as libjpeg does"""
    H, W, _ = rgb.shape
    h, v = SAMPLING[subsampling]
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    Hv = -(-H // v) * v
    yy = np.minimum(np.arange(Hv), H - 1)
    xx = np.minimum(np.arange(mx * 8 * h), W - 1)
    y, cb, cr = (p[yy][:, xx] for p in ycc(rgb))
    out = [y[np.minimum(np.arange(my * 8 * v), Hv - 1)]]
    for c in (cb, cr):
        if (h, v) == (2, 1):
            c = (c[:, 0::2] + c[:, 1::2] + (np.arange(c.shape[1] // 2) & 1)) >> 1
        elif (h, v) == (2, 2):
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 1 + (np.arange(c.shape[1] // 2) & 1)) >> 2
        out.append(c[np.minimum(np.arange(my * 8), c.shape[0] - 1)])
    return out


def _pass(d, first):
    """one jfdctint pass along the last axis of d (..., 8) int64"""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, n)
    o[6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(plane, q):
    """plane (8r, 8c) -> (r, c, 64) quantised coefficients in zigzag order"""
    r, c = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(r, 8, c, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    d = _pass(blk, True)
    d = _pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2).reshape(r, c, 64)
    div = 8 * q.astype(np.int64)
    mag = (np.abs(d) + (div >> 1)) // div
    return (np.sign(d) * mag)[..., ZIGZAG]


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out, self.stuffed = 0, 0, bytearray(), 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def encode_scan(rgb, tables, subsampling):
    """-> (the entropy-coded segment, {"zrl": count of F0 symbols, "stuffed": count of stuffed bytes})"""
    H, W, _ = rgb.shape
    h, v = SAMPLING[subsampling]
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    comp = planes(rgb, subsampling)
    coef = [fdct_quant(comp[0], tables[0]), fdct_quant(comp[1], tables[1]), fdct_quant(comp[2], tables[1])]
    wb, hb = -(-W // 8), -(-H // 8)
    dc = [huff_codes(*DC_LUMA), huff_codes(*DC_CHROMA)]
    ac = [huff_codes(*AC_LUMA), huff_codes(*AC_CHROMA)]
    bw = BitWriter()
    zrl = 0
    pred = [0, 0, 0]
    for j in range(my):
        for i in range(mx):
            blocks = []
            for dy in range(v):
                for dx in range(h):
                    by, bx = j * v + dy, i * h + dx
                    if by < hb and bx < wb:
                        blocks.append((0, coef[0][by, bx]))
                    else:                                   # a dummy block: the DC of the block before it in the MCU, no AC
                        z = np.zeros(64, np.int64)
                        z[0] = blocks[-1][1][0]
                        blocks.append((0, z))
            blocks += [(1, coef[1][j, i]), (2, coef[2][j, i])]
            for ci, b in blocks:
                t = 0 if ci == 0 else 1
                diff = int(b[0]) - pred[ci]
                pred[ci] = int(b[0])
                n = abs(diff).bit_length()
                bw.put(*dc[t][n])
                if n:
                    bw.put(diff if diff > 0 else diff - 1, n)
                run = 0
                for k in range(1, 64):
                    val = int(b[k])
                    if val == 0:
                        run += 1
                        continue
                    while run > 15:
                        bw.put(*ac[t][0xF0])
                        zrl += 1
                        run -= 16
                    n = abs(val).bit_length()
                    bw.put(*ac[t][run << 4 | n])
                    bw.put(val if val > 0 else val - 1, n)
                    run = 0
                if run:
                    bw.put(*ac[t][0])
    bw.flush()
    return bytes(bw.out), {"zrl": zrl, "stuffed": bw.stuffed}


def encode(rgb, quality, subsampling):
    """-> (the whole file, the counters of encode_scan)"""
    tables = quant_tables(quality)
    scan, stats = encode_scan(rgb, tables, subsampling)
    return header(rgb.shape[0], rgb.shape[1], tables, subsampling) + scan + b"\xff\xd9", stats
