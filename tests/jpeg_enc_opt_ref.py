"""A numpy restatement of JPEG encoding with optimised Huffman tables as libjpeg does it (two passes: the statistics of the scan's
own symbols, then jpeg_gen_optimal_table per histogram): the whole file that `PIL.Image.save(format="JPEG", quality=q,
subsampling=s, optimize=True)` writes.  Everything in front of the entropy coder is jpeg_enc_ref's.  It imports nothing from the
package; the GPU encoder and the package's header builder are compared with it and with Pillow."""
import io

import numpy as np

import jpeg_enc_ref as ref


def pillow_bytes(rgb, quality, subsampling):
    """Pillow sizes its output buffer from the image when optimize is set and fails on files past it (q >= 95 on noise), so the
    block size is raised for the call and put back"""
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 1 << 16, 16 * rgb.shape[0] * rgb.shape[1])
    try:
        Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality), subsampling=int(subsampling), optimize=True)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


def symbols(rgb, tables, subsampling):
    """the scan as a list of (table 0 / 1, is AC, symbol, extra bits, number of extra bits), dummy blocks included"""
    H, W, _ = rgb.shape
    h, v = ref.SAMPLING[subsampling]
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    comp = ref.planes(rgb, subsampling)
    coef = [ref.fdct_quant(comp[0], tables[0]), ref.fdct_quant(comp[1], tables[1]), ref.fdct_quant(comp[2], tables[1])]
    wb, hb = -(-W // 8), -(-H // 8)
    out = []
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
                out.append((t, 0, n, diff if diff > 0 else diff - 1, n))
                run = 0
                for k in range(1, 64):
                    val = int(b[k])
                    if val == 0:
                        run += 1
                        continue
                    while run > 15:
                        out.append((t, 1, 0xF0, 0, 0))
                        run -= 16
                    n = abs(val).bit_length()
                    out.append((t, 1, run << 4 | n, val if val > 0 else val - 1, n))
                    run = 0
                if run:
                    out.append((t, 1, 0x00, 0, 0))
    return out


def histograms(syms):
    """-> (2, 2, 256) int64: [is AC][table][symbol]"""
    hist = np.zeros((2, 2, 256), np.int64)
    for t, is_ac, s, _, _ in syms:
        hist[is_ac, t, s] += 1
    return hist


def optimal_table(freq256):
    """jpeg_gen_optimal_table: 256 counts -> (BITS (16 ints), HUFFVAL (list), the longest code size before limiting)"""
    freq = [int(f) for f in freq256] + [1]         # the pseudo-symbol 256: no code is all ones
    size = [0] * 257
    tree = [[s] for s in range(257)]

    def smallest(skip):
        best = -1
        for s in range(257):
            if freq[s] and s != skip and (best < 0 or freq[s] <= freq[best]):     # on a tie the larger symbol
                best = s
        return best

    while True:
        c1 = smallest(-1)
        c2 = smallest(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        tree[c1] += tree[c2]
        tree[c2] = []
        for s in tree[c1]:
            size[s] += 1
    longest = max(size)
    bits = [0] * (max(longest, 16) + 1)
    for s in range(257):
        if size[s]:
            bits[size[s]] += 1
    for i in range(len(bits) - 1, 16, -1):
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
    bits[i] -= 1
    vals = [s for ln in range(1, longest + 1) for s in range(256) if size[s] == ln]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals, longest


def tables_of(hist):
    """-> ([(BITS, HUFFVAL)] in the header's order DC0, AC0, DC1, AC1, the longest unlimited code size of the four)"""
    out, longest = [], 0
    for t in range(2):
        for is_ac in range(2):
            bits, vals, ln = optimal_table(hist[is_ac, t])
            out.append((bits, vals))
            longest = max(longest, ln)
    return out, longest


def header(H, W, tables, subsampling, huffman):
    h, v = ref.SAMPLING[subsampling]
    out = b"\xff\xd8" + ref._seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += ref._seg(0xDB, bytes([i]) + bytes(int(tables[i][z]) for z in ref.ZIGZAG))
    out += ref._seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, h << 4 | v, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), huffman):
        out += ref._seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + ref._seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(rgb, quality, subsampling):
    """-> (the whole file, {"huffman": the four (BITS, HUFFVAL), "longest": the longest code size before limiting})"""
    tables = ref.quant_tables(quality)
    syms = symbols(rgb, tables, subsampling)
    huffman, longest = tables_of(histograms(syms))
    codes = [[ref.huff_codes(*huffman[2 * t + is_ac]) for t in range(2)] for is_ac in range(2)]
    bw = ref.BitWriter()
    for t, is_ac, s, extra, n in syms:
        bw.put(*codes[is_ac][t][s])
        if n:
            bw.put(extra, n)
    bw.flush()
    head = header(rgb.shape[0], rgb.shape[1], tables, subsampling, huffman)
    return head + bytes(bw.out) + b"\xff\xd9", {"huffman": huffman, "longest": longest}
