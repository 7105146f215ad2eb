"""Baseline JPEG files from RGB u8 images on the device, byte for byte what `PIL.Image.save(format="JPEG", quality=q, subsampling=s)`
writes (Pillow on libjpeg-turbo).  The host builds the quantisation tables of a quality and the header, which
depends only on (H, W, tables, subsampling); colour conversion, downsampling, DCT, quantisation, Huffman coding and byte stuffing
run on the GPU (ops.jpeg_encode, csrc/jpeg_enc.hip), and only the coded bytes cross the bus.  optimize=True gives the files of
save(optimize=True), progressive=True those of save(progressive=True): there the host also places the DHT and SOS segments
between the ten scans (progressive_file)."""
import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# T.81 Annex K.1: the two example quantisation tables, natural order
_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18,
         22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103,
         99)
_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + \
    (99,) * 32
# T.81 Annex K.3: (BITS, HUFFVAL) of the four typical Huffman tables, in the order the header lists them
_DC_VALS = bytes(range(12))
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN = ((0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), _DC_VALS),
           (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)), _AC_LUMA_VALS),
           (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), _DC_VALS),
           (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)), _AC_CHROMA_VALS))
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}    # Pillow's subsampling -> the luma sampling factors (h, v); chroma is 1 x 1
LADDER = tuple(range(1, 96))                    # the qualities an anchor search tries


def quant_tables(quality):
    """libjpeg's jpeg_set_quality(quality, force_baseline) -> (2, 64) u16, luma and chroma, natural order"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be in 1..100, got {quality}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_LUMA, _CHROMA], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(H, W, tables, subsampling, huffman=None):
    """everything in front of the entropy-coded segment: SOI, APP0 (JFIF 1.01, no units, 1 x 1), two DQT, SOF0, four DHT, SOS.
    huffman: four (BITS, HUFFVAL) pairs in the order DC0, AC0, DC1, AC1 (an image's optimised tables); None: the Annex K tables"""
    return _header_front(H, W, tables, subsampling) + _header_back(huffman)


_SOS = _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def _header_front(H, W, tables, subsampling, sof=0xC0):
    """SOI .. SOF0 (sof: another frame marker): what an image's Huffman tables do not touch"""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"a JPEG frame is 1..65535 on a side, got {H}x{W}")
    h, v = SAMPLING[int(subsampling)]
    tables = np.asarray(tables)
    assert tables.shape == (2, 64) and tables.min() >= 1 and tables.max() <= 255, "two 8-bit tables in natural order"
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for i in range(2):
        out.append(_segment(0xDB, bytes((i,)) + bytes(int(tables[i][z]) for z in ZIGZAG)))
    out.append(_segment(sof, bytes((8,)) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes((3, 1, h << 4 | v, 0, 2, 0x11, 1, 3, 0x11, 1))))
    return b"".join(out)


def _header_back(huffman=None):
    """the four DHT segments and SOS"""
    if huffman is None:
        huffman = [(bits, vals) for _, bits, vals in HUFFMAN]
    elif len(huffman) != 4 or any(len(bits) != 16 or sum(bits) != len(vals) or len(vals) > 256 for bits, vals in huffman):
        raise ValueError("huffman is four (BITS of 16 counts, HUFFVAL of their sum) pairs")
    out = [_segment(0xC4, bytes((tc_th,)) + bytes(bits) + bytes(vals)) for (tc_th, _, _), (bits, vals) in zip(HUFFMAN, huffman)]
    out.append(_SOS)
    return b"".join(out)


# libjpeg's jpeg_simple_progression for Y Cb Cr: (components, Ss, Se, Ah, Al) of the ten scans Pillow's progressive=True writes
PROGRESSION = (((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
               ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0))


def progressive_file(H, W, tables, subsampling, huffman, segments):
    """a whole progressive file: SOI, APP0, two DQT, SOF2, then per scan its DHT segments (one per table), SOS and entropy-coded
    segment, then EOI.  huffman: the ten (BITS, HUFFVAL) pairs in file order: DC 0 and DC 1 of the first scan, then one AC table for
    every AC scan (id 0 for luma, 1 for chroma); the DC refinement scan has none.  segments: the ten entropy-coded segments."""
    if len(huffman) != 10 or len(segments) != 10 or any(len(b) != 16 or sum(b) != len(v) or len(v) > 256 for b, v in huffman):
        raise ValueError("a progressive file takes ten (BITS of 16 counts, HUFFVAL of their sum) pairs and ten segments")
    out = [_header_front(H, W, tables, subsampling, sof=0xC2)]
    tabs = iter(huffman)
    for (comps, ss, se, ah, al), seg in zip(PROGRESSION, segments):
        if ss == 0:      # a DC scan: the selector names Td; the refinement scan sends raw bits and needs no table
            if ah == 0:
                out += [_segment(0xC4, bytes((th,)) + bytes(b) + bytes(v)) for th, (b, v) in zip((0x00, 0x01), (next(tabs), next(tabs)))]
            sel = bytes(x for c in comps for x in (c + 1, 0 if ah or c == 0 else 0x10))
        else:            # an AC scan: one table, the selector names Ta
            th = 0 if comps[0] == 0 else 1
            b, v = next(tabs)
            out.append(_segment(0xC4, bytes((0x10 | th,)) + bytes(b) + bytes(v)))
            sel = bytes((comps[0] + 1, th))
        out += [_segment(0xDA, bytes((len(comps),)) + sel + bytes((ss, se, ah << 4 | al))), bytes(seg)]
    out.append(b"\xff\xd9")
    return b"".join(out)


def pick_quality(sizes_by_quality, budget):
    """the anchor rule: sizes_by_quality {quality: file size in bytes} -> (quality, over_rate): the largest quality whose file is not
    larger than budget; (the smallest quality, True) if no file fits.  Every entry is looked at: sizes need not grow with quality."""
    if not sizes_by_quality:
        raise ValueError("no sizes to pick from")
    fits = [q for q, size in sizes_by_quality.items() if size <= budget]
    return (max(fits), False) if fits else (min(sizes_by_quality), True)


def _raise_for(err):
    """the encoder's error words, not all zero: 1 a slot was too small, 2 (fitted tables: optimize, progressive) a code past 32 bits
    before limiting"""
    if (np.asarray(err) == 2).any():
        raise RuntimeError("JPEG encoder: a Huffman code longer than 32 bits before the length limiter; libjpeg refuses such an image too")
    raise RuntimeError(f"JPEG encoder: slot overflow, error words {np.asarray(err).ravel().tolist()}")


def encode_scans(rgb_u8, tables, subsampling, optimize=False):
    """(B, H, W, 3) u8 on the device, tables (B, 2, 64) -> list of B bytes objects: entropy-coded segment and EOI.  One read-back of
    the lengths and one of the bytes (the longest segment's length per image, not the slots).  optimize: -> (that list, a list of
    every image's four (BITS, HUFFVAL) pairs); the tables and their counts come back in one more read each."""
    from . import ops
    buf, lens, err, *tabs = ops.jpeg_encode(rgb_u8, tables, subsampling, optimize)
    lens_h, err_h = lens.cpu().numpy(), err.cpu().numpy()
    if err_h.any():
        _raise_for(err_h)
    host = buf[:, :int(lens_h.max())].cpu().numpy()
    scans = [host[b, :int(n)].tobytes() for b, n in enumerate(lens_h)]
    if not optimize:
        return scans
    raw, nval = tabs[0].cpu().numpy().tobytes(), tabs[1].cpu().numpy().ravel().tolist()      # 272 bytes and one count per table
    pairs = [(raw[o:o + 16], raw[o + 16:o + 16 + n]) for o, n in zip(range(0, len(raw), 272), nval)]
    return scans, [pairs[4 * b:4 * b + 4] for b in range(len(scans))]


def encode_progressive(rgb_u8, tables, subsampling):
    """(B, H, W, 3) u8 on the device, tables (B, 2, 64) -> list of B whole progressive files.  The lengths, error words and table
    counts come back in one read, the tables in one, the coded bytes in one (the longest image's, not the slots)."""
    import torch

    from . import ops
    buf, lens, err, huff, nval = ops.jpeg_encode(rgb_u8, tables, subsampling, progressive=True)
    B, H, W, _ = rgb_u8.shape
    meta = torch.cat([lens, nval, err[:, None]], dim=1).cpu().numpy()
    lens_h, nval_h, err_h = meta[:, :10], meta[:, 10:20], meta[:, 20]
    if err_h.any():
        _raise_for(err_h)
    host = buf[:, :int(lens_h.sum(axis=1).max())].cpu().numpy()
    raw = huff.cpu().numpy()
    files = []
    for b in range(B):
        ends = np.cumsum(lens_h[b])
        segments = [host[b, e - n:e].tobytes() for e, n in zip(ends, lens_h[b])]
        pairs = [(raw[b, j, :16].tobytes(), raw[b, j, 16:16 + int(n)].tobytes()) for j, n in enumerate(nval_h[b])]
        files.append(progressive_file(H, W, tables[b], subsampling, pairs, segments))
    return files


def encode_batch(rgb_u8, quality, subsampling=2, optimize=False, progressive=False):
    """(B, H, W, 3) u8 RGB on the device -> list of B whole JPEG files (bytes).  quality: an int, or one int per image.  optimize:
    the files of Pillow's save(optimize=True), every image with Huffman tables fitted to it.  progressive: the files of Pillow's
    save(progressive=True), ten scans with tables fitted to every scan; optimize changes nothing then, as in Pillow."""
    assert rgb_u8.dim() == 4 and rgb_u8.shape[3] == 3, "images are (B, H, W, 3)"
    B, H, W, _ = rgb_u8.shape
    qs = [int(quality)] * B if np.ndim(quality) == 0 else [int(q) for q in quality]
    if len(qs) != B:
        raise ValueError(f"{len(qs)} qualities for {B} images")
    if int(subsampling) not in SAMPLING:
        raise ValueError(f"subsampling must be 0, 1 or 2, got {subsampling}")
    by_q = {q: quant_tables(q) for q in set(qs)}
    tables = np.stack([by_q[q] for q in qs])
    if progressive:
        return encode_progressive(rgb_u8.contiguous(), tables, int(subsampling))
    if optimize:
        scans, huffman = encode_scans(rgb_u8.contiguous(), tables, int(subsampling), True)
        fronts = {q: _header_front(H, W, t, subsampling) for q, t in by_q.items()}
        return [fronts[q] + _header_back(hf) + s for q, s, hf in zip(qs, scans, huffman)]
    heads = {q: header(H, W, t, subsampling) for q, t in by_q.items()}
    scans = encode_scans(rgb_u8.contiguous(), tables, int(subsampling))
    return [heads[q] + s for q, s in zip(qs, scans)]


def ladder_sizes(rgb_u8, subsampling=2, qualities=LADDER, max_slot_bytes=1 << 30, optimize=False):
    """file size of every image at every quality -> (B, len(qualities)) int64 numpy array.  The images are encoded at several
    qualities per call (per-image tables), as many as keep the output slots below max_slot_bytes; only the lengths are read back.
    optimize: sizes with fitted Huffman tables; the header's length is then per (image, quality), from the four HUFFVAL counts,
    which are read back with the lengths."""
    import ctypes

    import torch

    from . import ops
    from ._lib import call
    B, H, W, _ = rgb_u8.shape
    cap = ctypes.c_size_t(0)
    call("sgic_jpeg_encode_opt_cap" if optimize else "sgic_jpeg_encode_cap", H, W, int(subsampling), ctypes.byref(cap))
    per_call = max(1, min(len(qualities), max_slot_bytes // (cap.value * B)))
    x = rgb_u8.contiguous()
    sizes = np.zeros((B, len(qualities)), dtype=np.int64)
    pending = []
    for s in range(0, len(qualities), per_call):
        qs = qualities[s:s + per_call]
        tabs = np.stack([quant_tables(q) for q in qs])                         # (n, 2, 64)
        rep = x.unsqueeze(0).expand(len(qs), B, H, W, 3).reshape(len(qs) * B, H, W, 3).contiguous()
        _, lens, err, *huff = ops.jpeg_encode(rep, np.repeat(tabs, B, axis=0), int(subsampling), optimize)
        rows = [lens, err]
        if optimize:        # the file's four HUFFVAL counts
            rows.append(huff[1].sum(dim=1, dtype=torch.int32))
        pending.append((s, qs, torch.stack(rows)))
    for s, qs, le in pending:
        le = le.cpu().numpy().reshape(-1, len(qs), B)
        if le[1].any():
            _raise_for(le[1])
        for j, q in enumerate(qs):
            if optimize:    # the header of a file: the front, four DHT segments of 2 + 2 + 1 + 16 bytes and their HUFFVAL, SOS
                sizes[:, s + j] = le[0, j] + len(_header_front(H, W, quant_tables(q), subsampling)) + 4 * 21 + le[2, j] + len(_SOS)
            else:
                sizes[:, s + j] = le[0, j] + len(header(H, W, quant_tables(q), subsampling))
    return sizes
