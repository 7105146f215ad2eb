"""Host side of the GPU JPEG decoder (csrc/jpeg.hip): marker parsing, Huffman lookup tables, removal of the 0xFF00
byte stuffing / RSTn markers -- byte shuffling only, no entropy decoding -- and the batch descriptor the kernels read.

Supported on the GPU (everything Pillow's `save(..., "JPEG")` and ordinary cameras / encoders write): baseline or extended-sequential
Huffman JPEG, 8-bit, one interleaved scan, greyscale or YCbCr with 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0 sampling, restart intervals,
custom Huffman / quantisation tables.  Anything else (progressive, arithmetic coding, CMYK / YCCK, RGB-coded, 12-bit, multi-scan,
chroma planes too narrow for the fancy upsampler) raises `Unsupported`, and the ingest falls back to the host decoder for that
batch -- the result is the same pixels either way, the GPU path being bit-exact with Pillow (tests/test_gpu_jpeg.py).

Files are untrusted input.  Also refused (`Unsupported`, never a bare IndexError), so that a damaged file reaches the host decoder and
its proper error instead of a kernel: a file cut short (no marker ends the entropy-coded segment, a marker segment longer than the
file, a truncated SOS / SOF / DHT / DQT / DRI payload), Tq > 3, Th > 3 or Tc > 1, DHT counts above 256 or above what the segment holds,
a DC table with a symbol above 15, H == 0 or W == 0, RSTn markers without a restart interval or not numbered 0, 1, .. 7, 0, ..  What
a parser cannot see -- a scan that ends before its last MCU in front of an intact EOI -- the kernels report as error code 3: they
compare the bytes consumed with the scan's unpadded length (P_SCAN_BYTES / S_SCAN_BYTES).  tests/jpeg_forge.py forges such files.

parse_scans() / ScanJpegBatch take progressive Huffman and multi-scan sequential files as well (and baseline files as one scan, so that
mixed batches decode together): one descriptor per scan, decoded by csrc/jpeg.hip jpeg_scan_kernel (tests/test_gpu_jpeg_scans.py)."""
import struct

import numpy as np

NP = 64
LOOK = 9
TAB_BYTES = 1424
CHUNK = 2048
P_SCAN_OFF, P_SCAN_LEN, P_TAB_OFF, P_QUANT_OFF, P_NCOMP, P_W, P_H, P_HMAX, P_VMAX, P_MCUS_X, P_MCUS_Y, P_RESTART, P_SEG_OFF, P_NSEG = range(14)
P_SCAN_BYTES = 14        # the scan's own length, without the zero padding of P_SCAN_LEN: decoding past it is error code 3
P_COMP0, P_CSTRIDE = 16, 12

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
                   56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)


class Unsupported(ValueError):
    """a JPEG variant the GPU decoder does not take (the caller decodes it on the host instead)"""


def huff_table(bits, vals):
    """JPEG DHT (16 code-length counts + symbols) -> the 1424-byte table of csrc/jpeg.hip:
    u16 fast[512] (nbits << 8 | symbol for codes of <= 9 bits, else 0) | i32 maxcode[18] | i32 valoff[17] | pad | u8 huffval[256]
    (the canonical code assignment of ITU T.81 Annex C, as jdhuff.c jpeg_make_d_derived_tbl)"""
    fast = np.zeros(1 << LOOK, dtype=np.uint16)
    maxcode = np.full(18, -1, dtype=np.int32)
    valoff = np.zeros(17, dtype=np.int32)
    huffval = np.zeros(256, dtype=np.uint8)
    huffval[:len(vals)] = vals
    code, k = 0, 0
    for l in range(1, 17):
        n = int(bits[l - 1])
        if n:
            valoff[l] = k - code
            for _ in range(n):
                if l <= LOOK:
                    lo = code << (LOOK - l)
                    fast[lo:lo + (1 << (LOOK - l))] = (l << 8) | int(vals[k])
                code += 1
                k += 1
            maxcode[l] = code - 1
        if code > (1 << l):
            raise Unsupported("bad Huffman table")
        code <<= 1
    maxcode[17] = 0x7fffffff
    out = np.zeros(TAB_BYTES, dtype=np.uint8)
    out[0:1024] = fast.view(np.uint8)
    out[1024:1096] = maxcode.view(np.uint8)
    out[1096:1164] = valoff.view(np.uint8)
    out[1168:1424] = huffval
    return out


class Parsed:
    __slots__ = ("W", "H", "ncomp", "comps", "hmax", "vmax", "quant", "tabs", "scan", "segs", "restart", "mcus_x", "mcus_y")


def _frame_geometry(frame, adobe_transform):
    """SOF (H, W, [(id, h, v, tq)]) -> (H, W, ncomp, hmax, vmax, comps); raises Unsupported for layouts outside the GPU path"""
    H, W, comps = frame
    nc = len(comps)
    if nc not in (1, 3):
        raise Unsupported(f"{nc} components")
    if nc == 3:
        ids = [c[0] for c in comps]
        if adobe_transform == 0 or (adobe_transform is None and ids == [ord("R"), ord("G"), ord("B")]):
            raise Unsupported("RGB-coded JPEG")
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if nc == 3:
        if (comps[0][1], comps[0][2]) != (hmax, vmax) or (comps[1][1:3] != comps[2][1:3]) or comps[1][1:3] != (1, 1) or hmax > 2 or vmax > 2:
            raise Unsupported("sampling factors outside 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0")
    else:
        hmax = vmax = 1                      # a single-component scan is never interleaved (T.81 A.2.2)
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    for (cid, h, v, tq) in comps:
        if (h < hmax or v < vmax) and -(-W * h // hmax) <= 2:
            raise Unsupported("chroma plane too narrow for the fancy upsampler")
    return H, W, nc, hmax, vmax, comps


# ---- checks on untrusted marker segments, shared by parse() and parse_scans(): a damaged file is refused (Unsupported), never
# ---- indexed past its end and never handed to a kernel with a table index or a symbol the kernels do not expect ----------------------
def _marker_segment(data, pos):
    """marker segment whose 2-byte length field is at `pos` -> (length, payload); the segment must lie inside the file"""
    if pos + 2 > len(data):
        raise Unsupported("truncated marker segment")
    ln = struct.unpack(">H", data[pos:pos + 2])[0]
    if ln < 2 or pos + ln > len(data):
        raise Unsupported("marker segment runs past the end of the file")
    return ln, data[pos + 2:pos + ln]


def _dqt_tables(seg):
    """DQT payload -> [(Tq, (64,) u16 table in natural order)]"""
    out, i = [], 0
    while i < len(seg):
        pq, tq = seg[i] >> 4, seg[i] & 15
        i += 1
        if tq > 3 or pq > 1:
            raise Unsupported("bad quantisation table id / precision")
        nb = 128 if pq else 64
        if i + nb > len(seg):
            raise Unsupported("truncated DQT")
        t = np.frombuffer(seg[i:i + nb], dtype=">u2" if pq else np.uint8).astype(np.uint16)
        i += nb
        nat = np.zeros(64, dtype=np.uint16)
        nat[ZIGZAG] = t
        out.append((tq, nat))
    return out


def _dht_tables(seg):
    """DHT payload -> [(Tc, Th, bits u8[16], symbols u8[sum(bits)])]"""
    out, i = [], 0
    while i < len(seg):
        if i + 17 > len(seg):
            raise Unsupported("truncated DHT")
        tc, th = seg[i] >> 4, seg[i] & 15
        if th > 3 or tc > 1:
            raise Unsupported("bad Huffman table slot")
        bits = np.frombuffer(seg[i + 1:i + 17], dtype=np.uint8)
        cnt = int(bits.sum())
        if cnt > 256 or i + 17 + cnt > len(seg):
            raise Unsupported("Huffman table with more symbols than 256 or than its segment holds")
        out.append((tc, th, bits, np.frombuffer(seg[i + 17:i + 17 + cnt], dtype=np.uint8)))
        i += 17 + cnt
    return out


def _sof_frame(seg):
    """SOF payload -> (H, W, [(id, h, v, Tq)]) of an 8-bit frame"""
    if len(seg) < 6:
        raise Unsupported("truncated SOF")
    prec, H, W, nc = struct.unpack(">BHHB", seg[:6])
    if prec != 8:
        raise Unsupported("not 8-bit")
    if len(seg) < 6 + 3 * nc:
        raise Unsupported("truncated SOF")
    if H == 0 or W == 0:
        raise Unsupported("empty frame (or a height left to a DNL marker)")
    comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
    if any(tq > 3 for _, _, _, tq in comps):
        raise Unsupported("bad quantisation table id")
    return H, W, comps


def _sos_header(seg):
    """SOS payload -> ([(component id, Td, Ta)], Ss, Se, Ah << 4 | Al)"""
    ns = seg[0] if len(seg) else 0
    if len(seg) < 4 + 2 * ns:
        raise Unsupported("truncated SOS")
    sel = [(seg[1 + 2 * c], seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
    return sel, seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]


def _restart_interval(seg):
    if len(seg) < 2:
        raise Unsupported("truncated DRI")
    return struct.unpack(">H", seg[:2])[0]


def _check_dc_table(tab):
    """a table used as a DC table codes a magnitude category: a symbol above 15 is corrupt (jdhuff.c jpeg_make_d_derived_tbl) and
    would have the kernels read that many extra bits"""
    if int(tab[1168:1424].max()) > 15:
        raise Unsupported("DC Huffman table with a symbol above 15")


def _clean_segment(data, pos, restart):
    """entropy-coded segment starting at byte `pos` -> (cleaned u8 bytes, restart offsets i32, position of the marker ending it).
    The segment runs up to the marker that is not RSTn / stuffing; un-stuff, drop the RSTn markers and remember where each restart
    interval starts in the cleaned stream.  `restart`: the restart interval in force.  Raises Unsupported when no marker ends the
    segment (a truncated file), when it holds RSTn markers although restart == 0, or when they are not numbered 0, 1, .. 7, 0, ..
    (libjpeg resynchronises on those, which the GPU path does not restate)"""
    if pos >= len(data):
        raise Unsupported("file ends at the scan header")
    raw = np.frombuffer(data, dtype=np.uint8, offset=pos)
    ff = np.nonzero(raw[:-1] == 0xFF)[0]
    nxt = raw[ff + 1]
    stop = ff[(nxt != 0) & ~((nxt >= 0xD0) & (nxt <= 0xD7)) & (nxt != 0xFF)]
    if not len(stop):
        raise Unsupported("truncated file: no marker ends the entropy-coded segment")
    end = int(stop[0])
    raw = raw[:end]
    ff = ff[ff < end - 1] if end > 0 else ff[:0]
    nxt = raw[ff + 1] if len(ff) else nxt[:0]
    keep = np.ones(len(raw), dtype=bool)
    stuffed = ff[nxt == 0]
    keep[stuffed + 1] = False
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7)]
    if len(rst) and (restart == 0 or (raw[rst + 1] != 0xD0 + (np.arange(len(rst)) & 7)).any()):
        raise Unsupported("restart markers without a restart interval, or out of sequence")
    keep[rst] = False
    keep[rst + 1] = False
    keep[ff[nxt == 0xFF]] = False                   # fill bytes (an 0xFF in front of another 0xFF) are not data (T.81 B.1.1.2)
    newpos = np.cumsum(keep) - keep                 # position of every original byte in the cleaned stream
    segs = np.concatenate([[0], newpos[rst]]).astype(np.int32) if len(rst) else np.zeros(1, dtype=np.int32)
    return raw[keep], segs, pos + end


def parse(data):
    """bytes of one JPEG file -> Parsed (tables, geometry, cleaned scan); raises Unsupported for variants outside the GPU path"""
    if data[:2] != b"\xff\xd8":
        raise Unsupported("not a JPEG")
    qt = {}
    ht = {}
    restart = 0
    frame = None
    adobe_transform = None
    pos = 2
    n = len(data)
    while True:
        if pos + 4 > n:
            raise Unsupported("truncated before SOS")
        if data[pos] != 0xFF:
            raise Unsupported("marker expected")
        while pos + 2 < n and data[pos + 1] == 0xFF:
            pos += 1
        m = data[pos + 1]
        pos += 2
        if m in (0x01,) or 0xD0 <= m <= 0xD7:
            continue
        ln, seg = _marker_segment(data, pos)
        if m == 0xDB:
            qt.update(_dqt_tables(seg))
        elif m == 0xC4:
            for tc, th, bits, vals in _dht_tables(seg):
                if th > 1:
                    raise Unsupported("more than two Huffman tables per class")
                ht[(tc, th)] = huff_table(bits, vals)
        elif m in (0xC0, 0xC1):
            frame = _sof_frame(seg)
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported("progressive / lossless / arithmetic JPEG")
        elif m == 0xDD:
            restart = _restart_interval(seg)
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe_transform = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Unsupported("SOS before SOF")
            sel, ss, se, ahal = _sos_header(seg)
            H, W, comps = frame
            if len(sel) != len(comps):
                raise Unsupported("non-interleaved multi-scan file")
            sel = {cid: (td, ta) for cid, td, ta in sel}
            if (ss, se, ahal) != (0, 63, 0):
                raise Unsupported("not a sequential scan")
            pos += ln
            break
        elif m == 0xD9:
            raise Unsupported("EOI before SOS")
        pos += ln
    H, W, nc, hmax, vmax, comps = _frame_geometry(frame, adobe_transform)
    p = Parsed()
    p.W, p.H, p.ncomp, p.hmax, p.vmax, p.restart = W, H, nc, hmax, vmax, restart
    p.mcus_x, p.mcus_y = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    p.comps = []
    for (cid, h, v, tq) in comps:
        if tq not in qt or cid not in sel or (0, sel[cid][0]) not in ht or (1, sel[cid][1]) not in ht:
            raise Unsupported("missing table")
        cw, ch = -(-W * h // hmax), -(-H * v // vmax)
        p.comps.append(dict(h=h, v=v, tq=tq, dc=sel[cid][0], ac=sel[cid][1], bw=p.mcus_x * h, bh=p.mcus_y * v, cw=cw, ch=ch))
    p.quant = np.zeros((4, 64), dtype=np.uint16)
    for k, t in qt.items():
        if k < 4:
            p.quant[k] = t
    p.tabs = np.zeros((4, TAB_BYTES), dtype=np.uint8)
    for (tc, th), t in ht.items():
        p.tabs[2 * tc + th] = t
    for d in p.comps:
        _check_dc_table(p.tabs[d["dc"]])
    p.scan, p.segs, _ = _clean_segment(data, pos, restart)
    if restart and len(p.segs) < -(-p.mcus_x * p.mcus_y // restart):
        raise Unsupported("restart markers missing")
    return p


def _geometry(ps, canvas):
    """-> ((H, W) of the decoded batch, per-image extents int32 (B, 2)).  Without a canvas every file must have one size.  With
    canvas = (H, W) each file (its own P_W x P_H in its params) is decoded at the top left of an H x W canvas it must fit in; the
    canvas outside an image's extent is NOT written (it holds whatever the output buffer held): a consumer reads each image within
    its extent only, as ops.u8canvas_to_f32chw_pad does"""
    hw = np.array([(p.H, p.W) for p in ps], dtype=np.int32).reshape(len(ps), 2)
    if canvas is None:
        if (hw != hw[0]).any():
            raise ValueError("a JPEG batch shares one geometry")
        return (int(hw[0, 0]), int(hw[0, 1])), hw
    H, W = int(canvas[0]), int(canvas[1])
    if (hw[:, 0] > H).any() or (hw[:, 1] > W).any():
        raise ValueError(f"an image of the batch is larger than the {H}x{W} canvas")
    return (H, W), hw


class JpegBatch:
    """host-side descriptor of a batch of equal-geometry JPEGs (or of JPEGs on one canvas): ONE contiguous blob
        params (B x 64 i32) | restart offsets (i32) | quant tables (B x 256 u16) | Huffman lookup tables (B x 4 x 1424 B) | cleaned scans
    so that the batch crosses PCIe in a single copy.  `alloc(nbytes) -> uint8 torch tensor` supplies the staging memory: the ingest
    passes PINNED slot buffers -- a copy from pageable memory is synchronous in HIP and, measured in the CLI trace, waited for the
    previous batch's GPU work (the decode then ran alone instead of under it)."""

    def __init__(self, datas, pool=None, alloc=None, canvas=None):
        """canvas = (H, W): files of different sizes, each decoded at the top left of an H x W canvas (_geometry)"""
        import torch
        ps = list(pool.map(parse, datas)) if pool is not None else [parse(d) for d in datas]
        self.last_err = None
        B = len(ps)
        (self.H, self.W), self.hw = _geometry(ps, canvas)
        self.B = B
        nseg = sum(len(p.segs) for p in ps)
        scan_len = [len(p.scan) + ((-len(p.scan)) % CHUNK or (CHUNK if len(p.scan) == 0 else 0)) for p in ps]
        al = lambda n: (n + 255) & ~255
        self.off_params, n = 0, al(B * NP * 4)
        self.off_segs, n = n, n + al(nseg * 4)
        self.off_quant, n = n, n + al(B * 256 * 2)
        self.off_tabs, n = n, n + al(B * 4 * TAB_BYTES)
        self.off_scan, n = n, n + sum(scan_len)
        self.nseg, self.nbytes = nseg, n
        blob = alloc(n + al(4 * B)) if alloc is not None else torch.empty(n + al(4 * B), dtype=torch.uint8)
        self.blob = blob[:n]
        self.err_host = blob[n:n + 4 * B].view(torch.int32)     # the error codes come back into the same (pinned) staging buffer
        host = self.blob.numpy()
        host[:self.off_scan] = 0
        params = host[self.off_params:self.off_params + B * NP * 4].view(np.int32).reshape(B, NP)
        segs = host[self.off_segs:self.off_segs + nseg * 4].view(np.int32)
        quant = host[self.off_quant:self.off_quant + B * 512].view(np.uint16).reshape(B, 256)
        tabs = host[self.off_tabs:self.off_tabs + B * 4 * TAB_BYTES].reshape(B, 4 * TAB_BYTES)
        scan = host[self.off_scan:]
        scan_off = seg_off = blk_off = plane_off = 0
        self.max_blocks = 0
        for b, p in enumerate(ps):
            r = params[b]
            r[P_SCAN_OFF], r[P_SCAN_LEN], r[P_TAB_OFF], r[P_QUANT_OFF] = scan_off, scan_len[b], b * 4 * TAB_BYTES, b * 256
            r[P_NCOMP], r[P_W], r[P_H], r[P_HMAX], r[P_VMAX] = p.ncomp, p.W, p.H, p.hmax, p.vmax
            r[P_MCUS_X], r[P_MCUS_Y], r[P_RESTART], r[P_SEG_OFF], r[P_NSEG] = p.mcus_x, p.mcus_y, p.restart, seg_off, len(p.segs)
            r[P_SCAN_BYTES] = len(p.scan)
            nblk = 0
            for c, d in enumerate(p.comps):
                o = P_COMP0 + c * P_CSTRIDE
                r[o:o + 11] = [d["h"], d["v"], d["tq"], d["dc"], d["ac"], d["bw"], d["bh"], d["cw"], d["ch"], blk_off + nblk, plane_off]
                nblk += d["bw"] * d["bh"]
                plane_off += (d["bw"] * 8 * d["bh"] * 8 + 15) & ~15
            self.max_blocks = max(self.max_blocks, nblk)
            blk_off += nblk
            scan[scan_off:scan_off + len(p.scan)] = p.scan
            scan[scan_off + len(p.scan):scan_off + scan_len[b]] = 0
            segs[seg_off:seg_off + len(p.segs)] = p.segs
            quant[b] = p.quant.reshape(-1)
            tabs[b] = p.tabs.reshape(-1)
            scan_off += scan_len[b]
            seg_off += len(p.segs)
        self.params, self.tabs, self.scan = params, tabs.reshape(-1), scan     # host views (tests)
        self.total_blocks, self.plane_bytes = blk_off, plane_off

    def decode(self, device, out=None, check=True):
        """-> (B, H, W, 3) u8 device tensor on the current stream.  check=True synchronises and raises if a stream is corrupt;
        check=False leaves the per-image error codes in self.last_err (device int32 tensor) for the caller to read later"""
        import torch
        from . import ops
        # a PINNED blob is read by the kernels in place (device-accessible host memory: no H2D copy to schedule -- an SDMA copy would
        # queue behind the previous batch's result copies and start the decode only when that batch has finished); else one copy
        dev = torch.device(device)
        with torch.cuda.device(dev):
            return self._decode(self.blob if self.blob.is_pinned() else self.blob.to(dev, non_blocking=True), out, check)

    def _decode(self, d, out, check):
        from . import ops
        B = self.B
        view = lambda off, nbytes: d[off:off + nbytes]
        params = view(self.off_params, B * NP * 4)
        segs = view(self.off_segs, max(4, self.nseg * 4))
        quant = view(self.off_quant, B * 512)
        tabs = view(self.off_tabs, B * 4 * TAB_BYTES)
        scan = d[self.off_scan:]
        out, self.last_err = ops.jpeg_decode_batch(params, scan, tabs, segs, quant, B, self.H, self.W, self.total_blocks,
                                                   self.plane_bytes, self.max_blocks, out=out, check=check)
        return out


# ---- multi-scan files: progressive Huffman (T.81 Annex G), multi-scan sequential, and baseline files as one scan ---------------------
S_IMG, S_MODE, S_NCOMP, S_COMP0, S_SS, S_SE, S_AH, S_AL, S_RESTART, S_SCAN_OFF, S_SCAN_LEN, S_SEG_OFF, S_NSEG = 0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14
S_GW, S_GH, S_NTAB, S_TAB0, S_DC0, S_AC0, S_FIRST, S_SCAN_BYTES = 15, 16, 17, 18, 22, 25, 28, 29
NS = 32
M_SEQ, M_DC_FIRST, M_DC_REFINE, M_AC_FIRST, M_AC_REFINE = range(5)


class Scan:
    """one scan: `comps` indices into ParsedScans.comps (scan order); `dc` / `ac` per scan component an index into ParsedScans.tabs
    (None where the scan reads no such table); `data` the cleaned entropy-coded bytes, `segs` the restart offsets into it; the scan walks
    `gw x gh` units (MCUs when interleaved, else the component's own ceil(cw/8) x ceil(ch/8) blocks), `restart` of them per interval;
    `level` (from 1): 1 + the highest level of an earlier scan sharing a component and overlapping it spectrally"""
    __slots__ = ("comps", "ss", "se", "ah", "al", "mode", "dc", "ac", "restart", "data", "segs", "gw", "gh", "level")


class ParsedScans:
    __slots__ = ("W", "H", "ncomp", "comps", "hmax", "vmax", "mcus_x", "mcus_y", "quant", "tabs", "scans", "progressive", "nlevels")


def parse_scans(data):
    """bytes of one JPEG file -> ParsedScans: frame geometry (the `comps` fields of parse(), MCU-padded block grid), quant tables,
    a deduplicated Huffman table pool and the list of scans.  Takes progressive Huffman (SOF2) and sequential (SOF0 / SOF1) files with
    one or several scans.  Raises Unsupported for what parse() refuses besides progression, for every progression on which libjpeg
    warns (jdphuff.c start_pass_phuff_decoder: JWRN_BOGUS_PROGRESSION), and for files whose coefficients 0..9 are not all complete
    (Al = 0) after the last scan -- libjpeg-turbo block-smooths those (jdcoefct.c smoothing_ok), which the GPU path does not restate."""
    if data[:2] != b"\xff\xd8":
        raise Unsupported("not a JPEG")
    qt, ht = {}, {}
    tabs, tab_idx = [], {}
    restart, frame, adobe_transform, progressive = 0, None, None, False
    p, coef_bits, scans = None, None, []
    pos, n = 2, len(data)
    while True:
        if pos + 2 > n or data[pos] != 0xFF:
            raise Unsupported("truncated file or marker expected")
        while pos + 2 < n and data[pos + 1] == 0xFF:
            pos += 1
        m = data[pos + 1]
        pos += 2
        if m == 0xD9:
            break
        if m in (0x01,) or 0xD0 <= m <= 0xD7:
            continue
        ln, seg = _marker_segment(data, pos)
        if m == 0xDB:
            if scans:
                raise Unsupported("quantisation table redefined between scans")
            qt.update(_dqt_tables(seg))
        elif m == 0xC4:
            for tc, th, bits, vals in _dht_tables(seg):
                t = huff_table(bits, vals)
                ht[(tc, th)] = tab_idx.setdefault(t.tobytes(), len(tabs))
                if ht[(tc, th)] == len(tabs):
                    tabs.append(t)
        elif m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise Unsupported("two frames")
            frame = _sof_frame(seg)
            progressive = m == 0xC2
        elif m in (0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported("lossless / hierarchical / arithmetic JPEG")
        elif m == 0xDD:
            restart = _restart_interval(seg)
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe_transform = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Unsupported("SOS before SOF")
            if p is None:
                p = _scan_frame(frame, adobe_transform, qt)
                p.progressive = progressive
                coef_bits = np.full((p.ncomp, 64), -1, dtype=np.int32)
            ids = [c[0] for c in frame[2]]
            sel, s_ss, s_se, s_ahal = _sos_header(seg)
            ns = len(sel)
            if not 1 <= ns <= 3 or any(cid not in ids for cid, _, _ in sel) or len({cid for cid, _, _ in sel}) != ns:
                raise Unsupported("bad scan component list")
            s = Scan()
            s.comps = [ids.index(cid) for cid, _, _ in sel]
            s.ss, s.se, s.ah, s.al = s_ss, s_se, s_ahal >> 4, s_ahal & 15
            s.mode = _check_progression(s, progressive, coef_bits)
            need_dc, need_ac = s.mode in (M_SEQ, M_DC_FIRST), s.mode in (M_SEQ, M_AC_FIRST, M_AC_REFINE)
            if (need_dc and any((0, td) not in ht for _, td, _ in sel)) or (need_ac and any((1, ta) not in ht for _, _, ta in sel)):
                raise Unsupported("missing Huffman table")
            s.dc = [ht[(0, td)] if need_dc else None for _, td, _ in sel]
            s.ac = [ht[(1, ta)] if need_ac else None for _, _, ta in sel]
            for t in s.dc:
                if t is not None:
                    _check_dc_table(tabs[t])
            if len({t for t in s.dc + s.ac if t is not None}) > 4:
                raise Unsupported("more than four Huffman tables in one scan")
            if ns == 1:
                d = p.comps[s.comps[0]]
                s.gw, s.gh = -(-d["cw"] // 8), -(-d["ch"] // 8)
            else:
                s.gw, s.gh = p.mcus_x, p.mcus_y
            s.restart = restart
            s.data, s.segs, pos = _clean_segment(data, pos + ln, restart)
            if restart and len(s.segs) < -(-s.gw * s.gh // restart):
                raise Unsupported("restart markers missing")
            s.level = 1 + max([t.level for t in scans if set(t.comps) & set(s.comps) and t.ss <= s.se and s.ss <= t.se], default=0)
            scans.append(s)
            continue
        pos += ln
    if p is None:
        raise Unsupported("no scan")
    if progressive and (coef_bits[:, :10] != 0).any():
        raise Unsupported("incomplete progression: libjpeg would block-smooth this file")
    if not progressive and (coef_bits[:, 0] != 0).any():
        raise Unsupported("component without a scan")
    p.tabs, p.scans, p.nlevels = tabs, scans, max(s.level for s in scans)
    return p


def _scan_frame(frame, adobe_transform, qt):
    H, W, nc, hmax, vmax, comps = _frame_geometry(frame, adobe_transform)
    p = ParsedScans()
    p.W, p.H, p.ncomp, p.hmax, p.vmax = W, H, nc, hmax, vmax
    p.mcus_x, p.mcus_y = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    p.comps = []
    for (cid, h, v, tq) in comps:
        if tq not in qt:
            raise Unsupported("missing quantisation table")
        p.comps.append(dict(h=h, v=v, tq=tq, bw=p.mcus_x * h, bh=p.mcus_y * v, cw=-(-W * h // hmax), ch=-(-H * v // vmax)))
    p.quant = np.zeros((4, 64), dtype=np.uint16)
    for k, t in qt.items():
        if k < 4:
            p.quant[k] = t
    return p


def _check_progression(s, progressive, coef_bits):
    """-> the scan's decode mode; tracks coef_bits (component x coefficient: Al of the last scan, -1 = not yet coded) as
    jdphuff.c start_pass_phuff_decoder does and raises Unsupported wherever libjpeg errors out or warns"""
    if not progressive:
        if (s.ss, s.se, s.ah, s.al) != (0, 63, 0, 0):
            raise Unsupported("sequential scan with a spectral band / successive approximation")
        if (coef_bits[s.comps, 0] >= 0).any():
            raise Unsupported("component coded in two sequential scans")
        coef_bits[s.comps] = 0
        return M_SEQ
    bad = s.se != 0 if s.ss == 0 else (s.ss > s.se or s.se > 63 or len(s.comps) != 1)
    if bad or (s.ah != 0 and s.al != s.ah - 1) or s.al > 13:
        raise Unsupported("bogus progression")
    for c in s.comps:
        cb = coef_bits[c]
        if s.ss != 0 and cb[0] < 0:
            raise Unsupported("AC scan before the DC scan")
        band = cb[s.ss:s.se + 1]
        if (np.maximum(band, 0) != s.ah).any() or (s.ah == 0 and (band >= 0).any()):
            raise Unsupported("bogus progression")     # (a first scan over coefficients already coded: libjpeg silently overwrites)
        band[:] = s.al
    if s.ss == 0:
        return M_DC_FIRST if s.ah == 0 else M_DC_REFINE
    return M_AC_FIRST if s.ah == 0 else M_AC_REFINE


class ScanJpegBatch:
    """host-side descriptor of a batch of equal-geometry JPEGs decoded SCAN BY SCAN (progressive, multi-scan sequential, and baseline
    files as one sequential scan each: mixed batches decode together).  ONE contiguous blob, read by the kernels in place when pinned:
        params (B x 64 i32, JpegBatch layout) | scan descriptors (nscans x 32 i32, sorted by dependency level) | restart offsets (i32) |
        quant tables (B x 256 u16) | Huffman table pool (npool x 1424 B, deduplicated over the batch) | cleaned scans
    decode() runs one kernel launch per dependency level (self.level_start), then the IDCT and colour kernels of the baseline path."""

    def __init__(self, datas, pool=None, alloc=None, canvas=None):
        """canvas = (H, W): files of different sizes, each decoded at the top left of an H x W canvas (_geometry)"""
        import torch
        ps = list(pool.map(parse_scans, datas)) if pool is not None else [parse_scans(d) for d in datas]
        self.last_err = None
        B = len(ps)
        (self.H, self.W), self.hw = _geometry(ps, canvas)
        self.B = B
        pool_idx, pool_tabs, remap = {}, [], []
        for p in ps:
            r = []
            for t in p.tabs:
                k = t.tobytes()
                if k not in pool_idx:
                    pool_idx[k] = len(pool_tabs)
                    pool_tabs.append(t)
                r.append(pool_idx[k])
            remap.append(r)
        items = sorted((s.level, b, i) for b, p in enumerate(ps) for i, s in enumerate(p.scans))
        self.nlevels = items[-1][0]
        self.level_start = np.searchsorted([it[0] for it in items], np.arange(1, self.nlevels + 2)).astype(np.int32)
        nsc = len(items)
        nseg = sum(len(s.segs) for p in ps for s in p.scans)
        padded = lambda n: n + ((-n) % CHUNK or (CHUNK if n == 0 else 0))
        al = lambda n: (n + 255) & ~255
        self.off_params, n = 0, al(B * NP * 4)
        self.off_descs, n = n, n + al(nsc * NS * 4)
        self.off_segs, n = n, n + al(nseg * 4)
        self.off_quant, n = n, n + al(B * 256 * 2)
        self.off_tabs, n = n, n + al(len(pool_tabs) * TAB_BYTES)
        self.off_scan, n = n, n + sum(padded(len(s.data)) for p in ps for s in p.scans)
        self.nseg, self.nscans, self.npool, self.nbytes = nseg, nsc, len(pool_tabs), n
        blob = alloc(n + al(4 * B)) if alloc is not None else torch.empty(n + al(4 * B), dtype=torch.uint8)
        self.blob = blob[:n]
        self.err_host = blob[n:n + 4 * B].view(torch.int32)     # the error codes come back into the same (pinned) staging buffer
        host = self.blob.numpy()
        host[:self.off_scan] = 0
        params = host[self.off_params:self.off_params + B * NP * 4].view(np.int32).reshape(B, NP)
        descs = host[self.off_descs:self.off_descs + nsc * NS * 4].view(np.int32).reshape(nsc, NS)
        segs = host[self.off_segs:self.off_segs + nseg * 4].view(np.int32)
        quant = host[self.off_quant:self.off_quant + B * 512].view(np.uint16).reshape(B, 256)
        tabs = host[self.off_tabs:self.off_tabs + len(pool_tabs) * TAB_BYTES].reshape(-1, TAB_BYTES)
        scan = host[self.off_scan:]
        for i, t in enumerate(pool_tabs):
            tabs[i] = t
        blk_off = plane_off = 0
        self.max_blocks = 0
        for b, p in enumerate(ps):
            r = params[b]
            r[P_QUANT_OFF], r[P_NCOMP], r[P_W], r[P_H], r[P_HMAX], r[P_VMAX] = b * 256, p.ncomp, p.W, p.H, p.hmax, p.vmax
            r[P_MCUS_X], r[P_MCUS_Y] = p.mcus_x, p.mcus_y
            nblk = 0
            for c, d in enumerate(p.comps):
                o = P_COMP0 + c * P_CSTRIDE
                r[o:o + 11] = [d["h"], d["v"], d["tq"], 0, 0, d["bw"], d["bh"], d["cw"], d["ch"], blk_off + nblk, plane_off]
                nblk += d["bw"] * d["bh"]
                plane_off += (d["bw"] * 8 * d["bh"] * 8 + 15) & ~15
            self.max_blocks = max(self.max_blocks, nblk)
            blk_off += nblk
            quant[b] = p.quant.reshape(-1)
        scan_off = seg_off = 0
        for j, (_, b, i) in enumerate(items):
            s = ps[b].scans[i]
            local = sorted({t for t in s.dc + s.ac if t is not None})
            d = descs[j]
            d[S_IMG], d[S_MODE], d[S_NCOMP] = b, s.mode, len(s.comps)
            d[S_COMP0:S_COMP0 + len(s.comps)] = s.comps
            d[S_SS], d[S_SE], d[S_AH], d[S_AL], d[S_RESTART] = s.ss, s.se, s.ah, s.al, s.restart
            d[S_SCAN_OFF], d[S_SCAN_LEN], d[S_SEG_OFF], d[S_NSEG] = scan_off, padded(len(s.data)), seg_off, len(s.segs)
            d[S_GW], d[S_GH], d[S_NTAB], d[S_FIRST], d[S_SCAN_BYTES] = s.gw, s.gh, len(local), int(i == 0), len(s.data)
            d[S_TAB0:S_TAB0 + len(local)] = [remap[b][t] for t in local]
            d[S_DC0:S_DC0 + len(s.comps)] = [local.index(t) if t is not None else 0 for t in s.dc]
            d[S_AC0:S_AC0 + len(s.comps)] = [local.index(t) if t is not None else 0 for t in s.ac]
            scan[scan_off:scan_off + len(s.data)] = s.data
            scan[scan_off + len(s.data):scan_off + padded(len(s.data))] = 0
            segs[seg_off:seg_off + len(s.segs)] = s.segs
            scan_off += padded(len(s.data))
            seg_off += len(s.segs)
        self.params, self.descs, self.tabs, self.scan = params, descs, tabs.reshape(-1), scan     # host views (tests)
        self.total_blocks, self.plane_bytes = blk_off, plane_off

    def decode(self, device, out=None, check=True):
        """-> (B, H, W, 3) u8 device tensor on the current stream; the contract of JpegBatch.decode (last_err, err_host)"""
        import torch
        dev = torch.device(device)
        with torch.cuda.device(dev):
            return self._decode(self.blob if self.blob.is_pinned() else self.blob.to(dev, non_blocking=True), out, check)

    def _decode(self, d, out, check):
        from . import ops
        B = self.B
        view = lambda off, nbytes: d[off:off + nbytes]
        out, self.last_err = ops.jpeg_decode_scans_batch(
            view(self.off_params, B * NP * 4), view(self.off_descs, self.nscans * NS * 4), d[self.off_scan:],
            view(self.off_tabs, self.npool * TAB_BYTES), view(self.off_segs, max(4, self.nseg * 4)), view(self.off_quant, B * 512),
            self.level_start, B, self.H, self.W, self.total_blocks, self.plane_bytes, self.max_blocks, out=out, check=check)
        return out
