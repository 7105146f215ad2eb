"""CPU restatements of the glue, layout and entropy-index kernels (csrc/misc.hip, csrc/decode.hip, csrc/entropy.hip), built from
library operations (F.unfold, F.pixel_shuffle, reshape / permute, torch.sort, torch.argmax, torch.clamp, torch.where) and fp64
arithmetic, not from the kernels' index arithmetic (dwconv_ordered32 restates an operation ORDER, in slices of whole tensors).
tests/test_kernels_ref_cpu.py checks them against each other and against the C
oracle; tests/test_gpu_kernels.py and tests/test_gpu_kernels_entropy.py compare the kernels with them.  The fp64 attention with
Swin-shaped bias variants, the window partition and the fp64 3x3 convolution serve tests/test_gpu_attention_rowmap.py,
tests/test_swin_rowmap_cpu.py and tests/test_gpu_conv_chain.py.

Tolerance rules used by those tests:
  * half-integer band (l2norm_u8): the u8 code must equal the fp64 code wherever (u * 0.5 + 0.5) * 255 is farther than Q_BAND from a
    half-integer; inside the band either neighbouring code passes, and the band may hold at most Q_BAND_SHARE of a case's elements.
  * VQ near-tie rule (vq_argmin): an index passes if its fp64 distance is within VQ_TOL of the fp64 minimum, and at most
    VQ_DIFF_SHARE of the tokens may differ from the fp64 argmin at all.
  * margin ulp rule (index_margins): both sides compute in fp64 and round once, so the margin agrees within one fp32 ulp of the
    reference value plus 1e-9; `alt` is exact except where two candidates tie within that tolerance."""
import numpy as np
import torch
import torch.nn.functional as F

Q_BAND = 2e-4
Q_BAND_SHARE = 2e-3
VQ_TOL = 2.0 ** -17
VQ_DIFF_SHARE = 5e-3
UNIT_TOL = 2.0 ** -21

LOG_MIN = np.log(0.11)
LOG_STEP = (np.log(64.0) - np.log(0.11)) / 255.0


# ---- layouts --------------------------------------------------------------------------------------------------------------------
def tm16(x_nhwc):
    """(B,H,W,C) -> rows in 16x16-tile-major order"""
    B, H, W, C = x_nhwc.shape
    return x_nhwc.reshape(B, H // 16, 16, W // 16, 16, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, C)


def from_tm16(rows, B, H, W):
    C = rows.shape[1]
    return rows.reshape(B, H // 16, W // 16, 16, 16, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


def bits(t):
    """fp32 tensor -> its int32 bit patterns (so that -0.0 and NaN payloads compare)"""
    return t.contiguous().view(torch.int32)


def special_values(t):
    """plant -0.0 and a NaN with a payload into the first elements of a copy-only test input"""
    flat = t.reshape(-1)
    flat[0] = -0.0
    if flat.numel() > 1:
        flat[1:2] = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)
    return t


def im2col_patch(x, P, mul, add, tile16):
    """x (B,C,H,W) fp32 -> (patches, C*P*P): fp32 x*mul then +add (two IEEE ops), F.unfold, patch rows plain or tile-major"""
    B, C, H, W = x.shape
    y = x * torch.tensor(mul, dtype=torch.float32) + torch.tensor(add, dtype=torch.float32)
    cols = F.unfold(y, kernel_size=P, stride=P).transpose(1, 2)            # (B, gh*gw, C*P*P)
    grid = cols.reshape(B, H // P, W // P, C * P * P)
    return (tm16(grid) if tile16 else grid.reshape(-1, C * P * P)).contiguous()


def im2col_2x2(rows, B, H, W, tile16):
    C = rows.shape[1]
    x = from_tm16(rows, B, H, W) if tile16 else rows.reshape(B, H, W, C)
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) * (W // 2), 4 * C).contiguous()


def pixel_shuffle2_tm16(rows, B, H, W, C):
    """rows (B*H*W, 4C) plain -> PixelShuffle(2) -> tile-major rows (B*2H*2W, C)"""
    nchw = rows.reshape(B, H, W, 4 * C).permute(0, 3, 1, 2)
    return tm16(F.pixel_shuffle(nchw, 2).permute(0, 2, 3, 1)).contiguous()


def fake2d_transpose(buf, seq_stride, N, T, D):
    flat = buf.reshape(-1)
    return torch.cat([flat[n * seq_stride:n * seq_stride + T * D].reshape(D, T).t() for n in range(N)]).contiguous()


def assemble_tokens(emb, cls, pos, lat, latpos, N, P, T, D):
    parts = [(cls + pos[0]).expand(N, 1, D), emb.reshape(N, P, D) + pos[1:1 + P]]
    if T:
        parts.append((lat + latpos).expand(N, T, D))
    return torch.cat(parts, dim=1).reshape(N * (1 + P + T), D)


def assemble_dec_tokens(emb, cls, mask, pos, latpos, N, P, T, D):
    parts = [(cls + pos[0]).expand(N, 1, D), (mask + pos[1:1 + P]).expand(N, P, D), emb.reshape(N, T, D) + latpos]
    return torch.cat(parts, dim=1).reshape(N * (1 + P + T), D)


def add_rows_bcast(inp, iseg, vec, Nn, Lr):
    """-> (Nn, Lr, D): block n is rows n*iseg .. n*iseg+Lr-1 of inp, plus vec (Lr, D) when given"""
    blocks = torch.stack([inp[n * iseg:n * iseg + Lr] for n in range(Nn)])
    return blocks + vec if vec is not None else blocks


def copy_row_blocks(x, rows, stride_rows, nblocks):
    return torch.cat([x[i * stride_rows:i * stride_rows + rows] for i in range(nblocks)])


def nhwc3_to_nchw_clamp(rows, B, H, W):
    return torch.clamp(rows[:, :3].reshape(B, H, W, 3).permute(0, 3, 1, 2), -1.0, 1.0).contiguous()


def halo_interior(rows, B, H, W, upsample, tile16):
    """the interior (B, OH, OW, C) that halo_copy writes"""
    C = rows.shape[1]
    x = from_tm16(rows, B, H, W) if tile16 else rows.reshape(B, H, W, C)
    if upsample:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return x


def embed_tokens(ids, table, pos, vocab):
    B, L = ids.shape
    return (table[torch.clamp(ids.long(), 0, vocab - 1)] + pos[:L]).reshape(B * L, -1)


def gather_eot_rows(ids, x, D):
    B, L = ids.shape
    first_max = torch.argmax(ids, dim=1)                                    # torch.argmax returns the first maximum
    return x.reshape(B, L, -1)[torch.arange(B), first_max, :D]


def topk_rows(s, k):
    r = torch.sort(s, dim=1, descending=True, stable=True)
    return r.values[:, :k], r.indices[:, :k]


# ---- single IEEE fp32 ops -------------------------------------------------------------------------------------------------------
def colop(x, v, mode):
    vv = v[torch.arange(x.shape[0]) % v.shape[0]]
    if mode == 0:
        return x * vv
    vc = torch.clamp(vv, min=0.5)
    return x / vc if mode == 1 else x * vc


def gated_lrelu(x):
    a, b = np.split(x.numpy(), 2, axis=1)
    o = np.where(a >= 0, a, np.float32(0.1) * a) + np.where(b >= 0, b, np.float32(0.01) * b)
    return torch.from_numpy(o.astype(np.float32))


def dwconv_ordered32(x, w, bias, prescale, k):
    """depthwise k x k convolution, stride 1, zero padding k // 2, in the kernels' own fp32 operation order, so that dwconv_kernel and
    dwconv_x4_kernel (csrc/misc.hip, built without contraction) must equal it bit for bit: x (B, H, W, C), w (k*k, C), bias (C) or
    None, prescale (C) or None.  The accumulator starts at the bias or at +0; taps go in (ky, kx) order; v = x * prescale when a
    prescale is given; acc = acc + v * w as two rounded operations; taps outside the image are skipped."""
    B, H, W, C = x.shape
    pad = k // 2
    acc = bias.expand(B, H, W, C).clone() if bias is not None else torch.zeros(B, H, W, C)
    v = x * prescale if prescale is not None else x
    for ky in range(k):
        for kx in range(k):
            dy, dx = ky - pad, kx - pad
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                acc[:, y0:y1, x0:x1] = acc[:, y0:y1, x0:x1] + v[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx] * w[ky * k + kx]
    assert acc.dtype == torch.float32
    return acc


# ---- the 4-step mask and the index builder --------------------------------------------------------------------------------------
def active_gather(a, k):
    """a (B, C, H, W) -> (B, C/4, H, W): at position (i, j) the channels of the quarter that step k codes, q = p ^ {0,3,2,1}[k] with
    the spatial phase p = 2 (i & 1) + (j & 1) (entropy/compression_model.py:277-280)"""
    B, C, H, W = a.shape
    quarters = a.reshape(B, 4, C // 4, H, W)
    q = _quarter(H, W, k)
    out = quarters[:, 0]
    for quarter in range(1, 4):
        out = torch.where(q == quarter, quarters[:, quarter], out)
    return out


def _quarter(H, W, k):
    ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return (2 * (ii & 1) + (jj & 1)) ^ (0, 3, 2, 1)[k]


def active_mask(C, H, W, k):
    """(H, W, C) bool: the (position, channel) entries step k reads and writes"""
    return (torch.arange(C) // (C // 4)).view(1, 1, C) == _quarter(H, W, k).unsqueeze(-1)


def scale_index(s, thr):
    """GaussianEncoder.build_indexes: trunc(clamp((fp32(log_fp64(max(s, 1e-5))) - fp32(ln 0.11)) / fp32(step), 0, 255)) in fp32 ops,
    -1 where s < thr"""
    s = np.asarray(s, dtype=np.float32)
    lg = np.log(np.maximum(s, np.float32(1e-5)).astype(np.float64)).astype(np.float32)
    fi = (lg - np.float32(LOG_MIN)) / np.float32(LOG_STEP)
    assert fi.dtype == np.float32
    idx = np.trunc(np.clip(fi, np.float32(0), np.float32(255))).astype(np.int16)
    if thr is not None:
        idx = np.where(s < np.float32(thr), np.int16(-1), idx)
    return idx


def entropy_scales(n, thr, seed):
    """n fp32 scales: the edge values first (0, 1e-6, 1e-5, around thr, 0.11, 64, 1e4, both fp32 neighbours of 40 bin edges spread
    over i = 1..255 and the rounded edges themselves), then log-uniform random ones"""
    t = np.float32(0.12 if thr is None else thr)
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    edges = np.exp(LOG_MIN + np.unique(np.linspace(1, 255, 40).round()) * LOG_STEP).astype(np.float32)
    special = np.concatenate([np.array([0, 1e-6, 1e-5, np.nextafter(t, dn), t, np.nextafter(t, up), 0.11, 64, 1e4], dtype=np.float32),
                              np.nextafter(edges, dn), edges, np.nextafter(edges, up)])
    assert n >= special.size, (n, special.size)
    rng = np.random.default_rng(seed)
    rest = np.exp(rng.uniform(np.log(0.05), np.log(70.0), n - special.size)).astype(np.float32)
    return np.concatenate([special, rest])


def index_margins(s, thr):
    """fp64 restatement of the doc comment of sgic_index_margins for scales s (any shape): -> (margin fp64, list of accepted alts per
    element as an (n_candidates, ...) int array with -2 where a candidate does not apply, the tolerance array).  Candidates: the
    skip threshold (when set), and for positions that are not skipped the interior bin edges 1..255 next to ln sigma; the index on
    the other side of edge e is e - 1 for a sigma coded >= e, else e."""
    s = np.asarray(s, dtype=np.float32)
    coded = scale_index(s, None).astype(np.int64)
    ls = np.log(np.maximum(s, np.float32(1e-5)).astype(np.float64))
    ti = (ls - LOG_MIN) / LOG_STEP
    cand_d, cand_alt = [], []
    skipped = np.zeros(s.shape, bool)
    if thr is not None:
        skipped = s < np.float32(thr)
        cand_d.append(np.abs(ls - np.log(np.float64(np.float32(thr)))) / LOG_STEP)
        cand_alt.append(np.where(skipped, coded, -1))
    for e in (np.clip(np.floor(ti), 1, 255), np.clip(np.floor(ti) + 1, 1, 255)):
        cand_d.append(np.where(skipped, np.inf, np.abs(ti - e)))
        cand_alt.append(np.where(coded >= e, e - 1, e).astype(np.int64))
    d, alt = np.stack(cand_d), np.stack(cand_alt)
    margin = d.min(axis=0)
    tol = np.spacing(margin.astype(np.float32)).astype(np.float64) + 1e-9
    accepted = np.where(d <= margin + tol, alt, -2)
    return margin, accepted, tol


# ---- tolerance kernels ----------------------------------------------------------------------------------------------------------
# (M, ncodes, dim, l2norm, ldz): M over {1, 3, 4, 5, 4097} (last workgroup padded with 3, 2, 0, 3, 3 clamped tokens), ncodes over
# {1, 7, 255, 256, 257, 4096} (below / at / above one pass of the 256 threads, 16 passes), dim over {1, 5, 12, 16}; seed = position
VQ_CASES = [(1, 1, 5, 1, 5), (3, 7, 5, 1, 8), (4, 255, 12, 1, 12), (5, 256, 16, 0, 16), (4097, 257, 12, 1, 16), (5, 4096, 12, 1, 12),
            (4, 256, 1, 0, 3), (3, 257, 16, 1, 20)]


def vq_inputs(M, ncodes, dim, seed):
    """tokens and codes of norm in [0.3, 1] (so every distance is <= 4 with or without l2norm); token M // 2 is a copy of code
    ncodes // 2"""
    rng = np.random.default_rng(seed)

    def rows(n):
        v = rng.standard_normal((n, dim))
        v *= rng.uniform(0.3, 1.0, (n, 1)) / np.linalg.norm(v, axis=1, keepdims=True)
        return v.astype(np.float32)
    z, cb = rows(M), rows(ncodes)
    z[M // 2] = cb[ncodes // 2]
    return z, cb


def vq_dist64(z, cb, l2norm):
    """(M, ncodes) fp64 |z|^2 + |e|^2 - 2 z.e of the (normalised) rows (titok/quantizer.py:46-61)"""
    z, cb = np.asarray(z, np.float64), np.asarray(cb, np.float64)
    if l2norm:
        z = z / np.maximum(np.linalg.norm(z, axis=1, keepdims=True), 1e-12)
        cb = cb / np.maximum(np.linalg.norm(cb, axis=1, keepdims=True), 1e-12)
    return (z * z).sum(1)[:, None] + (cb * cb).sum(1)[None, :] - 2.0 * (z @ cb.T)


def vq_dist32(z, cb, l2norm):
    """the same three-term distance carried in fp32 (sums over the code dimension in ascending order)"""
    z, cb = np.asarray(z, np.float32), np.asarray(cb, np.float32)

    def sq(a):
        s = np.zeros(a.shape[0], np.float32)
        for d in range(a.shape[1]):
            s = s + a[:, d] * a[:, d]
        return s
    if l2norm:
        z = z * (np.float32(1) / np.maximum(np.sqrt(sq(z)), np.float32(1e-12)))[:, None]
        cb = cb * (np.float32(1) / np.maximum(np.sqrt(sq(cb)), np.float32(1e-12)))[:, None]
    dot = np.zeros((z.shape[0], cb.shape[0]), np.float32)
    for d in range(z.shape[1]):
        dot = dot + z[:, d, None] * cb[None, :, d]
    dist = sq(z)[:, None] + sq(cb)[None, :] - np.float32(2) * dot
    assert dist.dtype == np.float32
    return dist


def vq_check(idx, d64):
    """the VQ near-tie rule -> (share of tokens that differ from the fp64 argmin, worst excess distance)"""
    idx = np.asarray(idx).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < d64.shape[1], (idx.min(), idx.max())
    best = d64.argmin(axis=1)
    excess = d64[np.arange(len(idx)), idx] - d64.min(axis=1)
    return float((idx != best).mean()), float(excess.max())


def codebook_gather_norm(idx, cb):
    e = np.asarray(cb, np.float64)[np.asarray(idx)]
    return e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)


L2_CASES = [(1, 64, 64), (5, 50, 50), (37, 512, 520), (9, 1000, 1000)]    # (M, D, ldx)


def l2norm_inputs(M, D, seed):
    """rows with scales from 1e-2 to 1e2"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((M, D)) * np.logspace(-2, 2, M)[:, None]).astype(np.float32)


def l2norm_u8_64(x):
    """-> (unit fp64, code fp64-rounded u8, in-band mask): band = (u * 0.5 + 0.5) * 255 within Q_BAND of a half-integer"""
    x = np.asarray(x, np.float64)
    u = x / np.linalg.norm(x, axis=1, keepdims=True)
    t = (u * 0.5 + 0.5) * 255.0
    band = np.abs(t - (np.floor(t) + 0.5)) <= Q_BAND
    return u, np.clip(np.rint(t), 0, 255).astype(np.uint8), band


def u8_from_unit32(unit):
    """the quantiser in numpy fp32 from a given fp32 unit row: clip(rint((unit * 0.5 + 0.5) * 255), 0, 255), single IEEE ops"""
    u = np.asarray(unit, np.float32)
    t = (u * np.float32(0.5) + np.float32(0.5)) * np.float32(255)
    assert t.dtype == np.float32
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def l2norm_u8_32(x):
    x = np.asarray(x, np.float32)
    u = x / np.sqrt((x * x).sum(axis=1, dtype=np.float32))[:, None]
    assert u.dtype == np.float32
    return u, u8_from_unit32(u)


def u8_check(q, q64, band):
    """the half-integer band rule: exact outside the band, either neighbour inside"""
    q, q64 = np.asarray(q).astype(np.int64), q64.astype(np.int64)
    assert np.array_equal(q[~band], q64[~band]), "u8 code differs from the fp64 code outside the half-integer band"
    assert np.abs(q[band] - q64[band]).max(initial=0) <= 1


def half_even_rows(n=16, D=64):
    """rows that pin round-half-to-even: row r has norm exactly 1 in fp32 and holds at index 3 a value u whose fp32 quantiser input
    (u * 0.5 + 0.5) * 255 is EXACTLY k + 0.5 with k even (rint -> k, floor(x + 0.5) -> k + 1), at index 40 the filler that makes
    the fp32 sum of squares round to a value whose root is 1.0f, zeros elsewhere (two non-zero squares: one fp32 add, whatever the
    summation order).  Found by scanning fp32 neighbours; -> (x (n, D) fp32, k (n,))"""
    rows, ks = [], []
    for k in range(10, 250, 2):
        u0 = np.float32(2.0 * (k + 0.5) / 255.0 - 1.0)
        cand = u0
        for _ in range(200):
            cand = np.nextafter(cand, np.float32(-np.inf))
        hit = None
        for _ in range(400):
            t = (cand * np.float32(0.5) + np.float32(0.5)) * np.float32(255)
            if t == np.float32(k + 0.5):
                hit = cand
                break
            cand = np.nextafter(cand, np.float32(np.inf))
        if hit is None:
            continue
        f = np.float32(np.sqrt(1.0 - float(hit) ** 2))
        for _ in range(8):
            f = np.nextafter(f, np.float32(-np.inf))
        fill = None
        for _ in range(16):
            if np.sqrt(hit * hit + f * f) == np.float32(1.0):
                fill = f
                break
            f = np.nextafter(f, np.float32(np.inf))
        if fill is None:
            continue
        row = np.zeros(D, np.float32)
        row[3], row[40] = hit, fill
        rows.append(row)
        ks.append(k)
        if len(rows) == n:
            break
    return np.stack(rows), np.array(ks)


# ---- attention and the Swin window layout ---------------------------------------------------------------------------------------
def window_grid(L):
    """(rows, cols) of the token grid of an L-token window: square when L is a square (256 -> 16 x 16), else 8 rows"""
    r = int(round(L ** 0.5))
    return (r, r) if r * r == L else (8, L // 8)


def attn_bias_variants(L, g):
    """(4, L, L) additive bias [plain | +upper-lower | +left-right | both] shaped like Swin's shift masks on the window's token grid
    (token t = (i, j)): with the grid cut at its lower half of rows (right half of columns), a query and a key on different sides
    of the cut are masked with -inf.  Every query keeps the keys of its own side, itself among them: no row is fully masked."""
    gh, gw = window_grid(L)
    assert gh * gw == L and gh >= 2 and gw >= 2
    i, j = torch.arange(L) // gw, torch.arange(L) % gw
    low, right = i >= gh - gh // 2, j >= gw - gw // 2
    ul = torch.zeros(L, L).masked_fill(low[:, None] != low[None, :], float("-inf"))
    lr = torch.zeros(L, L).masked_fill(right[:, None] != right[None, :], float("-inf"))
    pos = torch.randn(L, L, generator=g)
    b = torch.stack([pos, pos + ul, pos + lr, (pos + ul) + lr])
    assert bool(torch.isfinite(b).any(dim=-1).all())
    return b


def attention64(qkv, L, nseq, heads, bias, var, scale):
    """qkv (nseq * L, 3 * heads * 64) dense -> fp64 softmax(scale q k^T + bias[var[s]]) v as (nseq * L, heads * 64)"""
    D = heads * 64
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(nseq, L, heads, 64).permute(0, 2, 1, 3).double() for i in range(3))
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias[var.long()].double()[:, None]
    return (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(nseq * L, D)


def window_partition(x, win):
    """(B, H, W, C) -> (B * H/win * W/win, win * win, C): windows in raster order, tokens of a window in raster order"""
    B, H, W, C = x.shape
    return x.reshape(B, H // win, win, W // win, win, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, win * win, C)


def conv3x3_64(x, w, bias, res, act):
    """x (B, Cin, H, W), w (Cout, Cin, 3, 3), res (B, Cout, H, W) or None -> (pre-activation, result) as fp64 rows (B*H*W, Cout);
    act 0 / 2 (SiLU), the residual added after the activation"""
    pre = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    out = F.silu(pre) if act == 2 else pre
    if res is not None:
        out = out + res.double()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])  # noqa: E731
    return rows(pre), rows(out)


def gemm_batched64(a, w, bias, res, act):
    """a (b, M, K), w (b or 1, N, K), bias (N) or None, res (b, M, N) or None -> (pre-activation fp64, result fp64); act 0 / 2 (SiLU)"""
    pre = torch.matmul(a.double(), w.double().transpose(1, 2))
    if bias is not None:
        pre = pre + bias.double()
    out = F.silu(pre) if act == 2 else pre
    if res is not None:
        out = out + res.double()
    return pre, out
