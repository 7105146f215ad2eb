"""CPU restatement of the bf16x3 split arithmetic (csrc/split3.h, csrc/gemm_split.hip, the S3 variant of csrc/attn.hip,
sgic_conv3x3_split3_f32) and the inputs of the accuracy tests, shared by tests/test_split3_accuracy_cpu.py (no GPU) and
tests/test_gpu_split3_accuracy.py.

The claim under test: a product of two fp32 operands, each cut into three bf16 pieces, computed as SIX piece products with fp32
accumulation, is an fp32 product in accuracy.  The statistic is

    ratio = rms(err of X against fp64) / rms(err of a strict k-ordered fp32 multiply-add chain against fp64)

on the same inputs.  mm_split takes its list of piece products as a parameter, so the CPU test can show what the statistic does
with a product that has lost one of its third-order terms (a wrong plane, a bad term pairing, a misplaced k slot): the six-term
product stays under BOUND, every five-term mutant lies at three times BOUND or more.

Everything here is numpy / torch on the CPU; no index arithmetic of any kernel is restated."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

BOUND = 1.10            # the GEMM test's own: rms error of the split result <= 1.10 x the fp32 path's (tests/test_gpu_split3.py)
MAX_FACTOR = 1.5        # ... and its worst error <= 1.5 x the fp32 path's worst

# (piece of a, piece of b) in the order the kernels issue their six MFMAs, smallest term first
SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
# the five-term mutants: each third-order term left out in turn
MUTANTS = {"no_p3q1": tuple(t for t in SIX if t != (2, 0)),
           "no_p1q3": tuple(t for t in SIX if t != (0, 2)),
           "no_p2q2": tuple(t for t in SIX if t != (1, 1))}
MFMA_K = 16             # k extent of one v_mfma_f32_32x32x16_bf16 (attention); the GEMM and the convolution use GEMM_K
GEMM_K = 32             # ... of one v_mfma_f32_16x16x32_bf16 (gemm_split.hip)


def _bf16_rne(x):
    """fp32 array -> the nearest bf16 (ties to even), returned as fp32; finite inputs only"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """-> (p1, p2, p3), bf16 values held in fp32: p1 = bf16(x), p2 = bf16(x - p1), p3 = bf16((x - p1) - p2), each difference an exact
    fp32 operation (s3_split_pair)"""
    x = np.asarray(x, dtype=np.float32)
    p1 = _bf16_rne(x)
    r = x - p1
    p2 = _bf16_rne(r)
    s = r - p2
    return p1, p2, _bf16_rne(s)


def mm_split(a, b, terms=SIX, kblock=MFMA_K, lead_alone=False):
    """a (..., M, K) @ b (..., K, N) as the split product: per block of `kblock` k and per term of `terms`, in order, the sum of the
    piece products of that block is added to an fp32 accumulator.  A product of two bf16 values is exact in fp32 and a block's sum
    is taken in fp64 (the matrix core adds the products of one instruction before it rounds into the accumulator); kblock = 1 rounds
    after every single product instead.  lead_alone: the leading term p1 q1 has an accumulator of its own and the other terms share
    a second one, added at the end -- the score product of csrc/attn.hip's S3 variant."""
    pa, pb = split3(a), split3(b)
    K = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (b.shape[-1],), np.float32)
    lead = np.zeros_like(acc)
    pa64, pb64 = [p.astype(np.float64) for p in pa], [p.astype(np.float64) for p in pb]
    for k0 in range(0, K, kblock):
        for i, j in terms:
            blk = np.matmul(pa64[i][..., k0:k0 + kblock], pb64[j][..., k0:k0 + kblock, :])
            if lead_alone and (i, j) == (0, 0):
                lead = (lead.astype(np.float64) + blk).astype(np.float32)
            else:
                acc = (acc.astype(np.float64) + blk).astype(np.float32)
    return lead + acc if lead_alone else acc


def mm_scores_s3(a, b, terms=SIX):
    """the score product of the S3 variant of csrc/attn.hip: 16-k blocks, the leading term in a chain of its own"""
    return mm_split(a, b, terms=terms, kblock=MFMA_K, lead_alone=True)


def mm_chain(a, b):
    """a (..., M, K) @ b (..., K, N) as a strict k-ordered fp32 chain acc = fma(a_k, b_k, acc): the product is exact in fp64 and the
    sum is rounded once to fp32 (through fp64, which differs from a true fma only on rare double-rounding ties)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(a.shape[:-1] + (b.shape[-1],), np.float32)
    for k in range(a.shape[-1]):
        acc = (acc.astype(np.float64) + a[..., :, k, None].astype(np.float64) * b[..., k, None, :].astype(np.float64)).astype(np.float32)
    return acc


def mm64(a, b):
    return np.matmul(np.asarray(a, np.float64), np.asarray(b, np.float64))


LOG2E = np.float32(1.4426950408889634)


def attention(q, k, v, mm_scores, mm_pv, scale=0.125, bias=None, softmax="exact"):
    """q, k, v (units, L, 64) fp32, bias (units, L, L) fp32 or None -> (units, L, 64) fp32: the two products through the given
    multiplications.  softmax = "exact": everything between them the same for every choice (fp32 scores + bias, row maximum, exp
    rounded once to fp32, row sum in fp64 rounded to fp32, one fp32 division), so that two results differ by their products alone.
    "f32" / "s3": the roundings the two variants of csrc/attn.hip add around an exact exp2 -- f32: exp2 of the rounded product
    (s - m) * log2(e) (__expf); s3: q carries scale * log2(e) (one rounding per element of q), the bias enters as
    fma(bias, log2(e), s), and exp2 takes s - m directly."""
    q, k, v = (np.asarray(t, np.float32) for t in (q, k, v))
    if softmax == "s3":
        s = mm_scores(q * np.float32(np.float32(scale) * LOG2E), np.swapaxes(k, -1, -2))
        if bias is not None:
            s = (np.asarray(bias, np.float64) * np.float64(LOG2E) + s).astype(np.float32)
    else:
        s = mm_scores(q * np.float32(scale), np.swapaxes(k, -1, -2))
        if bias is not None:
            s = s + np.asarray(bias, np.float32)
    assert s.dtype == np.float32
    m = s.max(axis=-1, keepdims=True)
    if softmax == "exact":
        p = np.exp(s.astype(np.float64) - m).astype(np.float32)
    else:
        d = s - m if softmax == "s3" else (s - m) * LOG2E
        assert d.dtype == np.float32
        p = np.exp2(d.astype(np.float64)).astype(np.float32)
    l = p.sum(axis=-1, keepdims=True, dtype=np.float64).astype(np.float32)
    return mm_pv(p, v) / l


def scores_mfma_f32(q, kt):
    """q (..., L, 64) @ kt (..., 64, L) as the f32 variant of csrc/attn.hip takes it: v_mfma_f32_32x32x2_f32 adds the two products of
    one instruction (d = 8 c + t and 8 c + 4 + t) before it rounds into the accumulator, and d = 0..31 / 32..63 go into two
    accumulators that are added at the end: 16 roundings of a half-length partial sum and one more, where a strict chain has 64"""
    q64, k64 = np.asarray(q, np.float64), np.swapaxes(np.asarray(kt, np.float64), -1, -2)
    acc = [np.zeros(q.shape[:-1] + (kt.shape[-1],), np.float32) for _ in range(2)]
    for half in range(2):
        for c in range(4):
            for t in range(4):
                d0, d1 = 32 * half + 8 * c + t, 32 * half + 8 * c + 4 + t
                pair = q64[..., :, None, d0] * k64[..., None, :, d0] + q64[..., :, None, d1] * k64[..., None, :, d1]
                acc[half] = (acc[half].astype(np.float64) + pair).astype(np.float32)
    return acc[0] + acc[1]


def pv_mfma_f32(p, v):
    """p (..., L, L) @ v (..., L, 64) the same way: per 32-key tile 16 instructions of two keys each (e & 3) + 8 (e >> 2) and + 4"""
    L = p.shape[-1]
    p64, v64 = np.asarray(p, np.float64), np.asarray(v, np.float64)
    acc = np.zeros(p.shape[:-1] + (v.shape[-1],), np.float32)
    for t0 in range(0, L, 32):
        for e in range(16):
            keys = [x for x in (t0 + (e & 3) + 8 * (e >> 2) + 4 * h for h in range(2)) if x < L]
            if keys:
                blk = sum(p64[..., :, x, None] * v64[..., None, x, :] for x in keys)
                acc = (acc.astype(np.float64) + blk).astype(np.float32)
    return acc


def conv3x3(x, w, bias, mm):
    """x (B, Cin, H, W), w (Cout, Cin, 3, 3), bias (Cout) -> pre-activation rows (B*H*W, Cout) fp32: im2col (F.unfold, zero padding)
    with the k axis in the kernels' (ky, kx, cin) order, the product through `mm`, one fp32 add of the bias"""
    B, Cin, H, W = x.shape
    cols = F.unfold(x, kernel_size=3, padding=1).reshape(B, Cin, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * Cin)
    wk = w.permute(0, 2, 3, 1).reshape(w.shape[0], 9 * Cin)
    return mm(cols.numpy(), wk.numpy().T) + bias.numpy()


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def ratio(x, chain, ref):
    """the statistic: rms error of x over rms error of the fp32 chain, both against the fp64 reference"""
    return rms(np.asarray(x, np.float64) - ref) / rms(np.asarray(chain, np.float64) - ref)


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
FAMILIES_GEMM = ("randn", "wide")
# (M, N, K, family) of the shared GEMM cases: the small ragged shape, and the wide family at a shape the GEMM test already has
GEMM_CASES = [(70, 52, 96, "randn"), (70, 52, 96, "wide"), (289, 768, 768, "wide")]


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K, family):
    """-> a (M, K), w (N, K) fp32.  randn: the GEMM test's own scaling.  wide: the rows of a scaled by exp(4 randn) as in
    test_split_is_exact, and the k columns of w by exp(2 randn), so that the terms of one dot product differ by orders of magnitude"""
    g = torch.Generator().manual_seed(M + N + K + sum(map(ord, family)))
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.03
    if family == "wide":
        a = a * torch.exp(4 * torch.randn(M, 1, generator=g))
        w = w * torch.exp(2 * torch.randn(1, K, generator=g))
    return a.contiguous(), w.contiguous()


# (B, H, W, Cin, Cout): K = 288 and 576.  Cin <= 64: at K = 1152 the weakest mutant is only at 4 x the chain's error
CONV_ACC_CASES = [(3, 7, 5, 32, 36), (2, 9, 11, 64, 70)]
FAMILIES_CONV = ("randn", "wide")


@functools.lru_cache(maxsize=None)
def conv_inputs(case, family):
    """-> x (B, Cin, H, W), w (Cout, Cin, 3, 3) scaled as CONV_CASES of test_gpu_conv_chain.py, bias (Cout), residual rows
    (B*H*W, Cout).  wide: every pixel scaled by its own exp(4 randn), so one 3x3 window mixes exponents that far apart"""
    B, H, W, Cin, Cout = CONV_ACC_CASES[case]
    g = torch.Generator().manual_seed(77 * case + Cout + sum(map(ord, family)))
    x = torch.randn(B, Cin, H, W, generator=g)
    if family == "wide":
        x = x * torch.exp(4 * torch.randn(B, 1, H, W, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=g)
    res = torch.randn(B * H * W, Cout, generator=g)
    return x.contiguous(), w, bias, res


# (L, with bias): masked tail (CLIP); whole tiles; ragged key and query rows (TiTok); whole tiles with a bias holding a -inf band
ATTN_CASES = [(50, False), (96, False), (289, False), (256, True)]
FAMILIES_ATTN = ("randn", "sharp", "ascending")
ATTN_NSEQ, ATTN_HEADS = 2, 2
# ascending: natural-log score levels of consecutive 32-key tiles rise by SMALL and BIG in turn
ASC_SMALL, ASC_BIG, ASC_NOISE, ASC_BIAS = 2.0, 6.0, 0.2, 0.5
AT_DEFER = 6.0          # csrc/attn.hip: powers of two by which a row's maximum may grow before O and l are rescaled


def asc_levels(L):
    """level of every key: tile t = key // 32 sits SMALL above tile t - 1 for odd t and BIG above it for even t"""
    steps = np.array([0.0] + [ASC_SMALL if t % 2 else ASC_BIG for t in range(1, (L + 31) // 32 + 1)])
    return torch.from_numpy(np.cumsum(steps)[np.arange(L) // 32]).float()


@functools.lru_cache(maxsize=None)
def attn_inputs(case, family):
    """-> qkv (nseq * L, 3 * heads * 64) fp32, bias (2, L, L) or None, var (nseq) int32 or None.
    randn: unit normal q, k, v (scores about N(0, 1)): the family on which a lost term shows.
    sharp: q and k times 3 (scores about N(0, 9)): a few keys carry each row.
    ascending: in every head q[:, 0] = 8 and k[key, 0] = level(key // 32), so with scale 1/8 the first coordinate contributes exactly
      level(tile) to every score of a tile; the other 63 coordinates of q and k are uniform in +-ASC_NOISE and contribute at most
      63 * ASC_NOISE^2 / 8 = 0.315 in magnitude, the bias (uniform in +-ASC_BIAS for this family) at most 0.5.  Two scores of one row
      in tiles t - 1 and t therefore differ by step(t) +- 1.63: by 0.37 .. 3.63 (0.53 .. 5.24 powers of two) over a SMALL step, and
      by at least 4.37 over a BIG one.  So every row's maximum rises with every tile that has a key left; after a tile that raised the running maximum,
      the next (SMALL) tile stays below 2^AT_DEFER for all 32 rows of a block -- no rescale, P up to 2^5.24 -- and the one after
      (SMALL + BIG >= 4.74 above the adopted maximum, 6.8 powers of two) forces the rescale for every row.  The -inf band of the
      bias case masks the same keys for every row; a tile it masks whole leaves the maximum where it was.
      test_split3_accuracy_cpu.py replays the decisions in fp64 and asserts that both kinds of tile occur."""
    L, with_bias = ATTN_CASES[case]
    D = ATTN_HEADS * 64
    g = torch.Generator().manual_seed(1000 * case + sum(map(ord, family)))
    qkv = torch.randn(ATTN_NSEQ * L, 3 * D, generator=g)
    if family == "sharp":
        qkv[:, :2 * D] *= 3.0
    elif family == "ascending":
        qk = (torch.rand(ATTN_NSEQ * L, 2 * D, generator=g) * 2 - 1) * ASC_NOISE
        qk[:, 0:D:64] = 8.0
        qk[:, D:2 * D:64] = asc_levels(L).repeat(ATTN_NSEQ)[:, None]
        qkv[:, :2 * D] = qk
    bias = var = None
    if with_bias:
        bias = (torch.rand(2, L, L, generator=g) * 2 - 1) * ASC_BIAS if family == "ascending" else torch.randn(2, L, L, generator=g)
        bias[1, :, L // 3: L // 2] = float("-inf")          # a masked band, as Swin's shift masks hold
        var = torch.arange(ATTN_NSEQ, dtype=torch.int32) % 2
    return qkv.contiguous(), bias, var


def attn_units(qkv, L, bias, var):
    """qkv rows -> q, k, v as (nseq * heads, L, 64) numpy fp32 and the bias per unit (or None)"""
    D = ATTN_HEADS * 64
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(ATTN_NSEQ, L, ATTN_HEADS, 64).permute(0, 2, 1, 3).reshape(-1, L, 64).contiguous().numpy()
               for i in range(3))
    b = None
    if bias is not None:
        b = bias[var.long()].repeat_interleave(ATTN_HEADS, dim=0).numpy()
    return q, k, v, b


def attn_rows(o, L):
    """(nseq * heads, L, 64) -> (nseq * L, heads * 64), the kernels' row layout"""
    return np.asarray(o).reshape(ATTN_NSEQ, ATTN_HEADS, L, 64).transpose(0, 2, 1, 3).reshape(ATTN_NSEQ * L, ATTN_HEADS * 64)


def deferral_replay(q, k, b, scale=0.125):
    """the S3 kernel's rescale decisions replayed in fp64 on the exact scores of one unit: per 32-row query block and 32-key tile the
    running maximum (log2 domain) is raised only when some row's tile maximum exceeds it by more than AT_DEFER.
    -> (tiles that kept the old maximum, tiles after the first that raised it, largest P = 2^(s - m_run) met)"""
    L = q.shape[0]
    s = (q.astype(np.float64) * scale) @ k.astype(np.float64).T
    if b is not None:
        s = s + b
    s = s * np.log2(np.e)
    kept = raised = 0
    pmax = 0.0
    for r0 in range(0, L - L % 32 if L % 32 in (1, 2) and L > 32 else L, 32):
        rows = s[r0:r0 + 32]
        m_run = np.full(rows.shape[0], -np.inf)
        for t0 in range(0, L, 32):
            mx = rows[:, t0:t0 + 32].max(axis=1)
            if np.any((mx > m_run + AT_DEFER) | (np.isinf(m_run) & ~np.isinf(mx))):
                raised += int(t0 > 0)
                m_run = np.maximum(m_run, mx)
            else:
                kept += 1
            pmax = max(pmax, float(np.exp2(rows[:, t0:t0 + 32] - m_run[:, None]).max()))
    return kept, raised, pmax
