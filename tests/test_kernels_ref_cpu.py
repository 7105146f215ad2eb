"""The CPU references of tests/kernels_ref.py checked against each other and against the C oracle, and the caps the GPU tests
rely on checked on the very seeds those tests use -- so a cap is known to hold for the reference alone before a kernel is
looked at.  Every measured figure is printed (pytest -s)."""
import numpy as np
import torch

import kernels_ref as kr
from oracle import orc


def test_tile_major_round_trip_and_layout_refs_agree():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 32, 16, 8, generator=g)
    assert torch.equal(kr.from_tm16(kr.tm16(x), 2, 32, 16), x)
    rows = x.reshape(-1, 8)
    assert torch.equal(kr.im2col_2x2(kr.tm16(x).contiguous(), 2, 32, 16, True), kr.im2col_2x2(rows, 2, 32, 16, False))
    # PixelShuffle(2) followed by the 2x2 im2col is the identity up to the (c, ij) <-> (ij, c) transpose of a row
    src = torch.randn(2 * 8 * 16, 4 * 5, generator=g)
    shuffled = kr.from_tm16(kr.pixel_shuffle2_tm16(src, 2, 8, 16, 5), 2, 16, 32).reshape(-1, 5)
    back = kr.im2col_2x2(shuffled, 2, 16, 32, False).reshape(-1, 4, 5).transpose(1, 2).reshape(-1, 20)
    assert torch.equal(back, src)
    # a PxP patch im2col with P = 2 would be the 2x2 im2col with the channel axis outermost; check P = 4 against a direct loop
    img = torch.randn(2, 3, 8, 12, generator=g)
    cols = kr.im2col_patch(img, 4, 0.3, -0.7, False)
    y = img * torch.tensor(0.3) + torch.tensor(-0.7)
    for (b, gy, gx) in [(0, 0, 0), (1, 1, 2), (0, 1, 1)]:
        assert torch.equal(cols[(b * 2 + gy) * 3 + gx], y[b, :, gy * 4:gy * 4 + 4, gx * 4:gx * 4 + 4].reshape(-1))


def test_scale_index_ref_equals_oracle_quant_step():
    """the fp32 index reference == the idx of oracle.orc.quant_step (validated against the reference's goldens) on the edge values,
    and active_gather == the oracle's (C/4, H, W) layout of the coded quarter"""
    for thr in (0.12, None):
        for (H, W) in [(3, 5), (4, 4), (6, 8)]:
            C = 64
            sc = kr.entropy_scales(C * H * W, thr, seed=H * W).reshape(H, W, C).transpose(2, 0, 1).copy()
            zeros = np.zeros_like(sc)
            for k in range(4):
                _, idx = orc.quant_step(zeros, sc, zeros, k, thr, np.zeros_like(sc))
                active = kr.active_gather(torch.from_numpy(sc)[None], k)[0].numpy()
                assert np.array_equal(idx, kr.scale_index(active, thr)), (thr, H, W, k)
    s = kr.entropy_scales(400, 0.12, seed=1)
    got = kr.scale_index(s, 0.12)
    assert list(got[:9]) == [-1, -1, -1, -1, 3, 3, -1, 255, 255] and got.min() == -1 and got.max() == 255
    assert list(kr.scale_index(s, None)[:9]) == [0, 0, 0, 3, 3, 3, 0, 255, 255]
    assert len(set(kr.scale_index(s[9:9 + 120], None).tolist())) >= 32            # the neighbours of >= 32 distinct bin edges


def test_index_margin_ref_nudged_sigma_lands_on_alt():
    """the property the GPU test asserts of the kernel, here of the fp64 reference and the fp32 index reference alone"""
    for thr in (0.12, None):
        s = kr.entropy_scales(960, thr, seed=3)
        margin, accepted, _ = kr.index_margins(s, thr)
        cur = kr.scale_index(s, thr).astype(np.int64)
        near = margin < 0.5
        assert near.sum() > 300
        alt = accepted.max(axis=0)                                               # -2 marks "not a candidate"; ties are rare
        up = np.where(alt == -1, False, np.where(cur == -1, True, alt > cur))
        ls = np.log(np.maximum(s, np.float32(1e-5)).astype(np.float64)) + np.where(up, 1, -1) * (margin + 1e-3) * kr.LOG_STEP
        nudged = kr.scale_index(np.exp(ls).astype(np.float32), thr)
        assert np.array_equal(nudged[near], alt[near])
        assert margin[near].min() < 1e-4                                         # the bin-edge neighbours are in the set


def test_vq_fp32_emulation_within_the_near_tie_rule():
    for seed, (M, ncodes, dim, l2norm, _) in enumerate(kr.VQ_CASES):
        z, cb = kr.vq_inputs(M, ncodes, dim, seed)
        d64 = kr.vq_dist64(z, cb, l2norm)
        d32 = kr.vq_dist32(z, cb, l2norm)
        share, excess = kr.vq_check(d32.argmin(axis=1), d64)
        err = float(np.abs(d32 - d64).max())
        print(f"vq case {seed} M={M} ncodes={ncodes} dim={dim} l2norm={l2norm}: fp32 distance error {err:.3g}, "
              f"differ from fp64 argmin {share:.4%}, worst excess {excess:.3g}, max distance {d64.max():.3f}")
        assert d64.max() <= 4.0 + 1e-9
        assert err < kr.VQ_TOL / 2                                               # two such errors cannot exceed the tolerance
        assert share <= kr.VQ_DIFF_SHARE and excess <= kr.VQ_TOL
        assert share == 0.0                                                      # on these seeds the fp32 emulation differs on no token
        # the planted copy: its code is the fp64 argmin and no other code is within the tolerance, so the rule admits that code alone
        row = np.sort(d64[M // 2])
        assert d64[M // 2].argmin() == ncodes // 2 and (ncodes == 1 or row[1] - row[0] > kr.VQ_TOL)


def test_u8_fp32_emulation_differs_only_inside_the_half_integer_band():
    for seed, (M, D, _) in enumerate(kr.L2_CASES):
        x = kr.l2norm_inputs(M, D, seed)
        u64, q64, band = kr.l2norm_u8_64(x)
        u32, q32 = kr.l2norm_u8_32(x)
        share = float(band.mean())
        print(f"l2norm_u8 case {seed} ({M}, {D}): unit fp32 error {np.abs(u32 - u64).max():.3g}, band share {share:.3g}, "
              f"codes differing {int((q32 != q64).sum())}")
        assert np.abs(u32 - u64).max() <= kr.UNIT_TOL
        assert share <= kr.Q_BAND_SHARE
        kr.u8_check(q32, q64, band)
    onehot = np.zeros((2, 64), np.float32)
    onehot[0, 5], onehot[1, 9] = 3.0, -0.25
    _, q = kr.l2norm_u8_32(onehot)
    assert q[0, 5] == 255 and q[1, 9] == 0 and (np.delete(q[0], 5) == 128).all() and (np.delete(q[1], 9) == 128).all()


def test_half_even_rows_have_the_property_they_are_built_for():
    x, ks = kr.half_even_rows()
    assert len(ks) == 16 and (ks % 2 == 0).all()
    u, q = kr.l2norm_u8_32(x)
    assert np.array_equal(u, x)                                                  # the norm is exactly 1.0f
    t = (u[:, 3] * np.float32(0.5) + np.float32(0.5)) * np.float32(255)
    assert np.array_equal(t, (ks + 0.5).astype(np.float32))
    assert np.array_equal(q[:, 3], ks) and np.array_equal(np.floor(t + np.float32(0.5)), ks + 1)
    _, q64, band = kr.l2norm_u8_64(x)
    kr.u8_check(q, q64, band)


def test_attention_and_conv_refs_against_direct_loops():
    """attention64 against a per-(sequence, head) loop with the mask applied by DROPPING the masked keys (no -inf arithmetic);
    the bias variants: plain is finite, every row keeps its own key, UL / LR mask different key sets and variant 3 their union;
    conv3x3_64 against a direct sum over the nine taps at two pixels"""
    g = torch.Generator().manual_seed(4)
    L, nseq, heads = 64, 4, 2
    b = kr.attn_bias_variants(L, g)
    fin = torch.isfinite(b)
    assert bool(fin[0].all()) and bool(fin[:, torch.arange(L), torch.arange(L)].all())
    assert not torch.equal(fin[1], fin[2]) and torch.equal(fin[3], fin[1] & fin[2])
    assert int((~fin[1]).sum()) == 2 * 32 * 32 and int((~fin[2]).sum()) == 2 * 32 * 32      # half the keys of every query
    assert bool(fin[1, 0, :32].all()) and not bool(fin[1, 0, 32:].any())                    # token 0: upper rows only
    assert bool(fin[2, 0].reshape(8, 8)[:, :4].all()) and not bool(fin[2, 0].reshape(8, 8)[:, 4:].any())   # ... left columns only
    qkv = torch.randn(nseq * L, 3 * heads * 64, generator=g)
    var = torch.tensor([1, 2, 3, 0], dtype=torch.int32)
    got = kr.attention64(qkv, L, nseq, heads, b, var, 0.2)
    D = heads * 64
    for s in range(nseq):
        for h in range(heads):
            q, k, v = (qkv[s * L:(s + 1) * L, i * D + h * 64:i * D + (h + 1) * 64].double() for i in range(3))
            for t in (0, 31, 63):
                keep = fin[var[s], t]
                w = torch.softmax((k[keep] @ q[t]) * 0.2 + b[var[s], t][keep].double(), dim=0)
                assert float((w @ v[keep] - got[s * L + t, h * 64:(h + 1) * 64]).abs().max()) < 1e-12
    x, w4 = torch.randn(2, 4, 5, 6, generator=g), torch.randn(3, 4, 3, 3, generator=g)
    bias, res = torch.randn(3, generator=g), torch.randn(2, 3, 5, 6, generator=g)
    pre, out = kr.conv3x3_64(x, w4, bias, res, 2)
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    for (n, y, xx) in [(0, 0, 0), (1, 4, 5)]:
        want = (xp[n, :, y:y + 3, xx:xx + 3][None] * w4.double()).sum(dim=(1, 2, 3)) + bias.double()
        row = (n * 5 + y) * 6 + xx
        assert float((pre[row] - want).abs().max()) < 1e-12
        assert float((out[row] - (want * torch.sigmoid(want) + res[n, :, y, xx].double())).abs().max()) < 1e-12


def test_dwconv_ordered_ref_against_fp64_conv2d():
    """the ordered fp32 restatement is a depthwise convolution: within fp32 rounding of F.conv2d in fp64 for every combination of
    bias and prescale, an image smaller than the window included.  Bound: each of the k * k taps adds three roundings (prescale,
    product, sum) of at most 2^-24 of a partial sum that stays below 10: 3 * 10 * 6e-8 < 2e-6 per tap"""
    g = torch.Generator().manual_seed(4)
    for (B, H, W, C, k) in [(2, 6, 10, 8, 3), (1, 2, 4, 8, 5), (1, 9, 7, 4, 7), (2, 3, 3, 4, 1)]:
        x = torch.randn(B, H, W, C, generator=g)
        w = torch.randn(k * k, C, generator=g)
        for bias in (None, torch.randn(C, generator=g)):
            for ps in (None, torch.rand(C, generator=g) + 0.5):
                got = kr.dwconv_ordered32(x, w, bias, ps, k)
                xin = (x.double() * ps.double() if ps is not None else x.double()).permute(0, 3, 1, 2)
                ref = torch.nn.functional.conv2d(xin, w.double().t().reshape(C, 1, k, k), None if bias is None else bias.double(),
                                                 padding=k // 2, groups=C).permute(0, 2, 3, 1)
                assert got.shape == ref.shape and float((got.double() - ref).abs().max()) < 2e-6 * k * k, (B, H, W, C, k)
