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
