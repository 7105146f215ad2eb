"""GPU unit tests of the entropy-side index kernels (csrc/entropy.hip: sgic_scale_to_index, sgic_index_step, sgic_index_margins,
sgic_dequant_step, and sgic_quant_step as the encoder twin) against the CPU references of tests/kernels_ref.py.  The decoder must
rebuild bit for bit the indexes the encoder coded with, otherwise rANS desynchronises; the scales therefore hold the edge values:
0, 1e-6, 1e-5, the fp32 values around the skip threshold, 0.11, 64, 1e4 and both fp32 neighbours of 40 bin edges."""
import numpy as np
import pytest
import torch

import kernels_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT16 = 0x5A5A
SENT_BITS = 0x7FA5C3D2
SHAPES = [(1, 3, 5), (2, 4, 4)]


def _api():
    import sgic_amd  # noqa
    from sgic_amd import ops
    return ops


def _sent(*shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sent(t):
    return t.cpu().contiguous().view(torch.int32) == SENT_BITS


def _scales(B, H, W, C, thr, ld):
    """-> (scales NCHW numpy, device rows (B*H*W, ld) with the scales in the first C columns and NaN beyond)"""
    nhwc = kr.entropy_scales(B * H * W * C, thr, seed=B * H * W + C).reshape(B, H, W, C)
    rows = torch.full((B * H * W, ld), float("nan"))
    rows[:, :C] = torch.from_numpy(nhwc).view(-1, C)
    return np.ascontiguousarray(nhwc.transpose(0, 3, 1, 2)), rows.to(DEV)


def _ref_idx(sc_nchw, thr):
    """(B, 4, C/4, H, W) int16 reference indexes of the four steps"""
    t = torch.from_numpy(sc_nchw)
    return np.stack([kr.scale_index(kr.active_gather(t, k).numpy(), thr) for k in range(4)], axis=1)


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("thr", [0.12, None])
def test_index_step_equals_quant_step_and_the_reference(B, H, W, thr):
    ops = _api()
    C, ld = 64, 2 * 64 + 4
    sc, d_sc = _scales(B, H, W, C, thr, ld)
    ref = _ref_idx(sc, thr)
    g = torch.Generator().manual_seed(H)
    y = (torch.randn(B * H * W, C, generator=g) * 3).to(DEV)
    means = torch.randn(B * H * W, ld, generator=g).to(DEV)
    yhat = _sent(B * H * W, C + 4)
    shape = (B, 4, C // 4, H, W)
    idx_dec = torch.full(shape, SENT16, dtype=torch.int16, device=DEV)
    idx_enc, sym = idx_dec.clone(), idx_dec.clone()
    for k in range(4):
        ops.index_step(d_sc, ld, B, H, W, C, k, thr, idx_dec)
        ops.quant_step(y, d_sc, means, ld, yhat, C + 4, B, H, W, C, k, thr, sym, idx_enc)
        h = idx_dec.cpu().numpy()
        assert np.array_equal(h[:, k], ref[:, k]), k
        assert (h[:, k + 1:] == SENT16).all()                     # only the step-k slice is written
        assert torch.equal(idx_enc, idx_dec), k                   # decoder twin == encoder, bit for bit
    assert bool(_is_sent(yhat[:, C:]).all()) and not bool(_is_sent(yhat[:, :C]).any())
    flat = torch.full((d_sc.numel() + 3,), SENT16, dtype=torch.int16, device=DEV)
    dense = torch.from_numpy(np.ascontiguousarray(sc)).to(DEV)
    ops.scale_indexes(dense, flat, thr)
    assert np.array_equal(flat[:dense.numel()].cpu().numpy(), kr.scale_index(sc.reshape(-1), thr)) and bool((flat[dense.numel():] == SENT16).all())


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("C", [4, 64])
def test_dequant_step_writes_only_the_active_quarter(B, H, W, C):
    """y_hat[active] = (float)sym + mu, a single IEEE add; every other entry keeps the sentinel"""
    ops = _api()
    ld_sm, ld_y = C + 8, C + 4
    g = torch.Generator().manual_seed(B * H + C)
    sym = torch.randint(-300, 300, (B, 4, C // 4, H, W), generator=g, dtype=torch.int16)
    sym[0, :, 0, 0, 0] = torch.tensor([30000, -30000, 0, 1], dtype=torch.int16)
    means = torch.randn(B * H * W, ld_sm, generator=g)
    for k in range(4):
        yhat = _sent(B * H * W, ld_y)
        ops.dequant_step(sym.to(DEV), means.to(DEV), ld_sm, yhat, ld_y, B, H, W, C, k)
        full = sym[:, k].repeat(1, 4, 1, 1).permute(0, 2, 3, 1).reshape(B * H * W, C).float() + means[:, :C]   # every quarter
        mask = kr.active_mask(C, H, W, k).expand(B, H, W, C).reshape(B * H * W, C)
        got = yhat.cpu()
        assert torch.equal(got[:, :C][mask], full[mask]), k
        assert bool(_is_sent(got[:, :C])[~mask].all()) and bool(_is_sent(got[:, C:]).all())


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("thr", [0.12, None])
def test_index_margins_vs_fp64_and_nudged_sigma(B, H, W, thr):
    """margin within one fp32 ulp of the fp64 reference plus 1e-9 (both sides compute in fp64 and round once); alt exact unless two
    candidates tie within that tolerance.  Independent property: a sigma with margin < 0.5 nudged (margin + 1e-3) steps past its
    near boundary is coded as alt by sgic_index_step."""
    ops = _api()
    C, ld = 64, 64 + 4
    Q = C // 4
    sc, d_sc = _scales(B, H, W, C, thr, ld)
    shape = (B, 4, Q, H, W)
    margin = _sent(*shape)
    alt = torch.full(shape, SENT16, dtype=torch.int16, device=DEV)
    cur = torch.full(shape, SENT16, dtype=torch.int16, device=DEV)
    t = torch.from_numpy(sc)
    for k in range(4):
        ops.index_margins(d_sc, ld, B, H, W, C, k, thr, margin, alt)
        ops.index_step(d_sc, ld, B, H, W, C, k, thr, cur)
        assert bool(_is_sent(margin[:, k + 1:]).all()) and bool((alt[:, k + 1:] == SENT16).all())
    got_m, got_a, got_c = margin.cpu().numpy().astype(np.float64), alt.cpu().numpy().astype(np.int64), cur.cpu().numpy().astype(np.int64)
    active = np.stack([kr.active_gather(t, k).numpy() for k in range(4)], axis=1)            # the sigma behind every output
    ref_m, accepted, tol = kr.index_margins(active, thr)
    bad = np.abs(got_m - ref_m) > tol
    assert not bad.any(), (active[bad][:5], got_m[bad][:5], ref_m[bad][:5])
    wrong = ~(accepted == got_a[None]).any(axis=0)
    assert not wrong.any(), (active[wrong][:5], got_a[wrong][:5], accepted[:, wrong][:, :5])
    # the property check, through the kernels only
    near = got_m < 0.5
    assert near.sum() > 100
    up = np.where(got_a == -1, False, np.where(got_c == -1, True, got_a > got_c))
    ls = np.log(np.maximum(active, np.float32(1e-5)).astype(np.float64)) + np.where(up, 1, -1) * (got_m + 1e-3) * kr.LOG_STEP
    nudged_nchw = np.zeros_like(sc)
    nudged_idx = torch.full(shape, SENT16, dtype=torch.int16, device=DEV)
    for k in range(4):                                                                      # scatter step k's sigmas back to NHWC rows
        mask = kr.active_mask(C, H, W, k).permute(2, 0, 1).expand(B, C, H, W).numpy()
        tiled = np.tile(np.exp(ls[:, k]).astype(np.float32), (1, 4, 1, 1))
        nudged_nchw = np.where(mask, tiled, nudged_nchw)
    rows = torch.from_numpy(np.ascontiguousarray(nudged_nchw.transpose(0, 2, 3, 1))).view(-1, C).to(DEV)
    for k in range(4):
        ops.index_step(rows, C, B, H, W, C, k, thr, nudged_idx)
    moved = nudged_idx.cpu().numpy().astype(np.int64)
    miss = near & (moved != got_a)
    assert not miss.any(), (active[miss][:5], got_m[miss][:5], got_a[miss][:5], moved[miss][:5])


def test_grid_stride_quant_step_index_step_and_scale_indexes():
    """more than 4096 workgroups of 256: 257 x 256 positions x 16 channels per quarter, and a flat array of 4096 * 256 + 333"""
    ops = _api()
    B, H, W, C = 1, 257, 256, 64
    rng = np.random.default_rng(8)
    sc = np.exp(rng.uniform(np.log(0.05), np.log(70.0), (B, C, H, W))).astype(np.float32)
    rows = torch.from_numpy(np.ascontiguousarray(sc.transpose(0, 2, 3, 1))).view(-1, C).to(DEV)
    y = torch.zeros(B * H * W, C, device=DEV)
    yhat = torch.zeros_like(y)
    shape = (B, 4, C // 4, H, W)
    idx_dec = torch.full(shape, SENT16, dtype=torch.int16, device=DEV)
    idx_enc, sym = idx_dec.clone(), idx_dec.clone()
    for k in range(4):
        ops.index_step(rows, C, B, H, W, C, k, 0.12, idx_dec)
        ops.quant_step(y, rows, y, C, yhat, C, B, H, W, C, k, 0.12, sym, idx_enc)
    assert np.array_equal(idx_dec.cpu().numpy(), _ref_idx(sc, 0.12)) and torch.equal(idx_enc, idx_dec)
    n = 4096 * 256 + 333
    flat = torch.full((n + 3,), SENT16, dtype=torch.int16, device=DEV)
    ops.scale_indexes(rows.view(-1)[:n], flat, 0.12)
    assert np.array_equal(flat[:n].cpu().numpy(), kr.scale_index(rows.view(-1)[:n].cpu().numpy(), 0.12)) and bool((flat[n:] == SENT16).all())
