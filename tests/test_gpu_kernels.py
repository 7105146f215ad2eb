"""GPU unit tests of the secondary kernels against plain PyTorch (fp64) references of the same op -- LayerNorm
(titok/blocks.py:36,42), GroupNorm + swish into a zero-halo buffer (taming model.py:38-48), depthwise convolutions in
both feature-map layouts (blocks/conv_blocks.py:63-67, blocks/dcvc.py:21,35), row softmax, exact top-k.  The model-level
tests exercise them only at the shapes the codec uses; these cover ragged shapes and every layout flag."""
import numpy as np
import pytest
import torch

import kernels_ref as kr
from kernels_ref import from_tm16 as _from_tm16, tm16 as _tm16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("M,C,act", [(9248, 1024, 0), (1000, 768, 0), (77, 512, 0), (2048, 128, 2), (5, 64, 0)])
def test_layernorm_vs_torch(M, C, act):
    import sgic_amd  # noqa
    from sgic_amd import ops
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g) * 3 + 1
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (C,), w.double(), b.double(), eps=1e-5)
    if act == 2:
        ref = torch.nn.functional.silu(ref)
    got = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), act=act).cpu().double()
    assert float((got - ref).abs().max()) < 2e-5
    # segment maps: normalise the first 3 rows of every 5-row segment into the first 3 rows of every 4-row segment
    if M >= 20:
        n = M // 5
        out = torch.zeros(n * 4, C, device=DEV)
        ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), out=out, M=n * 3, x_seg=(3, 5), y_seg=(3, 4), act=act)
        o = out.cpu().double().view(n, 4, C)
        assert float((o[:, :3] - ref.view(-1, C)[:n * 5].view(n, 5, C)[:, :3]).abs().max()) < 2e-5     # ref is silu(ref) when act == 2
        assert float(o[:, 3].abs().max()) == 0.0


@pytest.mark.parametrize("B,H,W,C,swish,halo", [(2, 16, 16, 128, True, True), (3, 8, 24, 256, False, False), (1, 32, 32, 64, True, False)])
def test_groupnorm_vs_torch(B, H, W, C, swish, halo):
    import sgic_amd  # noqa
    from sgic_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.5
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = torch.nn.functional.group_norm(x.double(), 32, w.double(), b.double(), eps=1e-6)
    if swish:
        ref = ref * torch.sigmoid(ref)
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous().to(DEV)
    out = ops.groupnorm(rows, w.to(DEV), b.to(DEV), B, H, W, swish=swish, halo=halo).cpu().double()
    if halo:
        o = out.view(B, H + 2, W + 2, C)
        assert float(o[:, 0].abs().max()) == 0.0 and float(o[:, :, 0].abs().max()) == 0.0 and float(o[:, -1].abs().max()) == 0.0
        out = o[:, 1:-1, 1:-1]
    got = out.reshape(B, H, W, C).permute(0, 3, 1, 2)
    assert float((got - ref).abs().max()) < 3e-5


@pytest.mark.parametrize("B,H,W,C,k,tile16,pre", [(2, 16, 16, 768, 5, True, True), (3, 8, 8, 64, 3, False, False), (1, 32, 16, 128, 5, True, False),
                                                   (2, 6, 10, 32, 3, False, True), (1, 16, 16, 64, 7, False, False)])
def test_dwconv_vs_torch(B, H, W, C, k, tile16, pre):
    """both kernels (4-pixels-per-thread for k in {3,5} and W % 4 == 0, generic otherwise), both layouts"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    g = torch.Generator().manual_seed(H * W + k)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, k, k, generator=g)
    b = torch.randn(C, generator=g)
    ps = torch.rand(C, generator=g) + 0.5 if pre else None
    xin = x * ps.view(1, C, 1, 1) if pre else x
    ref = torch.nn.functional.conv2d(xin.double(), w.double(), b.double(), padding=k // 2, groups=C).permute(0, 2, 3, 1)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    rows = (_tm16(nhwc) if tile16 else nhwc.reshape(B * H * W, C)).contiguous().to(DEV)
    wk = w.reshape(C, k * k).t().contiguous().to(DEV)
    out = ops.dwconv(rows, wk, b.to(DEV), ps.to(DEV) if pre else None, B, H, W, k, tile16=tile16).cpu()
    got = (_from_tm16(out, B, H, W) if tile16 else out.reshape(B, H, W, C)).double()
    assert float((got - ref).abs().max()) < 2e-5


def test_softmax_rows_and_topk_vs_torch():
    import sgic_amd  # noqa
    from sgic_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(300, 256, generator=g) * 4
    got = ops.softmax_rows(x.to(DEV).contiguous(), 256, scale=0.5).cpu().double()
    assert float((got - torch.softmax(x.double() * 0.5, dim=-1)).abs().max()) < 1e-6
    s = torch.randn(9, 5000, generator=g)
    s[3, 100] = s[3, 7] = 9.0                                  # a tie: the lower index must come first
    val, idx = ops.topk_rows(s.to(DEV).clone(), 20)
    ref = torch.sort(s, dim=1, descending=True, stable=True)
    assert torch.equal(idx.cpu().long(), ref.indices[:, :20]) and torch.equal(val.cpu(), ref.values[:, :20])
    assert idx[3, 0].item() == 7 and idx[3, 1].item() == 100


def test_pad_replicate_vs_torch():
    """compress.py:258-261 (get_padding_size + F.pad replicate): bit-exact data movement"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    g = torch.Generator().manual_seed(1)
    for (B, H, W, pad) in [(2, 200, 300, (0, 212, 0, 56)), (1, 256, 256, (0, 0, 0, 0)), (3, 17, 9, (2, 3, 1, 4))]:
        x = torch.randn(B, 3, H, W, generator=g)
        ref = torch.nn.functional.pad(x, pad, mode="replicate")
        got = ops.pad_replicate(x.to(DEV), *pad).cpu()
        assert got.shape == ref.shape and torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------------------
# Glue, layout and elementwise kernels behind the C ABI (csrc/misc.hip, csrc/decode.hip) against tests/kernels_ref.py.  Every
# output is pre-filled with a sentinel bit pattern that must survive wherever the operation does not write.
# ------------------------------------------------------------------------------------------------------------------------------
SENT_BITS = 0x7FA5C3D2                      # a NaN pattern no kernel here produces


def _sent(*shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sent(t):
    return t.cpu().contiguous().view(torch.int32) == SENT_BITS


def _same_bits(got, ref):
    return torch.equal(kr.bits(got.cpu()), kr.bits(ref))


def _api():
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd._lib import call
    return ops, call


@pytest.mark.parametrize("P,C,tile16", [(P, C, t) for P in (4, 16, 32) for C in (1, 3) for t in (False, True)])
def test_im2col_patch_vs_unfold(P, C, tile16):
    ops, call = _api()
    B, gh, gw = (2, 16, 32) if tile16 else (2, 2, 3)
    x = torch.randn(B, C, gh * P, gw * P, generator=torch.Generator().manual_seed(P + C))
    x[0, 0, 0, 0] = -0.0
    for mul, add in [(1.0, 0.0), (0.5, 0.5), (0.3, -0.7)]:
        out = _sent(B * gh * gw + 1, C * P * P)
        ops.im2col_patch(x.to(DEV), P, mul, add, tile16=tile16, out=out)
        assert _same_bits(out[:-1], kr.im2col_patch(x, P, mul, add, tile16)), (mul, add)
        assert bool(_is_sent(out[-1]).all())


@pytest.mark.parametrize("B,H,W,C,tile16", [(2, 6, 10, 4, False), (1, 32, 16, 36, True), (3, 2, 2, 128, False)])
def test_im2col_2x2_vs_reshape(B, H, W, C, tile16):
    ops, call = _api()
    x = kr.special_values(torch.randn(B * H * W, C, generator=torch.Generator().manual_seed(H)))
    out = _sent(B * H * W // 4 + 1, 4 * C)
    ops.im2col_2x2(x.to(DEV), B, H, W, tile16=tile16, out=out)
    assert _same_bits(out[:-1], kr.im2col_2x2(x, B, H, W, tile16)) and bool(_is_sent(out[-1]).all())


@pytest.mark.parametrize("B,H,W,C", [(2, 8, 16, 5), (1, 8, 8, 64)])
def test_pixel_shuffle2_tm16_vs_torch(B, H, W, C):
    ops, call = _api()
    x = kr.special_values(torch.randn(B * H * W, 4 * C, generator=torch.Generator().manual_seed(C)))
    out = _sent(B * 4 * H * W + 1, C)
    call("sgic_pixel_shuffle2_tm16", x.to(DEV), B, H, W, C, out)
    assert _same_bits(out[:-1], kr.pixel_shuffle2_tm16(x, B, H, W, C)) and bool(_is_sent(out[-1]).all())


@pytest.mark.parametrize("extra", [0, 8])
def test_fake2d_transpose_vs_reshape(extra):
    ops, call = _api()
    N, T, D = 3, 5, 12
    stride = T * D + extra
    buf = kr.special_values(torch.randn(N * stride, generator=torch.Generator().manual_seed(extra)))
    out = _sent(N * T + 1, D)
    call("sgic_fake2d_transpose", buf.to(DEV), ops._cl(stride), out, N, T, D)
    assert _same_bits(out[:-1], kr.fake2d_transpose(buf, stride, N, T, D)) and bool(_is_sent(out[-1]).all())


@pytest.mark.parametrize("T", [0, 3])
def test_assemble_tokens_vs_cat(T):
    ops, call = _api()
    N, P, D = 2, 4, 8
    g = torch.Generator().manual_seed(T)
    emb, cls, pos = torch.randn(N * P, D, generator=g), torch.randn(D, generator=g), torch.randn(1 + P, D, generator=g)
    lat, latpos = (torch.randn(T, D, generator=g), torch.randn(T, D, generator=g)) if T else (None, None)
    out = _sent(N * (1 + P + T) + 1, D)
    ops.assemble_tokens(emb.to(DEV), cls.to(DEV), pos.to(DEV), lat.to(DEV) if T else None, latpos.to(DEV) if T else None, N, P, T, D,
                        out=out)
    assert _same_bits(out[:-1], kr.assemble_tokens(emb, cls, pos, lat, latpos, N, P, T, D)) and bool(_is_sent(out[-1]).all())


def test_assemble_dec_tokens_vs_cat():
    ops, call = _api()
    N, P, T, D = 3, 4, 2, 8
    g = torch.Generator().manual_seed(9)
    emb, cls, mask = torch.randn(N * T, D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    pos, latpos = torch.randn(1 + P, D, generator=g), torch.randn(T, D, generator=g)
    out = _sent(N * (1 + P + T) + 1, D)
    call("sgic_assemble_dec_tokens", emb.to(DEV), cls.to(DEV), mask.to(DEV), pos.to(DEV), latpos.to(DEV), N, P, T, D, out)
    assert _same_bits(out[:-1], kr.assemble_dec_tokens(emb, cls, mask, pos, latpos, N, P, T, D)) and bool(_is_sent(out[-1]).all())


@pytest.mark.parametrize("with_vec", [True, False])
@pytest.mark.parametrize("iseg,oseg", [(0, 5), (7, 8), (5, 5)])
def test_add_rows_bcast_slices_and_broadcast(with_vec, iseg, oseg):
    """iseg = 0: one block broadcast to all Nn (bottleneck.py:132); input and output are column slices of wider buffers; oseg > Lr
    leaves rows between the segments untouched"""
    ops, call = _api()
    Nn, Lr, D = 3, 5, 8
    g = torch.Generator().manual_seed(iseg + oseg)
    wide_in = torch.randn(max(iseg * (Nn - 1), 0) + Lr, 24, generator=g)
    inp = wide_in[:, 4:4 + D]
    if not with_vec:
        kr.special_values(inp[0])
    vec = torch.randn(Lr, D, generator=g) if with_vec else None
    wide_out = _sent(oseg * (Nn - 1) + Lr + 2, 32)
    ops.add_rows_bcast(wide_in.to(DEV)[:, 4:4 + D], iseg, vec.to(DEV) if with_vec else None, wide_out[:, 8:8 + D], oseg, Nn, Lr)
    ref = kr.add_rows_bcast(inp, iseg, vec, Nn, Lr)
    got = wide_out.cpu()
    written = torch.zeros(got.shape, dtype=torch.bool)
    for n in range(Nn):
        assert _same_bits(got[n * oseg:n * oseg + Lr, 8:8 + D], ref[n]), n
        written[n * oseg:n * oseg + Lr, 8:8 + D] = True
    assert bool(_is_sent(got)[~written].all())


@pytest.mark.parametrize("nblocks", [1, 5])
def test_copy_row_blocks_exact(nblocks):
    ops, call = _api()
    rows, stride, C = 3, 7, 12
    x = kr.special_values(torch.randn((nblocks - 1) * stride + rows, C, generator=torch.Generator().manual_seed(nblocks)))
    big = _sent(nblocks * rows + 1, C)
    ops.copy_row_blocks(x.to(DEV), rows, stride, nblocks, out=big[:nblocks * rows])
    assert _same_bits(big[:-1], kr.copy_row_blocks(x, rows, stride, nblocks)) and bool(_is_sent(big[-1]).all())


@pytest.mark.parametrize("ld", [3, 4, 8])
def test_nhwc3_to_nchw_clamp_vs_torch(ld):
    ops, call = _api()
    B, H, W = 2, 5, 7
    x = torch.randn(B * H * W, ld, generator=torch.Generator().manual_seed(ld)) * 2
    one = np.float32(1)
    edge = [1.0, -1.0, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), -np.nextafter(one, np.float32(2)),
            -np.nextafter(one, np.float32(0)), -0.0, 0.0]
    x.view(-1)[:len(edge) * ld:ld] = torch.tensor(np.array(edge, dtype=np.float32))
    out = _sent(B * 3 * H * W + 5)
    call("sgic_nhwc3_to_nchw_clamp", x.to(DEV), ld, B, H, W, out)
    assert _same_bits(out[:-5].view(B, 3, H, W), kr.nhwc3_to_nchw_clamp(x, B, H, W)) and bool(_is_sent(out[-5:]).all())


@pytest.mark.parametrize("B,H,W,C,tile16", [(2, 16, 32, 8, False), (2, 16, 32, 8, True), (1, 3, 5, 4, False)])
@pytest.mark.parametrize("upsample", [False, True])
def test_halo_copy_interior_and_border(B, H, W, C, tile16, upsample):
    ops, call = _api()
    x = kr.special_values(torch.randn(B * H * W, C, generator=torch.Generator().manual_seed(H + C)))
    s = 2 if upsample else 1
    out = _sent(B, H * s + 2, W * s + 2, C)
    ops.halo_copy(x.to(DEV), B, H, W, C, upsample=upsample, tile16=tile16, out=out)
    got = out.cpu()
    assert _same_bits(got[:, 1:-1, 1:-1], kr.halo_interior(x, B, H, W, upsample, tile16).contiguous())
    border = torch.ones(got.shape, dtype=torch.bool)
    border[:, 1:-1, 1:-1] = False
    assert bool(_is_sent(got)[border].all())


def test_embed_tokens_clamps_out_of_range_ids():
    ops, call = _api()
    B, L, D, vocab = 2, 7, 8, 11
    g = torch.Generator().manual_seed(2)
    table, pos = torch.randn(vocab, D, generator=g), torch.randn(L, D, generator=g)
    ids = torch.tensor([[-5, 0, vocab - 1, vocab, 10 ** 6, 3, -2 ** 31], [2 ** 31 - 1, 1, 2, vocab + 1, -1, 9, 10]], dtype=torch.int32)
    out = _sent(B * L + 1, D)
    call("sgic_embed_tokens", ids.to(DEV), table.to(DEV), pos.to(DEV), out, B, L, D, vocab)
    assert _same_bits(out[:-1], kr.embed_tokens(ids, table, pos, vocab)) and bool(_is_sent(out[-1]).all())


@pytest.mark.parametrize("L", [1, 63, 77, 130])
@pytest.mark.parametrize("D", [4, 100])
def test_gather_eot_rows_first_maximum(L, D):
    """the maximum at 0 and at L - 1, and duplicated: in one lane's stride (l, l + 64), in neighbouring lanes, in both halves of the
    shuffle tree, and a later iteration of a low lane against a higher lane -- the first position wins, as torch.argmax"""
    ops, call = _api()
    places = [(0,), (L - 1,), (2, 66), (5, 6), (5, 37), (3, 64), (1, 33, 65, 129), (70, 69), tuple(range(L))]
    places = [t for t in places if max(t) < L]
    B, ldx = len(places) + 2, D + 3
    g = torch.Generator().manual_seed(L + D)
    ids = torch.randint(0, 1000, (B, L), generator=g, dtype=torch.int32)
    for b, t in enumerate(places):
        ids[b, list(t)] = 49407
    x = kr.special_values(torch.randn(B * L, ldx, generator=g))
    out = _sent(B + 1, D)
    call("sgic_gather_eot_rows", ids.to(DEV), x.to(DEV), ldx, out, B, L, D)
    assert _same_bits(out[:-1], kr.gather_eot_rows(ids, x, D).contiguous()) and bool(_is_sent(out[-1]).all())


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_topk_rows_vs_stable_sort(n):
    """row 2 has fewer finite scores than k = n: the -inf entries must follow in index order, each once (a kernel that marks taken
    entries with -inf returns the lowest of them again and again)"""
    ops, call = _api()
    g = torch.Generator().manual_seed(n)
    s = torch.randn(4, n, generator=g)
    s[1] = 0.25                                                   # all equal: indices 0 .. k-1 in order
    s[2, torch.randperm(n, generator=g)[:max(n - 3, 1)]] = -float("inf")   # fewer finite scores than k = n
    s[3, ::2] = s[3, 0]                                           # many ties among random values
    for k in (1, n):
        val, idx = ops.topk_rows(s.to(DEV).clone(), k)
        ref_v, ref_i = kr.topk_rows(s, k)
        assert torch.equal(idx.cpu().long(), ref_i), (n, k)
        assert torch.equal(val.cpu(), ref_v), (n, k)
    assert torch.equal(idx[1].cpu().long(), torch.arange(n))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("vrows", [1, 7])
def test_colop_bit_exact_with_slices(mode, vrows):
    """single IEEE ops (misc.hip is built without contraction): bit-equal to torch fp32, the division of mode 1 included"""
    ops, call = _api()
    M, C = 30, 8
    g = torch.Generator().manual_seed(mode * 10 + vrows)
    xw, vw = torch.randn(M, 16, generator=g) * 3, torch.rand(vrows, 12, generator=g) * 1.5 - 0.25
    vw[0, 4:8] = torch.tensor([0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), float(np.nextafter(np.float32(0.5), np.float32(1))), -0.0])
    xw[0, 4] = -0.0
    out = _sent(M + 1, 20)
    ops.colop(xw.to(DEV)[:, 4:4 + C], vw.to(DEV)[:, 4:4 + C], mode, out=out[:M, 8:8 + C])
    got = out.cpu()
    assert _same_bits(got[:M, 8:8 + C], kr.colop(xw[:, 4:4 + C], vw[:, 4:4 + C], mode).contiguous())
    written = torch.zeros(got.shape, dtype=torch.bool)
    written[:M, 8:8 + C] = True
    assert bool(_is_sent(got)[~written].all())


@pytest.mark.parametrize("C2", [4, 132])
def test_gated_lrelu_bit_exact(C2):
    ops, call = _api()
    M = 5
    x = torch.randn(M, 2 * C2, generator=torch.Generator().manual_seed(C2))
    x[0, :4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    x[0, C2:C2 + 4] = torch.tensor([0.0, 0.0, -0.0, -0.0])
    out = _sent(M + 1, C2)
    ops.gated_lrelu(x.to(DEV), out=out[:M])
    assert _same_bits(out[:-1], kr.gated_lrelu(x)) and bool(_is_sent(out[-1]).all())


# ---- tolerance against fp64 -----------------------------------------------------------------------------------------------------
def _vq(ops, z, cb, l2norm, ldz):
    wide = torch.full((z.shape[0], ldz), float("nan"))
    wide[:, :z.shape[1]] = torch.from_numpy(z)
    return ops.vq_argmin(wide.to(DEV)[:, :z.shape[1]], torch.from_numpy(cb).to(DEV), l2norm=bool(l2norm)).cpu().numpy()


@pytest.mark.parametrize("case", range(len(kr.VQ_CASES)))
def test_vq_argmin_vs_fp64(case):
    """an index passes if its fp64 distance is within 2^-17 of the fp64 minimum (fp32 error of the three-term distance on vectors of
    norm <= 1: 1.1e-6 measured on the CPU, test_kernels_ref_cpu.py); at most 0.5 % of the tokens may differ from the fp64 argmin"""
    ops, call = _api()
    M, ncodes, dim, l2norm, ldz = kr.VQ_CASES[case]
    z, cb = kr.vq_inputs(M, ncodes, dim, case)                   # token M // 2 equals code ncodes // 2 and must return it
    idx = _vq(ops, z, cb, l2norm, ldz)
    share, excess = kr.vq_check(idx, kr.vq_dist64(z, cb, l2norm))
    print(f"vq case {case}: differ from fp64 argmin {share:.4%}, worst excess {excess:.3g}")
    assert excess <= kr.VQ_TOL and share <= kr.VQ_DIFF_SHARE
    assert idx[M // 2] == ncodes // 2


@pytest.mark.parametrize("l2norm", [1, 0])
def test_vq_argmin_exact_ties_resolve_to_the_lowest_code(l2norm):
    """codebook row j copied to j + 1 (neighbouring thread), j + 64 (another wave), j + 256 (same thread, later pass): each level of
    the reduction decides one of the ties; tokens equal to the row must return the lowest duplicate, exactly"""
    ops, call = _api()
    M, ncodes, dim = 9, 600, 12
    z, cb = kr.vq_inputs(M, ncodes, dim, 77)
    for t, (j, dup) in enumerate([(10, 11), (20, 84), (30, 286), (255, 256), (63, 64), (40, 41)]):
        cb[dup] = cb[j]
        z[t] = cb[j] * np.float32(0.5 if l2norm else 1.0)
    cb[[105, 361]] = cb[40]                                       # row 40: every level at once (41, 105, 361)
    idx = _vq(ops, z, cb, l2norm, 16)
    assert list(idx[:6]) == [10, 20, 30, 255, 63, 40]
    share, excess = kr.vq_check(idx, kr.vq_dist64(z, cb, l2norm))
    assert excess <= kr.VQ_TOL


@pytest.mark.parametrize("l2norm", [1, 0])
def test_vq_argmin_nan_inf_and_zero_tokens_stay_in_range(l2norm):
    """a token holding NaN or +Inf makes every distance NaN: the kernel returns code 0 there (torch.argmin of an all-NaN row), and
    the other tokens of the same workgroup are unaffected; an all-zero token returns an index in range"""
    ops, call = _api()
    M, ncodes, dim = 8, 300, 12
    z, cb = kr.vq_inputs(M, ncodes, dim, 5)
    clean = _vq(ops, z, cb, l2norm, 12)
    bad = z.copy()
    bad[1, 3], bad[6, 0], bad[4] = np.nan, np.inf, 0.0
    idx = _vq(ops, bad, cb, l2norm, 12)
    assert idx.min() >= 0 and idx.max() < ncodes
    assert idx[1] == 0 and idx[6] == 0
    keep = [0, 2, 3, 5, 7]
    assert np.array_equal(idx[keep], clean[keep])


@pytest.mark.parametrize("dim,ld", [(5, 5), (5, 16), (5, 32), (12, 12), (12, 16), (12, 32)])
@pytest.mark.parametrize("M", [1, 65, 130])
def test_codebook_gather_norm_vs_fp64(dim, ld, M):
    ops, call = _api()
    rng = np.random.default_rng(dim * 100 + M)
    cb = (rng.standard_normal((50, dim)) * rng.uniform(0.1, 10, (50, 1))).astype(np.float32)
    idx = rng.integers(0, 50, M).astype(np.int32)
    out = _sent(M + 1, ld)
    call("sgic_codebook_gather_norm", torch.from_numpy(idx).to(DEV), torch.from_numpy(cb).to(DEV), M, dim, ld, out)
    got = out.cpu()
    assert float(np.abs(got[:M, :dim].double().numpy() - kr.codebook_gather_norm(idx, cb)).max()) <= 2.0 ** -21
    assert _same_bits(got[:M, dim:], torch.zeros(M, ld - dim)) and bool(_is_sent(got[M]).all())


def _l2(call, x, ldx):
    M, D = x.shape
    wide = torch.full((M, ldx), float("nan"))
    wide[:, :D] = torch.from_numpy(x)
    unit, q = _sent(M + 1, D), torch.full((M + 1, D), 77, dtype=torch.uint8, device=DEV)
    call("sgic_l2norm_u8", wide.to(DEV), ldx, M, D, unit, q)
    assert bool(_is_sent(unit[M]).all()) and bool((q[M] == 77).all())
    return unit[:M].cpu().numpy(), q[:M].cpu().numpy()


@pytest.mark.parametrize("case", range(len(kr.L2_CASES)))
def test_l2norm_u8_vs_fp64_and_its_own_unit(case):
    """(a) unit within 2^-21 of fp64; (b) q == the quantiser recomputed in numpy fp32 from the kernel's own unit, exactly; (c) q == the
    fp64 code outside the half-integer band (2e-4), either neighbour inside; the band holds at most 0.2 % of the elements"""
    ops, call = _api()
    M, D, ldx = kr.L2_CASES[case]
    x = kr.l2norm_inputs(M, D, case)
    unit, q = _l2(call, x, ldx)
    u64, q64, band = kr.l2norm_u8_64(x)
    print(f"l2norm_u8 case {case}: unit error {np.abs(unit - u64).max():.3g}, band share {band.mean():.3g}")
    assert np.abs(unit - u64).max() <= kr.UNIT_TOL
    assert np.array_equal(q, kr.u8_from_unit32(unit))
    assert band.mean() <= kr.Q_BAND_SHARE
    kr.u8_check(q, q64, band)


def test_l2norm_u8_one_hot_half_even_and_zero_row():
    ops, call = _api()
    x = kr.l2norm_inputs(6, 64, 11)
    x[1], x[2] = 0.0, 0.0
    x[1, 5], x[2, 9] = 3.0, -0.25
    unit, q = _l2(call, x, 64)
    assert q[1, 5] == 255 and (np.delete(q[1], 5) == 128).all()          # 127.5 -> 128 (round half to even)
    assert q[2, 9] == 0 and (np.delete(q[2], 9) == 128).all()
    # rows whose quantiser input is exactly k + 0.5 with k even: rint gives k (floor(x + 0.5) would give k + 1)
    rows, ks = kr.half_even_rows()
    unit_h, q_h = _l2(call, rows, 64)
    assert np.array_equal(unit_h, rows) and np.array_equal(q_h[:, 3], ks)
    assert np.array_equal(q_h, kr.u8_from_unit32(unit_h))
    # an all-zero row in the batch leaves the other rows unchanged
    withzero = x.copy()
    withzero[3] = 0.0
    unit_z, q_z = _l2(call, withzero, 64)
    keep = [0, 1, 2, 4, 5]
    assert np.array_equal(unit_z[keep], unit[keep]) and np.array_equal(q_z[keep], q[keep])


@pytest.mark.parametrize("L", [1, 63, 65, 289, 4096])
@pytest.mark.parametrize("M", [1, 5])
def test_softmax_rows_ragged_lengths(L, M):
    ops, call = _api()
    x = torch.randn(M, L, generator=torch.Generator().manual_seed(L + M)) * 4
    x[0] = 1.5                                                    # a constant row
    if M > 1:
        x[1] = torch.linspace(0.0, 500.0, L) if L > 1 else 0.0    # scaled spread 250: the tail underflows to exact zeros
    out = _sent(M + 1, L)
    ops.softmax_rows(x.to(DEV), L, scale=0.5, out=out[:M])
    got = out[:M].cpu().double()
    assert float((got - torch.softmax(x.double() * 0.5, dim=-1)).abs().max()) < 1e-6
    assert float((got.sum(dim=1) - 1).abs().max()) < 1e-5 and bool(_is_sent(out[M]).all())
    if M > 1 and L >= 63:
        assert float(got[1, 0]) == 0.0 and float(got[1, -1]) > 0.0


@pytest.mark.parametrize("M,N,K,shared,act,pad", [(70, 52, 36, True, 2, 4), (33, 7, 64, False, 0, 3), (70, 52, 36, False, 0, 5), (33, 7, 64, True, 2, 1)])
def test_gemm_batched_strides_bias_residual(M, N, K, shared, act, pad):
    """tolerance: the project's own, 3e-6 sqrt(K) max(1, max|pre|) against fp64 (test_gemm_fuzz_all_tile_modes_identical_and_close_to_fp64)"""
    ops, call = _api()
    batch = 3
    g = torch.Generator().manual_seed(M + K + act)
    lda, ldw, ldr, ldc = K + 4, K + 8, N + 2 * pad, N + pad          # pad = 4: the float4 epilogue, otherwise the scalar one
    sa, sw, sr, sc = M * lda + 12, (0 if shared else N * ldw + 4), M * ldr + 3 * pad, M * ldc + 2 * pad
    A = torch.randn(batch * sa, generator=g)
    Wt = torch.randn((1 if shared else batch) * (N * ldw + 4), generator=g)
    R = torch.randn(batch * sr, generator=g)
    bias = torch.randn(N, generator=g)
    out = _sent(batch * sc)
    ops.gemm_batched(A.to(DEV), lda, sa, Wt.to(DEV), ldw, sw, out, ldc, sc, M, N, K, batch, bias=bias.to(DEV), residual=R.to(DEV), ldr=ldr,
                     sr=sr, act=act)
    view = lambda t, s, ld, rows, cols: torch.stack([t[b * s:b * s + rows * ld].view(rows, ld)[:, :cols] for b in range(batch)])  # noqa: E731
    a = view(A, sa, lda, M, K)
    w = Wt[:N * ldw].view(1, N, ldw)[:, :, :K] if shared else view(Wt, sw, ldw, N, K)
    pre, ref = kr.gemm_batched64(a, w, bias, view(R, sr, ldr, M, N), act)
    got = out.cpu()
    written = torch.zeros(got.shape, dtype=torch.bool)
    for b in range(batch):
        blk = got[b * sc:b * sc + M * ldc].view(M, ldc)
        err = float((blk[:, :N].double() - ref[b]).abs().max())
        assert err < 3e-6 * (K ** 0.5) * max(1.0, float(pre.abs().max())), (b, err)
        written[b * sc:b * sc + M * ldc].view(M, ldc)[:, :N] = True
    assert bool(_is_sent(got)[~written].all())


# ---- grid-stride loops: more work items than the capped grid holds, and not a multiple of it ------------------------------------
def test_grid_stride_colop():
    ops, call = _api()
    M, C = 524288 + 77, 16                                        # (M * C / 4) float4 items = 8192 * 256 + 308
    g = torch.Generator().manual_seed(1)
    x, v = torch.randn(M, C, generator=g), torch.rand(7, C, generator=g) + 0.1
    out = _sent(M + 1, C)
    ops.colop(x.to(DEV), v.to(DEV), 1, out=out[:M])
    assert _same_bits(out[:M], kr.colop(x, v, 1)) and bool(_is_sent(out[M]).all())


def test_grid_stride_im2col_2x2():
    ops, call = _api()
    B, H, W, C = 1, 1028, 1024, 8                                 # 514 * 512 * 4 * 2 float4 items = 8192 * 256 + 8192
    x = torch.randn(B * H * W, C, generator=torch.Generator().manual_seed(2))
    out = _sent(B * H * W // 4 + 1, 4 * C)
    ops.im2col_2x2(x.to(DEV), B, H, W, out=out)
    assert _same_bits(out[:-1], kr.im2col_2x2(x, B, H, W, False)) and bool(_is_sent(out[-1]).all())


def test_grid_stride_add_rows_bcast():
    ops, call = _api()
    Nn, Lr, D, oseg = 74910, 7, 16, 8                             # 74910 * 7 * 4 float4 items = 8192 * 256 + 328
    g = torch.Generator().manual_seed(3)
    inp, vec = torch.randn(Nn * Lr, D, generator=g), torch.randn(Lr, D, generator=g)
    out = _sent(Nn * oseg, D)
    ops.add_rows_bcast(inp.to(DEV), Lr, vec.to(DEV), out, oseg, Nn, Lr)
    got = out.cpu().view(Nn, oseg, D)
    assert _same_bits(got[:, :Lr], kr.add_rows_bcast(inp, Lr, vec, Nn, Lr)) and bool(_is_sent(got[:, Lr:]).all())


def test_grid_stride_nhwc3_to_nchw_clamp():
    ops, call = _api()
    B, H, W = 1, 1183, 1183                                       # 3 * 1183^2 items = 16384 * 256 + 4163 (decode.hip caps at 16384)
    x = torch.randn(B * H * W, 3, generator=torch.Generator().manual_seed(4)) * 1.5
    out = _sent(B * 3 * H * W + 3)
    call("sgic_nhwc3_to_nchw_clamp", x.to(DEV), 3, B, H, W, out)
    assert _same_bits(out[:-3].view(B, 3, H, W), kr.nhwc3_to_nchw_clamp(x, B, H, W)) and bool(_is_sent(out[-3:]).all())
