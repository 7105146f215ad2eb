"""GPU unit tests of row-mapped attention (csrc/attn.hip, the d_rowmap argument): every Swin layer runs through it, and the only
other coverage is one whole-block golden at L = 256 with a row space of exactly nseq * L.  Here the row map is a random
permutation into a LARGER row space, combined with every sequence-length class of the kernel (full tiles, the ragged VALU rows of
L % 32 in {1, 2}, workgroups that span two units, masked tails, L = 1), every launch mode and both score arithmetics, and a
4-variant additive bias with -inf bands (blocks/swin_transformer.py:42-55,115-117).  Three references:
  * fp64 softmax(scale q k^T + bias[var[s]]) v on the gathered rows, within the 2e-5 of test_attention_vs_torch;
  * ONE dense launch (no row map, same mode and arithmetic) on the physically gathered q / k / v: the row map only changes
    addresses, so the mapped rows must carry the same bits;
  * a sentinel in every row outside the map, in the columns beyond D and in the row behind the row space."""
import pytest
import torch

import kernels_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BITS = 0x7FA5C3D2                      # a NaN pattern no kernel here produces
PLANE_PAT = 0x7FB7                          # a bf16 NaN: no piece of a split finite value
EXTRA = 37                                  # rows of the row space that no (sequence, token) maps to

# (L, nseq, heads, bias, scale)
CASES = [(256, 3, 2, True, 0.125),          # the production window
         (64, 5, 1, True, 0.125),
         (64, 5, 1, True, 0.2),             # a scale that is not a power of two
         (96, 4, 3, True, 0.125),
         (289, 2, 2, False, 0.125),         # ragged VALU rows; workgroups spanning two units
         (545, 1, 1, False, 0.125),
         (65, 3, 3, False, 0.125),
         (33, 2, 1, False, 0.125),
         (50, 3, 2, False, 0.125),          # masked tail
         (1, 2, 2, False, 0.125)]
PLANES_CASES = [(256, 3, 2, True, 0.125), (289, 2, 2, False, 0.125)]


def _sent(*shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sent(t):
    return t.contiguous().view(torch.int32) == SENT_BITS


def _same_bits(got, ref):
    return torch.equal(kr.bits(got), kr.bits(ref))


def _setup(L, nseq, heads, bias, scale):
    """-> dict: qkv (R, 3D), rowmap, bias (4, L, L) / biasvar or None, the fp64 reference on the gathered rows (nseq * L, D)"""
    g = torch.Generator().manual_seed(L * 131 + nseq * 17 + heads)
    D, R = heads * 64, nseq * L + EXTRA
    qkv = torch.randn(R, 3 * D, generator=g)
    rowmap = torch.randperm(R, generator=g)[:nseq * L].to(torch.int32)
    b = var = None
    if bias:
        b = kr.attn_bias_variants(L, g)
        var = ((torch.arange(nseq) + 1) % 4).to(torch.int32)          # 1, 2, 3, 0, ...: the corner-window variants first
    ref = kr.attention64(qkv[rowmap.long()], L, nseq, heads, b, var, scale)
    return {"D": D, "R": R, "qkv": qkv.to(DEV), "rowmap": rowmap.to(DEV), "bias": b.to(DEV) if bias else None,
            "var": var.to(DEV) if bias else None, "ref": ref.to(DEV)}


@pytest.mark.parametrize("L,nseq,heads,bias,scale", CASES)
def test_rowmap_vs_fp64_and_dense_launch(L, nseq, heads, bias, scale):
    import sgic_amd  # noqa
    from sgic_amd import ops
    s = _setup(L, nseq, heads, bias, scale)
    D, R, qkv, rowmap = s["D"], s["R"], s["qkv"], s["rowmap"]
    rows = rowmap.long()
    gathered = qkv[rows].contiguous()                                  # (nseq * L, 3D): what the row map addresses, made dense
    written = torch.zeros(R + 1, D + 4, dtype=torch.bool, device=DEV)
    written[rows, :D] = True
    kw = dict(bias=s["bias"], biasvar=s["var"], scale=scale)
    for precision in ("f32", "split3"):
        first, worst = None, 0.0
        for mode in (0,) + ops.ATTN_MODES:
            out = _sent(R + 1, D + 4)
            ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out[:, :D], L, nseq, heads, rowmap=rowmap, mode=mode,
                          precision=precision, **kw)
            dense = _sent(nseq * L, D)
            ops.attention(gathered[:, :D], gathered[:, D:2 * D], gathered[:, 2 * D:], dense, L, nseq, heads, mode=mode,
                          precision=precision, **kw)
            got = out[rows, :D]
            err = float((got.double() - s["ref"]).abs().max())
            worst = max(worst, err)
            assert err < 2e-5, (L, mode, precision, err)
            assert _same_bits(got, dense), ("row-mapped launch != dense launch on the gathered rows", L, mode, precision)
            first = got if first is None else first
            assert _same_bits(got, first), ("modes differ", L, mode, precision)
            assert bool(_is_sent(out)[~written].all()), ("a write outside the mapped rows / the D columns", L, mode, precision)
        print(f"[attn-rowmap] L={L} nseq={nseq} heads={heads} bias={int(bias)} scale={scale} {precision}: worst |err| vs fp64 {worst:.3e}")


@pytest.mark.parametrize("L,nseq,heads,bias,scale", PLANES_CASES)
def test_rowmap_planes_output(L, nseq, heads, bias, scale):
    """the out-projection's operand written as bf16x3 planes over a row space LARGER than nseq * L: mapped rows == the split of the
    fp32 result, every other row of all three planes untouched"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    s = _setup(L, nseq, heads, bias, scale)
    D, R, qkv, rowmap = s["D"], s["R"], s["qkv"], s["rowmap"]
    rows = rowmap.long()
    unmapped = torch.ones(R, dtype=torch.bool, device=DEV)
    unmapped[rows] = False
    kw = dict(rowmap=rowmap, bias=s["bias"], biasvar=s["var"], scale=scale)
    old = ops.PRECISION
    ops.set_precision("split3")
    try:
        for mode in (0,) + ops.ATTN_MODES:
            out = _sent(R + 1, D + 4)
            ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out[:, :D], L, nseq, heads, mode=mode, **kw)
            pl = ops.Planes(R, D, DEV)
            pl.t.fill_(PLANE_PAT)
            got = ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], pl, L, nseq, heads, mode=mode, to_gemm=True, **kw)
            assert got is pl
            p = pl.rowmajor()
            assert torch.equal(p[:, rows], ops.split3(out[rows, :D].contiguous())), (L, mode)
            assert bool((p[:, unmapped] == PLANE_PAT).all()), ("a write into an unmapped row of the planes", L, mode)
    finally:
        ops.set_precision(old)
