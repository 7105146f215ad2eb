"""Last layer of both towers computes only the rows that are read (ops.attention window=..., encoder.rab_forward_last).
Both sides of every comparison run the same kernels on the same inputs, and a surviving query row stays in the 32-row block it is
in today, so every check is torch.equal on bit patterns -- no tolerance anywhere in this file."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (L, nseq, heads, q_tok0, Lq): 289 / 545 have the ragged query row and the VALU key tail, 50 a partial key tile (and drops
# row block 1), 96 a window that is the last of three full blocks
CASES = [(289, 2, 2, 256, 33), (545, 1, 2, 512, 33), (50, 3, 2, 0, 32), (96, 2, 1, 64, 32)]


@pytest.fixture(params=["f32", "split3"])
def precision(request):
    from sgic_amd import ops
    old = ops.PRECISION
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


def _window_rows(L, nseq, q_tok0, Lq):
    return (torch.arange(nseq, device=DEV)[:, None] * L + q_tok0 + torch.arange(Lq, device=DEV)[None, :]).reshape(-1)


def _check_window(L, nseq, heads, q_tok0, Lq, qkv, bias=None, biasvar=None):
    """every attn_mode 0..7 under both score arithmetics (+8), fp32 output and planes output, against ONE full launch each"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    D = heads * 64
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    rows = _window_rows(L, nseq, q_tok0, Lq)
    qw = q[rows].contiguous()
    old = ops.PRECISION
    ops.set_precision("split3")          # a planes output needs the split path to be the active one
    try:
        for prec in ("f32", "split3"):
            full = ops.attention(q, k, v, None, L, nseq, heads, bias=bias, biasvar=biasvar, mode=0, precision=prec)
            full_pl = ops.attention(q, k, v, None, L, nseq, heads, bias=bias, biasvar=biasvar, mode=0, precision=prec, to_gemm=True)
            assert isinstance(full_pl, ops.Planes)
            want, want_pl = full[rows], full_pl.rowmajor()[:, rows]
            assert torch.equal(want_pl, ops.split3(want.contiguous()))      # the two references agree with each other
            for mode in range(8):
                out = torch.full((nseq * Lq, D), float("nan"), device=DEV)
                ops.attention(qw, k, v, out, L, nseq, heads, bias=bias, biasvar=biasvar, mode=mode, precision=prec, window=(q_tok0, Lq))
                assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (L, mode, prec, "fp32 output")
                pl = ops.attention(qw, k, v, None, L, nseq, heads, bias=bias, biasvar=biasvar, mode=mode, precision=prec, to_gemm=True,
                                   window=(q_tok0, Lq))
                assert pl.shape == (nseq * Lq, D)
                assert torch.equal(pl.rowmajor(), want_pl), (L, mode, prec, "planes output")
    finally:
        ops.set_precision(old)


@pytest.mark.parametrize("L,nseq,heads,q_tok0,Lq", CASES)
def test_window_attention_equals_full_on_surviving_rows(L, nseq, heads, q_tok0, Lq):
    g = torch.Generator(device="cpu").manual_seed(100 + L)
    qkv = torch.randn(nseq * L, 3 * heads * 64, generator=g).to(DEV)
    _check_window(L, nseq, heads, q_tok0, Lq, qkv)


def test_window_attention_with_additive_bias():
    L, nseq, heads, q_tok0, Lq = 96, 2, 1, 64, 32
    g = torch.Generator(device="cpu").manual_seed(7)
    qkv = torch.randn(nseq * L, 3 * heads * 64, generator=g).to(DEV)
    bias = torch.randn(2, L, L, generator=g)
    bias[1, :, 5::7] = float("-inf")
    _check_window(L, nseq, heads, q_tok0, Lq, qkv, bias=bias.to(DEV).contiguous(), biasvar=torch.tensor([1, 0], dtype=torch.int32, device=DEV))


def test_window_attention_scores_far_apart():
    """q x 40: the scores of a row span hundreds of powers of two across tiles, so the deferred running maximum (AT_DEFER) is
    raised in some tiles and not in others -- the decision is per 32-row block, which the window keeps whole"""
    L, nseq, heads, q_tok0, Lq = 289, 2, 2, 256, 33
    g = torch.Generator(device="cpu").manual_seed(11)
    qkv = torch.randn(nseq * L, 3 * heads * 64, generator=g)
    qkv[:, :heads * 64] *= 40.0
    _check_window(L, nseq, heads, q_tok0, Lq, qkv.to(DEV))


def test_window_attention_rejects_rowmap_and_split_blocks():
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd._lib import SgicError
    L, nseq, heads = 96, 2, 1
    qkv = torch.randn(nseq * L, 192, device=DEV)
    q, k, v = qkv[:, :64], qkv[:, 64:128], qkv[:, 128:]
    out = torch.empty(nseq * 40, 64, device=DEV)
    rowmap = torch.arange(nseq * L, dtype=torch.int32, device=DEV)
    with pytest.raises(SgicError):
        ops.attention(q, k, v, out, L, nseq, heads, rowmap=rowmap, mode=1, window=(64, 32))
    with pytest.raises(SgicError):      # the window must start on a row block ...
        ops.attention(q, k, v, out, L, nseq, heads, mode=1, window=(48, 32))
    with pytest.raises(SgicError):      # ... and end on one (or at L)
        ops.attention(q, k, v, out, L, nseq, heads, mode=1, window=(32, 40))


def _rab_weights(D, seed):
    from sgic_amd.encoder import RabW
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    sd = {"b.ln_1.weight": 1 + r(D, scale=0.1), "b.ln_1.bias": r(D, scale=0.1),
          "b.attn.in_proj_weight": r(3 * D, D, scale=D ** -0.5), "b.attn.in_proj_bias": r(3 * D, scale=0.1),
          "b.attn.out_proj.weight": r(D, D, scale=D ** -0.5), "b.attn.out_proj.bias": r(D, scale=0.1),
          "b.ln_2.weight": 1 + r(D, scale=0.1), "b.ln_2.bias": r(D, scale=0.1),
          "b.mlp.c_fc.weight": r(4 * D, D, scale=D ** -0.5), "b.mlp.c_fc.bias": r(4 * D, scale=0.1),
          "b.mlp.c_proj.weight": r(D, 4 * D, scale=(4 * D) ** -0.5), "b.mlp.c_proj.bias": r(D, scale=0.1)}
    return RabW(sd, "b", torch.device(DEV)), g


@pytest.mark.parametrize("D,heads,L,nseq,tok0,Lq,keep", [(512, 8, 289, 2, 256, 33, None), (128, 2, 50, 3, 0, 32, None), (128, 2, 50, 3, 0, 32, 1)],
                         ids=["w512_L289", "w128_L50", "w128_L50_keep1"])
def test_rab_forward_last_equals_rab_forward(precision, D, heads, L, nseq, tok0, Lq, keep):
    import sgic_amd  # noqa
    from sgic_amd.encoder import rab_forward, rab_forward_last
    w, g = _rab_weights(D, 3 + D)
    X = torch.randn(nseq * L, D, generator=g).to(DEV)
    X[tok0 + 1, 3] = -0.0                      # the residual rows are copied, not recomputed
    X0 = X.clone()
    Xq = rab_forward_last(X, w, L, nseq, heads, tok0, Lq, keep=keep)
    assert torch.equal(X.view(torch.int32), X0.view(torch.int32)), "rab_forward_last must leave X untouched"
    full = rab_forward(X0.clone(), w, L, nseq, heads)
    want = full[_window_rows(L, nseq, tok0, keep or Lq)]
    assert Xq.shape == want.shape
    assert torch.equal(Xq.view(torch.int32), want.view(torch.int32))


def test_small_encoder_prune_last_bit_equal(precision):
    import sgic_amd  # noqa
    from sgic_amd import weights as W
    from sgic_amd.config import SMALL
    from sgic_amd.data import synth_images
    from sgic_amd.encoder import HybridEncoderHIP
    sd = W.synth_weights(W.encoder_spec(SMALL) + W.codec_misc_spec(SMALL) + W.bottleneck_spec(SMALL), seed=1234)
    enc = HybridEncoderHIP(sd, SMALL, torch.device(DEV))
    assert enc.prune_last
    x = synth_images(2, 256, 256, 21).cuda()
    z1, h1, s1 = enc.forward(x)
    enc.prune_last = False
    z0, h0, s0 = enc.forward(x)
    assert s0 == s1 and z0.shape == z1.shape and h0.shape == h1.shape
    assert torch.equal(z1.view(torch.int32), z0.view(torch.int32))
    assert torch.equal(h1.view(torch.int32), h0.view(torch.int32))


def test_clip_tiny_tower_prune_last_bit_equal(precision):
    import sgic_amd  # noqa
    from sgic_amd import weights as W
    from sgic_amd.codec import ClipCodec
    from sgic_amd.config import CLIP_TINY
    codec = ClipCodec(W.synth_weights(W.clip_spec(CLIP_TINY), seed=5), CLIP_TINY, DEV)
    assert codec.model.prune_last
    g = torch.Generator(device="cpu").manual_seed(9)
    pre = torch.randn(3, 3, CLIP_TINY.image_size, CLIP_TINY.image_size, generator=g).to(DEV)
    unit1, code1 = codec.model.tower(pre)
    codec.model.prune_last = False
    unit0, code0 = codec.model.tower(pre)
    assert torch.equal(unit1.view(torch.int32), unit0.view(torch.int32))
    assert torch.equal(code1, code0)
