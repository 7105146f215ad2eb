"""GPU parity of the HIP transform path (through the C ABI) against
  (1) golden outputs of the REAL reference modules (tests/golden/nn_small_*.npz, made by
      oracle/gen_golden_nn.py in the build container), and
  (2) the torch-CPU fp32 restatement oracle/torch_ref.py on the same seeded inputs/weights.
Floating point: tolerance 2e-5 * max|ref| (measured 1e-6 ... 3e-6 with both GEMM arithmetics: fp32 accumulation-order noise);
integer outputs (VQ indices, symbols, indexes): mismatch RATE bounds, and the rANS bytes are bit-exact
for whatever (symbols, indexes) the GPU produced."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import orc
from oracle import torch_ref as TR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_pillow_ref import pillow_from_f32  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-5


@pytest.fixture(scope="module")
def small():
    import sgic_amd  # noqa
    from sgic_amd import weights as W
    from sgic_amd.config import SMALL
    spec = W.encoder_spec(SMALL) + W.codec_misc_spec(SMALL) + W.bottleneck_spec(SMALL)
    sd = W.synth_weights(spec, seed=1234)
    return SMALL, sd


@pytest.fixture(scope="module")
def enc(small):
    from sgic_amd.encoder import HybridEncoderHIP
    cfg, sd = small
    return HybridEncoderHIP(sd, cfg, torch.device("cuda:0"))


@pytest.fixture(scope="module")
def bott(small):
    from sgic_amd.bottleneck import BottleneckHIP
    cfg, sd = small
    b = BottleneckHIP(sd, cfg, torch.device("cuda:0"))
    b.update(force=True)
    return b


def _relerr(a, b):
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def _z_to_ref_layout(z, N, T, C):  # [(n,t), c] -> (N, C, 1, T)
    return z.reshape(N, T, C).permute(0, 2, 1).reshape(N, C, 1, T)


def _h_to_ref_layout(h, B, hh, ww):  # [(b,y,x), F] -> (B, F, hh, ww)
    return h.reshape(B, hh, ww, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_encoder_vs_reference_golden(case, small, enc, golden_dir):
    from sgic_amd.data import synth_images
    cfg, sd = small
    g = np.load(os.path.join(golden_dir, f"nn_small_{case}.npz"))
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    x = synth_images(B, H, W, int(g["seed"])).cuda()
    z, h, stack = enc.forward(x)
    N = g["z"].shape[0]
    z_ref, h_ref = torch.from_numpy(g["z"]), torch.from_numpy(g["h"])
    zz = _z_to_ref_layout(z.cpu(), N, cfg.num_latent_tokens, cfg.token_size)
    hh = _h_to_ref_layout(h.cpu(), B, H // 32, W // 32)
    ez, eh = _relerr(zz, z_ref), _relerr(hh, h_ref)
    print(f"case {case}: rel err z {ez:.2e}  h {eh:.2e}")
    assert ez < TOL and eh < TOL
    # VQ indices (argmin over 4096 codes; near-ties may flip): <= 1 % mismatches
    from sgic_amd import ops
    vq = ops.vq_argmin(z, sd["hybrid_codec.quantize.embedding.weight"].cuda().contiguous(), True).cpu().numpy()
    mism = int((vq != g["vq_idx"]).sum())
    print(f"   vq index mismatches {mism} of {vq.size}")
    assert mism <= 1                                   # measured 0; one nearest-code tie of headroom


def test_encoder_intermediate_taps_vs_torch_ref(small, enc):
    """localises a failure: patch-embed/token assembly/ln_pre, feat_in Swin stack, first ViT layer"""
    from sgic_amd.data import synth_images
    cfg, sd = small
    x = synth_images(1, 256, 512, 3)
    taps_ref, taps = {}, {}
    TR.encoder_forward(x * 0.5 + 0.5, sd, cfg, taps=taps_ref)
    enc.forward(x.cuda(), taps=taps)
    N = 2
    e1 = _relerr(taps["x_ln_pre"].cpu().reshape(N, -1, cfg.width), taps_ref["x_ln_pre"])
    # feature map: TM16 rows (n, p) -> (B, F, H, W) with tiles side by side along W
    f = taps["feat_in"].cpu().reshape(1, 1, 2, 16, 16, cfg.feat_dim).permute(0, 5, 1, 3, 2, 4).reshape(1, cfg.feat_dim, 16, 32)
    e2 = _relerr(f, taps_ref["feat_in"])
    e3 = _relerr(taps["x_layer0"].cpu().reshape(N, -1, cfg.width), taps_ref["x_layer0"])
    print(f"taps rel err: ln_pre {e1:.2e} feat_in {e2:.2e} layer0 {e3:.2e}")
    assert e1 < 1e-5 and e2 < TOL and e3 < TOL


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_bottleneck_vs_reference_golden(case, small, bott, golden_dir):
    cfg, sd = small
    g = np.load(os.path.join(golden_dir, f"nn_small_{case}.npz"))
    B, hh, ww = g["h"].shape[0], g["h"].shape[2], g["h"].shape[3]
    h = torch.from_numpy(g["h"]).permute(0, 2, 3, 1).reshape(B * hh * ww, -1).contiguous().cuda()
    y = bott.analysis(h, B, hh, ww)
    y_ref = torch.from_numpy(g["y"])
    ey = _relerr(y.cpu().reshape(B, hh, ww, -1).permute(0, 3, 1, 2), y_ref)
    print(f"case {case}: analysis rel err {ey:.2e}")
    assert ey < TOL
    # 4-step quantiser on the REFERENCE y: symbols / indexes vs the reference's
    yr = y_ref.permute(0, 2, 3, 1).reshape(B * hh * ww, -1).contiguous().cuda()
    sym, idx, _, _ = bott.quantise(yr, B, hh, ww)
    s_m = float((sym.cpu().numpy() != g["sym"]).mean())
    i_m = float((idx.cpu().numpy() != g["idx"]).mean())
    print(f"   4-step mismatch rate: symbols {s_m:.5f} indexes {i_m:.5f}")
    assert s_m == 0.0 and i_m <= 2e-4                  # measured: 0 symbols, at most 1 index in 16 384 (a sigma on a bin edge)
    # the coder itself is bit-exact for the (symbols, indexes) the GPU produced ...
    from sgic_amd import ops
    n = sym[0].numel()
    out, meta = ops.rans_encode_batch(bott.tables.handles[bott.group], sym, idx, B, n)
    streams = bott.streams_to_host(out, meta)
    tab = orc.Table(*bott.cdf_info)
    for b in range(B):
        assert streams[b] == orc.rans_encode(sym[b].cpu().numpy(), idx[b].cpu().numpy(), tab)
        # ... and equals the reference's h_bit_stream whenever the symbols agree
        if np.array_equal(sym[b].cpu().numpy(), g["sym"][b]) and np.array_equal(idx[b].cpu().numpy(), g["idx"][b]):
            assert streams[b] == g[f"stream_{b}"].tobytes()
            print(f"   image {b}: h_bit_stream byte-identical to the reference ({len(streams[b])} B)")


def test_cdf_table_built_by_product_matches_reference(bott, golden_dir):
    t = np.load(os.path.join(golden_dir, "cdf_table.npz"))
    cdf, ln, off = bott.cdf_info
    assert np.array_equal(cdf, t["cdf"]) and np.array_equal(ln, t["cdf_length"]) and np.array_equal(off, t["offset"])


def test_batch_invariance(small, enc):
    """B=3 batch == three B=1 calls, bitwise (fixed reduction order)"""
    from sgic_amd.data import synth_images
    x = synth_images(3, 256, 256, 21).cuda()
    z, h, _ = enc.forward(x)
    for b in range(3):
        zb, hb, _ = enc.forward(x[b:b + 1].contiguous())
        assert torch.equal(zb, z[b * 32:(b + 1) * 32]) and torch.equal(hb, h[b * 64:(b + 1) * 64])


def test_clip_preprocess_bit_exact_vs_pillow():
    import sgic_amd  # noqa
    from sgic_amd import weights as W
    from sgic_amd.clip import ClipHIP
    from sgic_amd.config import CLIP_TINY
    from sgic_amd.data import synth_images
    sd = W.synth_weights(W.clip_spec(CLIP_TINY), seed=5)
    clip = ClipHIP(sd, CLIP_TINY, torch.device("cuda:0"))
    mean, std = np.float32(CLIP_TINY.mean), np.float32(CLIP_TINY.std)
    for (H, W_) in [(256, 256), (300, 256), (256, 437), (512, 512)]:
        x = synth_images(2, H, W_, 31 + H + W_)
        got = clip.preprocess(x.cuda()).cpu().numpy()
        for b in range(2):
            assert np.array_equal(got[b], pillow_from_f32(x[b], 224, mean, std)), (H, W_, b)
    # what compress.py hands over: the batch padded to multiples of 256, H x W the real image.  The padding is not read
    H, W_ = 300, 437
    img = synth_images(2, H, W_, 31 + H + W_)
    outs = []
    for fill in (-1.0, 0.25):
        x = torch.full((2, 3, 512, 512), fill)
        x[:, :, :H, :W_] = img
        outs.append(clip.preprocess(x.cuda(), H, W_).cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    for b in range(2):
        assert np.array_equal(outs[0][b], pillow_from_f32(img[b], 224, mean, std)), b


def test_clip_tower_vs_torch_ref():
    import sgic_amd  # noqa
    from sgic_amd import weights as W
    from sgic_amd.clip import ClipHIP
    from sgic_amd.config import CLIP_TINY
    sd = W.synth_weights(W.clip_spec(CLIP_TINY), seed=5)
    clip = ClipHIP(sd, CLIP_TINY, torch.device("cuda:0"))
    torch.manual_seed(0)
    pre = torch.randn(3, 3, 224, 224)
    unit, q = clip.tower(pre.cuda())
    ref = TR.clip_tower(pre, sd, CLIP_TINY)
    cos = torch.nn.functional.cosine_similarity(unit.cpu(), ref, dim=-1)
    print("clip cosine", cos.tolist(), "max abs err", float((unit.cpu() - ref).abs().max()))
    assert float(cos.min()) > 0.99999 and float((unit.cpu() - ref).abs().max()) < 1e-4
    qref = np.clip(np.round((ref.numpy() * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
    assert float((q.cpu().numpy() != qref).mean()) <= 0.01


def _clip_tokens(cfg, lens, seed):
    """open_clip layout: <start> words... <end>, zero padded; <end> = vocab-1 is the largest id"""
    rng = np.random.default_rng(seed)
    toks = np.zeros((len(lens), cfg.ctx), dtype=np.int64)
    for b, n in enumerate(lens):
        toks[b, 0] = cfg.vocab - 2
        toks[b, 1:1 + n] = rng.integers(1, cfg.vocab - 2, n)
        toks[b, 1 + n] = cfg.vocab - 1
    return toks


@pytest.mark.parametrize("name", ["tiny", "b32"])
def test_clip_text_tower_vs_torch_ref(name):
    """CLIP text tower (search.py:93-97 -> open_clip encode_text): HIP vs the torch oracle, which
    tests/test_oracle_clip_hf.py pins against HuggingFace's CLIP.  Tolerance: cosine > 0.99999, max abs 1e-4 on unit vectors."""
    import sgic_amd  # noqa
    from sgic_amd import weights as W
    from sgic_amd.clip import ClipTextHIP
    from sgic_amd.config import CLIP_B32, CLIP_TINY
    cfg = CLIP_TINY if name == "tiny" else CLIP_B32
    sd = W.synth_weights(W.clip_text_spec(cfg), seed=6)
    model = ClipTextHIP(sd, cfg, torch.device("cuda:0"))
    toks = _clip_tokens(cfg, (1, 5, cfg.ctx - 2, 9, 0), 3)
    unit = model.encode_text(toks).cpu()
    with torch.no_grad():
        ref = TR.clip_text_tower(toks, sd, cfg)
    cos = torch.nn.functional.cosine_similarity(unit, ref, dim=-1)
    print("clip text cosine", cos.tolist(), "max abs err", float((unit - ref).abs().max()))
    assert float(cos.min()) > 0.99999 and float((unit - ref).abs().max()) < 1e-4
    # the padding after <end> must not matter (causal mask): same prompt, garbage after EOT -> same vector
    t2 = toks.copy()
    t2[1, 8:] = 7
    assert torch.equal(model.encode_text(t2).cpu()[1], unit[1])
    with pytest.raises(ValueError):
        model.encode_text(toks[:, :-1])


def test_profile_window_times_every_gemm_launch():
    """sgic_profiler_begin/end (bench.py's roofline figure): one duration per GEMM / conv launch, in launch order.  Results and
    bookkeeping only; the latency figure of the small launch is asserted in test_single_tile_latency_f32 (marked perf)."""
    import sgic_amd  # noqa
    from sgic_amd import ops
    a = torch.randn(2048, 512, device="cuda:0")
    w = torch.randn(1024, 512, device="cuda:0")
    ref = ops.gemm(a, w, precision="f32")
    ops.gemm(a[:64], w[:64], precision="f32")
    ops.profile_begin(16)
    outs = [ops.gemm(a, w, precision="f32") for _ in range(3)]
    small = ops.gemm(a[:64], w[:64], precision="f32")
    recs = ops.profile_end()
    assert ops.PROFILE is None and len(recs) == 4
    assert all(ms > 0.0 for _, ms, _ in recs) and recs[0][0] == 2.0 * 2048 * 1024 * 512 and recs[3][2][:3] == (64, 64, 512)
    assert all(torch.equal(o, ref) for o in outs) and torch.equal(small, ref[:64, :64])
    with pytest.raises(Exception):
        ops.profile_end()                                 # no open window


@pytest.mark.perf
def test_single_tile_latency_f32():
    """latency of a single-tile GEMM with the exact-fp32 kernels (the B = 1 building block of encode_only under SGIC_GEMM=f32): one
    64x64 tile, K = 512, by dispatch timestamps.  Timing, not parity (collected last); bound = the in-situ figure with 2x headroom,
    see tests/test_gpu_split3.py::test_single_tile_latency for what a lone dispatch's timestamps contain."""
    import sgic_amd  # noqa
    from sgic_amd import ops
    a = torch.randn(64, 512, device="cuda:0")
    w = torch.randn(64, 512, device="cuda:0")
    for _ in range(10):
        ops.gemm(a, w, precision="f32")
    torch.cuda.synchronize()
    ops.profile_begin(16)
    for _ in range(8):
        ops.gemm(a, w, precision="f32")
    recs = ops.profile_end()
    best = min(ms for _, ms, _ in recs)
    print(f"[latency] 64x64x512 fp32 GEMM, dispatch timestamps: best {best * 1e3:.1f} us, all {[round(ms * 1e3, 1) for _, ms, _ in recs]}")
    assert all(ms < 1.0 for _, ms, _ in recs)             # kernel durations (microseconds), not wall-clock junk
    assert len(recs) == 8 and best < 0.024, f"64x64x512 GEMM took {best * 1e3:.1f} us"


def test_gemm_fuzz_all_tile_modes_identical_and_close_to_fp64():
    """sgic_gemm_f32 over random shapes (ragged M/N, K with and without a 32-tail, bias / residual / activation /
    row maps): all 15 launch modes give BITWISE the same result (fixed k order; persistent, mixed, 64x64 launches and the
    16x16x4-MFMA latency kernel included) and that result is within 3e-6 * sqrt(K) * max|ref| of an fp64 reference."""
    import sgic_amd  # noqa
    from sgic_amd import ops
    rng = np.random.default_rng(11)
    dev = torch.device("cuda:0")
    old = ops.AUTOTUNE
    ops.AUTOTUNE = False
    try:
        shapes = [(9248, 1024, 256), (289, 3072, 1024), (1600, 768, 96), (70000, 128, 128), (5000, 200, 64), (129, 132, 36),
                  (9248, 4096, 128), (17440, 3072, 96), (20000, 1156, 64), (12345, 2052, 160)]   # several rounds of the 512 resident workgroups
        shapes += [(int(rng.integers(1, 3000)), int(rng.integers(1, 600)) * 4, int(rng.integers(1, 80)) * 4) for _ in range(10)]
        for (M, N, K) in shapes:
            a = torch.from_numpy(rng.standard_normal((M, K), dtype=np.float32)).to(dev)
            w = torch.from_numpy(rng.standard_normal((N, K), dtype=np.float32)).to(dev)
            b = torch.from_numpy(rng.standard_normal(N, dtype=np.float32)).to(dev)
            res = torch.from_numpy(rng.standard_normal((M, N), dtype=np.float32)).to(dev) if rng.random() < 0.5 else None
            act = int(rng.integers(0, 5))
            outs = []
            for mode in ops.TUNE_MODES:
                outs.append(ops.gemm(a, w, b, residual=res, act=act, tile=mode, precision="f32"))
            outs.append(ops.gemm(a, w, b, residual=res, act=act, tile=0, precision="f32"))     # built-in heuristic
            assert all(torch.equal(o, outs[0]) for o in outs[1:]), (M, N, K, act)
            pre = a.double() @ w.double().T + b.double()
            f = {0: lambda v: v, 1: lambda v: torch.nn.functional.gelu(v), 2: lambda v: torch.nn.functional.silu(v), 3: torch.tanh,
                 4: lambda v: torch.nn.functional.leaky_relu(v, 0.01)}[act]
            ref = f(pre) + (res.double() if res is not None else 0.0)
            err = float((outs[0].double() - ref).abs().max())
            assert err < 3e-6 * (K ** 0.5) * max(1.0, float(pre.abs().max())), (M, N, K, act, err)
        # row maps: write C into a token slice of a larger buffer, read A through a segment map (cross blocks)
        n, L, Lr, D = 7, 40, 25, 64
        buf = torch.zeros(n * L, D, device=dev)
        a = torch.from_numpy(rng.standard_normal((n * L, 32), dtype=np.float32)).to(dev)
        w = torch.from_numpy(rng.standard_normal((D, 32), dtype=np.float32)).to(dev)
        for mode in (0, 1, 4, 11, 12, 13, 15):
            buf.zero_()
            ops.gemm(a, w, out=buf, M=n * Lr, a_seg=(Lr, L), c_seg=(Lr, L), tile=mode, precision="f32")
            ref = (a.view(n, L, 32)[:, :Lr].double() @ w.double().T).float()
            got = buf.view(n, L, D)
            assert float((got[:, :Lr] - ref).abs().max()) < 1e-4 and float(got[:, Lr:].abs().max()) == 0.0, mode
    finally:
        ops.AUTOTUNE = old


@pytest.mark.parametrize("L,nseq,heads,bias", [(289, 3, 4, False), (545, 2, 3, False), (256, 4, 2, True), (50, 5, 12, False),
                                                 (33, 2, 1, False), (34, 2, 2, False), (2, 3, 1, False), (1, 2, 2, False), (100, 2, 2, True),
                                                 (65, 3, 3, False), (129, 2, 5, False), (80, 3, 8, True), (77, 3, 8, False), (290, 1, 7, False), (545, 1, 1, False),
                                                 (64, 5, 3, False), (96, 7, 1, True)])
def test_attention_vs_torch(L, nseq, heads, bias):
    """sgic_attention_f32 vs softmax(q k^T / 8 + bias) v in fp64 for every sequence-length class of the path: full
    tiles, the 1-2 key ragged tail folded in on the VALU (L % 32 in {1, 2}), masked tails (other L), additive bias with
    -inf entries, ragged query rows on the VALU workgroups (L % 32 in {1, 2}, L >= 64), workgroups that span two
    units, and every attn_mode (single / double-buffered K/V ring, start-up stagger).  Tolerance 2e-5 absolute on O(1)
    outputs; all modes bitwise equal."""
    import sgic_amd  # noqa
    from sgic_amd import ops
    g = torch.Generator().manual_seed(L * 7 + heads)
    D = heads * 64
    qkv = torch.randn(nseq * L, 3 * D, generator=g)
    b = None
    if bias:
        b = torch.randn(2, L, L, generator=g)
        b[1, :, L // 3: L // 2] = float("-inf")            # a masked band (Swin shift masks contain -inf)
    var = torch.arange(nseq, dtype=torch.int32) % 2
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(nseq, L, heads, 64).permute(0, 2, 1, 3).double() for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125
    if bias:
        s = s + b[var.long()].double()[:, None]
    ref = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(nseq * L, D)
    d = qkv.cuda()
    old = ops.AUTOTUNE
    ops.AUTOTUNE = False
    try:
        for precision in ("f32", "split3"):      # fp32-MFMA scores / bf16x3 split scores (attn_mode bit 3): each bitwise stable over its modes
            first = None
            for mode in (0,) + ops.ATTN_MODES:
                out = torch.full((nseq * L, D), float("nan"), device="cuda:0")
                ops.attention(d[:, :D], d[:, D:2 * D], d[:, 2 * D:], out, L, nseq, heads, bias=b.cuda() if bias else None,
                              biasvar=var.cuda() if bias else None, mode=mode, precision=precision)
                err = float((out.cpu().double() - ref).abs().max())
                assert err < 2e-5, (L, mode, precision, err)
                first = out if first is None else first
                assert torch.equal(out, first), (L, mode, precision)
    finally:
        ops.AUTOTUNE = old
