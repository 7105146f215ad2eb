"""No GPU: the evidence that tests/test_gpu_split3_accuracy.py (and the GEMM's test_error_not_above_fp32_path) would fail for a subtly
wrong kernel.  On every input those tests use, the CPU restatement of the split arithmetic (tests/split3_ref.py) is compared with a
strict fp32 multiply-add chain, both against fp64:

    ratio = rms(err of X) / rms(err of the fp32 chain)

  * the six-term product has ratio <= BOUND (1.10, the GEMM test's own bound);
  * every five-term mutant -- one third-order term (p3 q1, p1 q3, p2 q2) left out -- has ratio >= 3 BOUND on the randn family of
    every case, for the GEMM, the 3x3 convolution, and attention's score product and P.V product each on its own;
  * attention's two variants restated as they round -- the f32 variant is no strict chain but an fp32 MFMA with two half-length
    accumulators, the S3 variant works in the log2 domain and keeps the leading term of a score in a chain of its own -- stand to
    each other at 0.42 - 0.87 (the GPU test prints 0.58 - 0.82), under BOUND.  With all six terms of a score in ONE chain, as the kernel had
    them before these tests, the same restatement gives 1.16 - 1.21 on the sharp family, where the GPU measured 1.17 - 1.28.

The sharp and ascending attention families are there for the clean kernel's behaviour (a few dominant keys; the deferred rescale):
their score error dominates the output, so a P.V mutant can hide there, and nothing is asserted of mutants on them.  The ratios are
printed (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import kernels_ref as kr
import split3_ref as sr

NEED = 3 * sr.BOUND
VARIANTS, ONE_CHAIN = "[S3 variant / fp32-MFMA variant]", "[the same with one score chain]"


def test_split3_pieces_are_bf16_and_exact():
    """the pieces are what torch's round-to-nearest-even bf16 conversion gives, and their sum is the value"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(257, 64, generator=g) * torch.exp(4 * torch.randn(257, 1, generator=g))
    x[0, :6] = torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0, 1e30])
    x[1, :4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0 + 2.0 ** -7])     # ties of the first piece: to even
    p1, p2, p3 = sr.split3(x.numpy())
    t1 = x.bfloat16().float()
    t2 = (x - t1).bfloat16().float()
    t3 = ((x - t1) - t2).bfloat16().float()
    assert np.array_equal(p1, t1.numpy()) and np.array_equal(p2, t2.numpy()) and np.array_equal(p3, t3.numpy())
    assert np.array_equal(p1.astype(np.float64) + p2 + p3, x.double().numpy())


def test_all_nine_piece_products_give_the_exact_product():
    """mm_split's own sanity: with every product of pieces present (nine terms) in one block, only the nine roundings into the fp32
    accumulator separate the result from fp64: at most 9 half-ulps of the largest partial sum"""
    a, w = (t.numpy() for t in sr.gemm_inputs(70, 52, 96, "randn"))
    nine = tuple((i, j) for i in range(3) for j in range(3))
    got = sr.mm_split(a, w.T, terms=nine, kblock=96)
    assert np.all(np.abs(got - sr.mm64(a, w.T)) <= 9 * 2.0 ** -24 * sr.mm64(np.abs(a), np.abs(w.T)))


def _report(tag, clean, mutants):
    print(f"[split3 cpu] {tag}: six terms {clean:.3f}   " + "   ".join(f"{n} {r:.2f}" for n, r in mutants.items()))


@functools.lru_cache(maxsize=None)
def _gemm(case):
    M, N, K, family = sr.GEMM_CASES[case]
    a, w = (t.numpy()[:96] for t in sr.gemm_inputs(M, N, K, family))          # the large case: a 96 x 96 corner of the product, full K
    ref, chain = sr.mm64(a, w.T), sr.mm_chain(a, w.T)
    clean = sr.ratio(sr.mm_split(a, w.T, kblock=sr.GEMM_K), chain, ref)
    mutants = {n: sr.ratio(sr.mm_split(a, w.T, terms=t, kblock=sr.GEMM_K), chain, ref) for n, t in sr.MUTANTS.items()}
    return clean, mutants


@pytest.mark.parametrize("case", range(len(sr.GEMM_CASES)))
def test_gemm_ratio(case):
    M, N, K, family = sr.GEMM_CASES[case]
    clean, mutants = _gemm(case)
    _report(f"gemm ({M},{N},{K}) {family}", clean, mutants)
    assert clean <= sr.BOUND
    if family == "randn":
        assert min(mutants.values()) >= NEED, mutants


@functools.lru_cache(maxsize=None)
def _conv(case, family):
    x, w, bias, _ = sr.conv_inputs(case, family)
    ref = kr.conv3x3_64(x, w, bias, None, 0)[0].numpy()
    chain = sr.conv3x3(x, w, bias, sr.mm_chain)
    clean = sr.ratio(sr.conv3x3(x, w, bias, functools.partial(sr.mm_split, kblock=sr.GEMM_K)), chain, ref)
    mutants = {n: sr.ratio(sr.conv3x3(x, w, bias, functools.partial(sr.mm_split, terms=t, kblock=sr.GEMM_K)), chain, ref)
               for n, t in sr.MUTANTS.items()}
    return clean, mutants


@pytest.mark.parametrize("family", sr.FAMILIES_CONV)
@pytest.mark.parametrize("case", range(len(sr.CONV_ACC_CASES)))
def test_conv3x3_ratio(case, family):
    clean, mutants = _conv(case, family)
    _report(f"conv3x3 {sr.CONV_ACC_CASES[case]} {family}", clean, mutants)
    assert clean <= sr.BOUND
    if family == "randn":
        assert min(mutants.values()) >= NEED, mutants


@functools.lru_cache(maxsize=None)
def _attn(case, family):
    L, _ = sr.ATTN_CASES[case]
    qkv, bias, var = sr.attn_inputs(case, family)
    q, k, v, b = sr.attn_units(qkv, L, bias, var)
    ref = kr.attention64(qkv, L, sr.ATTN_NSEQ, sr.ATTN_HEADS, bias, var, 0.125).numpy()
    run = lambda mm_s, mm_pv: sr.attn_rows(sr.attention(q, k, v, mm_s, mm_pv, bias=b), L)  # noqa: E731
    chain = run(sr.mm_chain, sr.mm_chain)
    clean = sr.ratio(run(sr.mm_scores_s3, sr.mm_split), chain, ref)
    # the two variants of csrc/attn.hip as they round: the S3 variant against the fp32-MFMA variant, and what it was with one chain
    f32 = sr.attn_rows(sr.attention(q, k, v, sr.scores_mfma_f32, sr.pv_mfma_f32, bias=b, softmax="f32"), L)
    s3 = sr.attn_rows(sr.attention(q, k, v, sr.mm_scores_s3, sr.mm_split, bias=b, softmax="s3"), L)
    one = sr.attn_rows(sr.attention(q, k, v, sr.mm_split, sr.mm_split, bias=b, softmax="s3"), L)
    mutants = {VARIANTS: sr.ratio(s3, f32, ref), ONE_CHAIN: sr.ratio(one, f32, ref)}
    for n, t in sr.MUTANTS.items():
        mutants["scores " + n] = sr.ratio(run(functools.partial(sr.mm_scores_s3, terms=t), sr.mm_split), chain, ref)
        mutants["pv " + n] = sr.ratio(run(sr.mm_scores_s3, functools.partial(sr.mm_split, terms=t)), chain, ref)
    return clean, mutants


@pytest.mark.parametrize("family", sr.FAMILIES_ATTN)
@pytest.mark.parametrize("case", range(len(sr.ATTN_CASES)))
def test_attention_ratio(case, family):
    L, with_bias = sr.ATTN_CASES[case]
    clean, mutants = _attn(case, family)
    _report(f"attention L={L} bias={int(with_bias)} {family}", clean, mutants)
    assert clean <= sr.BOUND
    mutants = dict(mutants)
    assert mutants.pop(VARIANTS) <= sr.BOUND
    mutants.pop(ONE_CHAIN)
    if family == "randn":
        assert min(mutants.values()) >= NEED, mutants


@pytest.mark.parametrize("case", range(len(sr.ATTN_CASES)))
def test_ascending_family_defers_and_rescales(case):
    """the construction's promise (attn_inputs), replayed in fp64: in every unit some tiles keep the old running maximum with P above 1
    (the deferred rescale happens) and, from three tiles on, some tiles after the first raise it"""
    L, _ = sr.ATTN_CASES[case]
    qkv, bias, var = sr.attn_inputs(case, "ascending")
    q, k, v, b = sr.attn_units(qkv, L, bias, var)
    for u in range(q.shape[0]):
        kept, raised, pmax = sr.deferral_replay(q[u], k[u], None if b is None else b[u])
        print(f"[split3 cpu] ascending L={L} unit {u}: tiles that kept the maximum {kept}, raised it {raised}, largest P {pmax:.1f}")
        assert kept >= 1 and 1.0 < pmax <= 2.0 ** sr.AT_DEFER
        assert raised >= 1 or L <= 64
    # and on the randn family the maximum is adopted once and hardly ever raised: the family does not reach the rescale
    qkv, bias, var = sr.attn_inputs(case, "randn")
    q, k, v, b = sr.attn_units(qkv, L, bias, var)
    kept, raised, pmax = sr.deferral_replay(q[0], k[0], None if b is None else b[0])
    print(f"[split3 cpu] randn L={L} unit 0: kept {kept}, raised {raised}, largest P {pmax:.1f}")
