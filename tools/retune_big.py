#!/usr/bin/env python3
"""Re-race the launch modes of the split GEMM / implicit-GEMM convolution for every LARGE shape the in-tree tile cache knows
(after a kernel change: round 3 moved the 128x256 / 256x128 tiles to LDS-DMA staging and added modes 16 / 17).
Durations are dispatch timestamps (ops.profile_begin / profile_end), median of `reps` launches per mode, two interleaved passes.
Writes gpurun_out/retune_big.json = {"picks": {key: mode}, "table": {key: {mode: us}}}; merge into the in-tree cache with --merge.
--attn: the attention launches instead (attn_modes 1-7, both arithmetics) -> gpurun_out/retune_attn.json.
--small: the split GEMMs of single-image sized launches instead (M <= ops.SPLIT3_SMALL_M: the small register-staged tiles against the
ring kernel's modes 18-22) -> gpurun_out/retune_small.json.
--keys K1,K2,...: only these keys of the in-tree cache (e.g. "gemm3|9248|1024|4096|1|0").
--merge writes no gemm3 / conv3 pick above INTREE_MAX_SPLIT3 into the in-tree file: tests/test_tile_cache_cpu.py pins the in-tree
picks of these kinds to 0..31.  Mode 32 (160x256 tiles) is raced here for the table; in the tree it is reached through mode 26,
which takes it by arithmetic (csrc/gemm_split.hip: s3_plan).
(Replaces the round-2 one-off scripts gemm_big_modes.py / conv_modes.py / gemm_shapes_modes.py.)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SMALL = "--small" in sys.argv
ATTN = "--attn" in sys.argv
OUT = os.path.join(ROOT, "gpurun_out", "retune_attn.json" if ATTN else ("retune_small.json" if SMALL else "retune_big.json"))
SMALL_MODES = (3, 4, 5, 18, 19, 20, 21, 22, 23, 24, 25)
GEMM_MODES = (1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 26, 27, 28, 29, 30, 31, 32)
CONV_MODES = (1, 2, 3, 5, 10, 11, 14, 15, 16, 17, 30, 32)
INTREE_MAX_SPLIT3 = 31
KEYS = set(sys.argv[sys.argv.index("--keys") + 1].split(",")) if "--keys" in sys.argv else None


def mergeable(new):
    """(picks that may go into the in-tree cache, picks refused)"""
    refused = {k: v for k, v in new.items() if k.split("|")[0] in ("gemm3", "conv3") and v > INTREE_MAX_SPLIT3}
    return {k: v for k, v in new.items() if k not in refused}, refused


def merge():
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    new, refused = mergeable(json.load(open(OUT))["picks"])
    if refused:
        print(f"NOT merged (the in-tree cache holds gemm3 / conv3 picks 0..{INTREE_MAX_SPLIT3} only -- tests/test_tile_cache_cpu.py; "
              f"these shapes keep their in-tree pick):", refused)
    d = json.load(open(ops._INTREE_CACHE))
    changed = {k: (d["picks"].get(k), v) for k, v in new.items() if d["picks"].get(k) != v}
    d["picks"].update(new)
    with open(ops._INTREE_CACHE, "w") as f:
        json.dump(d, f, indent=0, sort_keys=True)
    print(f"merged {len(new)} picks, {len(changed)} changed:", changed)


def main():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    cache = json.load(open(ops._INTREE_CACHE))["picks"]
    picks, table = {}, {}

    def race(fn_of_mode, modes, reps=6):
        t = {m: [] for m in modes}
        for _ in range(2):
            for m in modes:
                fn_of_mode(m)
                ops.profile_begin(4 * reps)
                for _ in range(reps):
                    fn_of_mode(m)
                recs = ops.profile_end()
                # a launch mode made of two kernels is one record spanning both
                t[m].append(sorted(r[1] for r in recs)[len(recs) // 2] * 1e3)
        return {m: min(v) for m, v in t.items()}

    for key, old in sorted(cache.items()):
        kind, *nums = key.split("|")
        nums = [int(x) for x in nums]
        if KEYS is not None and key not in KEYS:
            continue
        if ATTN:
            if kind not in ("attn", "attn3"):
                continue
            nseq, L, heads, has_bias = nums
            D = heads * 64
            qkv = torch.randn(nseq * L, 3 * D, device=dev, generator=g)
            out = torch.empty(nseq * L, D, device=dev)
            b = torch.randn(1, L, L, device=dev, generator=g) if has_bias else None
            prec = "split3" if kind == "attn3" else "f32"
            t = {}
            for _ in range(2):
                for m in ops.ATTN_MODES:
                    for _ in range(2):
                        ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, L, nseq, heads, bias=b, mode=m, precision=prec)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(6):
                        ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, L, nseq, heads, bias=b, mode=m, precision=prec)
                    e1.record()
                    e1.synchronize()
                    t[m] = min(t.get(m, 1e9), e0.elapsed_time(e1) / 6 * 1e3)
            fl = 4.0 * L * L * 64 * heads * nseq
        elif kind == "gemm3":
            M, N, K, res, act = nums
            if SMALL:
                if M > ops.SPLIT3_SMALL_M or M * N < (1 << 16):
                    continue
            elif M * N < (1 << 21) or old in (3, 4):
                continue
            a = torch.randn(M, K, device=dev, generator=g)
            w = torch.randn(N, K, device=dev, generator=g) * 0.03
            b = torch.randn(N, device=dev, generator=g)
            r = torch.randn(M, N, device=dev, generator=g) if res else None
            ap = ops.split3_planes(a)
            out = torch.empty(M, N, device=dev)
            modes = list(SMALL_MODES) if SMALL else [m for m in GEMM_MODES if m <= ops._MAX_MODE["gemm3"] and not (m in (1, 6, 8, 10, 12, 26, 27, 30, 31, 32) and N < 256) and not (m in (28, 29) and N < 192)]
            t = race(lambda m: ops.gemm(ap, w, b, residual=r, act=act, out=out, tile=m, precision="split3"), modes)
            fl = 2.0 * M * N * K
        elif kind == "conv3":
            M, H, W, Cin, Cout, res, act = nums
            B = M // (H * W)
            if SMALL or M * Cout < (1 << 21) or old in (3, 4):
                continue
            halo = torch.zeros(B, H + 2, W + 2, Cin, device=dev)
            halo[:, 1:-1, 1:-1] = torch.randn(B, H, W, Cin, device=dev, generator=g)
            w = torch.randn(Cout, 9 * Cin, device=dev, generator=g) * 0.02
            b = torch.randn(Cout, device=dev, generator=g)
            r = torch.randn(M, Cout, device=dev, generator=g) if res else None
            hp = ops.halo_planes_buffer(dev, B, H, W, Cin)
            ops.split3_planes(halo.view(-1, Cin), out=ops.Planes(halo.numel() // Cin, Cin, dev, buf=hp.t))
            out = torch.empty(M, Cout, device=dev)
            modes = [m for m in CONV_MODES if m <= ops._MAX_MODE["conv3"] and not (m in (1, 10, 30, 32) and Cout < 256)]
            t = race(lambda m: ops.conv3x3(hp, w, b, B, H, W, Cin, Cout, residual=r, act=act, out=out, tile=m, precision="split3"), modes)
            fl = 2.0 * M * Cout * 9 * Cin
            del halo
        else:
            continue
        if ATTN and old in t and t[min(t, key=t.get)] > 0.97 * t[old]:
            t[old] = min(t.values())   # keep a standing pick unless another mode is >= 3 % faster (event timing noise on short launches)
        best = min(t, key=t.get)
        picks[key], table[key] = best, {str(m): round(v, 1) for m, v in t.items()}
        print(f"{key:>40}: old m{old} {t.get(old, float('nan')):7.1f} us -> m{best} {t[best]:7.1f} us  {fl / t[best] / 1e6:6.1f} TFLOP/s   "
              + " ".join(f"m{m}={v:.0f}" for m, v in t.items()), flush=True)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        json.dump({"picks": picks, "table": table}, open(OUT, "w"), indent=0)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    merge() if "--merge" in sys.argv else main()
