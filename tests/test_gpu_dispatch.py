"""GPU tests of the launch-mode layer of sgic_amd.ops as production calls it (tile=None / mode=None): _pick_and_launch -> _lookup /
_tune / _ctx_launch, and the inline race of attention().  This layer launches a kernel many times into the CALLER's buffers and
has to leave exactly one result behind; every other kernel test pins the mode and never reaches it.

Two references throughout:
  * the same call with tile=0 / mode=0 on fresh copies of the inputs: bit for bit (all launch modes are bitwise identical by design);
  * an fp64 result on the CPU, within the bound the kernel's own test uses for that arithmetic:
      f32 GEMM    3e-6 sqrt(K) max(1, max|pre|)      (test_gemm_fuzz_all_tile_modes_identical_and_close_to_fp64)
      split GEMM  rms error <= 1.10 x the fp32 path's + 1e-9 rms(ref), worst error <= 1.5 x the fp32 path's, on the same inputs
                                                     (test_gpu_split3.py::test_error_not_above_fp32_path)
      attention   2e-5 against kernels_ref.attention64 (test_attention_vs_torch)
      conv3x3     3e-6 sqrt(9 Cin) max(1, max|pre|)  (test_conv3x3_vs_fp64_all_tile_modes), both arithmetics.
Every output is a window of a larger buffer filled with a sentinel bit pattern that no kernel produces; what lies outside the
window must keep it.  A spy around ops.call counts the launches by symbol, one around ops._tune the races.

No test asserts WHICH mode wins, how long anything takes or how many probes a race makes: the fixture prints the tuning launches
and the wall time of each test."""
import functools
import json
import time

import pytest
import torch
import torch.nn.functional as F

import kernels_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BITS = 0x7FA5C3D2                      # a NaN pattern no kernel here produces
PLANE_PAT = 0x7FB7                          # a signalling bf16 NaN: no piece of a split value
GEMM_SYM = {"f32": "sgic_gemm_f32", "split3": "sgic_gemm_split3_f32"}
CONV_SYM = {"f32": "sgic_conv3x3_f32", "split3": "sgic_conv3x3_split3_f32"}
RING = (18, 19, 20, 21, 22, 23, 24, 25)     # written out here: a change of ops.SPLIT3_RING_MODES / _split3_modes must show up
PRECISIONS = ("f32", "split3")


# ---- state fixture and launch spy -------------------------------------------------------------------------------------------------
class Spy:
    """records the symbol of every ops.call and the (key, modes) of every ops._tune, and forwards both"""

    def __init__(self, ops, monkeypatch):
        self.ops, self.calls, self.races, self.tuning = ops, [], [], 0
        real_call, real_tune = ops.call, ops._tune

        def call(name, *args):
            self.calls.append(name)
            return real_call(name, *args)

        def tune(key, launch, modes=None):
            self.races.append((key, modes))
            i0 = self.mark()
            best = real_tune(key, launch, modes)
            self.tuning += len(self.kernels(i0))
            return best
        monkeypatch.setattr(ops, "call", call)
        monkeypatch.setattr(ops, "_tune", tune)

    def mark(self):
        return len(self.calls)

    def kernels(self, since):
        """the tuned kernels launched since mark(): GEMM, convolution and attention symbols (not the split / pack passes around them)"""
        return [n for n in self.calls[since:] if n in GEMM_SYM.values() or n in CONV_SYM.values() or n.startswith("sgic_attention")]


@pytest.fixture()
def tuner(tmp_path, monkeypatch, request):
    """empty launch-mode tables, a user cache under tmp_path, AUTOTUNE on; everything is put back afterwards, so a test leaves
    no pick behind and no dirty flag for the atexit writer"""
    import sgic_amd  # noqa
    from sgic_amd import ops
    monkeypatch.setenv("SGIC_TILE_CACHE", str(tmp_path / "cache.json"))
    saved = (dict(ops._TILE), {k: dict(v) for k, v in ops._FAMILY.items()}, ops._DIRTY, dict(ops._CTX), ops.AUTOTUNE, ops.PRECISION,
             ops.LAST_TILE)
    for table in (ops._TILE, ops._FAMILY, ops._CTX):
        table.clear()
    ops._DIRTY, ops.AUTOTUNE, ops.LAST_TILE = False, True, 0
    spy = Spy(ops, monkeypatch)
    t0 = time.perf_counter()
    try:
        yield spy
    finally:
        torch.cuda.synchronize()
        print(f"\n[dispatch] {request.node.name}: {len(spy.races)} races, {spy.tuning} tuning launches, {time.perf_counter() - t0:.2f} s")
        if ops.PROFILE is not None:          # a test failed inside its window
            try:
                ops.profile_end()
            except Exception:   # noqa: BLE001
                ops.PROFILE = None
        for table, old in ((ops._TILE, saved[0]), (ops._FAMILY, saved[1]), (ops._CTX, saved[3])):
            table.clear()
            table.update(old)
        ops._DIRTY, ops.AUTOTUNE, ops.PRECISION, ops.LAST_TILE = saved[2], saved[4], saved[5], saved[6]


def _clear(ops):
    for table in (ops._TILE, ops._FAMILY, ops._CTX):
        table.clear()
    ops._DIRTY = False


def _sent(*shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _all_sent(t):
    return bool((t.contiguous().view(torch.int32) == SENT_BITS).all())


def _planes_buf(rows, cols):
    return torch.full((3 * rows * cols + 64,), PLANE_PAT, dtype=torch.int16, device=DEV)


def _eq(got, ref):
    if got.dtype == torch.float32:
        return torch.equal(kr.bits(got), kr.bits(ref))
    return got.dtype == ref.dtype and torch.equal(got, ref)


def _install_ctx(ops, key, cands):
    """a pending in-context race as _tune leaves it: the first candidate is the isolated race's pick"""
    ops._remember(key, cands[0], dirty=False)
    ops._CTX[key] = {"cands": list(cands), "t": {m: [] for m in cands}, "i": 0}


def _ctx_well_formed(ops, key, modes):
    """the entry _tune may leave behind for a key: absent, or 2..CTX_CANDS candidates out of `modes`, led by the pick, no sample yet"""
    c = ops._CTX.get(key)
    if c is None:
        return True
    return (2 <= len(c["cands"]) <= ops.CTX_CANDS and len(set(c["cands"])) == len(c["cands"]) and set(c["cands"]) <= set(modes)
            and c["cands"][0] == ops._TILE[key] and list(c["t"]) == c["cands"] and not any(c["t"].values()) and c["i"] == 0)


def _drain(tuner, c, want, sym, modes):
    """call until the pending in-context race of c.key (if any) is over: every call is ONE launch with the right bits"""
    ops = tuner.ops
    pending = len(ops._CTX[c.key]["cands"]) * ops.CTX_REPS if c.key in ops._CTX else 0
    for i in range(pending + 1):
        assert (c.key in ops._CTX) == (i < pending), i
        i0 = tuner.mark()
        got, buf = c.run()
        assert tuner.kernels(i0) == [sym], (i, tuner.kernels(i0))
        assert _eq(got, want), ("call %d after the race differs from the forced launch" % i)
        c.check_outside(buf)
    assert c.key not in ops._CTX and ops._TILE[c.key] in modes and ops.LAST_TILE == ops._TILE[c.key]


# ---- GEMM calls -------------------------------------------------------------------------------------------------------------------
ACT64 = {0: lambda v: v, 1: F.gelu, 2: F.silu}
SEGMENTS = {256: 8, 257: 1, 2304: 8, 255: 5, 2048: 8}      # A's row map of the in-place c_seg case: M = segments x rows (257 is prime)
GAP = 5


@functools.lru_cache(maxsize=None)
def _gemm_inputs(M, N, K):
    """CPU inputs and the fp64 product of one shape, computed once and never written to"""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    return a, w, bias, res, a.double() @ w.double().T


class GemmCall:
    """one production-style GEMM call (tile=None) and its forced twin.  Epilogues:
      plain          out = a w^T into a column slice of a sentinel buffer (ldc = N + 4)
      bias_gelu      gelu(a w^T + bias), same placement
      inplace_slice  X += a w^T with X that column slice (residual is out)
      inplace_cseg   the same through c_seg = (M, M + GAP): one segment, GAP gap rows behind it, and A read through an a_seg row map
                     of several segments out of a sentinel buffer.  (More than one C segment cannot be in place: the kernels read the
                     residual by logical row and write through the map; ops.gemm refuses it, test_inplace_residual_multi_segment_refused.)
      planes         gelu(a w^T + bias) written as bf16x3 planes (to_gemm=True), split arithmetic only"""

    def __init__(self, ops, M, N, K, epi, precision):
        a, w, bias, res, pre = _gemm_inputs(M, N, K)
        self.ops, self.M, self.N, self.K, self.epi, self.precision = ops, M, N, K, epi, precision
        self.a, self.w = a.to(DEV), w.to(DEV)
        with_bias = epi in ("bias_gelu", "planes")
        self.bias = bias.to(DEV) if with_bias else None
        self.act = ops.ACT_GELU if with_bias else ops.ACT_NONE
        self.res0 = res.to(DEV) if epi.startswith("inplace") else None
        self.pre = pre + bias.double() if with_bias else pre
        self.ref = ACT64[self.act](self.pre) + (res.double() if self.res0 is not None else 0.0)
        self.key = ("gemm3" if precision == "split3" else "gemm", M, N, K, int(self.res0 is not None), self.act)
        self.a_arg, self.maps = self.a, {}
        if epi == "inplace_cseg":
            n = SEGMENTS[M]
            Lr, La = M // n, M // n + 3
            self.a_arg = _sent(n * La, K)
            self.a_arg.view(n, La, K)[:, :Lr] = self.a.view(n, Lr, K)
            self.maps = dict(M=M, a_seg=(Lr, La), c_seg=(M, M + GAP))

    def forced(self, precision=None):
        """the out-of-place launch with the built-in heuristic (tile=0) on fresh dense copies -> fp32 (M, N)"""
        return self.ops.gemm(self.a.clone(), self.w, self.bias, residual=None if self.res0 is None else self.res0.clone(), act=self.act,
                             tile=0, precision=precision or self.precision)

    def run(self, tile=None):
        """-> (result, the whole buffer it lives in); result: fp32 (M, N), or for `planes` the Planes object"""
        ops, M, N = self.ops, self.M, self.N
        kw = dict(act=self.act, tile=tile, precision=self.precision, **self.maps)
        if self.epi == "planes":
            buf = _planes_buf(M, N)
            pl = ops.Planes(M, N, DEV, buf=buf)
            assert ops.gemm(self.a_arg, self.w, self.bias, out=pl, to_gemm=True, **kw) is pl
            return pl, buf
        rows = M + GAP if self.epi == "inplace_cseg" else M
        buf = _sent(rows + 1, N + 4)
        X = buf[:rows, :N]
        if self.res0 is not None:
            X[:M] = self.res0
            ops.gemm(self.a_arg, self.w, self.bias, residual=X, out=X, **kw)
        else:
            ops.gemm(self.a_arg, self.w, self.bias, out=X, **kw)
        return buf[:M, :N], buf

    def check_outside(self, buf):
        """gap rows, slack columns and the row behind the buffer keep the sentinel"""
        if self.epi == "planes":
            assert bool((buf[3 * self.M * self.N:] == PLANE_PAT).all()), "a write behind the three planes"
            return
        assert _all_sent(buf[self.M:]) and _all_sent(buf[:, self.N:]), "a write outside the M x N window"
        if self.epi == "inplace_cseg":
            assert _all_sent(self.a_arg.view(SEGMENTS[self.M], -1, self.K)[:, self.M // SEGMENTS[self.M]:]), "A's gap rows were written"

    def values(self, got):
        return got.float() if self.epi == "planes" else got

    def same(self, got, want):
        if self.epi == "planes":
            return torch.equal(got.rowmajor(), self.ops.split3(want.contiguous()))
        return _eq(got, want)

    def check_fp64(self, got, f32_got=None):
        """f32_got: the fp32 path's forced result on the same inputs (the yardstick of the split arithmetic)"""
        got64 = self.values(got).cpu().double()
        err = float((got64 - self.ref).abs().max())
        if self.precision == "f32":
            bound = 3e-6 * self.K ** 0.5 * max(1.0, float(self.pre.abs().max()))
            print(f"[dispatch] gemm {self.M}x{self.N}x{self.K} {self.epi} f32: worst |err| vs fp64 {err:.3e} (bound {bound:.3e})")
            assert err < bound, (err, bound)
            return
        f64 = f32_got.cpu().double()
        e3, e1 = float((got64 - self.ref).pow(2).mean().sqrt()), float((f64 - self.ref).pow(2).mean().sqrt())
        scale, m1 = float(self.ref.pow(2).mean().sqrt()), float((f64 - self.ref).abs().max())
        print(f"[dispatch] gemm {self.M}x{self.N}x{self.K} {self.epi} split3: rms err {e3:.3e} (fp32 path {e1:.3e}), worst {err:.3e} ({m1:.3e})")
        assert e3 <= 1.10 * e1 + 1e-9 * scale, (e3, e1)
        assert err <= 1.5 * m1, (err, m1)


def _gemm_candidates(ops, precision, M):
    if precision == "f32":
        return tuple(ops.TUNE_MODES)
    return tuple(range(1, 33)) if M <= 2048 else tuple(m for m in range(1, 33) if m not in RING)


# ---- a. cold GEMM race ------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(256, 256, 96),              # M N exactly at the 1 << 16 threshold; K % 64 != 0: ring modes 18, 19, 20, 25 fall back
               (257, 260, 160),             # ragged M and N
               (2304, 512, 64),             # M > SPLIT3_SMALL_M: the ring modes are not raced
               (255, 256, 64)]              # below the threshold: no race
GEMM_CASES = [(s, p, e) for s in GEMM_SHAPES for p in PRECISIONS for e in ("plain", "bias_gelu", "inplace_slice", "inplace_cseg", "planes")
              if not (e == "planes" and (p == "f32" or s[1] % 32))]        # planes: the split path's output, N % 32 == 0


@pytest.mark.parametrize("shape,precision,epi", GEMM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_cold_gemm_race(tuner, shape, precision, epi):
    ops, (M, N, K), sym = tuner.ops, shape, GEMM_SYM[precision]
    c = GemmCall(ops, M, N, K, epi, precision)
    want = c.forced()
    f32 = c.forced("f32") if precision == "split3" else None
    i0 = tuner.mark()
    got, buf = c.run()
    launches = tuner.kernels(i0)
    assert c.same(got, want), "the cold call differs from the forced launch (for an in-place call: the product was not added ONCE)"
    c.check_outside(buf)
    c.check_fp64(got, f32)
    if M * N < (1 << 16):
        assert launches == [sym] and tuner.races == [] and not ops._TILE and not ops._CTX and not ops._DIRTY and ops.LAST_TILE == 0
        return
    cands = _gemm_candidates(ops, precision, M)
    assert tuner.races == [(c.key, None if precision == "f32" else cands)], tuner.races
    assert set(launches) == {sym} and len(launches) > len(cands)
    assert ops._TILE[c.key] in cands and ops.LAST_TILE == ops._TILE[c.key] and ops._DIRTY and c.key not in ops._CTX
    assert ops._FAMILY[(c.key[0],) + c.key[2:]] == {M: ops._TILE[c.key]}
    # the second call: the pick, one launch, the same bits
    i1 = tuner.mark()
    got2, buf2 = c.run()
    assert tuner.kernels(i1) == [sym] and len(tuner.races) == 1 and ops.LAST_TILE == ops._TILE[c.key]
    assert c.same(got2, want)
    c.check_outside(buf2)


def test_inplace_residual_multi_segment_refused(tuner):
    """out is residual with a c_seg map of several segments: the residual is read at row m, the result written at row
    (m // seg) * stride + m % seg -- not an in-place update, and a launch would read rows that others of its workgroups write"""
    ops = tuner.ops
    X = torch.zeros(8 * 40, 256, device=DEV)
    a, w = torch.zeros(256, 64, device=DEV), torch.zeros(256, 64, device=DEV)
    for precision in PRECISIONS:
        i0 = tuner.mark()
        with pytest.raises(AssertionError, match="in-place residual through a c_seg"):
            ops.gemm(a, w, residual=X, out=X, M=256, c_seg=(32, 40), precision=precision)
        assert tuner.kernels(i0) == [] and not ops._TILE


# ---- b. the in-context race -------------------------------------------------------------------------------------------------------
BIG = (2048, 1024, 1280)                    # 2 M N K just over 5e9: M_big
CTX_MODES = {"f32": (1, 2, 14), "split3": (1, 21, 5)}      # three tile shapes each (128x128, 128x64, 64x64 / 128x256, 64x64 ring, 64x128)


@pytest.fixture(params=PRECISIONS)
def big(tuner, request):
    ops = tuner.ops
    c = GemmCall(ops, *BIG, "inplace_slice", request.param)
    assert ops.M_big(c.key)
    want = c.forced()
    c.check_fp64(want, c.forced("f32") if request.param == "split3" else None)
    return c, want, GEMM_SYM[request.param], CTX_MODES[request.param]


def test_seeded_in_context_race(tuner, big):
    """every sample of a pending in-context race IS the call's launch: one launch per call, the product added once"""
    ops, (c, want, sym, cands) = tuner.ops, big
    _install_ctx(ops, c.key, cands)
    n = len(cands) * ops.CTX_REPS
    for i in range(n):
        assert c.key in ops._CTX, i
        i0 = tuner.mark()
        got, buf = c.run()
        assert tuner.kernels(i0) == [sym], (i, tuner.kernels(i0))
        assert _eq(got, want), i
        c.check_outside(buf)
    assert c.key not in ops._CTX and ops._TILE[c.key] in cands and ops._DIRTY and tuner.races == []
    i0 = tuner.mark()
    got, buf = c.run()
    assert tuner.kernels(i0) == [sym] and ops.LAST_TILE == ops._TILE[c.key] and _eq(got, want)


def test_partial_in_context_race_is_closed_by_finalize_and_profile_begin(tuner, big):
    ops, (c, want, sym, cands) = tuner.ops, big
    _install_ctx(ops, c.key, cands)
    for _ in range(2):
        got, _ = c.run()
        assert _eq(got, want)
    ops.finalize_autotune()
    assert not ops._CTX and ops._TILE[c.key] in cands[:2] and ops._DIRTY        # the third candidate never ran
    # a window must not open over a pending race: profile_begin closes it (no sample: the isolated race's pick stays)
    _clear(ops)
    _install_ctx(ops, c.key, cands[::-1])
    ops.profile_begin(8)
    assert not ops._CTX and ops._TILE[c.key] == cands[-1]
    i0 = tuner.mark()
    got, _ = c.run()
    recs = ops.profile_end()
    assert tuner.kernels(i0) == [sym] and len(recs) == 1 and recs[0][2][:3] == BIG and _eq(got, want)
    assert list(ops.PROFILE_TILES) == [cands[-1]]


def test_natural_cold_race_of_a_big_gemm(tuner, big):
    """whether the isolated race leaves more than one leader is a timing accident: only the invariants"""
    ops, (c, want, sym, _) = tuner.ops, big
    modes = _gemm_candidates(ops, c.precision, BIG[0])
    got, buf = c.run()
    assert _eq(got, want)
    c.check_outside(buf)
    assert len(tuner.races) == 1 and ops._TILE[c.key] in modes and ops._DIRTY and _ctx_well_formed(ops, c.key, modes), ops._CTX
    _drain(tuner, c, want, sym, modes)
    assert len(tuner.races) == 1


# ---- c. profile window ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_tuning_inside_a_profile_window(tuner, precision):
    ops, sym = tuner.ops, GEMM_SYM[precision]
    c = GemmCall(ops, 256, 256, 96, "inplace_slice", precision)
    want = c.forced()
    ops.profile_begin(16)
    for _ in range(3):
        i0 = tuner.mark()
        got, _ = c.run()
        assert tuner.kernels(i0) == [sym] and _eq(got, want)
    recs = ops.profile_end()                                 # raises if the device timed another number of launches
    assert len(recs) == 3 and all(r[2][:3] == (256, 256, 96) for r in recs) and list(ops.PROFILE_TILES) == [0, 0, 0]
    assert tuner.races == [] and c.key not in ops._TILE and not ops._DIRTY
    # after the window the first call races
    got, _ = c.run()
    assert len(tuner.races) == 1 and c.key in ops._TILE and _eq(got, want)
    # a pending in-context race inside a window: the pick is launched once and recorded; the race waits
    pick = ops._TILE[c.key]
    ops.profile_begin(16)
    _install_ctx(ops, c.key, (pick, 2 if pick != 2 else 1))   # after profile_begin, which closes what is pending
    i0 = tuner.mark()
    got, _ = c.run()
    recs = ops.profile_end()
    assert tuner.kernels(i0) == [sym] and len(recs) == 1 and list(ops.PROFILE_TILES) == [pick] and _eq(got, want)
    assert ops._CTX[c.key]["i"] == 0 and not any(ops._CTX[c.key]["t"].values()) and len(tuner.races) == 1


# ---- d. borrowed picks on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M_known,M,N,K,modes", [
    ("gemm3", 2000, 3000, 256, 128, RING),          # a ring mode above SPLIT3_SMALL_M, where the race would never try it
    ("gemm3", 2000, 3000, 256, 96, RING),           # ... and with K % 64 != 0, where 18, 19, 20, 25 fall back inside the dispatcher
    ("gemm3", 320, 300, 256, 96, (32,)),            # the 160x256 tile for two tiles' worth of rows
    ("gemm", 2000, 3000, 256, 96, (15, 12))])       # fp32: the latency kernel / a persistent mixed launch
def test_borrowed_pick_on_the_device(tuner, kind, M_known, M, N, K, modes):
    ops = tuner.ops
    precision = "split3" if kind == "gemm3" else "f32"
    c = GemmCall(ops, M, N, K, "plain", precision)
    want = c.forced()
    c.check_fp64(want, c.forced("f32") if precision == "split3" else None)
    for mode in modes:
        _clear(ops)
        ops._remember((kind, M_known, N, K, 0, 0), mode, dirty=False)
        i0 = tuner.mark()
        got, buf = c.run()
        assert tuner.kernels(i0) == [GEMM_SYM[precision]] and ops.LAST_TILE == mode and ops._TILE[c.key] == mode, mode
        assert _eq(got, want), ("borrowed mode differs from the forced launch", mode)
        c.check_outside(buf)
        assert not ops._DIRTY and set(ops._FAMILY[(kind, N, K, 0, 0)]) == {M_known}
    assert tuner.races == []


# ---- e. conv3x3 -------------------------------------------------------------------------------------------------------------------
CONV = (1, 64, 64, 32, 256)                 # B H W Cout = 1 << 20: exactly at the race's threshold
CONV_MODES = {"f32": None, "split3": (1, 2, 3, 5, 10, 11, 14, 15, 16, 17, 30)}


@functools.lru_cache(maxsize=None)
def _conv_inputs():
    B, H, W, Cin, Cout = CONV
    g = torch.Generator().manual_seed(64 * Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=g)
    rw = torch.randn(B * H * W, Cout + 4, generator=g)                 # the residual is its column slice: ldr = Cout + 4
    r_nchw = rw[:, :Cout].reshape(B, H, W, Cout).permute(0, 3, 1, 2)
    refs = {False: kr.conv3x3_64(x, w, bias, None, 0), True: kr.conv3x3_64(x, w, bias, r_nchw, 2)}
    halo = torch.zeros(B, H + 2, W + 2, Cin)
    halo[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    return halo, w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous(), bias, rw, refs


class ConvCall:
    """conv3x3 with tile=None: plain (act 0) or SiLU + a non-aliased residual; fp32 halo input or producer-style HaloPlanes"""

    def __init__(self, ops, precision, res, planes_in):
        B, H, W, Cin, Cout = CONV
        halo, wk, bias, rw, refs = _conv_inputs()
        self.ops, self.precision, self.res, self.M = ops, precision, res, B * H * W
        self.wk, self.bias, self.rw = wk.to(DEV), bias.to(DEV), rw.to(DEV)
        self.pre, self.ref = refs[res]
        self.act = 2 if res else 0
        self.x = halo.to(DEV)
        if planes_in:
            rows = B * (H + 2) * (W + 2)
            self.x = ops.HaloPlanes(ops.split3_planes(self.x.view(rows, Cin)).t, B, H, W, Cin)
        self.key = ("conv3" if precision == "split3" else "conv3x3", self.M, H, W, Cin, Cout, int(res), self.act)

    def run(self, tile=None):
        B, H, W, Cin, Cout = CONV
        buf = _sent(self.M + 1, Cout + 4)
        self.ops.conv3x3(self.x, self.wk, self.bias, B, H, W, Cin, Cout, residual=self.rw[:, :Cout] if self.res else None, act=self.act,
                         out=buf[:self.M, :Cout], tile=tile, precision=self.precision)
        return buf[:self.M, :Cout], buf

    def check_outside(self, buf):
        assert _all_sent(buf[self.M:]) and _all_sent(buf[:, CONV[4]:]), "a write outside the M x Cout window"

    def check_fp64(self, got):
        err = float((got.cpu().double() - self.ref).abs().max())
        bound = 3e-6 * (9 * CONV[3]) ** 0.5 * max(1.0, float(self.pre.abs().max()))
        print(f"[dispatch] conv3x3 {CONV} res={int(self.res)} {self.precision}: worst |err| vs fp64 {err:.3e} (bound {bound:.3e})")
        assert err < bound, (err, bound)


CONV_CASES = [(p, r, pl) for p in PRECISIONS for r in (False, True) for pl in (False, True) if not (pl and p == "f32")]


@pytest.mark.parametrize("precision,res,planes_in", CONV_CASES)
def test_cold_conv_race(tuner, precision, res, planes_in):
    ops, sym = tuner.ops, CONV_SYM[precision]
    assert CONV[0] * CONV[1] * CONV[2] * CONV[4] == 1 << 20
    c = ConvCall(ops, precision, res, planes_in)
    want, _ = c.run(tile=0)
    c.check_fp64(want)
    modes = CONV_MODES[precision]
    cands = tuple(ops.TUNE_MODES) if modes is None else modes
    # inside a profile window: no race, one record per call
    ops.profile_begin(8)
    i0 = tuner.mark()
    got, _ = c.run()
    recs = ops.profile_end()
    assert tuner.kernels(i0) == [sym] and len(recs) == 1 and tuner.races == [] and not ops._TILE and _eq(got, want)
    # the cold call
    i0 = tuner.mark()
    got, buf = c.run()
    launches = tuner.kernels(i0)
    assert _eq(got, want), "the cold call differs from the forced launch"
    c.check_outside(buf)
    assert tuner.races == [(c.key, modes)] and set(launches) == {sym} and len(launches) > len(cands)
    assert ops._TILE[c.key] in cands and ops._DIRTY and _ctx_well_formed(ops, c.key, cands), ops._CTX
    _drain(tuner, c, want, sym, cands)
    assert len(tuner.races) == 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seeded_in_context_race_conv(tuner, precision):
    ops, sym = tuner.ops, CONV_SYM[precision]
    c = ConvCall(ops, precision, True, False)
    want, _ = c.run(tile=0)
    cands = (1, 3, 14) if precision == "split3" else (1, 2, 14)
    _install_ctx(ops, c.key, cands)
    _drain(tuner, c, want, sym, cands)
    assert tuner.races == [] and ops._DIRTY


@pytest.mark.parametrize("precision", PRECISIONS)
def test_conv_refuses_out_aliasing_residual(tuner, precision):
    """conv3x3 races with no restore: an output that is (or overlaps) its residual would keep every probe's addition"""
    ops = tuner.ops
    B, H, W, Cin, Cout = CONV
    c = ConvCall(ops, precision, True, False)
    big = torch.zeros(c.M + 1, Cout, device=DEV)
    for out, residual in ((big[:c.M], big[:c.M]), (big[:c.M], big[1:]), (big[1:], big[:c.M])):
        i0 = tuner.mark()
        with pytest.raises(AssertionError, match="out overlaps residual"):
            ops.conv3x3(c.x, c.wk, c.bias, B, H, W, Cin, Cout, residual=residual, out=out, precision=precision)
        assert tuner.kernels(i0) == [] and tuner.races == []
    # neighbours in one allocation do not overlap
    two = torch.zeros(2 * c.M, Cout, device=DEV)
    two[c.M:] = c.rw[:, :Cout]
    ops.conv3x3(c.x, c.wk, c.bias, B, H, W, Cin, Cout, residual=two[c.M:], act=2, out=two[:c.M], tile=0, precision=precision)
    want, _ = c.run(tile=0)
    assert _eq(two[:c.M], want)


# ---- f. the attention race --------------------------------------------------------------------------------------------------------
ATTN_CASES = [(64, 8, 8, False),            # nseq heads L = 4096: exactly at the threshold
              (289, 2, 8, False),           # ragged query rows
              (256, 4, 4, True),            # the production window with the 4-variant bias
              (63, 5, 13, False)]           # 4095: below the threshold
ATTN_WINDOWS = {64: (32, 32), 289: (256, 33), 256: (224, 32)}


@functools.lru_cache(maxsize=None)
def _attn_inputs(L, nseq, heads, bias):
    g = torch.Generator().manual_seed(L * 131 + nseq * 17 + heads)
    qkv = torch.randn(nseq * L, 3 * heads * 64, generator=g)
    b = kr.attn_bias_variants(L, g) if bias else None
    var = ((torch.arange(nseq) + 1) % 4).to(torch.int32) if bias else None
    return qkv, b, var, kr.attention64(qkv, L, nseq, heads, b, var, 0.125)


class AttnCall:
    def __init__(self, ops, L, nseq, heads, bias, precision):
        qkv, b, var, self.ref = _attn_inputs(L, nseq, heads, bias)
        self.ops, self.L, self.nseq, self.heads, self.precision, self.D = ops, L, nseq, heads, precision, heads * 64
        self.qkv = qkv.to(DEV)
        self.kw = dict(bias=b.to(DEV) if bias else None, biasvar=var.to(DEV) if bias else None, precision=precision)
        self.key = ("attn3" if precision == "split3" else "attn", nseq, L, heads, int(bias))

    def window_rows(self, window):
        q_tok0, Lq = window
        return (torch.arange(self.nseq, device=DEV)[:, None] * self.L + q_tok0 + torch.arange(Lq, device=DEV)[None, :]).reshape(-1)

    def run(self, mode=None, planes=False, window=None):
        ops, D = self.ops, self.D
        q, k, v = self.qkv[:, :D], self.qkv[:, D:2 * D], self.qkv[:, 2 * D:]
        if window is not None:
            q = q[self.window_rows(window)].contiguous()
        rows = q.shape[0]
        if planes:
            buf = _planes_buf(rows, D)
            pl = ops.Planes(rows, D, DEV, buf=buf)
            assert ops.attention(q, k, v, pl, self.L, self.nseq, self.heads, mode=mode, to_gemm=True, window=window, **self.kw) is pl
            assert bool((buf[3 * rows * D:] == PLANE_PAT).all()), "a write behind the three planes"
            return pl, buf
        buf = _sent(rows + 1, D + 4)
        ops.attention(q, k, v, buf[:rows, :D], self.L, self.nseq, self.heads, mode=mode, window=window, **self.kw)
        assert _all_sent(buf[rows:]) and _all_sent(buf[:, D:]), "a write outside the rows x D window"
        return buf[:rows, :D], buf


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("L,nseq,heads,bias", ATTN_CASES)
def test_attention_race(tuner, L, nseq, heads, bias, precision):
    ops = tuner.ops
    ops.set_precision("split3")              # a planes output needs the split path to be the active one (the fixture puts it back)
    c = AttnCall(ops, L, nseq, heads, bias, precision)
    races = nseq * heads * L >= 4096
    want, _ = c.run(mode=0)
    err = float((want.cpu().double() - c.ref).abs().max())
    print(f"[dispatch] attention L={L} nseq={nseq} heads={heads} bias={int(bias)} {precision}: worst |err| vs fp64 {err:.3e}")
    assert err < 2e-5, err
    # inside a profile window: one launch, no entry (attention takes no event slot: no record either)
    ops.profile_begin(4)
    i0 = tuner.mark()
    got, _ = c.run()
    assert ops.profile_end() == [] and tuner.kernels(i0) == ["sgic_attention_f32"] and not ops._TILE and not ops._DIRTY and _eq(got, want)
    # the cold call, fp32 output then planes output (each from empty tables)
    for planes in (False, True):
        _clear(ops)
        i0 = tuner.mark()
        got, _ = c.run(planes=planes)
        launches = tuner.kernels(i0)
        tuner.tuning += len(launches) - 1
        assert set(launches) == {"sgic_attention_split3_f32" if planes else "sgic_attention_f32"}
        same = (lambda g: torch.equal(g.rowmajor(), ops.split3(want.contiguous()))) if planes else (lambda g: _eq(g, want))
        assert same(got), ("the cold call differs from the mode=0 launch", planes)
        if not races:
            assert len(launches) == 1 and not ops._TILE and not ops._DIRTY
            continue
        assert len(launches) > len(ops.ATTN_MODES) and list(ops._TILE) == [c.key] and ops._TILE[c.key] in ops.ATTN_MODES and ops._DIRTY
        i0 = tuner.mark()
        got, _ = c.run(planes=planes)
        assert len(tuner.kernels(i0)) == 1 and same(got)
    assert tuner.races == []                 # attention races inline, not through _tune


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("L,nseq,heads,bias", ATTN_CASES[:3])
def test_attention_window_has_its_own_entry(tuner, L, nseq, heads, bias, precision):
    ops = tuner.ops
    c = AttnCall(ops, L, nseq, heads, bias, precision)
    window = ATTN_WINDOWS[L]
    full, _ = c.run()
    assert list(ops._TILE) == [c.key]
    i0 = tuner.mark()
    got, _ = c.run(window=window)
    launches = tuner.kernels(i0)
    tuner.tuning += len(launches) - 1
    # the full call's pick is not reused: the window launch races under its own key
    assert set(launches) == {"sgic_attention_window_f32"} and len(launches) > len(ops.ATTN_MODES)
    assert set(ops._TILE) == {c.key, c.key + window} and ops._TILE[c.key + window] in ops.ATTN_MODES
    assert _eq(got, full[c.window_rows(window)]), "a window row differs from the full call's row"
    i0 = tuner.mark()
    got, _ = c.run(window=window)
    assert len(tuner.kernels(i0)) == 1 and _eq(got, full[c.window_rows(window)])


# ---- g. round trip through the cache file -----------------------------------------------------------------------------------------
def test_picks_round_trip_through_the_cache_file(tuner, tmp_path):
    ops = tuner.ops
    intree = open(ops._INTREE_CACHE, "rb").read()
    calls = [GemmCall(ops, 256, 256, 96, "inplace_slice", "split3"), GemmCall(ops, 257, 260, 160, "bias_gelu", "f32"),
             GemmCall(ops, 2304, 512, 64, "plain", "split3")]
    wants = [c.forced() for c in calls]
    for c, want in zip(calls, wants):
        got, _ = c.run()
        assert _eq(got, want)
    att = AttnCall(ops, 64, 8, 8, False, "f32")
    att_want, _ = att.run(mode=0)
    att.run()
    picks = {k: ops._TILE[k] for k in [c.key for c in calls] + [att.key]}
    assert len(ops._TILE) == 4 and len(tuner.races) == 3
    borrowed = ("gemm3", 300, 256, 96, 1, 0)
    assert ops._lookup(borrowed) == picks[calls[0].key] and ops.tile_of((300, 256, 96, True, 0, "s3")) == picks[calls[0].key]
    path = ops.save_tile_cache()
    assert path == str(tmp_path / "cache.json") and not ops._DIRTY
    assert json.load(open(path))["picks"] == {"|".join(str(x) for x in k): m for k, m in picks.items()}     # measured picks only
    _clear(ops)
    ops._load_tile_cache()
    assert all(ops._TILE[k] == m for k, m in picks.items()) and borrowed not in ops._TILE and not ops._DIRTY
    for c, want in zip(calls, wants):
        i0 = tuner.mark()
        got, _ = c.run()
        assert tuner.kernels(i0) == [GEMM_SYM[c.precision]] and ops.LAST_TILE == picks[c.key] and _eq(got, want)
    i0 = tuner.mark()
    got, _ = att.run()
    assert len(tuner.kernels(i0)) == 1 and _eq(got, att_want)
    assert len(tuner.races) == 3 and not ops._DIRTY and ops.save_tile_cache() is None
    assert open(ops._INTREE_CACHE, "rb").read() == intree
