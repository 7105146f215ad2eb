"""Thin Python wrappers over the transform kernels of libsgic (C ABI, include/sgic.h).  Tensors are torch
CUDA tensors used purely as device-memory handles; all arithmetic happens in the HIP kernels."""
import ctypes
import json
import math
import os

import numpy as np
import torch

from ._lib import call, check, launch_opts, lib, require_gpu

ACT_NONE, ACT_GELU, ACT_SILU, ACT_TANH, ACT_LRELU = 0, 1, 2, 3, 4

# Optional live profiling of the dominant kernel (bench.py): while a window is open every GEMM / conv launch carries
# the profiler handle in its sgic_launch_opts, so its dispatch is timed by its own event pair, and (flops, shape key)
# is appended to PROFILE.  Host-side state of the launching thread (one process per GPU, one launching thread).
PROFILE = None
_PROFILER = None


def _profiler():
    global _PROFILER
    if _PROFILER is None:
        h = ctypes.c_void_p(0)
        check(lib.sgic_profiler_create(ctypes.byref(h)), "sgic_profiler_create")
        _PROFILER = h
    return _PROFILER


def profile_begin(max_launches=8192):
    """open a profile window: every GEMM / conv launch from now on is timed by its own dispatch (sgic_profiler_begin)"""
    global PROFILE
    finalize_autotune()
    check(lib.sgic_profiler_begin(_profiler(), int(max_launches)), "sgic_profiler_begin")
    PROFILE = []
    del PROFILE_TILES[:]


def profile_end():
    """close the window -> list of (flops, milliseconds, shape key) per launch, in launch order"""
    global PROFILE
    if PROFILE is None:
        raise RuntimeError("profile_end() without an open profile window")
    recs, PROFILE = PROFILE, None
    buf = (ctypes.c_float * max(1, len(recs)))()
    n = ctypes.c_int(0)
    check(lib.sgic_profiler_end(_profiler(), buf, len(recs), ctypes.byref(n)), "sgic_profiler_end")
    if n.value != len(recs):
        raise RuntimeError(f"profile window: {len(recs)} launches recorded on the host, {n.value} timed on the device")
    return [(fl, float(buf[i]), key) for i, (fl, key) in enumerate(recs)]


def _opts(tile=0, attn=0, prof=None, w_packed=0, a_packed=0):
    """prof: an explicit profiler handle (the tuner's probes); default: the bench's window when one is open"""
    return launch_opts(tile, attn, prof if prof is not None else (_PROFILER if PROFILE is not None else None), w_packed, a_packed)


def _rows(t):
    """a 2-D fp32 CUDA view whose last dim is contiguous -> (tensor, leading dimension)"""
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32 and t.is_cuda, (t.shape, t.stride(), t.dtype)
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))   # a 1-row view may carry any stride


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _cl(v):
    return ctypes.c_long(int(v))


def empty(*shape, like=None, dtype=torch.float32, device=None):
    return torch.empty(*shape, dtype=dtype, device=like.device if like is not None else device)


# Per-shape launch-mode autotuning ("measure, don't guess"): the first time a GEMM / conv / attention shape is seen and
# neither the tile cache nor a neighbouring M of the same (N, K, epilogue) family knows it, every launch mode of the
# kernel is timed with HIP events on the launch stream and the fastest is remembered.  All modes give bitwise identical
# results (the k order is fixed), so tuning never changes an output; the mode travels PER CALL in sgic_launch_opts (the
# library has no global launch state).  Picks persist in a JSON tile cache, so a second process -- or a new image
# geometry whose GEMMs only differ in M -- does not race again:
#   1. the in-tree cache  sgic_amd/tile_cache_gfx950.json  (committed; measured on an MI355X),
#   2. the user cache     $SGIC_TILE_CACHE or ~/.cache/sgic_amd/tile_cache_gfx950.json  (read after 1, written by
#      save_tile_cache(); bench.py and the CLI drivers call it at exit).
# AUTOTUNE = False uses the cache / built-in heuristic only.  Single-threaded by design (one launching thread).
AUTOTUNE = True
TUNE_MODES = (1, 2, 3, 4, 5, 7, 9, 10, 11, 12, 13, 14, 15)   # {128x128, 128x64} x {double, single LDS buffer}, staggered wide, mixed 128x128 + 64x64 tail, persistent (plain, mixed), 64x64, 16x16x4 latency kernel
ATTN_MODES = (1, 2, 3, 4, 5, 6, 7)                         # {single, double}-buffered K/V ring x start-up stagger {0, 4096, 8192} cycles; 7 = three row blocks per workgroup
_TILE = {}        # key -> mode (exact shapes)
_FAMILY = {}      # key without M -> {M: mode}
_DIRTY = False
_INTREE_CACHE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tile_cache_gfx950.json")


def _user_cache_path():
    return os.environ.get("SGIC_TILE_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "sgic_amd", "tile_cache_gfx950.json")


def _remember(key, mode, dirty=True):
    global _DIRTY
    _TILE[key] = mode
    _FAMILY.setdefault((key[0],) + tuple(key[2:]), {})[key[1]] = mode
    _DIRTY = _DIRTY or dirty


_MAX_MODE = {"gemm": 15, "conv3x3": 15, "gemm3": 32, "conv3": 32, "attn": 7, "attn3": 7}   # per kind of key


def _load_tile_cache():
    for path in (_INTREE_CACHE, _user_cache_path()):
        try:
            with open(path) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        for k, mode in d.get("picks", {}).items():
            parts = k.split("|")
            try:
                key = (parts[0],) + tuple(int(x) for x in parts[1:])
                mode = int(mode)
            except ValueError:
                continue
            # a cache written by another build may hold modes this library does not have: such a pick is dropped (re-raced)
            if not 0 <= mode <= _MAX_MODE.get(parts[0], -1):
                continue
            _remember(key, mode, dirty=False)


def save_tile_cache(path=None):
    """persist the picks of this process (merged over what the file already holds); atomic replace"""
    global _DIRTY
    if not _DIRTY and path is None:
        return None
    finalize_autotune()
    path = path or _user_cache_path()
    picks = {}
    try:
        with open(path) as f:
            picks = json.load(f).get("picks", {})
    except (OSError, ValueError):
        pass
    # measured picks only: _remember enters a measurement into its family as well, _lookup leaves a borrowed pick in _TILE alone
    picks.update({"|".join(str(int(x)) if not isinstance(x, str) else x for x in k): int(v) for k, v in _TILE.items()
                  if k[1] in _FAMILY.get((k[0],) + tuple(k[2:]), ())})
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump({"device": "gfx950", "format": "kind|M|...: launch mode (sgic_launch_opts)", "picks": dict(sorted(picks.items()))}, f, indent=0)
        os.replace(tmp, path)
    except OSError:
        return None
    _DIRTY = False
    return path


def _lookup(key):
    """exact pick, else the pick of the nearest M (within 2x) of the same (N, K, epilogue) family, else None"""
    m = _TILE.get(key)
    if m is not None:
        return m
    fam = _FAMILY.get((key[0],) + tuple(key[2:]))
    if fam:
        M = key[1]
        near = min(fam, key=lambda x: abs(x - M))
        if M <= 2 * near and near <= 2 * M:
            _TILE[key] = fam[near]          # a borrowed pick, not a measurement: tile_of reports it, save_tile_cache leaves it out
            return fam[near]
    return None


def tile_of(key, dev=None):
    """launch mode in use for a profile-record shape key (bench.py's by_shape table)"""
    if key and key[0] == "batched":
        return 0
    if key and key[0] in ("conv3x3", "conv3"):
        return _TILE.get(key)
    M, N, K, res, act = key[:5]
    kind = "gemm3" if len(key) > 5 and key[5] == "s3" else "gemm"
    return _TILE.get((kind, M, N, K, int(bool(res)), act))


_load_tile_cache()


def _save_at_exit():
    """every entry point (CLIs, service, tools, bench) leaves its new measurements behind for the next process"""
    try:
        if _DIRTY:
            save_tile_cache()
    except Exception:   # noqa: BLE001 -- never turn a clean exit into a failing one
        pass


import atexit  # noqa: E402

atexit.register(_save_at_exit)


_TUNE_PROF = None


def _tune_profiler():
    """a profiler handle of the tuner's own (the bench's window must not see the probes)"""
    global _TUNE_PROF
    if _TUNE_PROF is None:
        h = ctypes.c_void_p(0)
        check(lib.sgic_profiler_create(ctypes.byref(h)), "sgic_profiler_create")
        _TUNE_PROF = h
    return _TUNE_PROF


def _tune(key, launch, modes=None):
    """two interleaved passes over the modes, best-of per mode: a single short sample mis-ranks modes that are within
    a few percent of each other (clock ramp, cold L2 after the previous mode's different tile walk).
    Short launches are timed by the DISPATCH's own timestamps (sgic_profiler: hipExtLaunchKernel start / stop events), i.e.
    the kernel's duration alone: host-side event pairs around Python-issued launches cannot rank kernels shorter than the
    ~13 us a launch costs on the host, which is every GEMM of a single-image request."""
    prof = _tune_profiler()
    modes = TUNE_MODES if modes is None else modes
    reps = 3
    times = {}
    for _ in range(2):
        if M_big(key):
            # launches of >= ~50 us: host-side event pairs around four back-to-back launches, which also charge a mode for
            # what it costs BETWEEN kernels (the ramp of 512 persistent workgroups, the drain); measured better in the model
            for mode in modes:
                launch(mode)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(4):
                    launch(mode)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1)
                times[mode] = min(t, times.get(mode, t))
            continue
        check(lib.sgic_profiler_begin(prof, len(modes) * reps), "sgic_profiler_begin")
        for mode in modes:
            launch(mode)                               # warm, untimed
            for _ in range(reps):
                launch(mode, prof)
        buf = (ctypes.c_float * (len(modes) * reps))()
        n = ctypes.c_int(0)
        check(lib.sgic_profiler_end(prof, buf, len(modes) * reps, ctypes.byref(n)), "sgic_profiler_end")
        if n.value != len(modes) * reps:
            raise RuntimeError(f"tile tuner: {n.value} timed launches, expected {len(modes) * reps}")
        for i, mode in enumerate(modes):
            t = min(buf[i * reps + r] for r in range(reps))
            times[mode] = min(t, times.get(mode, t))
    order = sorted(times, key=times.get)
    best = order[0]
    _remember(key, best)
    # second stage, in context: the leaders of the isolated race (within 6 % of the best) are re-timed on the next real
    # occurrences of this shape, i.e. with the caches in the state the surrounding kernels leave them in
    cands = [m for m in order[:CTX_CANDS] if times[m] <= 1.06 * times[best]]
    if CTX_REPS > 0 and len(cands) > 1 and M_big(key):
        _CTX[key] = {"cands": cands, "t": {m: [] for m in cands}, "i": 0}
    return best


CTX_CANDS, CTX_REPS = 3, 2
_CTX = {}


def M_big(key):
    """in-context re-timing synchronises the stream once per sample: only worth it for launches of >= ~50 us"""
    if key[0] in ("conv3x3", "conv3"):
        return True
    return 2.0 * key[1] * key[2] * key[3] >= 5e9


def _ctx_launch(key, launch):
    """one in-context sample of the next candidate mode; picks the winner when every candidate has CTX_REPS samples"""
    c = _CTX[key]
    mode = c["cands"][c["i"] % len(c["cands"])]
    c["i"] += 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch(mode)
    e1.record()
    e1.synchronize()
    c["t"][mode].append(e0.elapsed_time(e1))
    if c["i"] >= len(c["cands"]) * CTX_REPS:
        _remember(key, min(c["cands"], key=lambda m: min(c["t"][m])))
        del _CTX[key]


def finalize_autotune():
    """close every pending in-context race with the samples it has (call before a timed region)"""
    for key in list(_CTX):
        c = _CTX.pop(key)
        done = [m for m in c["cands"] if c["t"][m]]
        if done:
            _remember(key, min(done, key=lambda m: min(c["t"][m])))


def _pick_and_launch(key, launch, big_enough, restore=None, modes=None):
    """shared tile-mode policy of gemm() / conv3x3(): cache -> family neighbour -> race (outside profile windows) -> heuristic.
    Returns True when the launch was already done by an in-context sample."""
    tile = 0
    if big_enough:
        tile = _lookup(key)
        if tile is None:
            if not AUTOTUNE or PROFILE is not None:
                tile = 0      # never tune inside a profile window (its probes would take event slots): built-in heuristic
            elif restore is not None:
                # in-place residual GEMMs (out is residual) are not idempotent: save / restore the buffer around tuning
                saved = restore.clone()
                tile = _tune(key, launch, modes)
                restore.copy_(saved)
            else:
                tile = _tune(key, launch, modes)
        elif key in _CTX and PROFILE is None:
            _ctx_launch(key, launch)
            return True
    global LAST_TILE
    LAST_TILE = tile
    launch(tile)
    return False


LAST_TILE = 0          # launch mode of the most recent _pick_and_launch (0 = the library's heuristic)
PROFILE_TILES = []     # launch mode actually used by each record of the current / last profile window (tools/pmc_by_shape.py)


# ---- GEMM arithmetic: "f32" = the exact-fp32 MFMA (csrc/gemm.hip), "split3" = fp32-accurate bf16x3 split on the bf16 matrix
# pipe (csrc/gemm_split.hip).  A process-level choice (SGIC_GEMM or set_precision): which kernel family a GEMM takes may
# depend on (N, K) and on the operands' kinds, never on M, so single-image and batched requests stay bitwise identical.
PRECISION = os.environ.get("SGIC_GEMM", "split3")
assert PRECISION in ("f32", "split3"), f"SGIC_GEMM={PRECISION!r}: expected f32 or split3"
SPLIT3_MODES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32)
SPLIT3_RING_MODES = (18, 19, 20, 21, 22, 23, 24, 25)   # small tiles, deep LDS-DMA ring: raced only for launches that cannot fill the chip (_split3_modes)
SPLIT3_SMALL_M = 2048


def _split3_modes(M):
    """candidate launch modes of a split GEMM with M rows: the ring kernel's 32..80-row tiles are for single-image sized launches"""
    return SPLIT3_MODES if M <= SPLIT3_SMALL_M else tuple(m for m in SPLIT3_MODES if m not in SPLIT3_RING_MODES)


_W3 = {}          # (data_ptr, N, K, ldw, version) -> (planes, w): the weight is pinned so its address cannot be reused
_W3_BYTES = 0
_W3_LIMIT = 24 << 30
_A3_WS = {}       # (device, stream) -> workspace for the activation planes


def set_precision(p):
    global PRECISION
    assert p in ("f32", "split3"), p
    PRECISION = p


class Planes:
    """an activation held as bf16x3 planes (int16 bit patterns) in the slice-major layout [3, cols / 32, rows, 32] (csrc/split3.h):
    the A operand of a split GEMM written directly by its producer (layernorm / attention / gemm epilogue / split3_planes), so no
    fp32 copy and no separate split pass exists"""
    __slots__ = ("t", "rows", "cols")

    def __init__(self, rows, cols, device, buf=None):
        n = 3 * rows * cols
        if buf is not None and buf.numel() >= n:
            self.t = buf
        else:
            self.t = torch.empty(n, device=device, dtype=torch.int16)
        self.rows, self.cols = rows, cols

    @property
    def shape(self):
        return (self.rows, self.cols)

    @property
    def device(self):
        return self.t.device

    def rowmajor(self):
        """the planes as a [3, rows, cols] tensor (tests / debugging): what ops.split3 returns for the same values"""
        p = self.t[:3 * self.rows * self.cols].view(3, self.cols // 32, self.rows, 32)
        return p.permute(0, 2, 1, 3).reshape(3, self.rows, self.cols)

    def float(self):
        """the fp32 values (tests / debugging): the sum of the three planes"""
        p = self.rowmajor()
        f = lambda q: (q.to(torch.int32) << 16).view(torch.float32)
        return (f(p[0]) + f(p[1])) + f(p[2])


def planes_ok(cols, precision=None):
    """may a producer hand its [rows, cols] output to the next GEMM as planes?"""
    return (precision or PRECISION) == "split3" and cols % 32 == 0


def split3(x, ld=None, rows=None, seg=(0, 0), out=None):
    """x[rows, cols] fp32 -> planes [3, rows, cols] (uint16 = bf16 bit patterns), x = p0 + p1 + p2 exactly"""
    x, ldx = _rows(x)
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1]
    if out is None:
        out = torch.empty(3, rows, cols, device=x.device, dtype=torch.int16)
    call("sgic_split3_f32", _p(x), ldx if ld is None else ld, rows, cols, seg[0], seg[1], _p(out))
    return out


def split3_planes(x, out=None):
    """x[rows, cols] fp32 -> a Planes object (slice-major layout): a pre-split A operand for gemm()"""
    x, ldx = _rows(x)
    rows, cols = x.shape
    assert cols % 32 == 0
    pl = out if isinstance(out, Planes) and out.shape == (rows, cols) else Planes(rows, cols, x.device)
    call("sgic_split3_pack_f32", _p(x), ldx, rows, cols, _p(pl.t))
    return pl


def weight_planes(w, ldw):
    """bf16x3 planes of a constant operand, split once (keyed by address + in-place version), in the slice-major layout
    [3][K / 32][N][32] of sgic_split3_pack_f32: consumers pass w_packed=1 (sgic_launch_opts)"""
    global _W3_BYTES
    N, K = w.shape
    key = (w.data_ptr(), N, K, ldw, w._version)
    hit = _W3.get(key)
    if hit is None:
        planes = torch.empty(3, N, K, device=w.device, dtype=torch.int16)
        call("sgic_split3_pack_f32", _p(w), ldw, N, K, _p(planes))
        nbytes = planes.numel() * 2
        while _W3 and _W3_BYTES + nbytes > _W3_LIMIT:      # oldest first
            old = next(iter(_W3))
            _W3_BYTES -= _W3.pop(old)[0].numel() * 2
        _W3[key] = hit = (planes, w)
        _W3_BYTES += nbytes
    return hit[0]


def _a3_workspace(dev, n_u16):
    key = (dev, _stream_key())
    ws = _A3_WS.get(key)
    if ws is None or ws.numel() < n_u16:
        ws = torch.empty(max(n_u16, 1 << 24), device=dev, dtype=torch.int16)
        _A3_WS[key] = ws
    return ws


def _stream_key():
    from ._lib import stream
    return stream().value


def gemm(a, w, bias=None, residual=None, act=ACT_NONE, out=None, M=None, a_seg=(0, 0), c_seg=(0, 0), tile=None, w_const=True,
         precision=None, to_gemm=False):
    """out[M,N] = act(a[M,K] @ w[N,K]^T + bias) + residual.  a_seg/c_seg = (seg, seg_stride) row maps:
    logical row m of A (resp. C) lives at physical row (m // seg) * seg_stride + m % seg.
    tile: force a launch mode (tests / tools); default = cache / autotuner.
    w_const: w is a constant (a model weight): under PRECISION == "split3" its bf16x3 planes are cached.  A `w` whose contents
    change between calls (the search index) must pass False and takes the fp32 MFMA kernel.
    a may be a Planes object (written by a producer called with to_gemm=True).  to_gemm=True: the result feeds only another
    GEMM as its A operand -> returned as Planes when the split path is active (else the fp32 tensor as always); `out` may
    then be a Planes object to reuse."""
    require_gpu()
    a_planes = a if isinstance(a, Planes) else None
    if a_planes is not None:
        K, lda = a_planes.cols, a_planes.cols
        assert a_seg[0] == 0 and (M is None or M == a_planes.rows)
        M = a_planes.rows
        dev = a_planes.device
    else:
        a, lda = _rows(a)
        K = a.shape[1]
        if M is None:
            M = a.shape[0]
        dev = a.device
    w, ldw = _rows(w)
    N = w.shape[0]
    assert w.shape[1] == K, ((M, K), w.shape)
    use3 = (precision or PRECISION) == "split3" and w_const and K % 32 == 0
    assert a_planes is None or use3, "a Planes operand needs the split path"
    out_planes = None
    if to_gemm and use3 and N % 32 == 0 and c_seg[0] == 0:
        out_planes = out if isinstance(out, Planes) and out.shape == (M, N) else Planes(M, N, dev, buf=out.t if isinstance(out, Planes) else None)
        out, ldc = None, N
    else:
        if isinstance(out, Planes):
            out = None
        if out is None:
            assert c_seg[0] == 0
            out = torch.empty(M, N, device=dev, dtype=torch.float32)
        out, ldc = _rows(out)
        assert out.shape[1] == N
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(residual)
        assert residual.shape[1] == N and residual.shape[0] >= M
    if bias is not None:
        assert bias.shape == (N,) and bias.is_contiguous()
    inplace = residual is not None and out is not None and out.data_ptr() == residual.data_ptr()
    # the kernels read the residual by logical row and write the output through c_seg: in place these are the same rows only
    # within the first segment -- beyond it a launch would read rows that other workgroups of the same launch write
    assert not (inplace and c_seg[0] and M > c_seg[0]), "gemm: in-place residual through a c_seg row map of more than one segment"

    if use3:
        wp = weight_planes(w, ldw)
        ap = a_planes.t if a_planes is not None else _a3_workspace(dev, 3 * M * K)
        a_f32 = None if a_planes is not None else a
        cp = out_planes.t if out_planes is not None else None

        def launch3(mode, prof=None):
            call("sgic_gemm_split3_f32", _p(a_f32), lda, a_seg[0], a_seg[1], _p(ap), _p(wp), _p(bias), _p(residual), ldr, _p(out), ldc,
                 _p(cp), M, N, K, act, c_seg[0], c_seg[1], _opts(tile=mode, prof=prof, w_packed=1, a_packed=1))

        if tile is not None:
            launch3(tile)
        else:
            key = ("gemm3", M, N, K, int(residual is not None), act)
            if _pick_and_launch(key, launch3, M * N >= (1 << 16), restore=out if inplace else None, modes=_split3_modes(M)):
                return out_planes if out_planes is not None else out
        if PROFILE is not None:
            PROFILE.append((2.0 * M * N * K, (M, N, K, residual is not None, act, "s3")))
            PROFILE_TILES.append(tile if tile is not None else LAST_TILE)
        return out_planes if out_planes is not None else out

    def launch(mode, prof=None):
        call("sgic_gemm_f32", _p(a), lda, _p(w), ldw, _p(bias), _p(residual), ldr, _p(out), ldc, M, N, K, act,
             a_seg[0], a_seg[1], c_seg[0], c_seg[1], _opts(tile=mode, prof=prof))

    if tile is not None:
        launch(tile)
    else:
        key = ("gemm", M, N, K, int(residual is not None), act)
        if _pick_and_launch(key, launch, M * N >= (1 << 16), restore=out if inplace else None):
            return out
    if PROFILE is not None:   # the launch took the next event pair of the open profile window (profile_begin)
        PROFILE.append((2.0 * M * N * K, (M, N, K, residual is not None, act)))
        PROFILE_TILES.append(tile if tile is not None else LAST_TILE)
    return out


def layernorm(x, gamma, beta, out=None, eps=1e-5, act=ACT_NONE, M=None, x_seg=(0, 0), y_seg=(0, 0), to_gemm=False):
    """to_gemm=True: the output feeds only a GEMM as its A operand -> written directly as bf16x3 Planes when the split path is
    active and the width allows it (`out` may be a Planes object to reuse); otherwise the fp32 tensor as always."""
    x, ldx = _rows(x)
    C = x.shape[1]
    if M is None:
        M = x.shape[0]
    assert gamma.shape == (C,) and beta.shape == (C,)
    if to_gemm and planes_ok(C) and C % 256 == 0 and C <= 2048 and y_seg[0] == 0:
        pl = out if isinstance(out, Planes) and out.shape == (M, C) else Planes(M, C, x.device, buf=out.t if isinstance(out, Planes) else None)
        call("sgic_layernorm_split3_f32", _p(x), ldx, x_seg[0], x_seg[1], _p(gamma), _p(beta), _p(pl.t), M, C, float(eps), act)
        return pl
    if isinstance(out, Planes):
        out = None
    if out is None:
        assert y_seg[0] == 0
        out = torch.empty(M, C, device=x.device, dtype=torch.float32)
    out, ldy = _rows(out)
    call("sgic_layernorm_f32", _p(x), ldx, x_seg[0], x_seg[1], _p(gamma), _p(beta), _p(out), ldy, y_seg[0], y_seg[1],
         M, C, float(eps), act)
    return out


def attention(q, k, v, out, L, nseq, nheads, rowmap=None, bias=None, biasvar=None, scale=0.125, mode=None, to_gemm=False, precision=None,
              window=None):
    """q,k,v,out: 2-D row-strided views (rows x nheads*64).  mode: force attn_mode (tests / tools).
    to_gemm=True: the output feeds only the out-projection GEMM -> written as bf16x3 Planes over q's row space when the split
    path is active (`out` may be None or a Planes object to reuse); otherwise into the fp32 `out` as always.
    window=(q_tok0, Lq): only the query tokens q_tok0 .. q_tok0+Lq-1 of every sequence (sgic_attention_window_f32): q and out
    hold Lq rows per sequence, k and v all L; every row is bitwise what the full call gives for that token."""
    q, ldq = _rows(q)
    k, ldk = _rows(k)
    v, ldv = _rows(v)
    D = nheads * 64
    pl = None
    if to_gemm and planes_ok(D):
        rows = q.shape[0]
        pl = out if isinstance(out, Planes) and out.shape == (rows, D) else Planes(rows, D, q.device, buf=out.t if isinstance(out, Planes) else None)
    else:
        if out is None or isinstance(out, Planes):
            out = torch.empty(q.shape[0], D, device=q.device, dtype=torch.float32)
        out, ldo = _rows(out)
    if rowmap is not None:
        assert rowmap.dtype == torch.int32 and rowmap.numel() == nseq * L and rowmap.is_contiguous()
    q_tok0, Lq = window if window is not None else (0, 0)
    if window is not None:
        assert Lq > 0 and q.shape[0] >= nseq * Lq and (pl is not None or out.shape[0] >= nseq * Lq), (window, q.shape)
    win = "_window" if window is not None else ""
    wargs = (int(q_tok0), int(Lq)) if window is not None else ()
    if bias is not None:
        assert bias.dim() == 3 and bias.shape[1] == L and bias.shape[2] == L and bias.is_contiguous()
    if biasvar is not None:
        assert biasvar.dtype == torch.int32 and biasvar.numel() == nseq

    s3 = 8 if (precision or PRECISION) == "split3" else 0     # attn_mode bit 3: S^T = K Q^T as a bf16x3 split product

    def launch(m):
        if pl is not None:
            call(f"sgic_attention{win}_split3_f32", _p(q), ldq, _p(k), ldk, _p(v), ldv, _p(pl.t), ctypes.c_long(pl.rows), L, nseq, nheads,
                 _p(rowmap), _p(bias), _p(biasvar), float(scale), *wargs, launch_opts(0, m | s3, None))
        else:
            call(f"sgic_attention{win}_f32", _p(q), ldq, _p(k), ldk, _p(v), ldv, _p(out), ldo, L, nseq, nheads, _p(rowmap), _p(bias),
                 _p(biasvar), float(scale), *wargs, launch_opts(0, m | s3, None))

    # K/V ring depth (single buffer + more workgroups per CU vs double buffer + one barrier per tile) depends on L and
    # on how many workgroups the launch has -> tuned per shape like the GEMM tiles; results are identical.
    if mode is None:
        mode = 0
        if nseq * nheads * L >= 4096:
            # a window launch has its own item list (a few row blocks per unit): its own entries, never a full launch's
            key = ("attn3" if s3 else "attn", nseq, L, nheads, int(bias is not None)) + wargs
            mode = _lookup(key)
            if mode is None:
                mode = 0
                if AUTOTUNE and PROFILE is None:
                    best_t = None
                    for cand in ATTN_MODES:
                        launch(cand)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(3):
                            launch(cand)
                        e1.record()
                        e1.synchronize()
                        t = e0.elapsed_time(e1)
                        if best_t is None or t < best_t:
                            mode, best_t = cand, t
                    _remember(key, mode)
    launch(mode)
    return pl if pl is not None else out


def copy_row_blocks(x, rows, stride_rows, nblocks, out=None):
    """out[(i, r)] = x[i*stride_rows + r], r < rows, i < nblocks: an exact strided device copy (keeps -0.0, NaN payloads)"""
    x, ldx = _rows(x)
    C = x.shape[1]
    assert ldx == C and stride_rows >= rows and x.shape[0] >= (nblocks - 1) * stride_rows + rows, (x.shape, rows, stride_rows, nblocks)
    if out is None:
        out = torch.empty(nblocks * rows, C, device=x.device, dtype=torch.float32)
    assert out.is_contiguous() and out.shape == (nblocks * rows, C)
    call("sgic_copy_blocks_f32", _p(x), _cl(stride_rows * C), _p(out), _cl(rows * C), _cl(rows * C), nblocks)
    return out


def im2col_patch(x, P, mul=1.0, add=0.0, tile16=False, out=None):
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty(B * (H // P) * (W // P), C * P * P, device=x.device, dtype=torch.float32)
    call("sgic_im2col_patch", _p(x), B, C, H, W, P, float(mul), float(add), int(tile16), _p(out))
    return out


def assemble_tokens(emb, cls, pos, lat, latpos, N, P, T, D, out=None):
    if out is None:
        out = torch.empty(N * (1 + P + T), D, device=emb.device, dtype=torch.float32)
    call("sgic_assemble_tokens", _p(emb), _p(cls), _p(pos), _p(lat), _p(latpos), N, P, T, D, _p(out))
    return out


def add_rows_bcast(inp, iseg, vec, out, oseg, Nn, Lr):
    inp, ldi = _rows(inp)
    out, ldo = _rows(out)
    D = inp.shape[1]
    assert out.shape[1] == D
    if vec is not None:
        assert vec.is_contiguous() and vec.numel() == Lr * D
    call("sgic_add_rows_bcast", _p(inp), ldi, iseg, _p(vec), _p(out), ldo, oseg, Nn, Lr, D)
    return out


def dwconv(x, w_kkc, bias, prescale, B, H, W, k, tile16=False, out=None):
    """x: (B*H*W, C) rows; w_kkc: (k*k, C)"""
    x, ldx = _rows(x)
    C = x.shape[1]
    assert ldx == C and w_kkc.shape == (k * k, C) and w_kkc.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    call("sgic_dwconv_nhwc", _p(x), _p(w_kkc), _p(bias), _p(prescale), _p(out), B, H, W, C, k, int(tile16))
    return out


def im2col_2x2(x, B, H, W, tile16=False, out=None):
    x, ldx = _rows(x)
    C = x.shape[1]
    assert ldx == C
    if out is None:
        out = torch.empty(B * (H // 2) * (W // 2), 4 * C, device=x.device, dtype=torch.float32)
    call("sgic_im2col_2x2", _p(x), B, H, W, C, int(tile16), _p(out))
    return out


def gated_lrelu(x, out=None):
    x, ldx = _rows(x)
    M, C2x2 = x.shape
    assert ldx == C2x2
    if out is None:
        out = torch.empty(M, C2x2 // 2, device=x.device, dtype=torch.float32)
    call("sgic_gated_lrelu", _p(x), _p(out), M, C2x2 // 2)
    return out


def colop(x, v, mode, out=None):
    """mode 0: x * v ; mode 1: x / max(v, 0.5);  v: (vrows, C) broadcast with row m % vrows"""
    x, ldx = _rows(x)
    v, ldv = _rows(v)
    M, C = x.shape
    if out is None:
        out = torch.empty(M, C, device=x.device, dtype=torch.float32)
    out, ldy = _rows(out)
    call("sgic_colop", _p(x), ldx, _p(v), ldv, v.shape[0], _p(out), ldy, M, C, mode)
    return out


def fake2d_transpose(x_base, seq_stride, N, T, D):
    out = torch.empty(N * T, D, device=x_base.device, dtype=torch.float32)
    call("sgic_fake2d_transpose", _p(x_base), _cl(seq_stride), _p(out), N, T, D)
    return out


def vq_argmin(z, codebook, l2norm=True):
    z, ldz = _rows(z)
    M, dim = z.shape
    assert codebook.is_contiguous() and codebook.shape[1] == dim
    idx = torch.empty(M, dtype=torch.int32, device=z.device)
    call("sgic_vq_argmin", _p(z), ldz, _p(codebook), codebook.shape[0], dim, M, int(l2norm), _p(idx))
    return idx


def l2norm_u8(x):
    x, ldx = _rows(x)
    M, D = x.shape
    unit = torch.empty(M, D, device=x.device, dtype=torch.float32)
    q = torch.empty(M, D, device=x.device, dtype=torch.uint8)
    call("sgic_l2norm_u8", _p(x), ldx, M, D, _p(unit), _p(q))
    return unit, q


# ---- entropy-side kernels (device-resident batch API) ----
def quant_step(y, scales, means, ld_sm, yhat, ld_yhat, B, H, W, C, k, thr, sym, idx):
    call("sgic_quant_step", _p(y), _p(scales), _p(means), ld_sm, _p(yhat), ld_yhat, B, H, W, C, k,
         float(-1.0 if thr is None else thr), _p(sym), _p(idx))


def scale_indexes(scales_flat, idx_out, thr):
    call("sgic_scale_to_index", _p(scales_flat), _cl(scales_flat.numel()), float(-1.0 if thr is None else thr), _p(idx_out))


def index_step(scales, ld_sm, B, H, W, C, k, thr, idx):
    call("sgic_index_step", _p(scales), ld_sm, B, H, W, C, k, float(-1.0 if thr is None else thr), _p(idx))


def index_margins(scales, ld_sm, B, H, W, C, k, thr, margin, alt):
    call("sgic_index_margins", _p(scales), ld_sm, B, H, W, C, k, float(-1.0 if thr is None else thr), _p(margin), _p(alt))


def dequant_step(sym, means, ld_sm, yhat, ld_yhat, B, H, W, C, k):
    call("sgic_dequant_step", _p(sym), _p(means), ld_sm, _p(yhat), ld_yhat, B, H, W, C, k)


def rans_encode_batch(table, sym, idx, B, n, cap=None):
    """-> (out (B,cap) u8, off (B,) i32, len (B,) i32, err (B,) i32); streams are end-aligned in their slot"""
    if cap is None:
        cap = 2 * n + 64
    dev = sym.device
    out = torch.empty(B, cap, dtype=torch.uint8, device=dev)
    meta = torch.empty(3, B, dtype=torch.int32, device=dev)
    call("sgic_rans_encode_batch", table, _p(sym), _p(idx), B, n, _p(out), cap, _p(meta[0]), _p(meta[1]), _p(meta[2]))
    return out, meta


def pack12_batch(idx_i32, B, n):
    nb = lib.sgic_pack12_size(n)
    out = torch.empty(B, nb, dtype=torch.uint8, device=idx_i32.device)
    call("sgic_pack12_batch", _p(idx_i32), B, n, _p(out))
    return out


# ---- decode-side kernels ----
def gemm_batched(a, lda, sa, w, ldw, sw, out, ldc, sc, M, N, K, batch, bias=None, residual=None, ldr=0, sr=0, act=ACT_NONE):
    """batch of GEMMs on raw pointers/strides (elements); a, w, out, residual are tensors used as base pointers"""
    call("sgic_gemm_batched_f32", _p(a), lda, _cl(sa), _p(w), ldw, _cl(sw), _p(bias), _p(residual), ldr, _cl(sr), _p(out), ldc,
         _cl(sc), M, N, K, act, batch, _opts())
    if PROFILE is not None:
        PROFILE.append((2.0 * M * N * K * batch, ("batched", batch, M, N, K, residual is not None, act)))
        PROFILE_TILES.append(0)
    return out


class HaloPlanes:
    """the zero-halo input of a 3x3 convolution held as slice-major bf16x3 planes [3, C / 32, B (H+2) (W+2), 32] (int16 bit patterns),
    written directly by groupnorm / halo_copy when the convolution runs as an implicit split GEMM"""
    __slots__ = ("t", "B", "H", "W", "C")

    def __init__(self, t, B, H, W, C):
        self.t, self.B, self.H, self.W, self.C = t, B, H, W, C


_HALO3 = {}


def halo_planes_buffer(dev, B, H, W, C):
    """cached like halo_buffer: producers only write the interior, the border planes stay zero"""
    key = (str(dev), B, H, W, C)
    if key not in _HALO3:
        _HALO3[key] = HaloPlanes(torch.zeros(3 * B * (H + 2) * (W + 2) * C, device=dev, dtype=torch.int16), B, H, W, C)
    return _HALO3[key]


def conv_planes_ok(Cin, Cout, residual=False, precision=None):
    """does conv3x3 with these channels run as an implicit split GEMM (so its producer may write halo planes directly)?"""
    return (precision or PRECISION) == "split3" and Cin % 32 == 0 and not (Cout == 3 and Cin == 128 and not residual)


def conv3x3(x_halo, w, bias, B, H, W, Cin, Cout, residual=None, act=ACT_NONE, out=None, tile=None, precision=None):
    """x_halo: zero-halo NHWC buffer (B, H+2, W+2, Cin); w: (Cout, 9*Cin) in (ky,kx,cin) order -> (B*H*W, Cout)"""
    hp = x_halo if isinstance(x_halo, HaloPlanes) else None
    if hp is not None:
        assert (hp.B, hp.H, hp.W, hp.C) == (B, H, W, Cin) and conv_planes_ok(Cin, Cout, residual is not None, precision)
        dev = hp.t.device
    else:
        assert x_halo.is_contiguous() and x_halo.numel() == B * (H + 2) * (W + 2) * Cin
        dev = x_halo.device
    assert w.shape == (Cout, 9 * Cin) and w.is_contiguous()
    if out is None:
        out = torch.empty(B * H * W, Cout, device=dev, dtype=torch.float32)
    out, ldc = _rows(out)
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(residual)
        # the launch-mode race below runs the kernel many times over `out` and restores nothing (unlike gemm's in-place residual)
        o0, r0, M = out.data_ptr(), residual.data_ptr(), B * H * W
        assert o0 + ((M - 1) * ldc + Cout) * 4 <= r0 or r0 + ((M - 1) * ldr + Cout) * 4 <= o0, \
            "conv3x3: out overlaps residual -- an in-place residual is not idempotent and the launch-mode race does not restore out"

    if conv_planes_ok(Cin, Cout, residual is not None, precision):
        # implicit split GEMM: the weight's planes are cached; the halo planes come from the producer, or from one split pass
        # over the fp32 halo buffer's rows
        rows = B * (H + 2) * (W + 2)
        wp = weight_planes(w, 9 * Cin)
        if hp is not None:
            ws = hp.t
        else:
            ws = _a3_workspace(dev, 3 * rows * Cin)
            call("sgic_split3_pack_f32", _p(x_halo), Cin, rows, Cin, _p(ws))

        def launch3(mode, prof=None):
            call("sgic_conv3x3_split3_f32", _p(ws), _p(wp), _p(bias), _p(residual), ldr, _p(out), ldc, B, H, W, Cin, Cout, act,
                 _opts(tile=mode, prof=prof, w_packed=1, a_packed=1))

        if tile is not None:
            launch3(tile)
        else:
            key = ("conv3", B * H * W, H, W, Cin, Cout, int(residual is not None), act)
            if _pick_and_launch(key, launch3, B * H * W * Cout >= (1 << 20), modes=(1, 2, 3, 5, 10, 11, 14, 15, 16, 17, 30)):
                return out
        if PROFILE is not None:
            PROFILE.append((2.0 * B * H * W * Cout * 9 * Cin, (B * H * W, Cout, 9 * Cin, residual is not None, act, "s3", "conv")))
            PROFILE_TILES.append(tile if tile is not None else LAST_TILE)
        return out

    def launch(mode, prof=None):
        call("sgic_conv3x3_f32", _p(x_halo), _p(w), _p(bias), _p(residual), ldr, _p(out), ldc, B, H, W, Cin, Cout, act,
             _opts(tile=mode, prof=prof))

    if tile is not None:
        launch(tile)
    else:
        # key[1] = M = B*H*W so that a different batch of the same geometry borrows the pick (family lookup)
        key = ("conv3x3", B * H * W, H, W, Cin, Cout, int(residual is not None), act)
        if _pick_and_launch(key, launch, B * H * W * Cout >= (1 << 20)):   # conv outputs never alias their residual
            return out
    if PROFILE is not None:   # the implicit-GEMM convolution is the same kernel: M = B*H*W, N = Cout, K = 9*Cin
        PROFILE.append((2.0 * B * H * W * Cout * 9 * Cin, (B * H * W, Cout, 9 * Cin, residual is not None, act, "f32", "conv")))
        PROFILE_TILES.append(tile if tile is not None else LAST_TILE)
    return out


_GN_WS = {}


def groupnorm(x, gamma, beta, B, H, W, swish=True, halo=False, groups=32, eps=1e-6, out=None, to_conv=None):
    """x (B*H*W, C) plain NHWC -> normalised (+swish); halo=True writes the interior of a (B,H+2,W+2,C) buffer
    whose border must already be zero (pass `out`, or a fresh zero buffer is allocated)."""
    x, ldx = _rows(x)
    C = x.shape[1]
    assert ldx == C
    dev = x.device
    key = (str(dev), B, C, groups)     # the statistics buffer is sized by `groups`
    if key not in _GN_WS:
        _GN_WS[key] = (torch.empty(B * 64 * C * 2, dtype=torch.float64, device=dev),
                       torch.empty(B * groups * 2, dtype=torch.float32, device=dev))
    ws, stats = _GN_WS[key]
    if halo and to_conv is not None and conv_planes_ok(C, to_conv[0], to_conv[1]):
        # to_conv = (Cout, has_residual) of the 3x3 convolution that consumes this halo buffer: written as its operand planes
        hp = halo_planes_buffer(dev, B, H, W, C)
        call("sgic_groupnorm_nhwc_split3", _p(x), _p(gamma), _p(beta), B, H, W, C, groups, float(eps), int(swish), _p(ws), _p(stats),
             _p(hp.t))
        return hp
    if out is None:
        out = halo_buffer(dev, B, H, W, C) if halo else torch.empty(B * H * W, C, device=dev)
    call("sgic_groupnorm_nhwc", _p(x), _p(gamma), _p(beta), B, H, W, C, groups, float(eps), int(swish), int(halo), _p(ws),
         _p(stats), _p(out))
    return out


_HALO = {}


def halo_buffer(dev, B, H, W, C):
    """zero-halo NHWC buffer (B, H+2, W+2, C), cached per shape: producers only ever write the interior, so the
    border stays zero and no per-call memset is needed.  Uses are strictly sequential on one stream (a halo
    buffer is consumed by the conv right after it is produced)."""
    key = (str(dev), B, H, W, C)
    if key not in _HALO:
        _HALO[key] = torch.zeros(B, H + 2, W + 2, C, device=dev, dtype=torch.float32)
    return _HALO[key]


def halo_copy(x, B, H, W, C, upsample=False, tile16=False, out=None, to_conv=None):
    s = 2 if upsample else 1
    if to_conv is not None and conv_planes_ok(C, to_conv[0], to_conv[1]):
        hp = halo_planes_buffer(x.device, B, H * s, W * s, C)
        call("sgic_halo_copy_split3", _p(x), B, H, W, C, int(upsample), int(tile16), _p(hp.t))
        return hp
    if out is None:
        out = halo_buffer(x.device, B, H * s, W * s, C)
    call("sgic_halo_copy", _p(x), B, H, W, C, int(upsample), int(tile16), _p(out))
    return out


def softmax_rows(x, L, scale=1.0, out=None):
    assert x.is_contiguous()
    M = x.numel() // L
    if out is None:
        out = torch.empty_like(x)
    call("sgic_softmax_rows", _p(x), _p(out), _cl(M), L, float(scale))
    return out


def pixel_shuffle2_tm16(x, B, H, W, C):
    out = torch.empty(B * 4 * H * W, C, device=x.device, dtype=torch.float32)
    call("sgic_pixel_shuffle2_tm16", _p(x), B, H, W, C, _p(out))
    return out


def assemble_dec_tokens(emb, cls, mask, pos, latpos, N, P, T, D):
    out = torch.empty(N * (1 + P + T), D, device=emb.device, dtype=torch.float32)
    call("sgic_assemble_dec_tokens", _p(emb), _p(cls), _p(mask), _p(pos), _p(latpos), N, P, T, D, _p(out))
    return out


def codebook_gather_norm(idx, codebook, ld=None):
    M, dim = idx.numel(), codebook.shape[1]
    ld = ld or dim
    out = torch.empty(M, ld, device=idx.device, dtype=torch.float32)
    call("sgic_codebook_gather_norm", _p(idx), _p(codebook), M, dim, ld, _p(out))
    return out


def nhwc3_to_nchw_clamp(x, ld, B, H, W):
    out = torch.empty(B, 3, H, W, device=x.device, dtype=torch.float32)
    call("sgic_nhwc3_to_nchw_clamp", _p(x), ld, B, H, W, _p(out))
    return out


def rans_decode_init(streams, cap, off, ln, B):
    state = torch.zeros(B, 4, dtype=torch.int32, device=streams.device)
    call("sgic_rans_decode_init_batch", _p(streams), cap, _p(off), _p(ln), B, _p(state))
    return state


def rans_decode_step(table, streams, cap, off, ln, B, state, idx, n, idx_stride, out, out_stride):
    call("sgic_rans_decode_batch", table, _p(streams), cap, _p(off), _p(ln), B, _p(state), _p(idx), n, idx_stride, _p(out),
         out_stride)


def unpack12_batch(streams_u8, B, n):
    out = torch.empty(B, n, dtype=torch.int32, device=streams_u8.device)
    call("sgic_unpack12_batch", _p(streams_u8), B, n, _p(out))
    return out


def pad_replicate(x, pl, pr, pt, pb):
    """F.pad(x, (pl, pr, pt, pb), mode="replicate") for a contiguous (B, C, H, W) fp32 device tensor"""
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
    B, C, H, W = x.shape
    if pl == pr == pt == pb == 0:
        return x
    out = torch.empty(B, C, H + pt + pb, W + pl + pr, device=x.device, dtype=torch.float32)
    call("sgic_pad_replicate", _p(x), _p(out), B * C, H, W, int(pl), int(pr), int(pt), int(pb))
    return out


def u8hwc_to_f32chw_pad(x_u8, pl=0, pr=0, pt=0, pb=0):
    """(B,H,W,3) u8 device tensor -> (B,3,H+pt+pb,W+pl+pr) fp32 in [-1,1]: ToTensor, *2-1, replicate pad (compress.py:161-164,258-261)"""
    assert x_u8.dim() == 4 and x_u8.shape[3] == 3 and x_u8.dtype == torch.uint8 and x_u8.is_contiguous() and x_u8.is_cuda
    B, H, W, _ = x_u8.shape
    out = torch.empty(B, 3, H + pt + pb, W + pl + pr, device=x_u8.device, dtype=torch.float32)
    call("sgic_u8hwc_to_f32chw_pad", _p(x_u8), _p(out), B, H, W, int(pl), int(pr), int(pt), int(pb))
    return out


def u8canvas_to_f32chw_pad(x_u8, hw, OH, OW):
    """(B,Hc,Wc,3) u8 canvas on the device, image b at its top left with extent hw[b] = (h, w) -> (B,3,OH,OW) fp32 in [-1,1]: ToTensor,
    *2-1, replicate pad from each image's own right / bottom edge (bit-identical per image to u8hwc_to_f32chw_pad on it alone)"""
    assert x_u8.dim() == 4 and x_u8.shape[3] == 3 and x_u8.dtype == torch.uint8 and x_u8.is_contiguous() and x_u8.is_cuda
    B, Hc, Wc, _ = x_u8.shape
    hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(B, 2)
    out = torch.empty(B, 3, int(OH), int(OW), device=x_u8.device, dtype=torch.float32)
    call("sgic_u8canvas_to_f32chw_pad", _p(x_u8), hw, _p(out), B, Hc, Wc, int(OH), int(OW))
    return out


def _clip_preprocess(entry, src, geo, S, mean, std, device):
    """the call both CLIP preprocessing routes make: `entry`(*src, B, geo, S, mean, std, workspace, its size, out), the workspace
    sized by `entry`_workspace"""
    B, S = len(geo), int(S)
    geo = np.ascontiguousarray(geo, dtype=np.int32).reshape(B, 6)
    mean, std = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (mean, std))
    nbytes = ctypes.c_size_t(0)
    call(entry + "_workspace", B, geo, S, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    out = torch.empty(B, 3, S, S, dtype=torch.float32, device=device)
    call(entry, *src, B, geo, S, mean, std, _p(work), ctypes.c_size_t(nbytes.value), _p(out))
    return out


def clip_preprocess_ragged(x, geo, S, mean, std):
    """(B,3,Hp,Wp) fp32 in [-1,1] on the device (any batch / channel / row strides, unit column stride), image b its top-left
    region with geo[b] = (H, W, OH, OW, top, left) (clip.resize_geometry) -> (B,3,S,S) fp32: trunc((x*0.5+0.5)*255) as ToPILImage
    does, then Pillow's bicubic resize, centre crop, / 255, (v - mean) / std, bit for bit.  mean, std: float32 numpy arrays of three"""
    assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32 and x.stride(3) == 1 and x.is_cuda and len(geo) == x.shape[0]
    src = (_p(x), ctypes.c_long(x.stride(0)), ctypes.c_long(x.stride(1)), int(x.stride(2)))
    return _clip_preprocess("sgic_clip_preprocess_ragged", src, geo, S, mean, std, x.device)


def clip_preprocess_u8canvas(x_u8, geo, S, mean, std):
    """(B,Hc,Wc,3) u8 canvas on the device, image b at its top left with geo[b] = (H, W, OH, OW, top, left) (clip.resize_geometry) ->
    (B,3,S,S) fp32: Pillow's bicubic resize of the bytes as they are, centre crop, / 255, (v - mean) / std, bit for bit.  mean, std:
    float32 numpy arrays of three"""
    assert x_u8.dim() == 4 and x_u8.shape[3] == 3 and x_u8.dtype == torch.uint8 and x_u8.is_contiguous() and x_u8.is_cuda
    assert len(geo) == x_u8.shape[0]
    src = (_p(x_u8), int(x_u8.shape[1]), int(x_u8.shape[2]))
    return _clip_preprocess("sgic_clip_preprocess_u8canvas", src, geo, S, mean, std, x_u8.device)


def clip_resize_coeffs(in_size, out_size, device):
    """Pillow's bicubic tables of an in_size -> out_size resample built on the device (what clip.pil_coeffs computes on the host)
    -> (bounds int32 (out,2), kk int32 (out,ksize), ksize)"""
    ksize = int(np.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1
    bounds = torch.empty(out_size, 2, dtype=torch.int32, device=device)
    kk = torch.empty(out_size, ksize, dtype=torch.int32, device=device)
    call("sgic_clip_resize_coeffs", int(in_size), int(out_size), ksize, _p(bounds), _p(kk))
    return bounds, kk, ksize


RESIZE_FILTERS = {"lanczos": 1, "bicubic": 2}      # the C ABI's filter codes (Pillow's Image.BICUBIC is 3: the names, not the numbers, are shared with Pillow)


def resize_u8(x_u8, OH, OW, filter="lanczos"):
    """(B,H,W,3) u8 on the device -> (B,OH,OW,3) u8: the bytes of Pillow's Image.fromarray(x[b]).resize((OW, OH), filter) for
    filter "lanczos" or "bicubic" (csrc/resize.hip).  Allocates the output and the workspace; does not synchronise"""
    assert x_u8.dim() == 4 and x_u8.shape[3] == 3 and x_u8.dtype == torch.uint8 and x_u8.is_contiguous() and x_u8.is_cuda
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, not {filter!r}")
    B, H, W, _ = x_u8.shape
    OH, OW, f = int(OH), int(OW), RESIZE_FILTERS[filter]
    nbytes = lib.sgic_resize_u8_work_bytes(B, H, W, OH, OW, f)      # 0: a geometry the call refuses (it says which)
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x_u8.device)
    out = torch.empty(B, max(OH, 0), max(OW, 0), 3, dtype=torch.uint8, device=x_u8.device)
    call("sgic_resize_u8_batch", _p(x_u8), B, H, W, _p(out), OH, OW, f, _p(work), ctypes.c_size_t(nbytes))
    return out


def resize_u8_coeffs(in_size, out_size, filter="lanczos"):
    """the tables resize_u8 uses for one axis, made on the host as the call makes them -> (bounds int32 (out,2), kk int32 (out,ksize))"""
    f = RESIZE_FILTERS[filter]
    ksize = int(math.ceil((2.0 if f == 2 else 3.0) * max(in_size / out_size, 1.0))) * 2 + 1
    bounds, kk = np.empty((out_size, 2), dtype=np.int32), np.empty((out_size, ksize), dtype=np.int32)
    call("sgic_resize_u8_coeffs", int(in_size), int(out_size), f, ksize, bounds, kk)
    return bounds, kk


def topk_rows(scores, k):
    """scores (nq, n) fp32 on device (consumed) -> (top scores (nq,k), indices (nq,k) int32)"""
    nq, n = scores.shape
    assert scores.is_contiguous()
    os_ = torch.empty(nq, k, device=scores.device, dtype=torch.float32)
    oi = torch.empty(nq, k, device=scores.device, dtype=torch.int32)
    call("sgic_topk_rows", _p(scores), nq, n, k, _p(os_), _p(oi))
    return os_, oi


def _search_inputs(q, r_q, db_codes, r_db, extra=()):
    """the checks the four fused searches share: q (nq, D) u8 codes with their r_q (nq,), or fp32 queries with r_q None; db_codes
    (n, D) u8, r_db (n,) fp32; `extra` further (tensor, dtype) pairs; all contiguous on db_codes' device -> (nq, n, D)"""
    require_gpu()
    qdt = torch.float32 if r_q is None else torch.uint8
    for t, dt in ((q, qdt), (db_codes, torch.uint8), (r_db, torch.float32)) + (() if r_q is None else ((r_q, torch.float32),)) + extra:
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == db_codes.device
    nq, D = q.shape
    n, Dd = db_codes.shape
    assert D == Dd and r_db.shape == (n,) and (r_q is None or r_q.shape == (nq,))
    return nq, n, D


def _search_topk(q, r_q, db_codes, r_db, k, splits):
    """sgic_search_codes_u8, or with r_q None sgic_search_codes_f32q: the checks, the workspace and the call"""
    nq, n, D = _search_inputs(q, r_q, db_codes, r_db)
    name = "sgic_search_codes_f32q" if r_q is None else "sgic_search_codes_u8"
    want = 0 if splits is None else int(splits)
    used, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
    call(name + "_work_bytes", nq, n, D, int(k), want, ctypes.byref(used), ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=db_codes.device) if nbytes.value else None
    os_ = torch.empty(nq, k, device=db_codes.device, dtype=torch.float32)
    oi = torch.empty(nq, k, device=db_codes.device, dtype=torch.int32)
    call(name, _p(q), *(() if r_q is None else (_p(r_q),)), _p(db_codes), _p(r_db), nq, n, D, int(k), want, _p(work),
         ctypes.c_size_t(nbytes.value), _p(os_), _p(oi))
    return os_, oi


def search_codes(q_codes, r_q, db_codes, r_db, k, splits=None):
    """fused exact search over u8 codes (csrc/search.hip): q_codes (nq, D) / db_codes (n, D) u8, r_q (nq,) / r_db (n,) fp32
    (search.code_rnorm), all contiguous on one device -> (scores (nq,k) fp32, idx (nq,k) int32), score descending, ties -> lower
    index.  D % 64 == 0, D <= 4096, k <= min(n, 128); `splits` forces the number of database splits (tests)."""
    return _search_topk(q_codes, r_q, db_codes, r_db, k, splits)


def search_codes_f32q(q, db_codes, r_db, k, splits=None):
    """fused exact search of fp32 queries over u8 codes (csrc/search.hip, F32Query): q (nq, D) fp32, db_codes (n, D) u8,
    r_db (n,) fp32 (search.code_rnorm), all contiguous on one device -> (scores (nq,k) fp32, idx (nq,k) int32), score descending,
    ties -> lower index.  The query is taken to 2^-22 fixed point (include/sgic.h has the arithmetic).  D % 64 == 0, D <= 2048,
    k <= min(n, 128); `splits` forces the number of database splits (tests)."""
    return _search_topk(q, None, db_codes, r_db, k, splits)


def _search_range_launch(q, r_q, db_codes, r_db, threshold, self_join, splits, capacity, count, out_q, out_d, out_score):
    """sgic_search_range_u8, or with r_q None sgic_search_range_f32q (no self_join): the checks and the call"""
    nq, n, D = _search_inputs(q, r_q, db_codes, r_db, ((count, torch.int64),))
    assert count.numel() == 1
    capacity = int(capacity)
    for t, dt in ((out_q, torch.int32), (out_d, torch.int32), (out_score, torch.float32)):
        assert (t is None and capacity == 0) or (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= capacity)
    head = (_p(q), _p(db_codes), _p(r_db), nq, n, D, float(threshold)) if r_q is None else \
        (_p(q), _p(r_q), _p(db_codes), _p(r_db), nq, n, D, float(threshold), bool(self_join))
    call("sgic_search_range_f32q" if r_q is None else "sgic_search_range_u8", *head, 0 if splits is None else int(splits),
         ctypes.c_longlong(capacity), _p(count), _p(out_q), _p(out_d), _p(out_score))


def search_codes_range_launch(q_codes, r_q, db_codes, r_db, threshold, self_join, splits, capacity, count, out_q, out_d, out_score):
    """one call of sgic_search_range_u8 (include/sgic.h), nothing else: `count` (1,) int64 on the device is ADDED to (the caller
    zeroes it), out_q / out_d int32 and out_score fp32 hold at least `capacity` entries each (None with capacity = 0: count only).
    No synchronisation; hits arrive in no particular order."""
    _search_range_launch(q_codes, r_q, db_codes, r_db, threshold, self_join, splits, capacity, count, out_q, out_d, out_score)


def search_codes_range_f32q_launch(q, db_codes, r_db, threshold, splits, capacity, count, out_q, out_d, out_score):
    """one call of sgic_search_range_f32q (include/sgic.h), nothing else: q (nq, D) fp32; `count`, the output arrays and
    `capacity` as in search_codes_range_launch (the counter is ADDED to).  No synchronisation; hits arrive in no particular order."""
    _search_range_launch(q, None, db_codes, r_db, threshold, False, splits, capacity, count, out_q, out_d, out_score)


def _range_collect(launch_into, nq, n, dev, threshold, capacity, max_pairs):
    """the host side both threshold searches share.  launch_into(cap, count, oq, od, os_) makes one launch into arrays of `cap`
    entries (None with cap = 0).  The first launch has room for `capacity` hits (default: four per row, at least 4096); a larger
    count allocates exactly `count` entries and launches once more -- the predicate is deterministic, the second count equals the
    first.  max_pairs: a count above it raises ValueError before that allocation.  -> (q int32, d int32, score fp32, count),
    sorted by (q, d) on the device, so the result does not depend on the order in which the waves appended their hits"""
    threshold = float(threshold)
    if not math.isfinite(threshold):
        raise ValueError(f"range search needs a finite threshold, got {threshold}")
    if capacity is None:
        capacity = min(nq * n, max(4096, 4 * max(nq, n)))
        if max_pairs is not None:
            capacity = min(capacity, int(max_pairs))
    capacity = int(capacity)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def launch(cap):
        oq = torch.empty(cap, dtype=torch.int32, device=dev) if cap else None
        od = torch.empty(cap, dtype=torch.int32, device=dev) if cap else None
        os_ = torch.empty(cap, dtype=torch.float32, device=dev) if cap else None
        count.zero_()
        launch_into(cap, count, oq, od, os_)
        return oq, od, os_, int(count.item())

    oq, od, os_, total = launch(capacity)
    if max_pairs is not None and total > int(max_pairs):
        raise ValueError(f"{total} pairs score >= {threshold}, more than max_pairs = {int(max_pairs)}: raise the threshold or max_pairs")
    if total > capacity:
        del oq, od, os_
        oq, od, os_, again = launch(total)
        assert again == total, f"range search counted {total} hits, then {again}"
    if total == 0:
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev), 0)
    key, order = torch.sort((oq[:total].to(torch.int64) << 32) | od[:total].to(torch.int64))
    return (key >> 32).to(torch.int32), (key & 0xFFFFFFFF).to(torch.int32), os_[:total][order], total


def search_codes_range(q_codes, r_q, db_codes, r_db, threshold, self_join=False, capacity=None, splits=None, max_pairs=None):
    """threshold (range) search over u8 codes (csrc/search.hip, search_range_kernel): every pair whose score -- the fp32 bits
    search_codes reports -- is >= threshold.  Inputs as for search_codes.  self_join: the queries are the database (pass the same
    tensors); only pairs d > q are returned and the tiles below the diagonal are not computed.
    -> (q int32, d int32, score fp32, count), sorted by (q, d) ascending on the device; capacity, the second launch after an
    overflow and max_pairs are _range_collect's."""
    def launch_into(cap, count, oq, od, os_):
        search_codes_range_launch(q_codes, r_q, db_codes, r_db, threshold, self_join, splits, cap, count, oq, od, os_)

    return _range_collect(launch_into, q_codes.shape[0], db_codes.shape[0], db_codes.device, threshold, capacity, max_pairs)


def search_codes_range_f32q(q, db_codes, r_db, threshold, capacity=None, splits=None, max_pairs=None):
    """threshold (range) search of fp32 queries over u8 codes (csrc/search.hip, search_range_kernel with F32Query): every pair whose score
    -- the fp32 bits search_codes_f32q reports -- is >= threshold.  Inputs as for search_codes_f32q (D % 64 == 0, D <= 2048).
    -> (q int32, d int32, score fp32, count), sorted by (q, d) ascending on the device; capacity, the second launch after an
    overflow and max_pairs are _range_collect's."""
    def launch_into(cap, count, oq, od, os_):
        search_codes_range_f32q_launch(q, db_codes, r_db, threshold, splits, cap, count, oq, od, os_)

    return _range_collect(launch_into, q.shape[0], db_codes.shape[0], db_codes.device, threshold, capacity, max_pairs)


def _search_rank(q, r_q, db_codes, r_db, targets, splits):
    """sgic_search_rank_u8, or with r_q None sgic_search_rank_f32q: the checks, the workspace and the call.  The ABI reads the
    targets on the device and cannot refuse them, so their length and range are checked here, before the launch"""
    require_gpu()
    if not isinstance(targets, torch.Tensor):
        targets = torch.from_numpy(np.ascontiguousarray(np.asarray(targets).reshape(-1), dtype=np.int64))
    if targets.dim() != 1 or targets.shape[0] != q.shape[0]:
        raise ValueError(f"{tuple(targets.shape)} targets for {q.shape[0]} queries: one target row per query is needed")
    if targets.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"targets must be int32 or int64 row indices, got {targets.dtype}")
    n = db_codes.shape[0]
    if targets.numel():
        lo, hi = (int(v) for v in torch.stack(torch.aminmax(targets)).tolist())
        if lo < 0 or hi >= n:
            raise ValueError(f"targets span [{lo}, {hi}], outside the {n} rows [0, {n}) of the database")
    targets = targets.to(device=db_codes.device, dtype=torch.int32).contiguous()
    nq, n, D = _search_inputs(q, r_q, db_codes, r_db, ((targets, torch.int32),))
    nbytes = ctypes.c_size_t(0)
    call("sgic_search_rank_work_bytes", nq, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=db_codes.device)
    rank = torch.empty(nq, dtype=torch.int32, device=db_codes.device)
    score = torch.empty(nq, dtype=torch.float32, device=db_codes.device)
    call("sgic_search_rank_f32q" if r_q is None else "sgic_search_rank_u8", _p(q), *(() if r_q is None else (_p(r_q),)), _p(db_codes),
         _p(r_db), _p(targets), nq, n, D, 0 if splits is None else int(splits), _p(work), ctypes.c_size_t(nbytes.value), _p(rank), _p(score))
    return rank, score


def search_codes_rank(q_codes, r_q, db_codes, r_db, targets, splits=0):
    """rank of one target row per query over u8 codes (csrc/search.hip, search_rank_kernel): inputs as for search_codes, `targets`
    (nq,) row indices (a tensor on either side, or an array) -> (rank (nq,) int32, score (nq,) fp32) on the device.  rank = the
    number of rows that search_codes orders before the target (higher key, or equal key and lower index), i.e. the target's
    position in the full result list; score = the fp32 bits search_codes reports for the pair.  Targets of another length or
    outside [0, n) are a ValueError before the launch (range check of a device tensor: one read-back; host targets: none).  No
    synchronisation otherwise; `splits` forces the number of database splits (tests)."""
    return _search_rank(q_codes, r_q, db_codes, r_db, targets, splits)


def search_codes_rank_f32q(q, db_codes, r_db, targets, splits=0):
    """search_codes_rank for fp32 queries (F32Query): inputs as for search_codes_f32q (D % 64 == 0, D <= 2048), the order and the
    score bits those of search_codes_f32q -> (rank (nq,) int32, score (nq,) fp32) on the device."""
    return _search_rank(q, None, db_codes, r_db, targets, splits)


def assign_codes(centroids, db_codes, r_db, return_int=False):
    """for every row of the u8 codes the best of K fp32 centroids (csrc/search.hip, assign_codes_kernel): centroids (K, D) fp32 rows
    of norm <= 1, db_codes (n, D) u8, r_db (n,) fp32 (search.code_rnorm), all contiguous on one device -> (cluster (n,) int32, score
    (n,) fp32).  The argmax runs on the integer M of search_codes_f32q (equal M -> the lower centroid index); score =
    (float32(M) * r_db) * 2^-22, the bits search_codes_f32q reports for that (centroid, row) pair.  return_int: -> (cluster, score,
    M (n,) int64).  D % 64 == 0, D <= 2048, K <= 65536.  No synchronisation."""
    require_gpu()
    for t, dt in ((centroids, torch.float32), (db_codes, torch.uint8), (r_db, torch.float32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == db_codes.device
    K, D = centroids.shape
    n, Dd = db_codes.shape
    assert D == Dd and r_db.shape == (n,)
    nbytes = ctypes.c_size_t(0)
    call("sgic_assign_codes_f32c_work_bytes", K, D, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=db_codes.device)
    oc = torch.empty(n, dtype=torch.int32, device=db_codes.device)
    oM = torch.empty(n, dtype=torch.int64, device=db_codes.device)
    call("sgic_assign_codes_f32c", _p(centroids), _p(db_codes), K, n, D, _p(work), ctypes.c_size_t(nbytes.value), _p(oc), _p(oM))
    score = (oM.to(torch.float32) * r_db) * (2.0 ** -22)
    return (oc, score, oM) if return_int else (oc, score)


def cluster_sums(db_codes, assign, K):
    """the exact integer sums of a partition (csrc/search.hip, cluster_sums_kernel): db_codes (n, D) u8 and assign (n,) int32 with
    every entry in [0, K), contiguous on one device -> (sums (K, D) int64, counts (K,) int64), sums[c] = sum of 2 code - 255 over
    the rows of cluster c.  The rows are sorted by cluster on the device first (stable).  One read-back, the range check of
    `assign`; an id outside [0, K) is a ValueError before the launch.  D % 16 == 0, D <= 4096."""
    require_gpu()
    for t, dt in ((db_codes, torch.uint8), (assign, torch.int32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == db_codes.device
    n, D = db_codes.shape
    K = int(K)
    assert assign.shape == (n,)
    if K < 1 or n < 1:
        raise ValueError(f"cluster_sums needs K >= 1 and at least one row, got K = {K}, n = {n}")
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(assign)).tolist())
    if lo < 0 or hi >= K:
        raise ValueError(f"cluster ids span [{lo}, {hi}], outside [0, {K})")
    sorted_assign, order = torch.sort(assign, stable=True)
    sums = torch.zeros(K, D, dtype=torch.int64, device=db_codes.device)
    counts = torch.zeros(K, dtype=torch.int64, device=db_codes.device)
    call("sgic_cluster_sums_u8", _p(db_codes), _p(order), _p(sorted_assign), n, D, K, _p(sums), _p(counts))
    return sums, counts


def quality_u8(a, b):
    """squared error and MS-SSIM level means of B pairs of u8 images (csrc/quality.hip): a (original) and b (reconstruction)
    (B, H, W, 3) u8, contiguous on one device, min(H, W) > 160 -> (sse (B, 3) int64, exact; levels (B, 3, 5, 2) float64: the mean
    ssim and the mean cs of every level and channel).  quality.combine turns them into psnr / ssim / ms_ssim.  No synchronisation."""
    require_gpu()
    for t in (a, b):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == a.device
    assert a.dim() == 4 and a.shape[3] == 3 and a.shape == b.shape
    B, H, W, _ = a.shape
    nbytes = ctypes.c_size_t(0)
    call("sgic_quality_u8_work_bytes", B, H, W, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=a.device)
    sse = torch.empty(B, 3, dtype=torch.int64, device=a.device)
    levels = torch.empty(B, 3, 5, 2, dtype=torch.float64, device=a.device)
    call("sgic_quality_u8", _p(a), _p(b), B, H, W, _p(work), ctypes.c_size_t(nbytes.value), _p(sse), _p(levels))
    return sse, levels


def niqe_blocks_u8(x):
    """the block sums of NIQE (csrc/niqe.hip): x (B, H, W, 3) u8 RGB, contiguous, 96 <= H, W <= 16384 -> (stats, sharp) float64 on
    x's device.  stats (B, H // 96, W // 96, 2, 5, 5): per block, scale (0: 96 x 96 luma samples, 1: 48 x 48 of the half-size plane)
    and map (the MSCN block n, then n * roll(n, s) for s = (0,1), (1,0), (1,1), (1,-1)): cnt_neg, cnt_pos, ssq_neg, ssq_pos, sabs.
    sharp (B, H // 96, W // 96): the mean of the local deviation sigma over the scale-0 block.  niqe.features turns stats into the
    36 numbers per block.  No synchronisation."""
    from .niqe import window_weights
    require_gpu()
    assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous() and x.dim() == 4 and x.shape[3] == 3
    B, H, W, _ = x.shape
    nbytes = ctypes.c_size_t(0)
    call("sgic_niqe_u8_work_bytes", B, H, W, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    stats = torch.empty(B, H // 96, W // 96, 2, 5, 5, dtype=torch.float64, device=x.device)
    sharp = torch.empty(B, H // 96, W // 96, dtype=torch.float64, device=x.device)
    call("sgic_niqe_u8", _p(x), B, H, W, np.array(window_weights(), dtype=np.float64), _p(work), ctypes.c_size_t(nbytes.value),
         _p(stats), _p(sharp))
    return stats, sharp


def hvs_luma_u8(x):
    """x (B, H, W, 3) u8 RGB, contiguous -> (B, H, W) float64 on x's device: Y = 0.299 R + 0.587 G + 0.114 B on the 0..255 scale,
    unrounded (csrc/hvs.hip), what the three measures below take.  No synchronisation."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous() and x.dim() == 4 and x.shape[3] == 3
    B, H, W, _ = x.shape
    y = torch.empty(B, H, W, dtype=torch.float64, device=x.device)
    call("sgic_hvs_luma_u8", _p(x), B, H, W, _p(y))
    return y


def _hvs_measure(name, ya, yb, out_cols, *extra):
    require_gpu()
    for t in (ya, yb):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.device == ya.device
    assert ya.dim() == 3 and ya.shape == yb.shape
    B, H, W = ya.shape
    nbytes = ctypes.c_size_t(0)
    call(f"sgic_hvs_{name}_work_bytes", B, H, W, ctypes.byref(nbytes))
    work = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=ya.device)
    out = torch.empty((B, out_cols) if out_cols else (B,), dtype=torch.float64, device=ya.device)
    call(f"sgic_hvs_{name}", _p(ya), _p(yb), B, H, W, *extra, _p(work), ctypes.c_size_t(nbytes.value), _p(out))
    return out


def hvs_vifp(ya, yb):
    """the two sums of pixel-domain VIF (csrc/hvs.hip): ya (original), yb (reconstruction) (B, H, W) float64
    luma, min(H, W) >= 41 -> (B, 2) float64 {numerator, denominator} over the four scales.  No synchronisation."""
    return _hvs_measure("vifp", ya, yb, 2)


def hvs_gmsd(ya, yb):
    """gradient magnitude similarity deviation of B luma pairs (csrc/hvs.hip) -> (B,) float64.  No synchronisation."""
    return _hvs_measure("gmsd", ya, yb, 0)


def hvs_psnr(ya, yb, q):
    """the block error sums of PSNR-HVS and PSNR-HVS-M (csrc/hvs.hip): (B, H, W) float64 luma pairs, min(H, W) >= 8; q: the 64 steps
    of the luminance quantisation table, natural order -> (B, 2) float64 {without masking, with masking}, summed over the
    (H // 8) (W // 8) whole blocks.  No synchronisation."""
    q = np.ascontiguousarray(q, dtype=np.int32)
    assert q.shape == (64,)
    return _hvs_measure("psnr", ya, yb, 2, q)


def fsim_planes_u8(x):
    """x (B, H, W, 3) u8 RGB, contiguous -> (B, 3, h, w) float64: the reduced Y, I, Q planes FSIM works on (csrc/fsim.hip; DESIGN.md
    section 21; (h, w) as quality.fsim_reduction says).  No synchronisation."""
    require_gpu()
    assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous() and x.dim() == 4 and x.shape[3] == 3
    from .quality import fsim_reduction
    B, H, W, _ = x.shape
    _, h, w = fsim_reduction(H, W)
    out = torch.empty(B, 3, h, w, dtype=torch.float64, device=x.device)
    call("sgic_fsim_planes_u8", _p(x), B, H, W, _p(out))
    return out


def _work(name, device, *dims):
    nbytes = ctypes.c_size_t(0)
    call(name, *dims, ctypes.byref(nbytes))
    return torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=device), ctypes.c_size_t(nbytes.value)


def fsim_phasecong(planes):
    """planes (B, h, w) float64, 2 <= h, w <= 2048 -> (B, h, w) float64: the phase congruency map of every plane (csrc/fsim.hip:
    dense fp64 DFT passes, the noise threshold from an exact median); 0 everywhere for a constant plane.  No synchronisation."""
    require_gpu()
    assert planes.is_cuda and planes.dtype == torch.float64 and planes.is_contiguous() and planes.dim() == 3
    B, h, w = planes.shape
    work, nbytes = _work("sgic_fsim_phasecong_work_bytes", planes.device, B, h, w)
    pc = torch.empty_like(planes)
    call("sgic_fsim_phasecong", _p(planes), B, h, w, _p(work), nbytes, _p(pc))
    return pc


def fsim(a, b):
    """a (originals), b (reconstructions) (B, H, W, 3) u8 RGB, contiguous -> (fsim, fsimc): (B,) float64 each (csrc/fsim.hip).
    No synchronisation."""
    require_gpu()
    for t in (a, b):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == a.device
    assert a.dim() == 4 and a.shape[3] == 3 and a.shape == b.shape
    B, H, W, _ = a.shape
    work, nbytes = _work("sgic_fsim_work_bytes", a.device, B, H, W)
    out = torch.empty(2, B, dtype=torch.float64, device=a.device)
    call("sgic_fsim", _p(a), _p(b), B, H, W, _p(work), nbytes, _p(out[0]), _p(out[1]))
    return out[0], out[1]


def _input_halo(symbol, img_u8, hp, image_offset):
    require_gpu()
    assert img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.dim() == 4 and img_u8.shape[3] == 3
    B, H, W, _ = img_u8.shape
    assert (hp.H, hp.W, hp.C) == (H, W, 32) and 0 <= image_offset and image_offset + B <= hp.B, ((hp.B, hp.H, hp.W, hp.C), img_u8.shape)
    call(symbol, _p(img_u8), B, H, W, hp.B, int(image_offset), _p(hp.t))
    return hp


def _halo_producer(symbol, x, B, H, W, C, OH, OW, *extra):
    """x (B*H*W, C) -> the cached HaloPlanes of (B, OH, OW, C), its interior written by `symbol` (extra: its arguments after C)"""
    require_gpu()
    x, ldx = _rows(x)
    assert ldx == C and x.shape == (B * H * W, C), (x.shape, (B, H, W, C))
    hp = halo_planes_buffer(x.device, B, OH, OW, C)
    call(symbol, _p(x), B, H, W, C, *extra, _p(hp.t))
    return hp


def lpips_input(img_u8, hp, image_offset=0):
    """the LPIPS input layer (csrc/lpips.hip): img_u8 (B, H, W, 3) u8 -> the interior of images image_offset .. image_offset+B-1 of
    hp, a HaloPlanes of (total images, H, W, 32) from halo_planes_buffer; channels 3..31 are zero.  No synchronisation."""
    return _input_halo("sgic_lpips_input_split3", img_u8, hp, image_offset)


def relu_pool_halo(x, B, H, W, C, pool=False):
    """x (B*H*W, C) fp32, a convolution's output before its ReLU -> ReLU, a 2x2 / stride 2 max-pool when pool (an odd last row or
    column is dropped) -> the next 3x3 convolution's zero-halo operand planes (HaloPlanes; csrc/lpips.hip).  C % 32 == 0."""
    return _halo_producer("sgic_relu_pool_halo_split3", x, B, H, W, C, H // 2 if pool else H, W // 2 if pool else W, int(bool(pool)))


def lpips_head(feat, w, B, H, W, out=None):
    """one LPIPS tap (csrc/lpips.hip): feat (2*B*H*W, C) fp32 before its ReLU, the first B images against the last B; w (C,) fp32
    -> d (B,) float64 = the pixel mean of sum_c w_c (u_a - u_b)^2 over the unit-normalised ReLU features.  No synchronisation."""
    require_gpu()
    feat, ldf = _rows(feat)
    C = feat.shape[1]
    assert ldf == C and feat.shape[0] == 2 * B * H * W and w.shape == (C,) and w.is_contiguous() and w.dtype == torch.float32
    nbytes = ctypes.c_size_t(0)
    call("sgic_lpips_head_work_bytes", B, H, W, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=feat.device)
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=feat.device)
    assert out.shape == (B,) and out.dtype == torch.float64 and out.is_contiguous()
    call("sgic_lpips_head", _p(feat), _p(w), B, H, W, C, _p(work), ctypes.c_size_t(nbytes.value), _p(out))
    return out


def dists_input(img_u8, hp, image_offset=0):
    """the DISTS input layer (csrc/dists.hip): img_u8 (B, H, W, 3) u8 -> (u / 255 - mean) / std in the interior of images image_offset
    .. image_offset+B-1 of hp, a HaloPlanes of (total images, H, W, 32) from halo_planes_buffer; channels 3..31 are zero.  No
    synchronisation."""
    return _input_halo("sgic_dists_input_split3", img_u8, hp, image_offset)


def dists_moments_u8(a, b, out=None):
    """tap 0 of DISTS (csrc/dists.hip): a, b (B, H, W, 3) u8, contiguous on one device -> (B, 3, 5) int64: the exact sums of a, b, a^2,
    b^2 and a b over the pixels of every pair and channel.  No synchronisation."""
    require_gpu()
    for t in (a, b):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == a.device
    assert a.dim() == 4 and a.shape[3] == 3 and a.shape == b.shape
    B, H, W, _ = a.shape
    if out is None:
        out = torch.empty(B, 3, 5, dtype=torch.int64, device=a.device)
    assert out.shape == (B, 3, 5) and out.dtype == torch.int64 and out.is_contiguous()
    call("sgic_dists_moments_u8", _p(a), _p(b), B, H, W, _p(out))
    return out


def relu_l2pool_halo(x, B, H, W, C):
    """x (B*H*W, C) fp32, a convolution's output before its ReLU -> ReLU, then DISTS's L2 pool sqrt(hanning3x3(f^2) + 1e-12) at stride
    2 with zero padding 1 (an odd last row or column is kept: ceil(n / 2)) -> the next 3x3 convolution's zero-halo operand planes
    (HaloPlanes; csrc/dists.hip).  C % 32 == 0."""
    return _halo_producer("sgic_relu_l2pool_halo_split3", x, B, H, W, C, (H + 1) // 2, (W + 1) // 2)


def dists_moments(feat, B, H, W):
    """one DISTS tap (csrc/dists.hip): feat (2*B*H*W, C) fp32 before its ReLU, the first B images against the last B -> (B, 5, C)
    float64: the sums of x, y, x^2, y^2 and x y over the pixels, x and y the ReLU'd sides.  No synchronisation."""
    require_gpu()
    feat, ldf = _rows(feat)
    C = feat.shape[1]
    assert ldf == C and feat.shape[0] == 2 * B * H * W and feat.dtype == torch.float32
    nbytes = ctypes.c_size_t(0)
    call("sgic_dists_moments_work_bytes", B, H, W, C, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=feat.device)
    sums = torch.empty(B, 5, C, dtype=torch.float64, device=feat.device)
    call("sgic_dists_moments", _p(feat), B, H, W, C, _p(work), ctypes.c_size_t(nbytes.value), _p(sums))
    return sums


def dists_head(sums, alpha, beta, H, W, out=None):
    """sums (B, 5, C) float64 of dists_moments over H*W pixels, alpha, beta (C,) fp32 -> (B, 2) float64: the tap's structure term
    sum_c alpha_c (1 - S1_c) and texture term sum_c beta_c (1 - S2_c), not yet divided by sum alpha + sum beta.  No synchronisation."""
    require_gpu()
    B, five, C = sums.shape
    assert five == 5 and sums.dtype == torch.float64 and sums.is_contiguous()
    for t in (alpha, beta):
        assert t.shape == (C,) and t.is_contiguous() and t.dtype == torch.float32 and t.device == sums.device
    if out is None:
        out = torch.empty(B, 2, dtype=torch.float64, device=sums.device)
    assert out.shape == (B, 2) and out.dtype == torch.float64 and out.is_contiguous()
    call("sgic_dists_head", _p(sums), _p(alpha), _p(beta), B, H, W, C, _p(out))
    return out


def lpips_alex_conv1_patches(img_u8, planes, image_offset=0):
    """the operand of AlexNet's first convolution (11x11, stride 4, pad 2) as a GEMM (csrc/lpips_alex.hip): img_u8 (B, H, W, 3) u8 ->
    rows image_offset*h1*w1 .. of `planes`, a Planes(total_images*h1*w1, 384) with h1 = (H - 7) // 4 + 1, w1 = (W - 7) // 4 + 1: column
    (ky*11 + kx)*3 + c of row (img, oy, ox) is the LPIPS input layer at pixel (4*oy - 2 + ky, 4*ox - 2 + kx), zero outside the image;
    columns 363..383 are zero.  The rows of other images are not touched.  No synchronisation."""
    require_gpu()
    assert img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.dim() == 4 and img_u8.shape[3] == 3
    B, H, W, _ = img_u8.shape
    assert H >= 7 and W >= 7, img_u8.shape
    per = ((H - 7) // 4 + 1) * ((W - 7) // 4 + 1)
    assert isinstance(planes, Planes) and planes.cols == 384 and planes.rows % per == 0, (planes.shape, img_u8.shape)
    total = planes.rows // per
    assert 0 <= image_offset and image_offset + B <= total, (image_offset, B, total)
    call("sgic_lpips_alex_conv1_patches_split3", _p(img_u8), B, H, W, total, int(image_offset), _p(planes.t))
    return planes


def relu_maxpool3_patches5(x, B, H, W, C):
    """x (B*H*W, C) fp32, a convolution's output before its ReLU -> ReLU -> max-pool 3x3, stride 2, no padding (floor) to PH x PW ->
    the 5x5, pad-2, stride-1 patches of the pooled map as a Planes(B*PH*PW, 25*C): column (ky*5 + kx)*C + c, zero where the tap is
    outside the pooled map (csrc/lpips_alex.hip).  C % 32 == 0."""
    require_gpu()
    x, ldx = _rows(x)
    assert ldx == C and x.shape == (B * H * W, C) and H >= 3 and W >= 3, (x.shape, (B, H, W, C))
    pl = Planes(B * ((H - 3) // 2 + 1) * ((W - 3) // 2 + 1), 25 * C, x.device)
    call("sgic_relu_maxpool3_patches5_split3", _p(x), B, H, W, C, _p(pl.t))
    return pl


def relu_maxpool3_halo(x, B, H, W, C):
    """x (B*H*W, C) fp32, a convolution's output before its ReLU -> ReLU -> max-pool 3x3, stride 2, no padding (floor) -> the next 3x3
    convolution's zero-halo operand planes (HaloPlanes from halo_planes_buffer; csrc/lpips_alex.hip).  C % 32 == 0."""
    assert H >= 3 and W >= 3, (H, W)
    return _halo_producer("sgic_relu_maxpool3_halo_split3", x, B, H, W, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1)


def fid_resize299(canvas_u8, desc, out=None):
    """the input step of the FID Inception (csrc/fid.hip): canvas_u8 (B, H, W, 3) u8 on the device, desc (n, 5) int32 numpy on the host,
    rows (image, y0, x0, h, w) -> (n, 299, 299, 3) fp32: 2 * bilinear299(u / 255) - 1 of every window.  Only the descriptors leave the
    host.  No synchronisation."""
    require_gpu()
    assert canvas_u8.is_cuda and canvas_u8.dtype == torch.uint8 and canvas_u8.is_contiguous() and canvas_u8.dim() == 4 and canvas_u8.shape[3] == 3
    desc = np.ascontiguousarray(desc, dtype=np.int32)
    assert desc.ndim == 2 and desc.shape[1] == 5 and desc.shape[0] >= 1, desc.shape
    B, H, W, _ = canvas_u8.shape
    n = desc.shape[0]
    if out is None:
        out = torch.empty(n, 299, 299, 3, dtype=torch.float32, device=canvas_u8.device)
    assert out.shape == (n, 299, 299, 3) and out.dtype == torch.float32 and out.is_contiguous()
    d_desc = torch.from_numpy(desc).to(canvas_u8.device)
    call("sgic_fid_resize299", _p(canvas_u8), B, H, W, desc, _p(d_desc), n, _p(out))
    return out


def conv_out(n, k, s, p):
    """output extent of a convolution or pool: input extent n, kernel k, stride s, padding p (floor)"""
    return (n + 2 * p - k) // s + 1


def patches_split3(x, B, H, W, kh, kw, sh=1, sw=1, ph=0, pw=0, relu=True, cols=None, out=None):
    """x (B*H*W, ld) fp32, contiguous; cols = (col0, C): the column slice that is the map (default: all of it, a slice of a concat buffer
    otherwise) -> ReLU when `relu` -> the kh x kw patches at stride (sh, sw) with zero padding (ph, pw) as a Planes(B*OH*OW, Kp), Kp =
    kh*kw*C rounded up to 32: column (ky*kw + kx)*C + c, zero outside the map and in the padding columns (csrc/fid.hip).  The A operand
    of that convolution as ops.gemm(planes, w (Cout, Kp), bias).  Any C >= 1.  out: a Planes of that shape to write into."""
    require_gpu()
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda and x.shape[0] == B * H * W, (x.shape, (B, H, W))
    ld = x.shape[1]
    col0, C = (0, ld) if cols is None else cols
    rows, Kp = B * conv_out(H, kh, sh, ph) * conv_out(W, kw, sw, pw), (kh * kw * C + 31) // 32 * 32
    pl = out if out is not None else Planes(rows, Kp, x.device)
    assert isinstance(pl, Planes) and pl.shape == (rows, Kp), (pl.shape, (rows, Kp))
    call("sgic_patches_split3", _p(x), ld, int(col0), B, H, W, int(C), kh, kw, sh, sw, ph, pw, int(bool(relu)), _p(pl.t))
    return pl


def _relu_pool3(name, x, B, H, W, OH, OW, out, col0):
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda and x.shape[0] == B * H * W, (x.shape, (B, H, W))
    C = x.shape[1]
    if out is None:
        out = torch.empty(B * OH * OW, C, dtype=torch.float32, device=x.device)
    assert out.dim() == 2 and out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == B * OH * OW and col0 + C <= out.shape[1]
    call(name, _p(x), B, H, W, C, _p(out), out.shape[1], int(col0))
    return out


def relu_maxpool3s2(x, B, H, W, out=None, col0=0):
    """x (B*H*W, C) fp32 before its ReLU -> ReLU -> max-pool 3x3, stride 2, no padding (floor) -> columns col0 .. col0+C-1 of `out`
    (B*OH*OW, ld) fp32, a concat buffer (default: a new (B*OH*OW, C) tensor); csrc/fid.hip.  C % 4 == 0."""
    require_gpu()
    assert H >= 3 and W >= 3, (H, W)
    return _relu_pool3("sgic_relu_maxpool3s2", x, B, H, W, (H - 3) // 2 + 1, (W - 3) // 2 + 1, out, col0)


def relu_avgpool3s1p1(x, B, H, W, out=None, col0=0):
    """as relu_maxpool3s2, the pool being the 3x3 / stride 1 / padding 1 average with count_include_pad=False: the taps inside the map,
    summed in row-major order in fp32, divided once by their number"""
    require_gpu()
    return _relu_pool3("sgic_relu_avgpool3s1p1", x, B, H, W, H, W, out, col0)


def relu_maxpool3s1p1(x, B, H, W, out=None, col0=0):
    """as relu_maxpool3s2, the pool being the 3x3 / stride 1 / padding 1 maximum"""
    require_gpu()
    return _relu_pool3("sgic_relu_maxpool3s1p1", x, B, H, W, H, W, out, col0)


def relu_mean_rows(x, B, R, out=None):
    """x (B*R, C) fp32 before its ReLU -> (B, C) fp32: the mean over the R rows of every image of relu(x), summed in row order in one
    fp32 accumulator per (image, channel) and divided once (csrc/fid.hip): independent of B."""
    require_gpu()
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda and x.shape[0] == B * R, (x.shape, (B, R))
    if out is None:
        out = torch.empty(B, x.shape[1], dtype=torch.float32, device=x.device)
    assert out.shape == (B, x.shape[1]) and out.dtype == torch.float32 and out.is_contiguous()
    call("sgic_relu_mean_rows", _p(x), B, R, x.shape[1], _p(out))
    return out


def gram_f64(a, b=None, ia=None, ib=None, out=None):
    """out[i][j] = sum_k a[ia[i]][k] * b[ib[j]][k] in fp64 from fp32 rows (csrc/fid.hip), k in order: a (ra, K), b (rb, K) fp32 (b
    defaults to a), ia / ib int32 row indices on the device (default: every row in order) -> (n, m) float64.  No synchronisation."""
    require_gpu()
    b = a if b is None else b
    a, lda = _rows(a)
    b, ldb = _rows(b)
    assert a.shape[1] == b.shape[1] and a.device == b.device
    for ix in (ia, ib):
        assert ix is None or (ix.dtype == torch.int32 and ix.is_cuda and ix.is_contiguous() and ix.dim() == 1 and ix.numel() >= 1)
    n = a.shape[0] if ia is None else ia.numel()
    m = b.shape[0] if ib is None else ib.numel()
    if out is None:
        out = torch.empty(n, m, dtype=torch.float64, device=a.device)
    assert out.shape == (n, m) and out.dtype == torch.float64 and out.is_contiguous()
    call("sgic_gram_f64", _p(a), _cl(lda), _p(ia), a.shape[0], n, _p(b), _cl(ldb), _p(ib), b.shape[0], m, a.shape[1], _p(out), _cl(m))
    return out


def jpeg_encode(rgb_u8, tables, subsampling, optimize=False, progressive=False):
    """baseline JPEG encode of B equal-size images (csrc/jpeg_enc.hip): rgb_u8 (B, H, W, 3) u8, contiguous on the device; tables
    (B, 2, 64) u16 numpy array on the host (luma and chroma quantisation table of every image, natural order); subsampling 0 / 1 / 2
    as Pillow's -> (buf (B, cap) u8: image b's entropy-coded segment and FF D9 in buf[b, :lens[b]], lens (B,) int32, err (B,) int32,
    nonzero where a slot was too small).  The header is jpeg_enc.header's.  optimize: Huffman tables fitted to every image (Pillow's
    optimize=True); the result is then (buf, lens, err, huff (B, 4, 272) u8: BITS and HUFFVAL of the image's tables DC0, AC0, DC1,
    AC1, nval (B, 4) int32: their HUFFVAL counts), which the header needs.  progressive: the ten scans of Pillow's progressive=True
    (optimize is then implied): buf[b] holds the ten entropy-coded segments back to back without EOI, lens is (B, 10), huff
    (B, 10, 272) and nval (B, 10) are the ten tables in file order (sgic_jpeg_encode_prog_batch).  No synchronisation."""
    require_gpu()
    assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous()
    assert rgb_u8.dim() == 4 and rgb_u8.shape[3] == 3
    B, H, W, _ = rgb_u8.shape
    tables = np.ascontiguousarray(tables, dtype=np.uint16)
    assert tables.shape == (B, 2, 64), f"tables must be ({B}, 2, 64), got {tables.shape}"
    stem = "sgic_jpeg_encode_prog" if progressive else "sgic_jpeg_encode_opt" if optimize else "sgic_jpeg_encode"
    cap, nbytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    call(stem + "_cap", H, W, int(subsampling), ctypes.byref(cap))
    call(stem + "_work_bytes", B, H, W, int(subsampling), ctypes.byref(nbytes))
    dev = rgb_u8.device
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    buf = torch.empty(B, cap.value, dtype=torch.uint8, device=dev)
    lens = torch.empty((B, 10) if progressive else (B,), dtype=torch.int32, device=dev)
    err = torch.empty(B, dtype=torch.int32, device=dev)
    args = (_p(rgb_u8), B, H, W, int(subsampling), ctypes.c_void_p(tables.ctypes.data), _p(work), ctypes.c_size_t(nbytes.value), _p(buf),
            ctypes.c_size_t(cap.value), _p(lens), _p(err))
    if not (optimize or progressive):
        call("sgic_jpeg_encode_batch", *args)
        return buf, lens, err
    ntab = 10 if progressive else 4
    huff = torch.empty(B, ntab, 272, dtype=torch.uint8, device=dev)
    nval = torch.empty(B, ntab, dtype=torch.int32, device=dev)
    call(stem + "_batch", *args, _p(huff), _p(nval))
    return buf, lens, err, huff, nval


def jpeg_decode_batch(params, scan, tabs, segs, quant, B, H, W, total_blocks, plane_bytes, max_blocks, out=None, check=True):
    """baseline JPEG batch -> (B,H,W,3) u8 on the device (csrc/jpeg.hip; descriptors built by sgic_amd.jpeg.JpegBatch)"""
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if not params.is_cuda else params.device   # inputs may be pinned host memory
    coef = torch.empty(total_blocks * 64, dtype=torch.int16, device=dev)
    wparams = torch.empty(B * 64, dtype=torch.int32, device=dev)
    wquant = torch.empty(B * 256, dtype=torch.int16, device=dev)
    planes = torch.empty(max(16, plane_bytes), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    assert out.shape == (B, H, W, 3) and out.dtype == torch.uint8 and out.is_contiguous()
    err = torch.empty(B, dtype=torch.int32, device=dev)
    call("sgic_jpeg_decode_batch", _p(params), _p(scan), _p(tabs), _p(segs), _p(quant), _p(wparams), _p(wquant), _p(coef), _p(planes), _p(out),
         _p(err), B, H, W, int(max_blocks))
    if check:
        e = err.cpu().numpy()
        if e.any():
            raise RuntimeError(f"corrupt JPEG stream(s) in the batch: error codes {e.tolist()}")
    return out, err


def jpeg_decode_scans_batch(params, descs, scan, tabs, segs, quant, level_start, B, H, W, total_blocks, plane_bytes, max_blocks, out=None,
                            check=True):
    """multi-scan (progressive / sequential / mixed) JPEG batch -> (B,H,W,3) u8 on the device (csrc/jpeg.hip jpeg_scan_kernel, one launch
    per dependency level; descriptors built by sgic_amd.jpeg.ScanJpegBatch).  level_start: host int32 array, nlevels + 1 entries"""
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if not params.is_cuda else params.device   # inputs may be pinned host memory
    coef = torch.empty(total_blocks * 64, dtype=torch.int16, device=dev)
    wparams = torch.empty(B * 64, dtype=torch.int32, device=dev)
    wquant = torch.empty(B * 256, dtype=torch.int16, device=dev)
    planes = torch.empty(max(16, plane_bytes), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    assert out.shape == (B, H, W, 3) and out.dtype == torch.uint8 and out.is_contiguous()
    err = torch.empty(B, dtype=torch.int32, device=dev)
    ls = np.ascontiguousarray(level_start, dtype=np.int32)
    call("sgic_jpeg_decode_scans_batch", _p(params), _p(descs), _p(scan), _p(tabs), _p(segs), _p(quant), _p(wparams), _p(wquant), _p(coef),
         _p(planes), _p(out), _p(err), B, H, W, _cl(total_blocks), int(max_blocks), ctypes.c_void_p(ls.ctypes.data), len(ls) - 1)
    if check:
        e = err.cpu().numpy()
        if e.any():
            raise RuntimeError(f"corrupt JPEG stream(s) in the batch: error codes {e.tolist()}")
    return out, err
