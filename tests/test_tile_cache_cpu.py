"""Host logic of the launch-mode cache (sgic_amd.ops): persistence, merge, nearest-M family lookup, and that the in-tree
cache file parses.  No GPU: nothing is launched."""
import json
import os

import pytest


@pytest.fixture()
def ops(tmp_path, monkeypatch):
    import sgic_amd  # noqa
    from sgic_amd import ops
    monkeypatch.setenv("SGIC_TILE_CACHE", str(tmp_path / "cache.json"))
    saved = (dict(ops._TILE), {k: dict(v) for k, v in ops._FAMILY.items()}, ops._DIRTY, dict(ops._CTX), ops.AUTOTUNE, ops.PROFILE,
             ops.LAST_TILE)
    ops._TILE.clear()
    ops._FAMILY.clear()
    ops._CTX.clear()
    ops._DIRTY = False
    yield ops
    ops._TILE.clear()
    ops._TILE.update(saved[0])
    ops._FAMILY.clear()
    ops._FAMILY.update(saved[1])
    ops._CTX.clear()
    ops._CTX.update(saved[3])
    ops._DIRTY, ops.AUTOTUNE, ops.PROFILE, ops.LAST_TILE = saved[2], saved[4], saved[5], saved[6]


def test_in_tree_cache_is_well_formed():
    import sgic_amd  # noqa
    from sgic_amd import ops
    d = json.load(open(ops._INTREE_CACHE))
    assert d["device"] == "gfx950" and len(d["picks"]) >= 40
    for k, v in d["picks"].items():
        kind, *nums = k.split("|")
        assert kind in ("gemm", "gemm3", "conv3x3", "conv3", "attn", "attn3") and all(n.lstrip("-").isdigit() for n in nums)
        assert 0 <= int(v) <= {"attn": 7, "attn3": 7, "gemm3": 31, "conv3": 31}.get(kind, 15)
    # the dominant GEMM shapes of the benchmarked configuration are covered: no process races them again
    for key in ("gemm|9248|4096|1024|0|1", "gemm|9248|1024|4096|1|0", "gemm|9248|3072|1024|0|0", "attn|32|289|16|0",
                "gemm3|9248|4096|1024|0|1", "gemm3|9248|1024|4096|1|0", "gemm3|9248|3072|1024|0|0"):   # gemm3: the bf16x3 split GEMM
        assert key in d["picks"], key


def test_save_merge_and_reload(ops, tmp_path):
    ops._remember(("gemm", 9248, 1024, 4096, 1, 0), 12)
    ops._remember(("attn", 32, 289, 16, 0), 5)
    path = ops.save_tile_cache()
    assert path == str(tmp_path / "cache.json")
    d = json.load(open(path))
    assert d["picks"] == {"attn|32|289|16|0": 5, "gemm|9248|1024|4096|1|0": 12}
    # a second process adds its own picks without losing the first one's
    ops._TILE.clear()
    ops._FAMILY.clear()
    ops._remember(("gemm", 8192, 768, 3072, 1, 0), 13)
    ops.save_tile_cache()
    assert set(json.load(open(path))["picks"]) == {"attn|32|289|16|0", "gemm|9248|1024|4096|1|0", "gemm|8192|768|3072|1|0"}
    ops._TILE.clear()
    ops._FAMILY.clear()
    ops._load_tile_cache()
    assert ops._lookup(("gemm", 9248, 1024, 4096, 1, 0)) == 12 and ops._lookup(("attn", 32, 289, 16, 0)) == 5
    assert ops.save_tile_cache() is None or True          # nothing dirty: no rewrite needed


def test_nearest_m_family_lookup(ops):
    """a ragged last batch / another batch size borrows the pick of the nearest M of the same (N, K, epilogue) family
    (within 2x) instead of racing 12 modes; a different epilogue or a far M does not match"""
    ops._remember(("gemm", 9248, 4096, 1024, 0, 1), 12)
    ops._remember(("gemm", 2312, 4096, 1024, 0, 1), 13)
    assert ops._lookup(("gemm", 8959, 4096, 1024, 0, 1)) == 12            # batch 31 of 32
    assert ops._lookup(("gemm", 2601, 4096, 1024, 0, 1)) == 13            # nearest of the two
    assert ops._lookup(("gemm", 289, 4096, 1024, 0, 1)) is None           # 8x away: measure it
    assert ops._lookup(("gemm", 9248, 4096, 1024, 1, 1)) is None          # other epilogue
    assert ops._lookup(("gemm", 9248, 4096, 768, 0, 1)) is None           # other K
    # a borrowed pick is what tile_of reports for its shape (bench.py's by_shape table) ...
    assert ops.tile_of((8959, 4096, 1024, False, 1)) == 12 and ops.tile_of((2601, 4096, 1024, False, 1)) == 13
    # ... and is not persisted as a measurement, nor does it become a neighbour that others borrow from
    assert set(ops._FAMILY[("gemm", 4096, 1024, 0, 1)]) == {9248, 2312}
    assert ops.save_tile_cache() == os.environ["SGIC_TILE_CACHE"]
    picks = json.load(open(os.environ["SGIC_TILE_CACHE"]))["picks"]
    assert picks == {"gemm|9248|4096|1024|0|1": 12, "gemm|2312|4096|1024|0|1": 13}
    # after a reload the two shapes resolve through the family again
    ops._TILE.clear()
    ops._FAMILY.clear()
    ops._load_tile_cache()
    for M in (8959, 2601):
        assert ("gemm", M, 4096, 1024, 0, 1) not in ops._TILE
    assert ops._lookup(("gemm", 8959, 4096, 1024, 0, 1)) == 12 and ops._lookup(("gemm", 2601, 4096, 1024, 0, 1)) == 13
    assert not {8959, 2601} & set(ops._FAMILY[("gemm", 4096, 1024, 0, 1)])      # (the in-tree cache's own sizes are in there too)


def test_tile_of_reads_profile_keys(ops):
    ops._remember(("gemm", 9248, 4096, 1024, 0, 1), 12)
    assert ops.tile_of((9248, 4096, 1024, False, 1)) == 12
    assert ops.tile_of(("batched", 32, 256, 256, 64, False, 0)) == 0
    assert ops.tile_of((1, 2, 3, False, 0)) is None


def test_picks_of_another_build_are_dropped(ops, tmp_path):
    """a user cache holding a launch mode this library does not have (written by a newer build) must not reach the C ABI"""
    p = tmp_path / "cache.json"
    p.write_text(json.dumps({"device": "gfx950", "picks": {"gemm3|9248|4096|1024|0|1": 99, "gemm|64|64|512|0|0": 15, "bogus|1|2": 1,
                                                         "gemm3|x|1": 2}}))
    ops._TILE.clear()
    ops._FAMILY.clear()
    ops._load_tile_cache()
    assert ops._TILE.get(("gemm", 64, 64, 512, 0, 0)) == 15
    assert ops._TILE.get(("gemm3", 9248, 4096, 1024, 0, 1)) != 99
    assert not any(k[0] == "bogus" for k in ops._TILE)


def test_mode_ranges_agree_between_the_layers():
    """the launch-mode ranges are written down in three places: the kernels' dispatchers (csrc), the tuner's mode lists (ops)
    and the cache validator (ops._MAX_MODE): they must agree, or a tuned pick can be rejected by the C ABI"""
    import re
    import sgic_amd  # noqa
    from sgic_amd import ops
    csrc = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "csrc")
    split_max = int(re.search(r"#define SGIC_SPLIT3_TILE_MODES (\d+)", open(os.path.join(csrc, "gemm_split.hip")).read()).group(1))
    f32_max = int(re.search(r"#define SGIC_TILE_MODES (\d+)", open(os.path.join(csrc, "gemm.hip")).read()).group(1))
    assert max(ops.SPLIT3_MODES) == split_max == ops._MAX_MODE["gemm3"] == ops._MAX_MODE["conv3"]
    assert max(ops.TUNE_MODES) == f32_max == ops._MAX_MODE["gemm"] == ops._MAX_MODE["conv3x3"]
    assert max(ops.ATTN_MODES) == ops._MAX_MODE["attn"] == ops._MAX_MODE["attn3"] == 7


def test_planes_rowmajor_inverts_the_slice_major_layout():
    """ops.Planes.rowmajor() (what the GPU tests compare producers' planes through) is the inverse of csrc/split3.h: s3_pack_off --
    element (row, col) of plane p sits at p * rows * cols + ((col / 32) * rows + row) * 32 + col % 32"""
    import torch
    import sgic_amd  # noqa
    from sgic_amd import ops
    rows, cols = 5, 96
    pl = ops.Planes(rows, cols, torch.device("cpu"))
    pl.t.copy_(torch.arange(3 * rows * cols, dtype=torch.int16))
    rm = pl.rowmajor()
    assert rm.shape == (3, rows, cols)
    for p in range(3):
        for r in range(rows):
            for c in (0, 1, 31, 32, 63, 64, 95):
                assert int(rm[p, r, c]) == p * rows * cols + ((c // 32) * rows + r) * 32 + c % 32


# ---- the policy of _pick_and_launch, with a fake launch: which mode is launched, how often, and what the buffer holds afterwards ----
KEY = ("gemm", 9248, 4096, 1024, 1, 0)
PROBES = 5


def _fake_launch(buf):
    """launch(mode, prof=None): buf += 1, like an in-place residual GEMM (not idempotent); -> (launch, list of the modes launched)"""
    log = []

    def launch(mode, prof=None):
        buf.add_(1.0)
        log.append(mode)
    return launch, log


def _fake_tune(ops, monkeypatch, best=7):
    """_tune replaced by PROBES launches and a remembered pick; -> list of (key, modes) per race"""
    races = []

    def tune(key, launch, modes=None):
        races.append((key, modes))
        for m in (ops.TUNE_MODES if modes is None else modes)[:PROBES]:
            launch(m)
        ops._remember(key, best)
        return best
    monkeypatch.setattr(ops, "_tune", tune)
    return races


def _buf():
    import torch
    return torch.full((6, 8), 5.0)


def test_policy_cache_hit_launches_the_pick_once(ops, monkeypatch):
    races = _fake_tune(ops, monkeypatch)
    ops._remember(KEY, 12, dirty=False)
    buf = _buf()
    launch, log = _fake_launch(buf)
    assert ops._pick_and_launch(KEY, launch, True) is False
    assert log == [12] and races == [] and ops.LAST_TILE == 12 and bool((buf == 6.0).all()) and not ops._DIRTY


def test_policy_family_hit_borrows_without_a_race(ops, monkeypatch):
    races = _fake_tune(ops, monkeypatch)
    ops._remember(KEY, 12, dirty=False)
    near = (KEY[0], 8959) + KEY[2:]
    buf = _buf()
    launch, log = _fake_launch(buf)
    assert ops._pick_and_launch(near, launch, True, restore=buf) is False
    assert log == [12] and races == [] and ops.LAST_TILE == 12 and bool((buf == 6.0).all())
    assert ops._TILE[near] == 12 and set(ops._FAMILY[(KEY[0],) + KEY[2:]]) == {9248} and not ops._DIRTY


def test_policy_autotune_off_takes_the_heuristic(ops, monkeypatch):
    races = _fake_tune(ops, monkeypatch)
    ops.AUTOTUNE = False
    buf = _buf()
    launch, log = _fake_launch(buf)
    assert ops._pick_and_launch(KEY, launch, True, restore=buf) is False
    assert log == [0] and races == [] and ops.LAST_TILE == 0 and bool((buf == 6.0).all()) and not ops._TILE and not ops._DIRTY


def test_policy_open_profile_window_never_races(ops, monkeypatch):
    races = _fake_tune(ops, monkeypatch)
    ops.PROFILE = []
    buf = _buf()
    launch, log = _fake_launch(buf)
    assert ops._pick_and_launch(KEY, launch, True, restore=buf) is False
    assert log == [0] and races == [] and ops.LAST_TILE == 0 and bool((buf == 6.0).all()) and not ops._TILE
    ops.PROFILE = None
    assert ops._pick_and_launch(KEY, launch, True, restore=buf) is False          # the first call after the window races
    assert len(races) == 1 and log[-1] == 7 and len(log) == 1 + PROBES + 1


def test_policy_race_restores_an_in_place_buffer(ops, monkeypatch):
    """restore is a column slice of a wider buffer: after the race it holds its saved value plus exactly ONE launch, and the
    columns beside it were never written"""
    import torch
    races = _fake_tune(ops, monkeypatch)
    wide = torch.full((6, 12), 5.0)
    wide[:, 8:] = -3.0
    buf = wide[:, :8]
    launch, log = _fake_launch(buf)
    modes = (1, 2, 3, 5, 10, 11, 14)
    assert ops._pick_and_launch(KEY, launch, True, restore=buf, modes=modes) is False
    assert races == [(KEY, modes)] and log == list(modes[:PROBES]) + [7] and ops.LAST_TILE == 7
    assert bool((wide[:, :8] == 6.0).all()) and bool((wide[:, 8:] == -3.0).all())
    assert ops._TILE[KEY] == 7 and ops._DIRTY
    # the second call: the pick, no race
    assert ops._pick_and_launch(KEY, launch, True, restore=buf, modes=modes) is False
    assert len(races) == 1 and log[-1] == 7 and bool((wide[:, :8] == 7.0).all())


def test_policy_race_without_restore_leaves_every_probe_behind(ops, monkeypatch):
    """the contract conv3x3 rests on: with restore=None nothing is put back, so the output must not feed the launch"""
    _fake_tune(ops, monkeypatch)
    buf = _buf()
    launch, log = _fake_launch(buf)
    assert ops._pick_and_launch(KEY, launch, True) is False
    assert len(log) == PROBES + 1 and bool((buf == 5.0 + PROBES + 1).all())


def test_policy_small_launch_skips_cache_and_race(ops, monkeypatch):
    races = _fake_tune(ops, monkeypatch)
    ops._remember(KEY, 12, dirty=False)
    ops.LAST_TILE = 9
    buf = _buf()
    launch, log = _fake_launch(buf)
    assert ops._pick_and_launch(KEY, launch, False, restore=buf) is False
    assert log == [0] and races == [] and ops.LAST_TILE == 0 and bool((buf == 6.0).all())


class _Clock:
    """stands in for torch.cuda.Event in _ctx_launch: record() reads a counter that the fake launch advances by its mode's cost"""
    now = 0.0

    def __init__(self, enable_timing=False):
        self.t = None

    def record(self):
        self.t = _Clock.now

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        return other.t - self.t


def _ctx_setup(ops, monkeypatch, cost):
    import torch
    monkeypatch.setattr(torch.cuda, "Event", _Clock)
    _Clock.now = 0.0
    buf = _buf()
    log = []

    def launch(mode, prof=None):
        buf.add_(1.0)
        log.append(mode)
        _Clock.now += cost[mode]
    cands = list(cost)
    ops._remember(KEY, cands[0], dirty=False)
    ops._CTX[KEY] = {"cands": cands, "t": {m: [] for m in cands}, "i": 0}
    return buf, launch, log


def test_policy_in_context_sample_is_the_launch(ops, monkeypatch):
    """a pending in-context race: every call is ONE launch of the next candidate and returns True (the caller skips its own); after
    CTX_REPS samples of each the fastest is remembered and the key leaves _CTX"""
    races = _fake_tune(ops, monkeypatch)
    cost = {12: 3.0, 1: 2.0, 30: 2.5}
    buf, launch, log = _ctx_setup(ops, monkeypatch, cost)
    n = len(cost) * ops.CTX_REPS
    for i in range(n):
        assert KEY in ops._CTX
        assert ops._pick_and_launch(KEY, launch, True, restore=buf) is True
        assert len(log) == i + 1 and bool((buf == 5.0 + i + 1).all())
    assert log == [12, 1, 30] * ops.CTX_REPS and KEY not in ops._CTX and ops._TILE[KEY] == 1 and ops._DIRTY and races == []
    assert ops._pick_and_launch(KEY, launch, True, restore=buf) is False
    assert log[-1] == 1 and ops.LAST_TILE == 1 and len(log) == n + 1


def test_policy_in_context_race_waits_outside_a_profile_window(ops, monkeypatch):
    cost = {12: 3.0, 1: 2.0, 30: 2.5}
    buf, launch, log = _ctx_setup(ops, monkeypatch, cost)
    ops.PROFILE = []
    assert ops._pick_and_launch(KEY, launch, True, restore=buf) is False           # the caller records this launch itself
    assert log == [12] and ops.LAST_TILE == 12 and ops._CTX[KEY]["i"] == 0 and not any(ops._CTX[KEY]["t"].values())


def test_finalize_autotune_picks_among_the_sampled_candidates(ops, monkeypatch):
    cost = {12: 3.0, 1: 2.0, 30: 0.5}
    buf, launch, log = _ctx_setup(ops, monkeypatch, cost)
    for _ in range(2):                                                             # 12 and 1 sampled; 30, the fastest, never ran
        assert ops._pick_and_launch(KEY, launch, True, restore=buf) is True
    ops.finalize_autotune()
    assert not ops._CTX and ops._TILE[KEY] == 1
    # no sample at all: the isolated race's pick stays
    other = ("gemm", 4624, 4096, 1024, 1, 0)
    ops._remember(other, 13)
    ops._CTX[other] = {"cands": [13, 2], "t": {13: [], 2: []}, "i": 0}
    ops.finalize_autotune()
    assert not ops._CTX and ops._TILE[other] == 13


def test_split3_candidates_depend_on_m_only_above_the_small_launches(ops):
    assert ops._split3_modes(ops.SPLIT3_SMALL_M) == ops.SPLIT3_MODES
    big = ops._split3_modes(ops.SPLIT3_SMALL_M + 1)
    assert set(ops.SPLIT3_MODES) - set(big) == set(ops.SPLIT3_RING_MODES) and len(big) == len(ops.SPLIT3_MODES) - len(ops.SPLIT3_RING_MODES)
