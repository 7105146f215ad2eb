"""CPU side of the clustering over the u8 codes: the numpy restatement (tests/cluster_codes_ref.py) against the fp64 argmax wherever
the fp64 margin exceeds the derived error bound, the host update step centroids_from_sums, the Lloyd loop on planted data, the
ordering rules of cluster_report and the refusals that need no GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_codes_ref as kref  # noqa: E402
import search_vectors_ref as ref  # noqa: E402


@pytest.mark.parametrize("dim", [64, 512, 2048])
def test_restatement_picks_the_fp64_argmax_outside_the_error_band(dim):
    """each score is within error_bound(D) of its fp64 value, so where the fp64 best leads the second best by more than twice that
    the restatement must pick it.  With 17 random centroids the margin between the two best is of the order 0.1 / sqrt(D / 64),
    thousands of times the bound: the share of rows above the margin is asserted, so the condition cannot hide the test"""
    rng = np.random.default_rng(dim)
    db = ref.quantised_unit_codes(rng, 400, dim)
    cent = ref.random_unit(rng, 17, dim)
    full = ref.fp64_scores(cent, db)                       # (K, n)
    top2 = np.sort(full, axis=0)[-2:]
    clear = (top2[1] - top2[0]) > 2 * ref.error_bound(dim)
    assert clear.mean() >= 0.95, clear.mean()
    a, s, M = kref.assign(cent, db, with_int=True)
    assert a.dtype == np.int32 and s.dtype == np.float32 and M.dtype == np.int64
    assert np.array_equal(a[clear], np.argmax(full, axis=0)[clear])
    assert np.abs(s.astype(np.float64) - full[a, np.arange(400)]).max() <= ref.error_bound(dim)
    assert np.array_equal(M, ref.int_scores(ref.quantise(cent), db)[a, np.arange(400)])


def test_restatement_ties_go_to_the_lower_centroid():
    rng = np.random.default_rng(3)
    db = ref.quantised_unit_codes(rng, 50, 64)
    cent = ref.random_unit(rng, 6, 64)
    cent[4] = cent[1]
    a, _ = kref.assign(cent, db)
    assert 1 in a and 4 not in a
    assert np.array_equal(kref.assign(np.repeat(cent[:1], 5, axis=0), db)[0], np.zeros(50, np.int32))


def test_centroids_from_sums():
    import sgic_amd  # noqa
    from sgic_amd.search import centroids_from_sums
    rng = np.random.default_rng(5)
    db = ref.quantised_unit_codes(rng, 300, 512)
    a = rng.integers(0, 6, 300).astype(np.int32)
    a[a == 4] = 0                                          # cluster 4 is empty
    db[a == 5] = 0
    db[np.flatnonzero(a == 5)[::2]] = 255                  # cluster 5: as many rows of -255 as of +255 -> an all-zero sum
    keep = np.flatnonzero(a == 5)
    if keep.size % 2:
        a[keep[-1]] = 0
    s, c = kref.sums(db, a, 6)
    assert c[4] == 0 and c[5] > 0 and not s[5].any() and s[:4].any(axis=1).all()
    prev = ref.random_unit(rng, 6, 512)
    got = centroids_from_sums(s, c, prev)
    assert got.dtype == np.float32 and got.shape == (6, 512)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert np.array_equal(got[4], prev[4]) and np.array_equal(got[5], prev[5])
    for j in range(4):                                     # the direction of the exact integer sum
        want = s[j].astype(np.float64)
        want /= np.sqrt((want * want).sum())
        assert np.array_equal(got[j], want.astype(np.float32))
    perm = rng.permutation(300)                            # member order does not matter: integer sums
    s2, c2 = kref.sums(db[perm], a[perm], 6)
    assert np.array_equal(s2, s) and np.array_equal(c2, c)
    assert np.array_equal(centroids_from_sums(s2, c2, prev).view(np.uint32), got.view(np.uint32))
    assert np.array_equal(prev, centroids_from_sums(np.zeros_like(s), np.zeros_like(c), prev))
    with pytest.raises(ValueError):
        centroids_from_sums(s[:5], c, prev)


def test_lloyd_recovers_a_planted_partition_and_stops_early():
    import sgic_amd  # noqa
    from sgic_amd.search import codes_to_unit
    rng = np.random.default_rng(8)
    db, group, dirs = kref.planted_corpus(rng, 600, 512, 8)
    full = ref.fp64_scores(dirs, db)                       # the planted direction is the unambiguous nearest one
    top2 = np.sort(full, axis=0)[-2:]
    assert np.array_equal(np.argmax(full, axis=0), group) and (top2[1] - top2[0]).min() > 0.5 > 2 * ref.error_bound(512)
    res = kref.lloyd(db, codes_to_unit(db[:8]), 10)        # rows 0 .. 7: one member of each group, in group order
    assert np.array_equal(res["assign"], group)
    assert res["moved"][0] == 600 and res["moved"][-1] == 0 and res["iters_run"] == len(res["moved"]) < 10
    assert np.array_equal(res["counts"], np.bincount(group, minlength=8)) and res["counts"].sum() == 600
    assert np.abs(np.linalg.norm(res["centroids"].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert (np.sum(res["centroids"].astype(np.float64) * dirs, axis=1) > 0.99).all()       # the mean of ~75 members: noise / sqrt(75)
    a, s = kref.assign(res["centroids"], db)               # assign and score belong to the returned centroids
    assert np.array_equal(a, res["assign"]) and np.array_equal(s.view(np.uint32), res["score"].view(np.uint32))
    cut = kref.lloyd(db, codes_to_unit(db[:8]), 1)         # iters used up: one update, then the final assign
    assert cut["moved"] == [600] and cut["iters_run"] == 1 and np.array_equal(cut["assign"], group)
    assert not np.array_equal(cut["centroids"], codes_to_unit(db[:8]))


def test_cluster_report_ordering_rules():
    import sgic_amd  # noqa
    from sgic_amd.search import cluster_report
    #                 row: 0    1    2    3    4    5    6    7    8
    assign = np.array([2,   0,   2,   5,   0,   2,   5,   0,   7], dtype=np.int32)
    score = np.array([0.5, 0.9, 0.7, 0.3, 0.9, 0.7, 0.3, 0.1, 0.4], dtype=np.float32)
    rep = cluster_report(assign, score)
    # sizes 3, 3, 2, 1: the tie between clusters 0 and 2 goes to the lower index; clusters 1, 3, 4, 6 are empty and absent
    assert [(c["cluster"], c["size"]) for c in rep] == [(0, 3), (2, 3), (5, 2), (7, 1)]
    # members score descending, equal scores to the lower row; the representative is the first
    assert [c["members"].tolist() for c in rep] == [[1, 4, 7], [2, 5, 0], [3, 6], [8]]
    assert [c["representative"] for c in rep] == [1, 2, 3, 8]
    assert cluster_report(np.zeros(0, np.int32), np.zeros(0, np.float32)) == []
    with pytest.raises(ValueError):
        cluster_report(assign, score[:5])


def test_exported_and_declared():
    import sgic_amd  # noqa
    from sgic_amd import _lib, ops
    for name in ("sgic_assign_codes_f32c", "sgic_assign_codes_f32c_work_bytes", "sgic_cluster_sums_u8"):
        assert hasattr(_lib.lib, name)
    assert callable(ops.assign_codes) and callable(ops.cluster_sums)


def test_refusals_run_before_the_device_library_is_loaded(tmp_path, capsys):
    """in a fresh interpreter state of the package: the argument errors of the command, of kmeans and of assign come before
    sgic_amd.ops (and with it libsgic.so) is imported, and nothing is sent to a device"""
    import sgic_amd  # noqa
    from sgic_amd import search
    from sgic_amd.search import CodeIndex
    loaded = {m: sys.modules.pop(m) for m in ("sgic_amd.ops", "sgic_amd._lib") if m in sys.modules}
    attrs = {a: getattr(sgic_amd, a) for a in ("ops", "_lib") if hasattr(sgic_amd, a)}
    for a in attrs:
        delattr(sgic_amd, a)                               # `from . import ops` would otherwise be served by the attribute
    try:
        rng = np.random.default_rng(9)
        ci = CodeIndex(ref.quantised_unit_codes(rng, 20, 64), [f"id{j}" for j in range(20)])
        ci.save(tmp_path / "index")
        base = ["clusters", "--index_dir", str(tmp_path / "index")]
        for bad, word in ((["--k", "0"], "--k"), (["--k", "65537"], "--k"), (["--k", "3", "--iters", "0"], "--iters"),
                          (["--k", "3", "--members", "-2"], "--members")):
            capsys.readouterr()
            with pytest.raises(SystemExit):
                search.main(base + bad)
            assert word in capsys.readouterr().err
        with pytest.raises(ValueError, match="k = 21"):
            search.main(base + ["--k", "21"])              # more clusters than rows: known once the index is read
        with pytest.raises(FileNotFoundError):
            search.main(["clusters", "--index_dir", str(tmp_path / "absent"), "--k", "2"])
        for k, iters in ((0, 10), (21, 10), (65537, 10), (3, 0)):
            with pytest.raises(ValueError):
                ci.kmeans(k, iters=iters)
        with pytest.raises(ValueError, match="init"):
            ci.kmeans(3, init=ref.random_unit(rng, 4, 64))
        with pytest.raises(ValueError, match="unit"):
            ci.kmeans(3, init=2.0 * ref.random_unit(rng, 3, 64))
        cent = ref.random_unit(rng, 3, 64)
        bad = cent.copy()
        bad[1, 7] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            ci.assign(bad)
        with pytest.raises(ValueError, match="unit"):
            ci.assign(2.0 * cent)
        with pytest.raises(ValueError, match="dim"):
            ci.assign(ref.random_unit(rng, 3, 128))
        with pytest.raises(ValueError, match="centroids"):
            ci.assign(np.zeros((0, 64), np.float32))
        big = CodeIndex(rng.integers(0, 256, (4, 4096), dtype=np.uint8), list("abcd"))
        with pytest.raises(ValueError, match="2048"):
            big.assign(ref.random_unit(rng, 1, 4096))
        with pytest.raises(ValueError, match="2048"):
            big.kmeans(2)
        assert ci._dev is None and big._dev is None
        assert "sgic_amd.ops" not in sys.modules and "sgic_amd._lib" not in sys.modules
    finally:
        sys.modules.update(loaded)
        for a, mod in attrs.items():
            setattr(sgic_amd, a, mod)
