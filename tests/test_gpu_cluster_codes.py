"""GPU: clustering over the u8 codes (csrc/search.hip assign_codes_kernel and cluster_sums_kernel through ops.assign_codes and
ops.cluster_sums, search.CodeIndex.assign / kmeans and the `clusters` command) against the numpy restatement
(tests/cluster_codes_ref.py): cluster ids, M, score bits, sums, counts, centroids -- bit for bit, everywhere."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_codes_ref as kref  # noqa: E402
import search_vectors_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# D = 512 keeps the database fragments in registers, every other D re-reads them; 16 centroids are one tile, 17 / 33 leave 15 pad
# slots, 300 is 19 tiles (several staging rounds at every D); 256 rows are one workgroup, 64 one wave, 16 one row tile
_D64 = [(n, K) for n in (1, 17, 64, 1000, 4097) for K in (1, 5, 16, 17, 33, 300)]
SHAPES = {64: _D64,
          512: [(1, 1), (17, 5), (64, 16), (1000, 17), (4097, 33), (1000, 300), (4097, 5), (64, 300)],
          576: [(17, 5), (1000, 33), (4097, 17), (64, 300), (1, 16)],
          2048: [(17, 5), (64, 33), (1000, 17), (1, 300), (300, 16)]}


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu_assign(cent, db):
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    c, s, M = ops.assign_codes(_up(np.asarray(cent, dtype=np.float32)), _up(db), _up(code_rnorm(db)), return_int=True)
    assert c.dtype == torch.int32 and s.dtype == torch.float32 and M.dtype == torch.int64 and c.shape == s.shape == M.shape == (db.shape[0],)
    return c.cpu().numpy(), s.cpu().numpy(), M.cpu().numpy()


def _same_assign(got, want, what):
    (gc, gs, gM), (wc, ws, wM) = got, want
    assert np.array_equal(gM, wM), (what, np.flatnonzero(gM != wM)[:4].tolist())
    assert np.array_equal(gc, wc), (what, np.flatnonzero(gc != wc)[:4].tolist())
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, np.flatnonzero(gs != ws)[:4].tolist())


def _check_assign(cent, db, what):
    _same_assign(_gpu_assign(cent, db), kref.assign(cent, db, with_int=True), what)


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_assign_bit_equal(dim):
    rng = np.random.default_rng(dim)
    for n, K in SHAPES[dim]:
        _check_assign(ref.random_unit(rng, K, dim), ref.quantised_unit_codes(rng, n, dim), (dim, n, K))


@pytest.mark.parametrize("dim", [64, 512])
def test_ties_go_to_the_lower_centroid(dim):
    rng = np.random.default_rng(dim + 1)
    db = ref.quantised_unit_codes(rng, 1000, dim)
    cent = ref.random_unit(rng, 300, dim)
    cent[290] = cent[3]                                    # equal M in different tiles, lane groups and staging rounds
    cent[17] = cent[16]                                    # and in neighbouring slots of one lane
    cent[200] = cent[8]
    want = kref.assign(cent, db, with_int=True)
    assert {3, 16, 8} <= set(want[0].tolist()) and not {290, 17, 200} & set(want[0].tolist())
    _same_assign(_gpu_assign(cent, db), want, ("duplicates", dim))
    same = np.repeat(ref.random_unit(rng, 1, dim), 33, axis=0)
    got = _gpu_assign(same, db)
    assert not got[0].any()
    _same_assign(got, kref.assign(same, db, with_int=True), ("all equal", dim))
    zero = np.zeros((33, dim), np.float32)                 # M = 0 everywhere
    got = _gpu_assign(zero, db)
    assert not got[0].any() and not got[2].any() and not got[1].any()


def test_plane_and_lane_placement_one_hot_centroids():
    """centroid 16 b + i holds 256^b * 2^-22 at coordinate p_i and 0 elsewhere: digit plane b is 1 there, every other digit 0, so
    M(16 b + i, j) = 256^b (2 c[j][p_i] - 255) on a database that is asymmetric in (row, coordinate).  A call
    with one centroid returns M(k, .) itself, so every (centroid, row) pair is checked; then the argmax over all 48, over each plane's
    16 and over 3 that straddle two planes.  A swapped plane, a wrong plane weight or a lane-map error of either MFMA operand gives a
    wrong integer"""
    dim, n = 512, 48
    pos = (np.arange(16) * 37 + 5) % dim
    cent = np.zeros((48, dim), np.float32)
    for b, val in enumerate((2.0 ** -22, 2.0 ** -14, 2.0 ** -6)):
        cent[16 * b + np.arange(16), pos] = val
    j, c = np.meshgrid(np.arange(n), np.arange(dim), indexing="ij")
    db = ((7 * j * j + 3 * c + 11 * j * c + (c >> 4)) % 256).astype(np.uint8)
    v = 2 * db.astype(np.int64) - 255
    want = np.concatenate([256 ** b * v[:, pos].T for b in range(3)])          # (48, n)
    assert np.array_equal(ref.int_scores(ref.quantise(cent), db), want)
    for k in range(48):                                    # one centroid: out_M is M(k, .) itself
        gc, _, gM = _gpu_assign(cent[k:k + 1], db)
        assert not gc.any() and np.array_equal(gM, want[k]), k
    for rows in (slice(0, 48), slice(0, 16), slice(16, 32), slice(32, 48), slice(30, 33)):
        gc, _, gM = _gpu_assign(cent[rows], db)
        assert np.array_equal(gM, want[rows].max(axis=0)) and np.array_equal(gc, want[rows].argmax(axis=0)), rows
    for dim2 in (64, 576):                                 # the path that re-reads the fragments
        pos2 = (np.arange(16) * 37 + 5) % dim2
        cent2 = np.zeros((48, dim2), np.float32)
        for b, val in enumerate((2.0 ** -22, 2.0 ** -14, 2.0 ** -6)):
            cent2[16 * b + np.arange(16), pos2] = val
        db2 = np.ascontiguousarray(np.resize(db, (n, dim2)))
        v2 = 2 * db2.astype(np.int64) - 255
        want2 = np.concatenate([256 ** b * v2[:, pos2].T for b in range(3)])
        gc, _, gM = _gpu_assign(cent2, db2)
        assert np.array_equal(gM, want2.max(axis=0)) and np.array_equal(gc, want2.argmax(axis=0)), dim2


def test_digit_edges_and_nan_coordinate():
    rng = np.random.default_rng(13)
    db = np.concatenate([ref.quantised_unit_codes(rng, 80, 64), rng.integers(0, 256, (20, 64), dtype=np.uint8)])
    cent = ref.random_unit(rng, 5, 64)
    cent[1] = np.resize(np.array(ref.EDGE_Q, dtype=np.float64) / ref.SCALE, 64).astype(np.float32)
    cent[1, 40] = np.nan                                   # the device takes it as 0; CodeIndex refuses such a centroid
    _check_assign(cent, db, "digit edges")


def test_scores_are_the_bits_of_the_fp32_query_search():
    import sgic_amd  # noqa
    from sgic_amd import ops
    from sgic_amd.search import code_rnorm
    rng = np.random.default_rng(31)
    n, K = 100, 5
    db, cent = ref.quantised_unit_codes(rng, n, 512), ref.random_unit(rng, K, 512)
    gc, gs, _ = _gpu_assign(cent, db)
    s, i = ops.search_codes_f32q(_up(cent), _up(db), _up(code_rnorm(db)), n)      # k = n: every (centroid, row) pair once
    s, i = s.cpu().numpy(), i.cpu().numpy()
    full = np.empty((K, n), np.float32)
    np.put_along_axis(full, i.astype(np.int64), s, axis=1)
    assert np.array_equal(gs.view(np.uint32), full[gc, np.arange(n)].view(np.uint32))
    assert np.array_equal(gs, full.max(axis=0))            # and it is the best score of the row


def test_padding_and_canaries():
    """the kernel reads K centroids of an oversized buffer whose rest is NaN, and writes n entries of oversized outputs"""
    import sgic_amd  # noqa
    from sgic_amd import _lib, ops
    from sgic_amd.search import code_rnorm
    import ctypes
    rng = np.random.default_rng(32)
    for dim, n, K in ((512, 300, 17), (64, 70, 5)):
        db, cent = ref.quantised_unit_codes(rng, n, dim), ref.random_unit(rng, K, dim)
        want = kref.assign(cent, db, with_int=True)
        buf = torch.full((K + 40, dim), float("nan"), dtype=torch.float32, device=DEV)
        buf[:K] = _up(cent)
        nbytes = ctypes.c_size_t(0)
        _lib.call("sgic_assign_codes_f32c_work_bytes", K, dim, ctypes.byref(nbytes))
        assert nbytes.value == (K + 15) // 16 * 16 * (3 * dim + 8)
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
        oc = torch.full((n + 512,), -7, dtype=torch.int32, device=DEV)
        oM = torch.full((n + 512,), -7, dtype=torch.int64, device=DEV)
        _lib.call("sgic_assign_codes_f32c", buf, _up(db), K, n, dim, work, ctypes.c_size_t(nbytes.value), oc, oM)
        assert bool((oc[n:] == -7).all()) and bool((oM[n:] == -7).all())
        assert np.array_equal(oc[:n].cpu().numpy(), want[0]) and np.array_equal(oM[:n].cpu().numpy(), want[2])
        # the sums: oversized outputs, the ABI call adds to what is there
        a = _up(want[0])
        sa, order = torch.sort(a, stable=True)
        sums = torch.full((K + 3, dim), 5, dtype=torch.int64, device=DEV)
        counts = torch.full((K + 3,), 5, dtype=torch.int64, device=DEV)
        _lib.call("sgic_cluster_sums_u8", _up(db), order, sa, n, dim, K, sums, counts)
        ws, wc = kref.sums(db, want[0], K)
        assert bool((sums[K:] == 5).all()) and bool((counts[K:] == 5).all())
        assert np.array_equal(sums[:K].cpu().numpy(), ws + 5) and np.array_equal(counts[:K].cpu().numpy(), wc + 5)


def _check_sums(db, a, K, what):
    import sgic_amd  # noqa
    from sgic_amd import ops
    a = np.asarray(a, dtype=np.int32)
    s, c = ops.cluster_sums(_up(db), _up(a), K)
    assert s.dtype == torch.int64 and c.dtype == torch.int64 and s.shape == (K, db.shape[1]) and c.shape == (K,)
    ws, wc = kref.sums(db, a, K)
    assert np.array_equal(c.cpu().numpy(), wc), what
    assert np.array_equal(s.cpu().numpy(), ws), what
    return s, c


@pytest.mark.parametrize("dim", [64, 512, 576, 2048])
def test_cluster_sums_bit_equal(dim):
    rng = np.random.default_rng(dim + 2)
    for n in (1, 17, 64, 1000, 4097) if dim != 2048 else (1, 17, 1000):
        db = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        for K in (1, 5, 33, 300):
            _check_sums(db, rng.integers(0, K, n), K, ("random", dim, n, K))
        _check_sums(db, np.zeros(n), 5, ("all rows in one cluster", dim, n))
        _check_sums(db, np.full(n, 4), 5, ("all rows in the last cluster", dim, n))
        _check_sums(db, rng.permutation(n), n, ("one row per cluster", dim, n))
        _check_sums(db, 7 * rng.integers(0, 3, n), 40, ("empty clusters", dim, n))


def test_cluster_sums_large_cluster_and_reproducibility():
    """5000 members of one cluster at D = 64 span five workgroup slices; extreme codes; the same partition given in another row
    order gives the same bytes"""
    rng = np.random.default_rng(40)
    n = 7000
    db = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    db[:3000] = 255
    db[3000:3500] = 0
    a = np.full(n, 2)
    a[5000:] = rng.integers(0, 6, 2000)
    s1, c1 = _check_sums(db, a, 6, "5000 members")
    assert int(c1[2]) >= 5000
    perm = rng.permutation(n)
    s2, c2 = _check_sums(db[perm], a[perm], 6, "shuffled")
    s3, c3 = _check_sums(db, a, 6, "again")
    for s, c in ((s2, c2), (s3, c3)):
        assert torch.equal(s, s1) and torch.equal(c, c1)


def _same_kmeans(got, want, what):
    assert got["iters_run"] == want["iters_run"] and got["moved"] == want["moved"], (what, got["moved"], want["moved"])
    assert np.array_equal(got["assign"], want["assign"]) and got["assign"].dtype == np.int32, what
    assert np.array_equal(got["centroids"].view(np.uint32), want["centroids"].view(np.uint32)), what
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), what
    assert np.array_equal(got["counts"], want["counts"]), what


@pytest.fixture(scope="module")
def planted():
    import sgic_amd  # noqa
    rng = np.random.default_rng(50)
    db, group, _ = kref.planted_corpus(rng, 2000, 512, 8)
    return db, group


def test_kmeans_against_the_restated_loop(planted):
    from sgic_amd.search import CodeIndex, codes_to_unit
    db, group = planted
    ci = CodeIndex(db, [str(j) for j in range(len(db))])
    init = codes_to_unit(db[:8])                           # one member of each planted group
    got = ci.kmeans(8, iters=10, init=init)
    _same_kmeans(got, kref.lloyd(db, init, 10), "planted, init")
    assert np.array_equal(got["assign"], group) and got["moved"][-1] == 0 and got["iters_run"] < 10
    _same_kmeans(ci.kmeans(8, iters=6, seed=1), kref.lloyd(db, kref.default_init(db, 8, 1), 6), "planted, seed 1")
    a, s = ci.assign(got["centroids"])                     # the public assignment, on the result's own centroids
    assert np.array_equal(a, got["assign"]) and np.array_equal(s.view(np.uint32), got["score"].view(np.uint32))
    one = ci.kmeans(1, iters=1)
    assert not one["assign"].any() and one["moved"] == [2000] and one["iters_run"] == 1 and one["counts"].tolist() == [2000]
    _same_kmeans(one, kref.lloyd(db, kref.default_init(db, 1, 0), 1), "k = 1")


def test_kmeans_random_codes():
    import sgic_amd  # noqa
    from sgic_amd.search import CodeIndex
    rng = np.random.default_rng(51)
    db = ref.quantised_unit_codes(rng, 1000, 512)
    ci = CodeIndex(db, [str(j) for j in range(1000)])
    want = kref.lloyd(db, kref.default_init(db, 17, 3), 4)
    assert want["moved"][-1] > 0                           # still moving: the final assign after the loop is exercised
    _same_kmeans(ci.kmeans(17, iters=4, seed=3), want, "random, k = 17")


def test_cli_clusters(planted, tmp_path, capsys):
    from sgic_amd import search
    from sgic_amd.search import CodeIndex, cluster_report
    db, group = planted
    ids = [f"img/{j:04d}.jpg" for j in range(len(db))]
    CodeIndex(db, ids).save(tmp_path / "index")
    want = kref.lloyd(db, kref.default_init(db, 8, 2), 10)
    rep = cluster_report(want["assign"], want["score"])
    capsys.readouterr()
    assert search.main(["clusters", "--index_dir", str(tmp_path / "index"), "--k", "8", "--seed", "2", "--members", "3",
                        "--save_dir", str(tmp_path / "saved")]) == 0
    cap = capsys.readouterr()
    lines = [json.loads(ln) for ln in cap.out.splitlines()]
    assert [(e["cluster"], e["size"]) for e in lines] == [(c["cluster"], c["size"]) for c in rep] and len(lines) >= 2
    assert [e["size"] for e in lines] == sorted((e["size"] for e in lines), reverse=True) and sum(e["size"] for e in lines) == 2000
    for e, c in zip(lines, rep):
        assert set(e) == {"cluster", "size", "representative", "mean_score", "members"}
        assert e["representative"] == ids[c["representative"]] == e["members"][0]["path"]
        assert e["members"] == [{"path": ids[r], "score": float(want["score"][r])} for r in c["members"][:3]]
        assert e["mean_score"] == float(want["score"][c["members"]].astype(np.float64).mean())
    assert "2000 rows" in cap.err and "k = 8" in cap.err and str(want["moved"]) in cap.err
    assert np.array_equal(np.load(tmp_path / "saved" / "centroids.npy").view(np.uint32), want["centroids"].view(np.uint32))
    assert np.array_equal(np.load(tmp_path / "saved" / "assign.npy"), want["assign"])
    assert json.loads((tmp_path / "saved" / "clusters.json").read_text()) == {
        "n": 2000, "dim": 512, "k": 8, "seed": 2, "iters_run": want["iters_run"], "moved": want["moved"]}
    out = tmp_path / "all.jsonl"                           # --members -1 lists every member, --out writes a file
    assert search.main(["clusters", "--index_dir", str(tmp_path / "index"), "--k", "8", "--seed", "2", "--members", "-1",
                        "--out", str(out)]) == 0
    assert capsys.readouterr().out == ""
    full = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert [len(e["members"]) for e in full] == [c["size"] for c in rep]
    assert [[m["path"] for m in e["members"]] for e in full] == [[ids[r] for r in c["members"]] for c in rep]


def test_refusals_come_before_any_launch():
    import sgic_amd  # noqa
    from sgic_amd import _lib, ops
    from sgic_amd.search import CodeIndex, code_rnorm
    import ctypes
    rng = np.random.default_rng(60)
    db = ref.quantised_unit_codes(rng, 70, 64)
    ddb, r = _up(db), _up(code_rnorm(db))
    for dim in (96, 2112, 4096):                           # D % 64, D > 2048
        with pytest.raises(_lib.SgicError):
            ops.assign_codes(_up(ref.random_unit(rng, 3, dim)), _up(rng.integers(0, 256, (70, dim), dtype=np.uint8)), r)
    with pytest.raises(_lib.SgicError):                    # K > 65536
        ops.assign_codes(torch.zeros(65537, 64, device=DEV), ddb, r)
    cent = _up(ref.random_unit(rng, 3, 64))
    nbytes = 48 * (3 * 64 + 8)
    work = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
    oc = torch.full((70,), -7, dtype=torch.int32, device=DEV)
    oM = torch.full((70,), -7, dtype=torch.int64, device=DEV)
    size = ctypes.c_size_t
    bad = [(cent, ddb, 0, 70, 64, work, size(nbytes), oc, oM),                # K < 1
           (cent, ddb, 3, 0, 64, work, size(nbytes), oc, oM),                 # n < 1
           (cent, ddb, 3, 70, 64, work, size(16 * (3 * 64 + 8) - 1), oc, oM),  # the workspace is too small
           (None, ddb, 3, 70, 64, work, size(nbytes), oc, oM),                # null pointers
           (cent, ddb, 3, 70, 64, None, size(nbytes), oc, oM),
           (cent, ddb, 3, 70, 64, work, size(nbytes), None, oM),
           (cent, ddb, 3, 70, 64, work[8:], size(nbytes), oc, oM),            # misaligned workspace and codes
           (cent, ddb.reshape(-1)[8:8 + 64 * 69].reshape(69, 64), 3, 69, 64, work, size(nbytes), oc, oM)]
    for args in bad:
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call("sgic_assign_codes_f32c", *args)
    assert bool((oc == -7).all()) and bool((oM == -7).all())
    a = _up(rng.integers(0, 5, 70).astype(np.int32))
    for wrong in (torch.where(a == 2, torch.full_like(a, 5), a), torch.where(a == 2, torch.full_like(a, -1), a)):
        with pytest.raises(ValueError, match="outside"):
            ops.cluster_sums(ddb, wrong, 5)
    with pytest.raises(_lib.SgicError, match="rc=-1"):     # D % 16
        ops.cluster_sums(_up(rng.integers(0, 256, (70, 72), dtype=np.uint8)), a, 5)
    ci = CodeIndex(db, [str(j) for j in range(70)])
    for k, iters in ((0, 10), (71, 10), (3, 0)):
        with pytest.raises(ValueError):
            ci.kmeans(k, iters=iters)
    with pytest.raises(ValueError):
        ci.assign(_up(2.0 * ref.random_unit(rng, 3, 64)))
    big = CodeIndex(rng.integers(0, 256, (4, 4096), dtype=np.uint8), list("abcd"))
    with pytest.raises(ValueError, match="2048"):
        big.assign(ref.random_unit(rng, 1, 4096))
    assert ci._dev is None and big._dev is None
