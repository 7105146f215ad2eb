"""CPU side of the threshold (range) search over the u8 codes: the numpy restatement (tests/search_range_ref.py) against an fp64 brute
force, the host union-find, the score a row has against itself, and the refusals of the CLI and of CodeIndex that need no GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as ref  # noqa: E402
import search_range_ref as rref  # noqa: E402


def _planted(rng, n, dim):
    """random quantised unit codes with exact copies and copies 1, 8, 64 and `dim` codes off planted among them"""
    db = ref.quantised_unit_codes(rng, n, dim)
    db[n - 1] = db[0]
    for row, count in ((n - 2, 1), (n - 3, 8), (n - 4, min(64, dim)), (n - 5, dim)):
        db[row] = rref.nudged(rng, db[1], count)
    return db


@pytest.mark.parametrize("dim", [64, 512])
def test_restatement_against_fp64_brute_force(dim):
    """membership equals the fp64 cosine's for every pair further than 2e-6 from T (five fp32 roundings of at most 2^-24 relative
    on |score| <= 1 are 3e-7); the thresholds are chosen so that no pair of this seeded corpus lies inside that band"""
    rng = np.random.default_rng(dim)
    db = _planted(rng, 300, dim)
    q = np.concatenate([db[:40], ref.quantised_unit_codes(rng, 10, dim)])
    vq, vd = 2.0 * q.astype(np.float64) - 255.0, 2.0 * db.astype(np.float64) - 255.0
    full = (vq @ vd.T) / np.sqrt((vq * vq).sum(axis=1))[:, None] / np.sqrt((vd * vd).sum(axis=1))[None, :]
    for T in (0.99999, 0.999, 0.99, 0.95, 0.3):
        assert np.abs(full - T).min() > 2e-6, (T, np.abs(full - T).min())
        hq, hd, hs, count = rref.range_hits(q, db, T)
        want = np.argwhere(full >= T)
        assert count == len(want) and np.array_equal(np.stack([hq, hd], axis=1), want), T
        assert np.abs(hs.astype(np.float64) - full[hq, hd]).max() <= 2e-6
        lims, s, idx = rref.range_search(q, db, T)
        assert lims[0] == 0 and lims[-1] == count and np.array_equal(np.diff(lims), (full >= T).sum(axis=1))
        assert np.array_equal(idx, hd) and np.array_equal(s.view(np.uint32), hs.view(np.uint32))
    # the self-join is the upper triangle of the corpus against itself
    fd = (vd @ vd.T) / np.sqrt((vd * vd).sum(axis=1))[:, None] / np.sqrt((vd * vd).sum(axis=1))[None, :]
    assert np.abs(fd - 0.99).min() > 2e-6
    hi, hj, _, count = rref.range_hits(db, db, 0.99, self_join=True)
    want = np.argwhere(np.triu(fd >= 0.99, 1))
    assert count == len(want) >= 4 and np.array_equal(np.stack([hi, hj], axis=1), want)
    assert rref.groups(hi, hj)[0] == [0, 299]
    if dim == 512:                                 # 1, 8 and 64 codes off stay above 0.99, all 512 off (about 0.985) does not
        assert rref.groups(hi, hj) == [[0, 299], [1, 296, 297, 298]]


@pytest.mark.parametrize("dim", [64, 512, 4096])
def test_self_score_is_one_of_four_values(dim):
    """a row against itself: float32(N) * r * r with N = sum (2c - 255)^2 lands on one of four fp32 values in [1 - 2^-23, 1 + 2^-23],
    so T = 1.0 would lose some identical pairs; 0.99999 keeps them all"""
    rng = np.random.default_rng(dim)
    codes = ref.quantised_unit_codes(rng, 2000, dim)
    r = ref.rnorm(codes)
    v = 2 * codes.astype(np.int64) - 255
    self_score = ((v * v).sum(axis=1).astype(np.float32) * r) * r
    _, score = ref.keys_and_scores(codes[:50], codes[:50])
    assert np.array_equal(np.diag(score).view(np.uint32), self_score[:50].view(np.uint32))
    four = np.array([1 - 2.0 ** -23, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23], dtype=np.float32)
    assert np.isin(self_score, four).all(), np.unique(self_score)
    assert (self_score < 1).any()                                   # why "identical" is not T = 1.0
    assert (self_score >= np.float32(0.99999)).all()


def test_near_duplicate_scores_are_well_separated():
    """the table behind the --threshold help, D = 512: one code off <= 0.99997, 64 off about 0.998, all off about 0.985, unrelated
    rows < 0.2"""
    rng = np.random.default_rng(1)
    db = ref.quantised_unit_codes(rng, 200, 512)
    one = np.stack([rref.nudged(rng, row, 1) for row in db])
    some = np.stack([rref.nudged(rng, row, 64) for row in db])
    every = np.stack([rref.nudged(rng, row, 512) for row in db])
    pair = lambda a: np.diag(ref.keys_and_scores(a, db)[1])   # noqa: E731
    assert pair(one).max() <= 0.99997
    assert 0.9975 < pair(some).min() and pair(some).max() < 0.9985
    assert 0.983 < pair(every).min() and pair(every).max() < 0.987
    _, score = ref.keys_and_scores(db, db)
    assert score[~np.eye(200, dtype=bool)].max() < 0.2


def test_duplicate_groups_on_pair_lists():
    import sgic_amd  # noqa
    from sgic_amd.search import duplicate_groups
    assert duplicate_groups([], []) == []
    assert duplicate_groups(np.zeros(0, np.int32), np.zeros(0, np.int32)) == []
    assert duplicate_groups([3], [9]) == [[3, 9]]
    assert duplicate_groups([0, 1, 2], [1, 2, 3]) == [[0, 1, 2, 3]]                        # a chain
    assert duplicate_groups([7, 5, 3], [9, 7, 5]) == [[3, 5, 7, 9]]                        # a chain given backwards
    assert duplicate_groups([2, 2, 2, 2], [3, 50, 7, 11]) == [[2, 3, 7, 11, 50]]           # a star
    assert duplicate_groups([10, 0, 11, 1], [11, 1, 12, 2]) == [[0, 1, 2], [10, 11, 12]]   # two groups, ordered by first member
    assert duplicate_groups([4, 1, 1, 6], [6, 8, 4, 8]) == [[1, 4, 6, 8]]                  # two chains joined late
    rng = np.random.default_rng(2)
    i = rng.integers(0, 400, 300)
    j = rng.integers(0, 400, 300)
    keep = i < j
    got = duplicate_groups(i[keep].astype(np.int32), j[keep].astype(np.int32))
    assert got == rref.groups(i[keep], j[keep])
    assert all(isinstance(m, int) for g in got for m in g)


def test_exported_from_the_library():
    import sgic_amd  # noqa
    from sgic_amd import _lib, ops
    assert hasattr(_lib.lib, "sgic_search_range_u8")
    assert callable(ops.search_codes_range) and callable(ops.search_codes_range_launch)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgic.h")).read()
    assert "int sgic_search_range_u8(" in header


def test_nan_threshold_is_refused_before_any_launch():
    """a ValueError, raised before the index would go to the device (which, without a GPU, is another error)"""
    import sgic_amd  # noqa
    from sgic_amd import search
    rng = np.random.default_rng(3)
    ci = search.CodeIndex(ref.quantised_unit_codes(rng, 8, 64), [f"f{j}" for j in range(8)])
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            ci.range_search(ci.codes[:2], bad)
        with pytest.raises(ValueError):
            ci.duplicate_pairs(bad)
        with pytest.raises(ValueError):
            ci.duplicate_groups(bad)
    assert ci._dev is None


def test_cli_arguments_and_refusals(tmp_path, capsys):
    import sgic_amd  # noqa
    from sgic_amd import search
    empty = tmp_path / "no_index"
    empty.mkdir()
    with pytest.raises(SystemExit):                       # there is deliberately no default threshold
        search.main(["duplicates", "--index_dir", str(empty)])
    with pytest.raises(SystemExit):
        search.main(["duplicates", "--index_dir", str(empty), "--threshold", "nan"])
    assert "finite" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        search.main(["duplicates", "--index_dir", str(empty), "--threshold", "high"])
    with pytest.raises(FileNotFoundError):                # parsed, then no codes.npy
        search.main(["duplicates", "--index_dir", str(empty), "--threshold", "0.99", "--max_pairs", "100", "--out", str(tmp_path / "o")])
    assert not (tmp_path / "o").exists()
    (empty / "ids.txt").write_text("a\nb")                # ids alone are not a code index
    with pytest.raises(FileNotFoundError):
        search.main(["duplicates", "--index_dir", str(empty), "--threshold", "0.99"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        search.main(["query-c2df", "--codes", "--index_dir", str(empty), "--c2df", "x.c2df", "--min_score", "nan"])
    assert "finite" in capsys.readouterr().err
    with pytest.raises(SystemExit):                       # the fp32 index files have no threshold search
        search.main(["query-c2df", "--index_dir", str(empty), "--c2df", "x.c2df", "--min_score", "0.9"])
    assert "--codes" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError):
        search.main(["query-c2df", "--codes", "--index_dir", str(tmp_path / "absent"), "--c2df", "x.c2df", "--min_score", "0.9"])
    with pytest.raises(SystemExit) as e:
        search.main(["duplicates", "--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "0.99999" in text and "0.98-0.99" in text and "2^-23" in text and "no default" in text
    with pytest.raises(SystemExit):
        search.main(["query-c2df", "--help"])
    assert "--topk is ignored" in " ".join(capsys.readouterr().out.split())
