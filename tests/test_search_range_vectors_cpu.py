"""CPU side of the threshold (range) search of fp32 queries over the u8 codes: the numpy restatement
(tests/search_range_vectors_ref.py) against the fp64 scores within the derived error bound, the >= at a pair's own score, and the
refusals of the CLI and of CodeIndex.range_search_vectors that need no GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_range_vectors_ref as rref  # noqa: E402
import search_vectors_ref as ref  # noqa: E402


@pytest.mark.parametrize("dim", [64, 512])
def test_restatement_against_fp64_within_the_error_bound(dim):
    """every pair whose fp64 score is >= T + error_bound(D) is a hit, no pair whose fp64 score is < T - error_bound(D) is; what lies
    inside the band may fall either way"""
    import sgic_amd  # noqa
    from sgic_amd.search import codes_to_unit
    rng = np.random.default_rng(dim)
    db = ref.quantised_unit_codes(rng, 300, dim)
    q = np.concatenate([codes_to_unit(db[:8]), ref.random_unit(rng, 32, dim)])     # planted: a row's own dequantised vector
    full = ref.fp64_scores(q, db)
    bound = ref.error_bound(dim)
    loose = 0.3 if dim == 64 else 0.1                                               # random pairs pass it too
    for T in (0.999, 0.99, loose, 0.0, -2.0):
        hq, hd, hs, count = rref.range_hits(q, db, T)
        hit = np.zeros(full.shape, dtype=bool)
        hit[hq, hd] = True
        assert count == hit.sum() == hq.size
        assert hit[full >= T + bound].all(), T
        assert not hit[full < T - bound].any(), T
        assert np.abs(hs.astype(np.float64) - full[hq, hd]).max() <= bound
        assert np.array_equal(np.stack([hq, hd], axis=1), np.argwhere(hit))         # (q, d) ascending
        lims, s, idx = rref.range_search(q, db, T)
        assert lims[0] == 0 and lims[-1] == count and np.array_equal(np.diff(lims), hit.sum(axis=1))
        assert np.array_equal(idx, hd) and np.array_equal(s.view(np.uint32), hs.view(np.uint32))
    assert all((j, j) in set(zip(*rref.range_hits(q, db, 0.999)[:2])) for j in range(8))
    assert 8 < rref.range_hits(q, db, loose)[3] < q.shape[0] * db.shape[0]


def test_own_score_is_kept_and_the_next_float_is_not():
    rng = np.random.default_rng(7)
    db = ref.quantised_unit_codes(rng, 100, 64)
    q = ref.random_unit(rng, 5, 64)
    _, score = ref.keys_and_scores(q, db)
    for pair in ((0, 0), (3, 77), (4, 99)):
        own = score[pair]
        hq, hd, hs, _ = rref.range_hits(q, db, own)
        at = [k for k, p in enumerate(zip(hq.tolist(), hd.tolist())) if p == pair]
        assert len(at) == 1 and hs[at[0]].view(np.uint32) == own.view(np.uint32)
        hq, hd, _, _ = rref.range_hits(q, db, np.nextafter(own, np.float32(np.inf)))
        assert pair not in set(zip(hq.tolist(), hd.tolist()))


def test_exported_from_the_library():
    import sgic_amd  # noqa
    from sgic_amd import _lib, ops
    assert hasattr(_lib.lib, "sgic_search_range_f32q")
    assert callable(ops.search_codes_range_f32q) and callable(ops.search_codes_range_f32q_launch)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgic.h")).read()
    assert "int sgic_search_range_f32q(" in header


def test_cli_refusals_run_before_any_load(tmp_path, capsys):
    import sgic_amd  # noqa
    from sgic_amd import search
    empty = tmp_path / "no_index"
    empty.mkdir()
    for cmd, arg in (("query-text", ["--text", "a dog"]), ("query-image", ["--image", str(tmp_path / "absent.png")])):
        base = [cmd, "--index_dir", str(empty)] + arg
        capsys.readouterr()
        with pytest.raises(SystemExit):                   # the fp32 index files have no threshold search
            search.main(base + ["--min_score", "0.3"])
        assert "--codes" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            search.main(base + ["--codes", "--min_score", "nan"])
        assert "finite" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            search.main(base + ["--codes", "--min_score", "inf"])
        assert "finite" in capsys.readouterr().err
        with pytest.raises(FileNotFoundError):            # parsed, then no codes.npy: before any tower is built
            search.main([cmd, "--index_dir", str(tmp_path / "absent")] + arg + ["--codes", "--min_score", "0.3", "--max_pairs", "100"])
        with pytest.raises(FileNotFoundError):
            search.main(base + ["--codes", "--min_score", "0.3"])
    for cmd in ("query-text", "query-image", "query-c2df"):
        with pytest.raises(SystemExit) as e:
            search.main([cmd, "--help"])
        assert e.value.code == 0
        text = " ".join(capsys.readouterr().out.split())
        assert "--min_score" in text and "--max_pairs" in text and "--topk is ignored" in text
        if cmd == "query-text":                            # no score ranges are promised for text queries
            assert "not been measured" in text and "0.98-0.99" not in text and "0.99999" not in text


def test_range_search_vectors_argument_errors_need_no_device():
    import sgic_amd  # noqa
    from sgic_amd.search import CodeIndex
    rng = np.random.default_rng(5)
    ci = CodeIndex(ref.quantised_unit_codes(rng, 20, 64), [f"id{j}" for j in range(20)])
    q = ref.random_unit(rng, 3, 64)
    for bad_t in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            ci.range_search_vectors(q, bad_t)
    bad = q.copy()
    bad[1, 7] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ci.range_search_vectors(bad, 0.5)
    bad[1, 7] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ci.range_search_vectors(bad, 0.5)
    with pytest.raises(ValueError, match="unit"):
        ci.range_search_vectors(2.0 * q, 0.5)
    with pytest.raises(ValueError, match="dim"):
        ci.range_search_vectors(ref.random_unit(rng, 3, 128), 0.5)
    big = CodeIndex(rng.integers(0, 256, (4, 2112), dtype=np.uint8), list("abcd"))
    with pytest.raises(ValueError, match="faiss.index"):
        big.range_search_vectors(ref.random_unit(rng, 1, 2112), 0.5)
    assert ci._dev is None and big._dev is None                     # nothing was sent to a device
