"""CPU side of the u8 code search: the integer identity behind the i8 kernel, the host reciprocal norms, the `build` sub-command
(containers -> index directory) and the restatement's distance from the fp32 path it stands beside."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_codes_ref as ref  # noqa: E402


def _edge_rows(dim):
    alt = np.tile(np.array([0, 255], dtype=np.uint8), dim // 2)
    return np.stack([np.zeros(dim, np.uint8), np.full(dim, 255, np.uint8), alt, alt[::-1]])


@pytest.mark.parametrize("dim", [64, 512, 4096])
def test_integer_identity(dim):
    rng = np.random.default_rng(dim)
    q = np.concatenate([_edge_rows(dim), rng.integers(0, 256, (5, dim), dtype=np.uint8), ref.quantised_unit_codes(rng, 5, dim)])
    db = np.concatenate([_edge_rows(dim), rng.integers(0, 256, (9, dim), dtype=np.uint8), ref.quantised_unit_codes(rng, 9, dim)])
    direct = (2 * q.astype(np.int64) - 255) @ (2 * db.astype(np.int64) - 255).T
    assert np.array_equal(ref.int_scores(q, db), direct)
    assert direct[0, 0] == 255 * 255 * dim and direct[0, 1] == -255 * 255 * dim      # the int32 bound is reached, both signs


def test_code_rnorm_against_fp64():
    import sgic_amd  # noqa
    from sgic_amd.search import code_rnorm
    rng = np.random.default_rng(1)
    codes = np.concatenate([_edge_rows(512), rng.integers(0, 256, (300, 512), dtype=np.uint8), ref.quantised_unit_codes(rng, 300, 512)])
    v = 2.0 * codes.astype(np.float64) - 255.0
    want = (1.0 / np.sqrt((v * v).sum(axis=1))).astype(np.float32)
    assert np.array_equal(code_rnorm(codes), want) and np.array_equal(code_rnorm(codes, chunk=7), want)
    assert np.array_equal(ref.rnorm(codes), want)
    assert code_rnorm(codes).dtype == np.float32 and np.isfinite(want).all() and (want > 0).all()


def _container(codes, model_id="ViT-B-32:test", with_clip=True):
    import sgic_amd  # noqa
    from sgic_amd.filemaker import pack_c2df
    from sgic_amd.zstd import Compressor
    enc = {"z_bit_stream": b"\x00\x01", "token_length": 3}
    if with_clip:
        enc["clip_stream"] = Compressor(3).compress(np.asarray(codes, dtype=np.uint8).tobytes())
        enc["clip_meta"] = {"model_id": model_id, "dim": int(len(codes)), "quant": "u8_symmetric_-1_1", "codec": "zstd"}
    return pack_c2df(enc, {"version": 2, "model_id": model_id})


def test_build_from_container_directory(tmp_path, golden_dir, capsys):
    import sgic_amd  # noqa
    from sgic_amd import search
    from sgic_amd.faiss_io import read_index_flat_ip
    apple_codes, _, apple_meta = search.embedded_clip_codes(os.path.join(golden_dir, "ref_apple.c2df"))
    dim = apple_codes.size
    rng = np.random.default_rng(2)
    mine = ref.quantised_unit_codes(rng, 3, dim)
    src = tmp_path / "c2df"
    (src / "sub").mkdir(parents=True)
    shutil.copy(os.path.join(golden_dir, "ref_apple.c2df"), src / "b_apple.c2df")
    meta0 = {"dim": dim, "quant": "u8_symmetric_-1_1"}            # the first container's clip_meta names no model
    from sgic_amd.filemaker import pack_c2df
    from sgic_amd.zstd import Compressor
    (src / "a_first.c2df").write_bytes(pack_c2df({"clip_stream": Compressor(3).compress(mine[0].tobytes()), "clip_meta": meta0},
                                                 {"version": 2}))
    (src / "sub" / "c_deep.c2df").write_bytes(_container(mine[1]))
    (src / "z_last.c2df").write_bytes(_container(mine[2], model_id="other"))
    (src / "m_noclip.c2df").write_bytes(_container(mine[0], with_clip=False))
    (src / "n_junk.c2df").write_bytes(b"this is not a container")
    out = tmp_path / "index"
    assert search.main(["build", "--c2df_dir", str(src), "--index_dir", str(out)]) == 0
    log = capsys.readouterr().out
    assert "[SKIP] m_noclip.c2df" in log and "[SKIP] n_junk.c2df" in log and log.count("[SKIP]") == 2
    want_ids = [str(src / "a_first.c2df"), str(src / "b_apple.c2df"), str(src / "sub" / "c_deep.c2df"), str(src / "z_last.c2df")]
    want_codes = np.stack([mine[0], apple_codes, mine[1], mine[2]])
    codes = np.load(out / "codes.npy")
    assert codes.dtype == np.uint8 and np.array_equal(codes, want_codes)
    for index_name, ids_name in (("faiss.index", "paths.json"), ("index.faiss", "ids.txt")):
        layout = tmp_path / ("only_" + ids_name)
        layout.mkdir()
        shutil.copy(out / index_name, layout / index_name)
        shutil.copy(out / ids_name, layout / ids_name)
        vecs, ids = search.load_index(layout)
        assert ids == want_ids
        assert vecs.dtype == np.float32 and np.array_equal(vecs, search.codes_to_unit(want_codes))
    assert np.array_equal(read_index_flat_ip(str(out / "faiss.index")), read_index_flat_ip(str(out / "index.faiss")))
    first_named = apple_meta.get("model_id") or "ViT-B-32:test"
    assert json.loads((out / "meta.json").read_text()) == {"dim": dim, "model_id": first_named}
    ci = search.CodeIndex.load(out)
    assert ci.ids == want_ids and np.array_equal(ci.codes, want_codes) and np.array_equal(ci.r, ref.rnorm(want_codes))


def test_build_refuses_empty_and_mixed_directories(tmp_path):
    import sgic_amd  # noqa
    from sgic_amd import search
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(RuntimeError):
        search.build_index(empty, tmp_path / "i0")
    only_bad = tmp_path / "bad"
    only_bad.mkdir()
    (only_bad / "x.c2df").write_bytes(_container(np.zeros(64, np.uint8), with_clip=False))
    with pytest.raises(RuntimeError):
        search.build_index(only_bad, tmp_path / "i1", log=lambda *_: None)
    mixed = tmp_path / "mixed"
    mixed.mkdir()
    (mixed / "a.c2df").write_bytes(_container(np.arange(64, dtype=np.uint8)))
    (mixed / "b.c2df").write_bytes(_container(np.arange(128, dtype=np.uint8)))
    with pytest.raises(ValueError):
        search.build_index(mixed, tmp_path / "i2")


def test_restatement_close_to_fp32_path():
    """scores of the code search vs the fp64 product of the fp32 codes_to_unit rows the existing path searches: within 1e-5, the
    bound test_search_topk_parity_10k_corpus puts on such scores"""
    import sgic_amd  # noqa
    from sgic_amd.search import codes_to_unit
    rng = np.random.default_rng(3)
    db = ref.quantised_unit_codes(rng, 2000, 512)
    q = np.concatenate([db[:3], ref.quantised_unit_codes(rng, 5, 512)])
    _, score = ref.keys_and_scores(q, db)
    full = codes_to_unit(q).astype(np.float64) @ codes_to_unit(db).astype(np.float64).T
    assert np.abs(score.astype(np.float64) - full).max() <= 1e-5
    s, i = ref.search(q, db, 10)
    assert i[0, 0] == 0 and i[1, 0] == 1 and i[2, 0] == 2
