"""CPU: the device-free parts of `search.py build-images` (file listing, selection, the parser) and compress.assemble_index's
unchanged positional signature."""
import os
import random

import numpy as np
import pytest


@pytest.fixture()
def folder(tmp_path):
    names = ["b/z.png", "a/k.JPG", "a/c.jpeg", "a/deep/er/m.webp", "b/a.bmp", "top.jpg", "b/notes.txt", "a/x.gif", "a/noext", "b/y.PnG"]
    for n in names:
        p = tmp_path / n
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"x")
    (tmp_path / "dir.jpg").mkdir()      # a directory with an image extension is not a file
    return tmp_path


def test_listing_is_recursive_sorted_and_filters_extensions(folder):
    import sgic_amd  # noqa: F401
    from sgic_amd import search
    got = search.list_images(folder)
    want = sorted(folder / n for n in ["b/z.png", "a/k.JPG", "a/c.jpeg", "a/deep/er/m.webp", "b/a.bmp", "top.jpg", "b/y.PnG"])
    assert got == want and got == sorted(got)
    assert search.list_images(folder, ["png", " .JPG "]) == sorted(folder / n for n in ["b/z.png", "a/k.JPG", "top.jpg", "b/y.PnG"])
    assert search.list_images(folder, ["gif"]) == [folder / "a/x.gif"]
    assert search.list_images(folder / "b" / "nothing-here") == []


def test_selection_follows_the_reference():
    import sgic_amd  # noqa: F401
    from sgic_amd.search import select_images
    files = [f"f{i:02d}" for i in range(10)]
    assert select_images(files) == files
    assert select_images(files, limit=3) == files[:3]
    assert select_images(files, limit=3, desired=5) == files[:5]            # desired wins over limit
    assert select_images(files, limit=3, desired=0) == files[:3]            # a non-positive desired does not
    assert select_images(files, limit=0) == files and select_images(files, limit=-2) == files
    assert select_images(files, limit=10) == files and select_images(files, limit=11) == files   # more than there are: all
    assert select_images(files, limit=4, random_pick=True, seed=3) == random.Random(3).sample(files, 4)
    assert select_images(files, desired=4, random_pick=True, seed=9) == random.Random(9).sample(files, 4)
    assert select_images(files, random_pick=True, seed=3) == files          # --random without a target: all, in order
    assert select_images(files, limit=11, random_pick=True, seed=3) == files


def test_parser_accepts_every_reference_flag_and_refuses_the_downloader(tmp_path, capsys, monkeypatch):
    import sgic_amd  # noqa: F401
    from sgic_amd import search
    seen = {}
    monkeypatch.setattr(search, "build_index_from_images", lambda *a, **k: seen.update(args=a, **k))
    argv = ["build-images", "--image_dir", str(tmp_path), "--index_dir", str(tmp_path / "ix"), "--model_id", "ViT-B-32:laion2b_s34b_b79k",
            "--batch_size", "8", "--exts", "jpg,png", "--limit", "7", "--desired", "5", "--random", "--seed", "11", "--small"]
    assert search.main(argv) == 0
    assert seen["args"] == (tmp_path, tmp_path / "ix") and seen["batch_size"] == 8 and seen["exts"] == ["jpg", "png"]
    assert (seen["limit"], seen["desired"], seen["random_pick"], seen["seed"], seen["small"], seen["clip_ckpt"]) == (7, 5, True, 11, True, None)
    seen.clear()
    for extra, word in ((["--auto_download"], "no downloader"), (["--download_dir", str(tmp_path)], "no downloader"),
                        (["--download_size", "512x512"], "no downloader"), (["--timeout", "20"], "no downloader"),
                        (["--model_id", "RN50"], "ViT-B-32")):
        with pytest.raises(SystemExit) as e:
            search.main(argv[:5] + extra)
        assert e.value.code != 0 and word in capsys.readouterr().err
    assert not seen and not (tmp_path / "ix").exists()


def test_assemble_index_keeps_its_five_positional_arguments(tmp_path):
    import sgic_amd  # noqa: F401
    from sgic_amd import search
    from sgic_amd.compress import assemble_index
    bit, idx = tmp_path / "bitstreams", tmp_path / "faiss"
    bit.mkdir()
    files = ["/x/b.png", "/x/a.jpg"]
    for s in ("a", "b"):
        (bit / f"{s}.c2df").write_bytes(b"")
    vecs = np.eye(2, 4, dtype=np.float32)
    ids = assemble_index(files, vecs, str(bit), str(idx), 4)
    assert ids == [os.path.join(str(bit), "a.c2df"), os.path.join(str(bit), "b.c2df")]
    got, got_ids = search.load_index(idx)
    assert got_ids == ids and np.allclose(got, vecs[::-1]) and not (idx / "codes.npy").exists()


def test_x_of_u8_truncates_back_to_u8():
    """the premise of test_gpu_clip_u8's comparison with the fp32 route, in fp32: x = (u + 0.5) / 255 * 2 - 1 ->
    trunc((clamp(x) * 0.5 + 0.5) * 255) == u for all 256 codes, while x = u / 255 * 2 - 1 (the compress route) loses one for 63 of them"""
    import torch
    u = torch.arange(256, dtype=torch.float32)
    back = lambda x: ((x.clamp(-1, 1) * 0.5 + 0.5) * 255.0).to(torch.uint8).float()
    assert torch.equal(back((u + 0.5) / 255.0 * 2.0 - 1.0), u)
    plain = back(u / 255.0 * 2.0 - 1.0)
    assert int((plain == u - 1).sum()) == 63 and int((plain == u).sum()) == 193


def _bounds(in_size, out_size):
    """(first index, count) per output of Pillow's bicubic resample: the bounds half of clip.pil_coeffs (checked against it below)"""
    scale = in_size / out_size
    support = 2.0 * max(scale, 1.0)
    c = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum((c - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((c + support + 0.5).astype(np.int64), in_size)
    return xmin, xmax - xmin


def test_row_window_fits_the_intermediate_the_host_sizes():
    """the CLIP preprocessing kernels (both routes) keep 3 x rows_cap x S bytes between the passes, rows_cap bounded on the host from
    the geometry alone, while the window itself, bounds_v[top].xmin .. bounds_v[top+S-1].xmin + count, exists only on the device.
    Over a sweep of geometries the window must fit: the workspace (host-only call, no device) minus the four tables (and, on the
    fp32 route, the planar u8 copy) is that buffer."""
    import ctypes
    import sgic_amd  # noqa: F401
    from sgic_amd._lib import call
    from sgic_amd.clip import pil_coeffs, resize_geometry
    for n_in, n_out in ((64, 2867), (517, 224), (5, 17), (300, 224), (224, 224)):      # _bounds restates pil_coeffs' bounds
        b, _, _ = pil_coeffs(n_in, n_out)
        xmin, cnt = _bounds(n_in, n_out)
        assert np.array_equal(b[:, 0], xmin) and np.array_equal(b[:, 1], cnt)
    a16 = lambda v: (v + 15) & ~15
    ksize = lambda i, o: int(np.ceil(2.0 * max(i / o, 1.0))) * 2 + 1
    rng = np.random.default_rng(71)
    cases = [(64, 5), (5, 64), (3, 96), (1, 1), (1, 65535), (65535, 1), (65535, 65535), (4000, 4001), (225, 224), (223, 224), (65535, 300),
             (300, 65535), (517, 301), (8, 65535)]
    cases += [tuple(int(v) for v in rng.integers(1, 65536, 2)) for _ in range(300)]
    cases += [tuple(int(v) for v in rng.integers(1, 600, 2)) for _ in range(300)]
    for S in (7, 224, 336):
        for H, W in cases:
            OH, OW, top, left = resize_geometry(H, W, S)
            if max(OH, OW) >= 1 << 30:      # refused by the entry points (2 * index + 1 into a bounds table is an int)
                continue
            geo = np.array([[H, W, OH, OW, top, left]], dtype=np.int32)
            nbytes, nbytes_f32 = ctypes.c_size_t(0), ctypes.c_size_t(0)
            call("sgic_clip_preprocess_u8canvas_workspace", 1, geo, S, ctypes.byref(nbytes))
            call("sgic_clip_preprocess_ragged_workspace", 1, geo, S, ctypes.byref(nbytes_f32))
            tables = a16(8 * OW) + a16(4 * OW * ksize(W, OW)) + a16(8 * OH) + a16(4 * OH * ksize(H, OH))
            rows_cap = (nbytes.value - tables) // (3 * S)          # 3 S >= 21 > the 15 bytes of alignment slack: exact
            assert (nbytes_f32.value - tables - a16(3 * H * W)) // (3 * S) == rows_cap      # the fp32 route: its planar u8 copy too
            xmin, cnt = _bounds(H, OH)
            rows = int(xmin[top + S - 1] + cnt[top + S - 1] - xmin[top])
            assert 1 <= rows <= rows_cap <= H, (S, H, W, rows, rows_cap)
            assert np.all(np.diff(xmin) >= 0) and np.all(np.diff(xmin + cnt) >= 0)      # what makes the two ends the window
