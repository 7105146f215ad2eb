"""Host side of batching images of different sizes that pad to one geometry (sgic_amd.ingest pad_to, sgic_amd.jpeg canvas=) --
no GPU: padded planning with its count and tile caps, canvases from the host decoder, per-image JPEG descriptors."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases  # noqa: E402
import jpeg_scans  # noqa: E402


def test_padded_plan_classes_order_and_count_cap():
    import sgic_amd  # noqa: F401
    from sgic_amd.ingest import plan_batches
    sizes = [(200, 300), (256, 256), (250, 260), (17, 300), (256, 511), (1, 1), (240, 255), (129, 257)]
    files = [f"f{i}" for i in range(len(sizes))]
    assert plan_batches(files, sizes, 2, pad_to=256) == [(256, 512, [0, 2]), (256, 512, [3, 4]), (256, 512, [7]),
                                                         (256, 256, [1, 5]), (256, 256, [6])]
    assert plan_batches(files, sizes, 3, pad_to=256) == [(256, 512, [0, 2, 3]), (256, 512, [4, 7]), (256, 256, [1, 5, 6])]
    # without pad_to every size is its own geometry, as before
    assert len(plan_batches(files, sizes, 32)) == len(sizes)


def test_padded_plan_tile_cap():
    import sgic_amd  # noqa: F401
    from sgic_amd.ingest import plan_batches
    sizes = [(1000, 1000)] + [(1024 - i, 900 + i) for i in range(20)]          # 21 distinct sizes of the 1024^2 class: 16 tiles each
    files = [f"f{i}" for i in range(len(sizes))]
    plan = plan_batches(files, sizes, 32, pad_to=256)                          # cap 4 x 32 = 128 tiles -> 8 images
    assert [(h, w) for h, w, _ in plan] == [(1024, 1024)] * 3 and [len(i) for _, _, i in plan] == [8, 8, 5]
    assert sum((i for _, _, i in plan), []) == list(range(len(sizes)))
    assert [len(i) for _, _, i in plan_batches(files, sizes, 32, pad_to=256, max_tiles=40)] == [2] * 10 + [1]
    # one image above the cap still makes a batch
    assert plan_batches(["a", "b"], [(2048, 2048), (2000, 1900)], 1, pad_to=256) == [(2048, 2048, [0]), (2048, 2048, [1])]


def test_uniform_corpus_keeps_the_exact_plan():
    """a corpus whose sizes are each alone in their padded geometry, all <= 512^2 padded: the padded plan IS today's plan"""
    import sgic_amd  # noqa: F401
    from sgic_amd.ingest import padded_size, plan_batches
    sizes = [(64, 64), (300, 200), (64, 64), (512, 512), (300, 200), (64, 64), (512, 512), (64, 64), (512, 512), (512, 512), (64, 64)]
    files = [f"f{i}" for i in range(len(sizes))]
    for bs in (1, 2, 3, 32):
        exact, padded = plan_batches(files, sizes, bs), plan_batches(files, sizes, bs, pad_to=256)
        assert [i for _, _, i in exact] == [i for _, _, i in padded]
        assert [padded_size(h, w, 256) for h, w, _ in exact] == [(h, w) for h, w, _ in padded]


@pytest.fixture()
def mixed_pngs(tmp_path):
    rng = np.random.default_rng(17)
    sizes = [(200, 240), (256, 256), (131, 77), (17, 300), (255, 129), (240, 400), (250, 511), (300, 200)]
    files = []
    for i, (h, w) in enumerate(sizes):
        p = str(tmp_path / f"im{i:02d}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        files.append(p)
    return files, sizes


def test_loader_canvases_hold_pillow_pixels_at_the_top_left(mixed_pngs):
    import sgic_amd  # noqa: F401
    from sgic_amd.ingest import ShardLoader, padded_size, plan_batches
    files, sizes = mixed_pngs
    ld = ShardLoader(files, batch_size=3, workers=2, depth=2, pin=False, gpu_jpeg=False, pad_to=256)
    assert ld.plan == plan_batches(files, sizes, 3, pad_to=256) and len(ld) == 4     # (256,256): 4 images; (256,512): 3; (512,256): 1
    seen = []
    for b in ld:
        n = len(b.indices)
        assert b.hw.dtype == np.int32 and b.hw.tolist() == [list(sizes[i]) for i in b.indices]
        assert (b.H, b.W) == (max(sizes[i][0] for i in b.indices), max(sizes[i][1] for i in b.indices))
        assert b.u8.shape == (n, b.H, b.W, 3)
        assert all(padded_size(h, w, 256) == b.pad_hw for h, w in b.hw.tolist())
        for j, i in enumerate(b.indices):
            h, w = sizes[i]
            assert np.array_equal(b.u8[j, :h, :w].numpy(), np.asarray(Image.open(files[i]).convert("RGB"))), files[i]
        seen += b.indices
        b.release()
    ld.close()
    assert sorted(seen) == list(range(len(files))) and len(seen) == len(files)
    assert ld.host_batches == 4


def test_loader_builds_canvas_jpeg_descriptors(tmp_path):
    """gpu_jpeg on a CPU box: the loader only builds the JPEG descriptors (the decode is DeviceIngest's); mixed sizes get a canvas"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    from sgic_amd.ingest import ShardLoader
    rng = np.random.default_rng(18)
    files, sizes = [], [(120, 136), (97, 250), (64, 72)]
    for i, (h, w) in enumerate(sizes):
        p = str(tmp_path / f"a{i}.jpg")
        Image.fromarray(jpeg_cases.natural_like(h, w, rng)).save(p, "JPEG", quality=85)
        files.append(p)
    ld = ShardLoader(files, batch_size=4, workers=2, depth=2, pin=False, gpu_jpeg=True, pad_to=256)
    (b,) = list(ld)
    assert isinstance(b.jpeg, J.JpegBatch) and b.u8 is None and (b.jpeg.H, b.jpeg.W) == (b.H, b.W) == (120, 250)
    assert b.jpeg.hw.tolist() == [list(s) for s in sizes]
    assert b.jpeg.params[:, J.P_H].tolist() == [h for h, _ in sizes] and b.jpeg.params[:, J.P_W].tolist() == [w for _, w in sizes]
    b.release()
    ld.close()
    assert ld.gpu_batches == 1


def test_jpeg_batches_take_a_canvas_and_keep_per_image_params():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    datas = [d for _, d in jpeg_cases.cases(small=True)]
    sizes = [Image.open(io.BytesIO(d)).size[::-1] for d in datas]
    assert len(set(sizes)) > 5
    with pytest.raises(ValueError, match="shares one geometry"):
        J.JpegBatch(datas)
    H, W = max(h for h, _ in sizes), max(w for _, w in sizes)
    b = J.JpegBatch(datas, canvas=(H, W))
    assert (b.H, b.W) == (H, W) and b.hw.tolist() == [list(s) for s in sizes]
    assert b.params[:, J.P_H].tolist() == [h for h, _ in sizes] and b.params[:, J.P_W].tolist() == [w for _, w in sizes]
    with pytest.raises(ValueError):
        J.JpegBatch(datas, canvas=(H - 1, W))
    # equal sizes: the canvas changes nothing in the descriptor
    same = [datas[0]] * 3
    assert np.array_equal(J.JpegBatch(same, canvas=sizes[0]).blob.numpy(), J.JpegBatch(same).blob.numpy())

    rng = np.random.default_rng(19)
    save = jpeg_scans._save
    scans = [save(jpeg_cases.natural_like(72, 88, rng), quality=80, progressive=True), save(jpeg_cases.natural_like(41, 99, rng), quality=70),
             open(jpeg_scans.GOLDEN_APPLE, "rb").read()]
    ssz = [Image.open(io.BytesIO(d)).size[::-1] for d in scans]
    with pytest.raises(ValueError, match="shares one geometry"):
        J.ScanJpegBatch(scans)
    SH, SW = max(h for h, _ in ssz), max(w for _, w in ssz)
    sb = J.ScanJpegBatch(scans, canvas=(SH, SW))
    assert (sb.H, sb.W) == (SH, SW) and sb.hw.tolist() == [list(s) for s in ssz]
    assert sb.params[:, J.P_H].tolist() == [h for h, _ in ssz] and sb.params[:, J.P_W].tolist() == [w for _, w in ssz]
    assert np.array_equal(J.ScanJpegBatch(scans[:1] * 2, canvas=ssz[0]).blob.numpy(), J.ScanJpegBatch(scans[:1] * 2).blob.numpy())
