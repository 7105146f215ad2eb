"""GPU: batches of images of different sizes that pad to one geometry.  Every kernel of the ragged path against an independent
reference -- per-image torch pad, Pillow's resample and clip.pil_coeffs, Pillow's JPEG decode -- and the compress CLI against a
per-image `encode_only` + `ClipCodec` (the reference loop, compress.py:248-291)."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases  # noqa: E402
import jpeg_scans  # noqa: E402
from clip_pillow_ref import pillow_from_f32, pillow_from_u8  # noqa: E402

pytestmark = pytest.mark.gpu


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_ragged_ingest_kernel_bit_exact_vs_per_image_torch_pad():
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    rng = np.random.default_rng(41)
    cases = [((256, 512), [(200, 300), (256, 512), (1, 1), (17, 300), (255, 129)]),
             ((64, 64), [tuple(int(v) for v in rng.integers(1, 49, 2)) for _ in range(37)])]      # > 32 images: two launches
    for (OH, OW), ext in cases:
        Hc, Wc = max(h for h, _ in ext), max(w for _, w in ext)
        canvas = rng.integers(0, 256, (len(ext), Hc, Wc, 3), dtype=np.uint8)
        canvas.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        got = ops.u8canvas_to_f32chw_pad(torch.from_numpy(canvas).cuda(), np.array(ext), OH, OW).cpu()
        assert got.shape == (len(ext), 3, OH, OW)
        for j, (h, w) in enumerate(ext):
            ref = torch.from_numpy(canvas[j, :h, :w].copy()).permute(2, 0, 1).float().div(255.0) * 2.0 - 1.0
            ref = torch.nn.functional.pad(ref[None], (0, OW - w, 0, OH - h), mode="replicate")[0]
            assert torch.equal(got[j], ref), (j, h, w)


def test_device_built_resize_tables_match_pil_coeffs():
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    from sgic_amd.clip import pil_coeffs
    rng = np.random.default_rng(42)
    pairs = [(100, 224), (17, 224), (300, int(224 * 300 / 17)), (224, 224), (4000, 224), (859, 224), (1000, 260), (1, 224), (255, 224),
             (129, 224), (255, int(224 * 255 / 129))]
    pairs += [(int(i), int(o)) for i, o in zip(rng.integers(1, 4097, 60), rng.integers(224, 700, 60))]
    for n_in, n_out in pairs:
        b, k, ks = pil_coeffs(n_in, n_out)
        db, dk, dks = ops.clip_resize_coeffs(n_in, n_out, "cuda:0")
        assert dks == ks and np.array_equal(db.cpu().numpy(), b) and np.array_equal(dk.cpu().numpy(), k), (n_in, n_out)


def test_ragged_clip_preprocess_bit_exact_vs_pillow():
    import sgic_amd  # noqa: F401
    from sgic_amd import weights as W
    from sgic_amd.clip import ClipHIP
    from sgic_amd.config import CLIP_TINY
    from sgic_amd.data import synth_images
    clip = ClipHIP(W.synth_weights(W.clip_spec(CLIP_TINY), seed=5), CLIP_TINY, torch.device("cuda:0"))
    S, mean, std = CLIP_TINY.image_size, np.float32(CLIP_TINY.mean), np.float32(CLIP_TINY.std)
    assert S == 224
    ext = [(300, 200), (200, 300), (17, 300), (255, 129), (859, 1000), (224, 224), (100, 150)]
    x = synth_images(len(ext), 1024, 1024, 77)
    got = clip.preprocess(x.cuda(), hw=ext).cpu().numpy()
    for j, (h, w) in enumerate(ext):
        assert np.array_equal(got[j], pillow_from_f32(x[j, :, :h, :w], S, mean, std)), (h, w)
    # 34 images (two launches): each equal to Pillow, and to the call on that image alone (an image's bits do not depend on the batch)
    rng = np.random.default_rng(43)
    ext = [tuple(int(v) for v in rng.integers(8, 65, 2)) for _ in range(34)]
    x = synth_images(len(ext), 64, 64, 78)
    got = clip.preprocess(x.cuda(), hw=ext)
    for j, (h, w) in enumerate(ext):
        assert np.array_equal(got[j].cpu().numpy(), pillow_from_f32(x[j, :, :h, :w], S, mean, std)), (h, w)
        assert torch.equal(got[j], clip.preprocess(x[j:j + 1, :, :h, :w].contiguous().cuda())[0]), (h, w)


def test_fp32_route_reads_only_the_row_window():
    """S = 3, a 64 x 8 image (OH = 24): the vertical pass reads the source rows bounds_v[top].first .. bounds_v[top + 2].first + count
    of clip.pil_coeffs(64, 24) and no other.  Rows outside that window change no output bit, one row inside it does"""
    import sgic_amd  # noqa: F401
    from sgic_amd import ops
    from sgic_amd.clip import pil_coeffs, resize_geometry
    H, Wd, S = 64, 8, 3
    OH, OW, top, left = resize_geometry(H, Wd, S)
    assert (OH, OW) == (24, 3) and top in (10, 11)
    bv, _, _ = pil_coeffs(H, OH)
    r0, r1 = int(bv[top, 0]), int(bv[top + S - 1].sum())
    assert 0 < r0 < r1 < H
    geo = np.array([[H, Wd, OH, OW, top, left]], dtype=np.int32)
    mean, std = np.float32([0.48, 0.45, 0.40]), np.float32([0.26, 0.27, 0.28])
    u = np.random.default_rng(46).integers(0, 256, (H, Wd, 3), dtype=np.uint8)
    to_x = lambda a: ((torch.from_numpy(a).float() + 0.5) / 255.0 * 2.0 - 1.0).permute(2, 0, 1)[None].contiguous().cuda()
    run = lambda a: ops.clip_preprocess_ragged(to_x(a), geo, S, mean, std)
    base = run(u)
    assert np.array_equal(base[0].cpu().numpy(), pillow_from_u8(u, S, mean, std))
    outside = u.copy()
    outside[:r0] = 255 - outside[:r0]
    outside[r1:] = 255 - outside[r1:]
    assert torch.equal(run(outside), base)
    inside = u.copy()
    mid = (r0 + r1) // 2
    inside[mid] = 255 - inside[mid]
    assert not torch.equal(run(inside), base)


def test_mixed_size_baseline_jpeg_batch_decodes_into_the_canvas():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    datas = [d for _, d in jpeg_cases.cases(small=True)]       # 4:2:0 / 4:4:4 / 4:2:2 / grey, restart intervals, odd sizes
    refs = [_pil(d) for d in datas]
    H, W = max(r.shape[0] for r in refs), max(r.shape[1] for r in refs)
    b = J.JpegBatch(datas, canvas=(H, W))
    got = b.decode("cuda:0").cpu().numpy()
    assert got.shape == (len(datas), H, W, 3)
    for i, r in enumerate(refs):
        assert np.array_equal(got[i, :r.shape[0], :r.shape[1]], r), i


def test_mixed_size_progressive_and_baseline_scan_batch_decodes_into_the_canvas():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    rng = np.random.default_rng(44)
    save, nat = jpeg_scans._save, jpeg_cases.natural_like
    datas = [open(jpeg_scans.GOLDEN_APPLE, "rb").read(), save(nat(1000, 801, rng), quality=85),
             save(nat(777, 859, rng), quality=90, progressive=True, subsampling=1),
             save(nat(901, 640, rng, grey=True), quality=80, progressive=True),
             save(nat(800, 850, rng), quality=75, progressive=True, subsampling=0, restart_marker_blocks=3)]
    refs = [_pil(d) for d in datas]
    H, W = max(r.shape[0] for r in refs), max(r.shape[1] for r in refs)
    b = J.ScanJpegBatch(datas, canvas=(H, W))
    got = b.decode("cuda:0").cpu().numpy()
    for i, r in enumerate(refs):
        assert np.array_equal(got[i, :r.shape[0], :r.shape[1]], r), i


def test_cli_batches_mixed_sizes_and_writes_the_per_image_bytes(tmp_path, capsys):
    """PNG, baseline and progressive JPEG, every size distinct, four padded geometries: the CLI runs the padded plan (5 batches,
    not 12), and every file is what `encode_only` + `ClipCodec` give for that image alone"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress
    from sgic_amd import weights as W
    from sgic_amd.codec import ClipCodec, Codec
    from sgic_amd.config import CLIP_TINY, SMALL
    from sgic_amd.entropy.compression_model import get_padding_size
    from sgic_amd.filemaker import unpack_c2df
    from sgic_amd.ingest import plan_batches
    src = tmp_path / "imgs"
    src.mkdir()
    rng = np.random.default_rng(45)
    spec = [("a0.png", 200, 240, None), ("a1.jpg", 256, 256, False), ("a2.jpg", 131, 77, True), ("a3.png", 255, 129, None),
            ("a4.jpg", 190, 250, False), ("b0.jpg", 17, 300, False), ("b1.png", 240, 400, None), ("b2.jpg", 250, 511, True),
            ("c0.jpg", 300, 200, False), ("c1.jpg", 400, 250, False), ("d0.jpg", 300, 300, True), ("d1.jpg", 511, 400, False)]
    for name, h, w, prog in spec:
        im = Image.fromarray(jpeg_cases.natural_like(h, w, rng))
        im.save(src / name) if prog is None else im.save(src / name, "JPEG", quality=88, progressive=prog)
    out = tmp_path / "out"
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4", "--gpu_progressive_jpeg"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    sizes = [(h, w) for _, h, w, _ in spec]
    plan = plan_batches([n for n, *_ in spec], sizes, 4, pad_to=256)
    assert len(plan) == 5
    assert rec["gpu_jpeg_batches"] + rec["gpu_scan_jpeg_batches"] + rec["host_decoded_batches"] == len(plan)
    # a: [a0 a1 a2 a3] has PNGs -> host, [a4] baseline GPU; b: PNG -> host; c: two baseline sizes -> GPU canvas; d: mixed -> scans
    assert (rec["gpu_jpeg_batches"], rec["gpu_scan_jpeg_batches"], rec["host_decoded_batches"]) == (2, 1, 2), rec
    sd = W.synth_weights(W.encoder_spec(SMALL) + W.codec_misc_spec(SMALL) + W.bottleneck_spec(SMALL), seed=1234)
    model = Codec(sd, SMALL, "cuda:0")
    model.hybrid_codec.quantize_feat.force_zero_thres = 0.12
    model.hybrid_codec.quantize_feat.update(force=True)
    clipc = ClipCodec(W.synth_weights(W.clip_spec(CLIP_TINY), seed=4321), CLIP_TINY, "cuda:0")
    for name, h, w, _ in spec:
        stem = name.split(".")[0]
        img = compress.load_image(str(src / name)).cuda()[None]
        pad = get_padding_size(h, w, p=256)
        ref = model.encode_only(torch.nn.functional.pad(img, pad, mode="replicate"))
        enc, hdr = unpack_c2df(out / "bitstreams" / f"{stem}.c2df")
        assert enc["h_bit_stream"] == ref["h_bit_stream"] and enc["z_bit_stream"] == ref["z_bit_stream"], name
        assert tuple(enc["img_shape"]) == tuple(ref["img_shape"]) and hdr["padding"] == list(pad) and hdr["image_hw"] == [h, w], name
        v = clipc.image_to_unit_vec(img[0])
        assert np.allclose(np.load(out / "clip_vecs" / f"{stem}.npy"), v, atol=1e-6), name
