"""GPU multi-scan JPEG decode (csrc/jpeg.hip jpeg_scan_kernel: progressive, multi-scan sequential, mixed batches) against the installed
Pillow -- the decoder behind the reference's `Image.open(path).convert("RGB")` (compress.py:160).  The bar is equality of every sample."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases  # noqa: E402
import jpeg_scans  # noqa: E402

pytestmark = pytest.mark.gpu


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _cases():
    return [(n, d) for n, d in jpeg_scans.pillow_cases(big=True)] + [(n, d) for n, d, _ in jpeg_scans.transcoded_cases()]


@pytest.mark.parametrize("name,data", _cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_gpu_scan_decode_is_bit_exact_with_pillow(name, data):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    ref = _pil(data)
    got = J.ScanJpegBatch([data]).decode("cuda:0").cpu().numpy()[0]
    assert got.shape == ref.shape
    bad = int((got != ref).sum())
    assert bad == 0, f"{name}: {bad} of {ref.size} samples differ (max {np.abs(got.astype(int) - ref.astype(int)).max()})"


def test_mixed_batch_of_baseline_and_progressive_files_in_one_call():
    """ten files of one geometry: baseline and progressive, different scripts, samplings, tables and restart intervals"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    rng = np.random.default_rng(21)
    save = jpeg_scans._save
    nat = lambda: jpeg_cases.natural_like(72, 88, rng)
    base = save(nat(), quality=85)
    datas = [save(nat(), quality=75), save(nat(), quality=90, progressive=True), save(nat(), quality=60, subsampling=1, progressive=True),
             save(nat(), quality=95, subsampling=0, optimize=True, progressive=True, restart_marker_blocks=3),
             jpeg_scans.transcode(base, jpeg_scans.SCRIPTS["split_bands_refined"], restart=4),
             jpeg_scans.transcode(base, jpeg_scans.SCRIPTS["al3_to_0"]),
             jpeg_scans.transcode(base, [((2,), 0, 63, 0, 0), ((0,), 0, 63, 0, 0), ((1,), 0, 63, 0, 0)], restart=5, sequential=True),
             save(nat(), quality=40, restart_marker_blocks=2),
             save(jpeg_cases.natural_like(72, 88, rng, grey=True), quality=80, progressive=True),
             save(nat(), quality=20, subsampling=2, progressive=True)]
    b = J.ScanJpegBatch(datas)
    assert b.nlevels == 4
    got = b.decode("cuda:0").cpu().numpy()
    for i, d in enumerate(datas):
        assert np.array_equal(got[i], _pil(d)), i


def test_corrupt_scan_is_reported_not_decoded_silently():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    rng = np.random.default_rng(22)
    good = jpeg_scans._save(jpeg_cases.natural_like(64, 64, rng), quality=90, optimize=True, progressive=True)
    other = jpeg_scans._save(jpeg_cases.natural_like(64, 64, rng) // 3, quality=40, optimize=True, progressive=True)
    b = J.ScanJpegBatch([good, other])
    d = b.descs
    first1 = d[(d[:, J.S_IMG] == 1) & (d[:, J.S_FIRST] == 1)][0]           # image 1's DC-first scan
    t = int(first1[J.S_TAB0 + first1[J.S_DC0]])
    used0 = {int(r[J.S_TAB0 + j]) for r in d[d[:, J.S_IMG] == 0] for j in range(r[J.S_NTAB])}
    assert t not in used0
    b.tabs[t * J.TAB_BYTES:(t + 1) * J.TAB_BYTES] = 0                    # an empty DC table: every code is invalid (a view into the blob)
    with pytest.raises(RuntimeError):
        b.decode("cuda:0")
    out = b.decode("cuda:0", check=False)
    err = b.last_err.cpu().tolist()
    assert err[0] == 0 and err[1] != 0
    assert np.array_equal(out[0].cpu().numpy(), _pil(good))


def test_ingest_puts_progressive_and_mixed_batches_on_the_gpu(tmp_path):
    """ShardLoader(gpu_progressive=True): progressive and mixed batches decoded scan by scan on the GPU, baseline batches on the
    baseline path, PNG on the host; the tensors the encoder receives equal the host path's"""
    import sgic_amd  # noqa: F401
    from PIL import Image
    from sgic_amd.ingest import DeviceIngest, ShardLoader
    rng = np.random.default_rng(23)
    files = []
    for i in range(4):                               # one all-progressive batch
        p = tmp_path / f"a{i}.jpg"
        Image.fromarray(jpeg_cases.natural_like(120, 136, rng)).save(p, "JPEG", quality=80 + i, progressive=True)
        files.append(str(p))
    for i in range(3):                               # one mixed batch
        p = tmp_path / f"b{i}.jpg"
        Image.fromarray(jpeg_cases.natural_like(64, 72, rng)).save(p, "JPEG", quality=70, progressive=i != 1)
        files.append(str(p))
    for i in range(2):                               # one baseline batch
        p = tmp_path / f"c{i}.jpg"
        Image.fromarray(jpeg_cases.natural_like(48, 40, rng)).save(p, "JPEG", quality=90)
        files.append(str(p))
    p = tmp_path / "d0.png"
    Image.fromarray(jpeg_cases.natural_like(64, 80, rng)).save(p)
    files.append(str(p))
    ing = DeviceIngest("cuda:0")
    for prog in (True, False):
        ld = ShardLoader(files, batch_size=4, workers=2, depth=2, gpu_progressive=prog)
        seen = 0
        for b in ld:
            x, done = ing(b, (0, 0, 0, 0))
            done.synchronize()
            if b.jpeg is not None:
                assert not b.jpeg.err_host.numpy()[:len(b.paths)].any()
            for j, i in enumerate(b.indices):
                ref = torch.from_numpy(np.asarray(Image.open(files[i]).convert("RGB")).copy()).permute(2, 0, 1).float().div(255.0) * 2.0 - 1.0
                assert torch.equal(x[j].cpu(), ref), files[i]
                seen += 1
            b.release()
        ld.close()
        assert seen == len(files)
        if prog:
            assert (ld.gpu_scan_batches, ld.gpu_batches, ld.host_batches) == (2, 1, 1)
        else:
            assert (ld.gpu_scan_batches, ld.gpu_batches, ld.host_batches) == (0, 1, 3)


def test_compress_cli_with_gpu_progressive_jpeg_is_byte_identical(tmp_path):
    import sgic_amd  # noqa: F401
    from PIL import Image
    from sgic_amd import compress
    src = tmp_path / "imgs"
    src.mkdir()
    rng = np.random.default_rng(24)
    for i in range(5):
        Image.fromarray(jpeg_cases.natural_like(256, 256, rng)).save(src / f"p{i}.jpg", "JPEG", quality=85, progressive=True)
    Image.fromarray(jpeg_cases.natural_like(256, 256, rng)).save(src / "q0.jpg", "JPEG", quality=90)
    with open(jpeg_scans.GOLDEN_APPLE, "rb") as f, open(src / "ref_apple.jpg", "wb") as g:
        g.write(f.read())
    outs = []
    for flag in ([], ["--gpu_progressive_jpeg"]):
        out = tmp_path / ("on" if flag else "off")
        assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"] + flag) == 0
        outs.append(out)
    names = sorted(os.listdir(outs[0] / "bitstreams"))
    assert len(names) == 7 and names == sorted(os.listdir(outs[1] / "bitstreams"))
    for n in names:
        assert (outs[0] / "bitstreams" / n).read_bytes() == (outs[1] / "bitstreams" / n).read_bytes(), n
        v = n[:-5] + ".npy"
        assert (outs[0] / "clip_vecs" / v).read_bytes() == (outs[1] / "clip_vecs" / v).read_bytes(), v
