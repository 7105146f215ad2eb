"""The contract of the JPEG ingest on files Pillow does not write (tests/jpeg_forge.py) -- CPU side: a file's pixels are Pillow's, or
both parsers refuse it (Unsupported -> the host decoder, which raises for a really broken file), or the decode reports an error.
The forge is checked against Pillow first; all comparisons are exact equality of u8 pixels."""
import io
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases  # noqa: E402
import jpeg_forge  # noqa: E402
import jpeg_scans  # noqa: E402


def _pillow(data):
    """-> (H, W, 3) u8 as the reference's `Image.open(path).convert("RGB")`, libjpeg's warnings silenced; raises what Pillow raises"""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


_ids = lambda v: v if isinstance(v, str) and len(v) < 60 else ""


@pytest.mark.parametrize("kw", [dict(quality=90, subsampling=0), dict(quality=75, subsampling=2), dict(quality=80, grey=True)],
                         ids=["444", "420", "grey"])
def test_forge_reproduces_pillow_files(kw):
    """the writer against the reference decoder, not against our code: a Pillow file's coefficients and tables written again by the
    forge (other Huffman tables, other bytes) decode in Pillow to exactly the original's pixels -- also with restart intervals"""
    kw = dict(kw)
    rng = np.random.default_rng(3)
    data = jpeg_scans._save(jpeg_cases.natural_like(45, 59, rng, grey=kw.pop("grey", False)), **kw)
    ref = _pillow(data)
    for extra in (dict(), dict(restart=3), dict(sof=0xC1)):
        forged = jpeg_forge.reforge(data, **extra)
        assert forged != data and np.array_equal(_pillow(forged), ref), extra


@pytest.mark.parametrize("name,data,expect", jpeg_forge.unusual_cases(), ids=_ids)
def test_unusual_files_decode_as_pillow_or_are_refused_as_listed(name, data, expect):
    """the expected pixels are Pillow's; only the cases listed as refused may be refused (a fix must not pass by refusing more)"""
    import sgic_amd  # noqa: F401
    from oracle import jpeg_ref
    from sgic_amd import jpeg as J
    ref = _pillow(data)                                   # must not raise
    assert expect in ("both", "scans_only", "refused")
    if expect == "both":
        got = jpeg_ref.decode(data)
        assert got.shape == ref.shape and np.array_equal(got, ref)
    else:
        with pytest.raises(J.Unsupported):
            J.parse(data)
    if expect == "refused":
        with pytest.raises(J.Unsupported):
            J.parse_scans(data)
    else:
        got = jpeg_scans.decode(data)
        assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("name,data,expect", jpeg_forge.malformed_cases(), ids=_ids)
def test_malformed_files_are_refused_or_fail_loudly(name, data, expect):
    import sgic_amd  # noqa: F401
    from oracle import jpeg_ref
    from sgic_amd import jpeg as J
    try:
        _pillow(data)
        pillow = "decodes"
    except OSError:                                       # UnidentifiedImageError is one
        pillow = "raises"
    assert pillow == jpeg_forge.MALFORMED_PILLOW[name], "the installed Pillow treats this file differently from the recorded table"
    assert expect in ("unsupported", "decode_error")
    if expect == "unsupported":
        for parser in (J.parse, J.parse_scans):
            with pytest.raises(J.Unsupported):            # a bare IndexError / struct.error / OverflowError does not count
                parser(data)
    else:
        J.parse(data)
        J.parse_scans(data)
        with pytest.raises(ValueError, match="scan ended"):
            jpeg_ref.decode(data)
        with pytest.raises(ValueError, match="scan ended"):
            jpeg_scans.decode(data)


def test_existing_corpora_never_read_past_their_scans():
    """the end-of-scan check must not fire on any valid file: the oracles (which now raise where the kernels set code 3) decode every
    file of the existing suites, Pillow-written and transcoded"""
    from oracle import jpeg_ref
    for name, data in jpeg_cases.cases(small=True):
        jpeg_ref.decode(data)
    for name, data in jpeg_scans.pillow_cases():
        jpeg_scans.decode(data)
    for name, data, _ in jpeg_scans.transcoded_cases():
        jpeg_scans.decode(data)


def test_batch_descriptors_carry_the_unpadded_scan_length():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    datas = [d for n, d in jpeg_forge.layout_batch()]
    b = J.JpegBatch(datas)
    assert b.params[:, J.P_SCAN_BYTES].tolist() == [len(J.parse(d).scan) for d in datas]
    assert (b.params[:, J.P_SCAN_BYTES] <= b.params[:, J.P_SCAN_LEN]).all() and (b.params[:, J.P_SCAN_LEN] % J.CHUNK == 0).all()
    s = J.ScanJpegBatch(datas)
    assert sorted(s.descs[:, J.S_SCAN_BYTES].tolist()) == sorted(len(J.parse_scans(d).scans[0].data) for d in datas)
    assert (s.descs[:, J.S_SCAN_BYTES] <= s.descs[:, J.S_SCAN_LEN]).all()
    short = [d for n, d, e in jpeg_forge.malformed_cases() if e == "decode_error"]
    assert J.JpegBatch(short).params[:, J.P_SCAN_BYTES].tolist() == [0, 3]


@pytest.mark.parametrize("bad_name", ["cut_in_half", "tq_5"])
def test_ingest_hands_a_broken_jpeg_to_the_host_decoder_which_raises(tmp_path, bad_name):
    """a folder of good JPEGs plus one broken file of the same size, GPU JPEG route on: the broken file's batch is never a GPU batch,
    and the consumer gets the OSError Pillow raises"""
    import sgic_amd  # noqa: F401
    from sgic_amd.ingest import ShardLoader
    bad = {n: d for n, d, _ in jpeg_forge.malformed_cases()}[bad_name]
    with pytest.raises(OSError) as pillow_err:
        _pillow(bad)
    files = []
    for i, data in enumerate([jpeg_forge.forged(40, 56, jpeg_forge.S420), jpeg_forge.forged(40, 56, jpeg_forge.S444), bad,
                              jpeg_forge.forged(40, 56, jpeg_forge.S440)]):
        files.append(str(tmp_path / f"im{i}.jpg"))
        with open(files[-1], "wb") as f:
            f.write(data)
    for batch_size in (4, 1):
        ld = ShardLoader(files, batch_size=batch_size, workers=2, depth=2, pin=False, gpu_jpeg=True)
        seen = []
        with pytest.raises(OSError) as err:
            for b in ld:
                assert files[2] not in b.paths or b.jpeg is None
                seen += b.paths
                b.release()
        ld.close()
        assert type(err.value) is type(pillow_err.value) and str(err.value) == str(pillow_err.value)
        assert files[2] not in seen
        if batch_size == 1:                               # the good files before it went the GPU route
            assert seen == files[:2] and ld.gpu_batches == 2
