"""CPU side of the multi-scan (progressive) GPU JPEG path: the host scan parser (sgic_amd.jpeg.parse_scans / ScanJpegBatch) and the
numpy restatement of the progressive coefficient decode (tests/jpeg_scans.py) against the installed Pillow -- what the reference's
Test_Dataset runs (compress.py:160) -- on Pillow's progressive files and on transcoded scan scripts Pillow cannot write.  Bit-exact."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases  # noqa: E402
import jpeg_scans  # noqa: E402


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name,data", jpeg_scans.pillow_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_scan_parser_geometry_scans_levels_tables(name, data):
    import sgic_amd  # noqa: F401
    from PIL import Image
    from sgic_amd import jpeg as J
    im = Image.open(io.BytesIO(data))
    p = J.parse_scans(data)
    assert p.progressive and (p.W, p.H) == im.size and p.ncomp == len(im.getbands())
    for k, t in im.quantization.items():
        assert np.array_equal(p.quant[k], np.asarray(t, dtype=np.uint16))
    # geometry: the comps fields parse() builds for the same image saved baseline
    base = J.parse(_pil_baseline(im, data))
    assert (p.hmax, p.vmax, p.mcus_x, p.mcus_y) == (base.hmax, base.vmax, base.mcus_x, base.mcus_y)
    for c, d in enumerate(p.comps):
        assert all(d[f] == base.comps[c][f] for f in ("h", "v", "bw", "bh", "cw", "ch"))
    # libjpeg's standard script (jpeg_simple_progression), 3 dependency levels
    std = jpeg_scans.STANDARD_COLOUR if p.ncomp == 3 else jpeg_scans.STANDARD_GREY
    assert [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in p.scans] == std
    assert p.nlevels == 3 and [s.level for s in p.scans] == ([1, 1, 1, 1, 1, 2, 2, 2, 2, 3] if p.ncomp == 3 else [1, 1, 1, 2, 2, 3])
    for s in p.scans:
        if len(s.comps) == 1:      # non-interleaved: the component's own block grid, not the MCU-padded one
            d = p.comps[s.comps[0]]
            assert (s.gw, s.gh) == (-(-d["cw"] // 8), -(-d["ch"] // 8))
        else:
            assert (s.gw, s.gh) == (p.mcus_x, p.mcus_y)
        assert s.segs[0] == 0 and np.all(np.diff(s.segs) > 0)
        if s.restart:
            assert len(s.segs) == -(-s.gw * s.gh // s.restart)
        for t in (s.dc if s.mode in (J.M_SEQ, J.M_DC_FIRST) else []) + (s.ac if s.mode in (J.M_AC_FIRST, J.M_AC_REFINE) else []):
            assert 0 <= t < len(p.tabs)
    assert len({t.tobytes() for t in p.tabs}) == len(p.tabs)       # the per-image pool is deduplicated


def _pil_baseline(im, data):
    from PIL import Image
    buf = io.BytesIO()
    sub = {(2, 2): 2, (2, 1): 1, (1, 1): 0}
    kw = {}
    if len(im.layer) == 3:
        kw["subsampling"] = sub[(im.layer[0][1], im.layer[0][2])]
    Image.open(io.BytesIO(data)).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_apple_luma_walks_its_own_block_rows():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    p = J.parse_scans(open(jpeg_scans.GOLDEN_APPLE, "rb").read())
    assert (p.W, p.H, p.hmax, p.vmax) == (859, 1000, 2, 2)
    y = [s for s in p.scans if s.comps == [0]]
    assert p.comps[0]["bh"] == 126 and all((s.gw, s.gh) == (108, 125) for s in y)


@pytest.mark.parametrize("name,data", jpeg_scans.pillow_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_restatement_is_bit_exact_with_pillow(name, data):
    got, ref = jpeg_scans.decode(data), _pil(data)
    assert got.shape == ref.shape and np.array_equal(got, ref), name


@pytest.mark.parametrize("name,data,base", jpeg_scans.transcoded_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_restatement_on_transcoded_scripts(name, data, base):
    """spectral selection only, non-interleaved DC, Al 3 -> 0, split bands with refinement, restart intervals in every scan,
    unusual scan order, multi-scan sequential: the transcoder is lossless (Pillow sees the original's pixels) and the restatement
    matches Pillow"""
    ref = _pil(base)
    assert np.array_equal(_pil(data), ref), "transcoder"
    assert np.array_equal(jpeg_scans.decode(data), ref), name


def test_incomplete_and_bogus_progressions_are_refused():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    base = jpeg_scans._save(jpeg_cases.natural_like(32, 40, np.random.default_rng(4)), quality=85)
    S = jpeg_scans.STANDARD_COLOUR
    # coefficient 1 of Y left at Al = 1: libjpeg would block-smooth the file
    incomplete = S[:9] + [((0,), 2, 63, 1, 0)]
    with pytest.raises(J.Unsupported):
        J.parse_scans(jpeg_scans.transcode(base, incomplete))
    # DC left at Al = 1
    with pytest.raises(J.Unsupported):
        J.parse_scans(jpeg_scans.transcode(base, S[:6] + S[7:]))
    for bogus in ([((0,), 1, 63, 0, 0)] + S,                                    # AC before DC
                  S[:5] + [((0,), 1, 63, 1, 0)] + S[6:],                        # refinement from the wrong bit (Ah 1, coded at 2)
                  S + [((0,), 1, 63, 0, 0)]):                                   # a first scan over coefficients already complete
        with pytest.raises(J.Unsupported):
            J.parse_scans(jpeg_scans.transcode(base, bogus))
    # Ss > Se, Se > 63, an interleaved AC scan, Al != Ah - 1: written by hand into a valid file's first AC scan header
    good = jpeg_scans.transcode(base, S)
    sos = good.find(b"\xff\xda", good.find(b"\xff\xda") + 2)            # scan 2: Y 1..5, Ah 0, Al 2
    assert good[sos + 7:sos + 10] == bytes([1, 5, 0x02])
    for hdr in (bytes([6, 5, 0x02]), bytes([1, 64, 0x02]), bytes([1, 5, 0x31])):
        with pytest.raises(J.Unsupported):
            J.parse_scans(good[:sos + 7] + hdr + good[sos + 10:])
    J.parse_scans(good)
    # parse() keeps refusing every multi-scan file
    with pytest.raises(J.Unsupported):
        J.parse(good)


def test_scan_batch_descriptors_mixed_baseline_and_progressive():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg as J
    rng = np.random.default_rng(6)
    img = jpeg_cases.natural_like(48, 56, rng)
    base = jpeg_scans._save(img, quality=80)
    datas = [base, jpeg_scans._save(img, quality=80, progressive=True), jpeg_scans.transcode(base, jpeg_scans.SCRIPTS["al3_to_0"]), base]
    b = J.ScanJpegBatch(datas)
    levels = [J.parse_scans(d).nlevels for d in datas]
    assert levels == [1, 3, 4, 1] and b.nlevels == 4
    assert b.level_start[0] == 0 and b.level_start[-1] == b.nscans == 1 + 10 + 16 + 1 and np.all(np.diff(b.level_start) > 0)
    d = b.descs
    # sorted by level, the first scan of every image (and only it) in level 1 copies the image's params
    assert sorted(d[d[:, J.S_FIRST] == 1, J.S_IMG].tolist()) == [0, 1, 2, 3]
    assert np.all(d[:b.level_start[1], J.S_FIRST] == 1) or b.level_start[1] > 4
    assert d[:, J.S_SCAN_LEN].min() >= J.CHUNK and np.all(d[:, J.S_SCAN_LEN] % J.CHUNK == 0)
    assert b.npool == len({bytes(b.tabs[i * J.TAB_BYTES:(i + 1) * J.TAB_BYTES]) for i in range(b.npool)})
    assert b.total_blocks == 4 * sum(c["bw"] * c["bh"] for c in J.parse_scans(base).comps)
    with pytest.raises(ValueError):
        J.ScanJpegBatch([base, jpeg_scans._save(img[:40], quality=80)])
