"""GPU: the progressive JPEG encoder (csrc/jpeg_enc.hip, sgic_jpeg_encode_prog_batch) writes the files of Pillow's
save(progressive=True), byte for byte."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_prog_ref as pref  # noqa: E402
import jpeg_enc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SGIC_EINVAL = -1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _encode(imgs, q, sub=2, **kw):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    return jpeg_enc.encode_batch(_dev(imgs), q, sub, progressive=True, **kw)


def test_case_list_equals_pillow():
    for name, img, q, sub in ref.case_images():
        got = _encode(img[None], q, sub)
        assert len(got) == 1 and got[0] == pref.pillow_bytes(img, q, sub), name


@pytest.mark.parametrize("h,w,q,sub", [(128, 128, 100, 0), (128, 128, 95, 2), (40, 128, 100, 0)])
def test_correction_bit_flush_equals_pillow(h, w, q, sub):
    """runs that libjpeg cuts because its correction-bit buffer is full (test_jpeg_enc_prog_cpu asserts that on the restatement):
    the doubling rounds have heads to find"""
    img = pref.tiled(h, w)
    assert _encode(img[None], q, sub) == [pref.pillow_bytes(img, q, sub)]


@pytest.mark.parametrize("column", [None, 8, 320])
def test_eobrun_limit_equals_pillow(column):
    """32 942 blocks per component: runs of 0x7FFF blocks and more, in first and in refinement scans"""
    img = pref.flat_large(column)
    assert _encode(img[None], 75, 0) == [pref.pillow_bytes(img, 75, 0)]


def test_link_pass_past_one_workgroup():
    """66 306 blocks per component are 260 workgroups of the flags pass, so the link pass walks them in two rounds with a carry.
    Textured blocks at raster blocks 800 and 65 540: the run between them is split twice, blocks of the second round look back to a
    coded block of the first, and blocks of the first look ahead to one of the second"""
    img = np.full((2056, 2064, 3), 97, np.uint8)
    rng = np.random.default_rng(5)
    for idx in (800, 65540):
        by, bx = divmod(idx, 258)
        img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = rng.integers(0, 256, (8, 8, 3))
    assert _encode(img[None], 90, 0) == [pref.pillow_bytes(img, 90, 0)]


@pytest.fixture(scope="module")
def trio():
    """three different 256 x 256 images (one is noise), their qualities, and Pillow's three progressive files"""
    imgs = np.stack([ref.image(kind, 256, 256, 70 + i) for i, kind in enumerate(("natural", "noise", "natural"))])
    qs = (10, 75, 95)
    return imgs, qs, [pref.pillow_bytes(im, q, 2) for im, q in zip(imgs, qs)]


def test_batch_independence(trio):
    imgs, qs, want = trio
    got = _encode(imgs, qs)
    assert got == want
    assert _encode(imgs, qs) == got                                    # two runs, the same bytes
    assert _encode(imgs, qs, optimize=True) == got                     # optimize changes nothing, as in Pillow
    for b in range(3):                                                 # tables and runs are per image
        assert _encode(imgs[b:b + 1], qs[b]) == want[b:b + 1], b


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_layouts_200x300(sub):
    img = ref.image("natural", 200, 300, 50 + sub)
    assert _encode(img[None], 85, sub) == [pref.pillow_bytes(img, 85, sub)]


@pytest.fixture(scope="module")
def pair():
    """two 8 x 8 images and Pillow's two progressive files at q = 75, 4:2:0"""
    imgs = [ref.image("natural", 8, 8, 31), ref.image("noise", 8, 8, 32)]
    want = [pref.pillow_bytes(im, 75, 2) for im in imgs]
    assert want[0] != want[1]
    return np.stack(imgs), want


@pytest.mark.parametrize("shift", [0, 1])
def test_image_loop_past_the_grid_cap(pair, shift):
    """32 770 images of 8 x 8: blockIdx.y stops at 32 768, so workgroups 0 and 1 of every pass take a second image; with shift 1 it
    is of the other kind than their first one (test_gpu_jpeg_enc_opt has the reasoning)"""
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc, ops
    imgs, want = pair
    B = 32770
    kind = (np.arange(B) + shift * (np.arange(B) // 32768)) % 2
    x = _dev(imgs)[torch.from_numpy(kind).to("cuda:0")].contiguous()
    tables = np.broadcast_to(jpeg_enc.quant_tables(75), (B, 2, 64))
    buf, lens, err, huff, nval = ops.jpeg_encode(x, tables, 2, progressive=True)
    assert not err.cpu().numpy().any()
    lens_h, nval_h = lens.cpu().numpy(), nval.cpu().numpy()
    host = buf[:, :int(lens_h.sum(axis=1).max())].cpu().numpy()
    huff_h = huff.cpu().numpy()
    assert not huff_h[:, :, 16:][np.arange(256) >= nval_h[:, :, None]].any()          # HUFFVAL is zero past the table's symbols
    files = {}
    for b in range(B):
        key = (host[b, :lens_h[b].sum()].tobytes(), lens_h[b].tobytes(), huff_h[b].tobytes())
        if key not in files:
            hf = [(h[:16].tobytes(), h[16:16 + int(n)].tobytes()) for h, n in zip(huff_h[b], nval_h[b])]
            ends = np.cumsum(lens_h[b])
            files[key] = jpeg_enc.progressive_file(8, 8, tables[0], 2, hf, [key[0][e - n:e] for e, n in zip(ends, lens_h[b])])
        assert files[key] == want[kind[b]], b
    assert len(files) == 2


def test_decoder_takes_the_output(trio):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg
    imgs, qs, want = trio
    got = _encode(imgs, qs)
    dec = jpeg.ScanJpegBatch(got).decode("cuda:0").cpu().numpy()
    for b in range(3):
        assert (dec[b] == np.array(Image.open(io.BytesIO(want[b])).convert("RGB"))).all()


def test_cap_and_lengths_on_noise_q100():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc, ops
    from sgic_amd._lib import lib
    img = ref.image("noise", 256, 256, 11)
    want, info = pref.encode(img, 100, 0)
    assert want == pref.pillow_bytes(img, 100, 0)
    tables = jpeg_enc.quant_tables(100)
    buf, lens, err, huff, nval = ops.jpeg_encode(_dev(img[None]), tables[None], 0, progressive=True)
    cap = ctypes.c_size_t(0)
    assert lib.sgic_jpeg_encode_prog_cap(256, 256, 0, ctypes.byref(cap)) == 0 and buf.shape == (1, cap.value)
    lens_h = lens[0].cpu().numpy()
    assert int(err[0]) == 0 and lens_h.tolist() == [len(s) for s in info["segments"]]
    assert all(n > 0 or not s for n, s in zip(lens_h, info["segments"])) and int(lens_h.sum()) <= cap.value
    assert bytes(buf[0, :int(lens_h.sum())].cpu().numpy()) == b"".join(info["segments"])
    tabs = [pl for scan in info["dht"] for pl in scan]
    hh, nv = huff[0].cpu().numpy(), nval[0].cpu().numpy()
    assert [(h[:16].tobytes(), h[16:16 + n].tobytes()) for h, n in zip(hh, nv)] == [(pl[1:17], pl[17:]) for pl in tabs]
    torch.cuda.synchronize()


def test_refusals_launch_nothing():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    from sgic_amd._lib import lib, stream
    H, W, B = 16, 24, 2
    x = _dev(np.stack([ref.image("natural", H, W, 1), ref.image("noise", H, W, 2)]))
    good = np.ascontiguousarray(np.broadcast_to(jpeg_enc.quant_tables(75), (B, 2, 64)))
    cap, nbytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sgic_jpeg_encode_prog_cap(H, W, 2, ctypes.byref(cap)) == 0
    assert lib.sgic_jpeg_encode_prog_work_bytes(B, H, W, 2, ctypes.byref(nbytes)) == 0
    work = torch.empty(nbytes.value + 16, dtype=torch.uint8, device="cuda:0")
    buf = torch.full((B, cap.value), 0xAB, dtype=torch.uint8, device="cuda:0")
    lens = torch.full((B, 10), -7, dtype=torch.int32, device="cuda:0")
    err = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    huff = torch.full((B, 10, 272), 0xAB, dtype=torch.uint8, device="cuda:0")
    nval = torch.full((B, 10), -7, dtype=torch.int32, device="cuda:0")
    args = dict(x=x.data_ptr(), B=B, H=H, W=W, sub=2, qt=good.ctypes.data, work=work.data_ptr(), nbytes=nbytes.value, buf=buf.data_ptr(),
                cap=cap.value, lens=lens.data_ptr(), err=err.data_ptr(), huff=huff.data_ptr(), nval=nval.data_ptr())

    def run(**kw):
        a = dict(args, **kw)
        return lib.sgic_jpeg_encode_prog_batch(a["x"], a["B"], a["H"], a["W"], a["sub"], a["qt"], a["work"], a["nbytes"], a["buf"], a["cap"],
                                               a["lens"], a["err"], a["huff"], a["nval"], stream())

    zero, big = good.copy(), good.copy()
    zero[1, 1, 63] = 0
    big[0, 0, 5] = 256
    bad = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(sub=3), dict(sub=-1),
           dict(qt=zero.ctypes.data), dict(qt=big.ctypes.data), dict(x=None), dict(qt=None), dict(work=None), dict(buf=None),
           dict(lens=None), dict(err=None), dict(work=work.data_ptr() + 4), dict(lens=lens.data_ptr() + 2), dict(err=err.data_ptr() + 1),
           dict(nbytes=nbytes.value - 1), dict(cap=cap.value - 1),
           dict(huff=None), dict(nval=None), dict(huff=huff.data_ptr() + 1), dict(nval=nval.data_ptr() + 2)]
    for kw in bad:
        assert run(**kw) == SGIC_EINVAL, kw
        assert lib.sgic_last_error()
    out = ctypes.c_size_t(0)
    assert lib.sgic_jpeg_encode_prog_cap(0, W, 2, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_prog_cap(H, W, 5, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_prog_cap(H, W, 2, None) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_prog_work_bytes(0, H, W, 2, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_prog_cap(16384, 16384, 2, ctypes.byref(out)) == SGIC_EINVAL
    # the block limit follows the 1605-bit bound of the largest scan: 2 675 992 coded blocks, 3 per MCU at 4:4:4
    assert lib.sgic_jpeg_encode_prog_cap(8 * 944, 8 * 944, 0, ctypes.byref(out)) == 0                  # 2 673 408 blocks
    assert lib.sgic_jpeg_encode_prog_cap(8 * 944, 8 * 945, 0, ctypes.byref(out)) == SGIC_EINVAL        # 2 676 240 blocks
    assert lib.sgic_jpeg_encode_opt_cap(8 * 944, 8 * 944, 0, ctypes.byref(out)) == SGIC_EINVAL         # past the optimised call's limit
    # at 4:2:0 the slot's 2^31 - 1 bytes bind before the blocks do (test_jpeg_enc_prog_cpu has all three layouts)
    assert lib.sgic_jpeg_encode_prog_cap(10240, 10144, 2, ctypes.byref(out)) == 0 and out.value <= 0x7FFFFFFF
    assert lib.sgic_jpeg_encode_prog_cap(10240, 10160, 2, ctypes.byref(out)) == SGIC_EINVAL
    torch.cuda.synchronize()
    assert (buf == 0xAB).all() and (lens == -7).all() and (err == -7).all() and (huff == 0xAB).all() and (nval == -7).all()   # nothing ran
    assert run() == 0                                                                      # and the good call does
    torch.cuda.synchronize()
    assert (err == 0).all() and (lens.sum(dim=1) > 0).all() and (nval[:, :2] > 0).all()
