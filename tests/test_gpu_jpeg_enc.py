"""GPU: the baseline JPEG encoder (csrc/jpeg_enc.hip, sgic_amd.jpeg_enc) writes the files Pillow writes, byte for byte."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SGIC_EINVAL = -1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def trio():
    """three different 256 x 256 images, their qualities, and Pillow's three files"""
    imgs = np.stack([ref.image(kind, 256, 256, 70 + i) for i, kind in enumerate(("natural", "noise", "natural"))])
    qs = (10, 75, 95)
    return imgs, qs, [ref.pillow_bytes(im, q, 2) for im, q in zip(imgs, qs)]


def test_case_list_equals_pillow():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    for name, img, q, sub in ref.case_images():
        got = jpeg_enc.encode_batch(_dev(img[None]), q, sub)
        assert len(got) == 1 and got[0] == ref.pillow_bytes(img, q, sub), name


def test_per_image_quality_and_slots(trio):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    imgs, qs, want = trio
    got = jpeg_enc.encode_batch(_dev(imgs), qs)
    assert got == want
    assert jpeg_enc.encode_batch(_dev(imgs), qs) == got            # two runs, the same bytes
    assert jpeg_enc.encode_batch(_dev(imgs[1:2]), 75) == want[1:2]   # and the same as the image alone


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_200x300_single(sub):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    img = ref.image("natural", 200, 300, 9)
    assert jpeg_enc.encode_batch(_dev(img[None]), 90, sub) == [ref.pillow_bytes(img, 90, sub)]


@pytest.fixture(scope="module")
def pair():
    """two 8 x 8 images and Pillow's two baseline files at q = 75, 4:2:0"""
    imgs = [ref.image("natural", 8, 8, 31), ref.image("noise", 8, 8, 32)]
    want = [ref.pillow_bytes(im, 75, 2) for im in imgs]
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
    assert [int(kind[b]) for b in (0, 1, 32767, 32768, 32769)] == ([0, 1, 1, 0, 1] if shift == 0 else [0, 1, 1, 1, 0])
    x = _dev(imgs)[torch.from_numpy(kind).to("cuda:0")].contiguous()
    tables = np.broadcast_to(jpeg_enc.quant_tables(75), (B, 2, 64))
    buf, lens, err = ops.jpeg_encode(x, tables, 2)
    assert not err.cpu().numpy().any()
    lens_h = lens.cpu().numpy()
    host = buf[:, :int(lens_h.max())].cpu().numpy()
    head = jpeg_enc.header(8, 8, tables[0], 2)
    files = set()
    for b in range(B):
        data = host[b, :lens_h[b]].tobytes()
        files.add(data)
        assert head + data == want[kind[b]], b
    assert len(files) == 2


def test_decoder_takes_the_output(trio):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg, jpeg_enc
    imgs, qs, want = trio
    got = jpeg_enc.encode_batch(_dev(imgs), qs)
    for data in got:
        p = jpeg.parse(data)
        assert (p.H, p.W, p.ncomp) == (256, 256, 3)
    dec = jpeg.JpegBatch(got).decode("cuda:0").cpu().numpy()
    for b in range(3):
        assert (dec[b] == np.array(Image.open(io.BytesIO(want[b])).convert("RGB"))).all()


def test_cap_and_lengths_on_noise_q100():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc, ops
    from sgic_amd._lib import lib
    img = ref.image("noise", 64, 64, 11)
    for sub in (0, 2):
        want = ref.pillow_bytes(img, 100, sub)
        tables = jpeg_enc.quant_tables(100)
        head = jpeg_enc.header(64, 64, tables, sub)
        buf, lens, err = ops.jpeg_encode(_dev(img[None]), tables[None], sub)
        cap = ctypes.c_size_t(0)
        assert lib.sgic_jpeg_encode_cap(64, 64, sub, ctypes.byref(cap)) == 0
        nblk = 64 * 3 if sub == 0 else 16 * 6
        assert cap.value == 416 * nblk + 2 and buf.shape == (1, cap.value)
        assert int(err[0]) == 0 and int(lens[0]) == len(want) - len(head) and int(lens[0]) <= cap.value
        assert bytes(buf[0, :int(lens[0])].cpu().numpy()) == want[len(head):]
    torch.cuda.synchronize()


def test_slots_past_4_gib():
    """7000 images of 256 x 256: the slots span more than 2^32 bytes, so the offsets between images must be 64-bit"""
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc, ops
    base = np.stack([ref.image("natural", 256, 256, 21), ref.image("flat", 256, 256, 22), ref.image("natural", 256, 256, 23)])
    B = 7000
    x = _dev(base)[torch.arange(B, device="cuda:0") % 3].contiguous()
    tables = np.broadcast_to(jpeg_enc.quant_tables(50), (B, 2, 64))
    buf, lens, err = ops.jpeg_encode(x, tables, 2)
    assert buf.numel() > 1 << 32
    lens_h = lens.cpu().numpy()
    assert not err.cpu().numpy().any()
    head = len(jpeg_enc.header(256, 256, tables[0], 2))
    want = [ref.pillow_bytes(im, 50, 2)[head:] for im in base]
    assert (lens_h == np.array([len(want[b % 3]) for b in range(B)])).all()
    for b in (0, 1, 2, 3500, 6561, 6998, 6999):          # 6561 is the first slot that starts past 2^32
        assert bytes(buf[b, :int(lens_h[b])].cpu().numpy()) == want[b % 3], b


def test_refusals_launch_nothing():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    from sgic_amd._lib import lib, stream
    H, W, B = 16, 24, 2
    x = _dev(np.stack([ref.image("natural", H, W, 1), ref.image("noise", H, W, 2)]))
    good = np.ascontiguousarray(np.broadcast_to(jpeg_enc.quant_tables(75), (B, 2, 64)))
    cap, nbytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sgic_jpeg_encode_cap(H, W, 2, ctypes.byref(cap)) == 0
    assert lib.sgic_jpeg_encode_work_bytes(B, H, W, 2, ctypes.byref(nbytes)) == 0
    work = torch.empty(nbytes.value + 16, dtype=torch.uint8, device="cuda:0")
    buf = torch.full((B, cap.value), 0xAB, dtype=torch.uint8, device="cuda:0")
    lens = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    err = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    args = dict(x=x.data_ptr(), B=B, H=H, W=W, sub=2, qt=good.ctypes.data, work=work.data_ptr(), nbytes=nbytes.value, buf=buf.data_ptr(),
                cap=cap.value, lens=lens.data_ptr(), err=err.data_ptr())

    def run(**kw):
        a = dict(args, **kw)
        return lib.sgic_jpeg_encode_batch(a["x"], a["B"], a["H"], a["W"], a["sub"], a["qt"], a["work"], a["nbytes"], a["buf"], a["cap"],
                                          a["lens"], a["err"], stream())

    zero, big = good.copy(), good.copy()
    zero[1, 1, 63] = 0
    big[0, 0, 5] = 256
    bad = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(sub=3), dict(sub=-1),
           dict(qt=zero.ctypes.data), dict(qt=big.ctypes.data), dict(x=None), dict(qt=None), dict(work=None), dict(buf=None),
           dict(lens=None), dict(err=None), dict(work=work.data_ptr() + 4), dict(lens=lens.data_ptr() + 2), dict(err=err.data_ptr() + 1),
           dict(nbytes=nbytes.value - 1), dict(cap=cap.value - 1)]
    for kw in bad:
        assert run(**kw) == SGIC_EINVAL, kw
        assert lib.sgic_last_error()
    out = ctypes.c_size_t(0)
    assert lib.sgic_jpeg_encode_cap(0, W, 2, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_cap(H, W, 5, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_work_bytes(0, H, W, 2, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_cap(16384, 16384, 2, ctypes.byref(out)) == SGIC_EINVAL     # more coded blocks than the documented limit
    assert lib.sgic_jpeg_encode_cap(8192, 8192, 2, ctypes.byref(out)) == 0
    torch.cuda.synchronize()
    assert (buf == 0xAB).all() and (lens == -7).all() and (err == -7).all()               # nothing ran
    assert run() == 0                                                                      # and the good call does
    torch.cuda.synchronize()
    assert (err == 0).all() and (lens > 0).all()
