"""GPU: the JPEG encoder with optimised Huffman tables (csrc/jpeg_enc.hip, sgic_jpeg_encode_opt_batch) writes the files of Pillow's
save(optimize=True), byte for byte."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_opt_ref as oref  # noqa: E402
import jpeg_enc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SGIC_EINVAL = -1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def trio():
    """three different 256 x 256 images (one is noise), their qualities, and Pillow's three optimised files"""
    imgs = np.stack([ref.image(kind, 256, 256, 70 + i) for i, kind in enumerate(("natural", "noise", "natural"))])
    qs = (10, 75, 95)
    return imgs, qs, [oref.pillow_bytes(im, q, 2) for im, q in zip(imgs, qs)]


def test_case_list_equals_pillow():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    for name, img, q, sub in ref.case_images():
        got = jpeg_enc.encode_batch(_dev(img[None]), q, sub, optimize=True)
        assert len(got) == 1 and got[0] == oref.pillow_bytes(img, q, sub), name


def test_limiter_case_equals_pillow():
    """the luma AC code of this image reaches 17 bits before limiting (test_jpeg_enc_opt_cpu asserts that on the restatement)"""
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    img = ref.image("natural", 256, 256, 5)
    assert jpeg_enc.encode_batch(_dev(img[None]), 100, 2, optimize=True) == [oref.pillow_bytes(img, 100, 2)]


def test_batch_independence(trio):
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    imgs, qs, want = trio
    got = jpeg_enc.encode_batch(_dev(imgs), qs, optimize=True)
    assert got == want
    assert jpeg_enc.encode_batch(_dev(imgs), qs, optimize=True) == got                       # two runs, the same bytes
    for b in range(3):                                                                       # tables are per image
        assert jpeg_enc.encode_batch(_dev(imgs[b:b + 1]), qs[b], optimize=True) == want[b:b + 1], b
    assert jpeg_enc.encode_batch(_dev(imgs), qs) == [ref.pillow_bytes(im, q, 2) for im, q in zip(imgs, qs)]   # and the default is today's


@pytest.fixture(scope="module")
def pair():
    """two 8 x 8 images whose fitted tables differ from each other and from those of their summed histograms (checked on the
    restatement), and Pillow's two optimised files at q = 75, 4:2:0"""
    imgs = [ref.image("natural", 8, 8, 31), ref.image("noise", 8, 8, 32)]
    hist = [oref.histograms(oref.symbols(im, ref.quant_tables(75), 2)) for im in imgs]
    alone, both = [oref.tables_of(h)[0] for h in hist], oref.tables_of(hist[0] + hist[1])[0]
    assert alone[0] != alone[1] and both != alone[0] and both != alone[1]
    # in each order some table of the first image has more symbols than the second's: a HUFFVAL that is not cleared shows
    assert any(len(a[1]) > len(b[1]) for a, b in zip(*alone)) and any(len(b[1]) > len(a[1]) for a, b in zip(*alone))
    want = [oref.pillow_bytes(im, 75, 2) for im in imgs]
    assert want[0] != want[1]
    return np.stack(imgs), want


@pytest.mark.parametrize("shift", [0, 1])
def test_image_loop_past_the_grid_cap(pair, shift):
    """32 770 images of 8 x 8: blockIdx.y stops at 32 768, so workgroup 0 takes images 0 and 32 768 and workgroup 1 images 1 and
    32 769; no other shape makes a workgroup of hist, tables, bits or pack meet a second image.  shift 0: the two kinds alternate
    throughout, so a workgroup's second image is of its first one's kind.  shift 1: the kinds swap at 32 768, so it is of the other
    kind, in both orders; counters, table words or HUFFVAL bytes that stayed from the first image give other bytes (the fixture
    checks that on the restatement)."""
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc, ops
    imgs, want = pair
    B = 32770
    kind = (np.arange(B) + shift * (np.arange(B) // 32768)) % 2
    assert [int(kind[b]) for b in (0, 1, 32767, 32768, 32769)] == ([0, 1, 1, 0, 1] if shift == 0 else [0, 1, 1, 1, 0])
    x = _dev(imgs)[torch.from_numpy(kind).to("cuda:0")].contiguous()
    tables = np.broadcast_to(jpeg_enc.quant_tables(75), (B, 2, 64))
    buf, lens, err, huff, nval = ops.jpeg_encode(x, tables, 2, optimize=True)
    assert not err.cpu().numpy().any()
    lens_h, nval_h = lens.cpu().numpy(), nval.cpu().numpy()
    host = buf[:, :int(lens_h.max())].cpu().numpy()
    huff_h = huff.cpu().numpy()
    assert not huff_h[:, :, 16:][np.arange(256) >= nval_h[:, :, None]].any()          # HUFFVAL is zero past the table's symbols
    files = {}
    for b in range(B):
        key = (host[b, :lens_h[b]].tobytes(), huff_h[b].tobytes())
        if key not in files:
            hf = [(h[:16].tobytes(), h[16:16 + int(n)].tobytes()) for h, n in zip(huff_h[b], nval_h[b])]
            files[key] = jpeg_enc.header(8, 8, tables[0], 2, hf) + key[0]
        assert files[key] == want[kind[b]], b
    assert len(files) == 2


def test_ladder_sizes():
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc
    imgs = np.stack([ref.image("natural", 33, 47, 41), ref.image("noise", 33, 47, 42)])
    got = jpeg_enc.ladder_sizes(_dev(imgs), 2, optimize=True)
    want = np.array([[len(oref.pillow_bytes(im, q, 2)) for q in jpeg_enc.LADDER] for im in imgs])
    assert got.shape == (2, 95) and (got == want).all()
    # several calls instead of one, and the default is today's sizes
    assert (jpeg_enc.ladder_sizes(_dev(imgs), 2, max_slot_bytes=1 << 16, optimize=True) == want).all()
    assert (jpeg_enc.ladder_sizes(_dev(imgs), 2) == np.array([[len(ref.pillow_bytes(im, q, 2)) for q in jpeg_enc.LADDER] for im in imgs])).all()


def test_decoder_takes_the_output(trio):
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg, jpeg_enc
    imgs, qs, want = trio
    got = jpeg_enc.encode_batch(_dev(imgs), qs, optimize=True)
    dec = jpeg.JpegBatch(got).decode("cuda:0").cpu().numpy()
    for b in range(3):
        assert (dec[b] == np.array(Image.open(io.BytesIO(got[b])).convert("RGB"))).all()


def _dht_lengths(data):
    """the HUFFVAL counts of a file's DHT segments, in file order"""
    out, i = [], 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == 0xC4:
            out.append(n - 2 - 1 - 16)
        i += 2 + n
    return out


def test_cap_and_lengths_on_noise_q100():
    import torch
    import sgic_amd  # noqa: F401
    from sgic_amd import jpeg_enc, ops
    from sgic_amd._lib import lib
    img = ref.image("noise", 64, 64, 11)
    for sub in (0, 2):
        want = oref.pillow_bytes(img, 100, sub)
        tables = jpeg_enc.quant_tables(100)
        buf, lens, err, huff, nval = ops.jpeg_encode(_dev(img[None]), tables[None], sub, optimize=True)
        cap = ctypes.c_size_t(0)
        assert lib.sgic_jpeg_encode_opt_cap(64, 64, sub, ctypes.byref(cap)) == 0
        nblk = 64 * 3 if sub == 0 else 16 * 6
        assert cap.value == 424 * nblk + 2 and buf.shape == (1, cap.value)          # 53 words of 4 bytes per block, doubled for stuffing
        hh, nv = huff[0].cpu().numpy(), nval[0].cpu().numpy()
        assert nv.tolist() == _dht_lengths(want) and all(int(h[:16].sum()) == n and not h[16 + n:].any() for h, n in zip(hh, nv))
        head = jpeg_enc.header(64, 64, tables, sub, [(h[:16].tobytes(), h[16:16 + n].tobytes()) for h, n in zip(hh, nv)])
        assert want[:len(head)] == head
        assert int(err[0]) == 0 and int(lens[0]) == len(want) - len(head) and int(lens[0]) < cap.value
        assert bytes(buf[0, :int(lens[0])].cpu().numpy()) == want[len(head):]
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
    assert lib.sgic_jpeg_encode_opt_cap(H, W, 2, ctypes.byref(cap)) == 0
    assert lib.sgic_jpeg_encode_opt_work_bytes(B, H, W, 2, ctypes.byref(nbytes)) == 0
    work = torch.empty(nbytes.value + 16, dtype=torch.uint8, device="cuda:0")
    buf = torch.full((B, cap.value), 0xAB, dtype=torch.uint8, device="cuda:0")
    lens = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    err = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    huff = torch.full((B, 4, 272), 0xAB, dtype=torch.uint8, device="cuda:0")
    nval = torch.full((B, 4), -7, dtype=torch.int32, device="cuda:0")
    args = dict(x=x.data_ptr(), B=B, H=H, W=W, sub=2, qt=good.ctypes.data, work=work.data_ptr(), nbytes=nbytes.value, buf=buf.data_ptr(),
                cap=cap.value, lens=lens.data_ptr(), err=err.data_ptr(), huff=huff.data_ptr(), nval=nval.data_ptr())

    def run(**kw):
        a = dict(args, **kw)
        return lib.sgic_jpeg_encode_opt_batch(a["x"], a["B"], a["H"], a["W"], a["sub"], a["qt"], a["work"], a["nbytes"], a["buf"], a["cap"],
                                              a["lens"], a["err"], a["huff"], a["nval"], stream())

    zero, big = good.copy(), good.copy()
    zero[1, 1, 63] = 0
    big[0, 0, 5] = 256
    base_cap = ctypes.c_size_t(0)
    assert lib.sgic_jpeg_encode_cap(H, W, 2, ctypes.byref(base_cap)) == 0 and base_cap.value < cap.value
    bad = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(sub=3), dict(sub=-1),
           dict(qt=zero.ctypes.data), dict(qt=big.ctypes.data), dict(x=None), dict(qt=None), dict(work=None), dict(buf=None),
           dict(lens=None), dict(err=None), dict(work=work.data_ptr() + 4), dict(lens=lens.data_ptr() + 2), dict(err=err.data_ptr() + 1),
           dict(nbytes=nbytes.value - 1), dict(cap=cap.value - 1), dict(cap=base_cap.value),
           dict(huff=None), dict(nval=None), dict(huff=huff.data_ptr() + 1), dict(nval=nval.data_ptr() + 2)]
    for kw in bad:
        assert run(**kw) == SGIC_EINVAL, kw
        assert lib.sgic_last_error()
    out = ctypes.c_size_t(0)
    assert lib.sgic_jpeg_encode_opt_cap(0, W, 2, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_opt_cap(H, W, 5, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_opt_cap(H, W, 2, None) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_opt_work_bytes(0, H, W, 2, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_opt_cap(16384, 16384, 2, ctypes.byref(out)) == SGIC_EINVAL
    # the block limit follows the 1665-bit bound: 1071 x 803 MCUs of 3 blocks are 2 580 039 blocks, which the baseline call takes
    assert lib.sgic_jpeg_encode_cap(8 * 803, 8 * 1071, 0, ctypes.byref(out)) == 0
    assert lib.sgic_jpeg_encode_opt_cap(8 * 803, 8 * 1071, 0, ctypes.byref(out)) == SGIC_EINVAL
    assert lib.sgic_jpeg_encode_opt_cap(8192, 8192, 2, ctypes.byref(out)) == 0
    torch.cuda.synchronize()
    assert (buf == 0xAB).all() and (lens == -7).all() and (err == -7).all() and (huff == 0xAB).all() and (nval == -7).all()   # nothing ran
    assert run() == 0                                                                      # and the good call does
    torch.cuda.synchronize()
    assert (err == 0).all() and (lens > 0).all() and (nval > 0).all()
