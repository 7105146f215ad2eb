"""GPU: FSIM / FSIMc of csrc/fsim.hip (quality.fsim, phase_congruency, ops.fsim_planes_u8) against the fp64 restatement
tests/fsim_ref.py.  Both sides are fp64; they differ in summation order and in a dense DFT against np.fft, which moved the pooled
values by 4e-16 relative on the CPU, so fsim / fsimc are held to the relative 1e-11 of tests/test_gpu_quality.py and the PC maps
(which sit at 0 on one side and 1e-17 on the other at the threshold) to the same figure as an absolute bound.  The reduced planes
have to be the restatement's bits.  Measured on an MI355X over these cases: PC maps within 3.5e-14 (640 x 642), fsim / fsimc within 4.8e-16."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsim_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-11
# 31 x 44: an odd and an even axis, an even count for the median; 31 x 45: an odd count; 47 x 47: prime; 64 x 64; 130 x 70: seams of
# the 16 x 32 pooling tiles, of the 64-line groups and of the 32-output groups of the transform; 2 x 2, 2 x 9: the smallest;
# 384 x 400: F = 2 (the even anchor); 640 x 642: F = 3 (the odd anchor), 214 x 214 after the reduction
SIZES = [(31, 44), (31, 45), (47, 47), (64, 64), (130, 70), (2, 2), (2, 9), (384, 400), (640, 642)]
KINDS = ("noise", "step", "blur")


def _up(x):
    return torch.from_numpy(np.array(x)).to(DEV)[None]        # a copy: the shared cases are read-only


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_parity_with_the_restatement(H, W, kind):
    import sgic_amd  # noqa: F401
    from sgic_amd import ops, quality
    a, b, want = ref.case(kind, H, W)
    F, h, w = quality.fsim_reduction(H, W)
    assert (F, h, w) == ref.reduction(H, W)
    da, db = _up(a), _up(b)
    for d, key in ((da, "planes_a"), (db, "planes_b")):
        got = ops.fsim_planes_u8(d)
        assert got.dtype == torch.float64 and got.shape == (1, 3, h, w)
        for c, name in enumerate("YIQ"):
            assert np.array_equal(got[0, c].cpu().numpy(), want[key][c]), (key, name)         # bit for bit
    ys = torch.from_numpy(np.stack([want["planes_a"][0], want["planes_b"][0]])).to(DEV)
    pc = quality.phase_congruency(ys)
    assert pc.dtype == np.float64 and pc.shape == (2, h, w)
    pc_err = max(float(np.abs(pc[0] - want["pc_a"]).max()), float(np.abs(pc[1] - want["pc_b"]).max()))
    f, fc = quality.fsim(da, db)
    f2, fc2 = quality.fsim(da, db)
    assert np.array_equal(da[0].cpu().numpy(), a) and np.array_equal(db[0].cpu().numpy(), b)            # inputs untouched
    assert f.dtype == np.float64 and f.shape == (1,) and fc.dtype == np.float64 and fc.shape == (1,)
    assert f.tobytes() == f2.tobytes() and fc.tobytes() == fc2.tobytes()                                # the same bits twice
    print(f"{H}x{W} {kind}: PC max abs error {pc_err:.3e} (PC max {pc.max():.3f}); fsim {float(f[0])!r} against {want['fsim']!r}, "
          f"relative error {_rel(float(f[0]), want['fsim']):.3e}; fsimc {float(fc[0])!r} against {want['fsimc']!r}, "
          f"relative error {_rel(float(fc[0]), want['fsimc']):.3e}")
    assert pc_err <= TOL
    assert pc.min() >= 0.0 and pc.max() <= 1.0
    assert _rel(float(f[0]), want["fsim"]) <= TOL and _rel(float(fc[0]), want["fsimc"]) <= TOL


def test_a_batch_equals_its_single_calls_bitwise():
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    pairs = [ref.case(kind, 64, 64)[:2] for kind in KINDS]
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
    b = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
    batch = quality.fsim(a, b)
    assert batch[0].shape == (3,) and batch[1].shape == (3,)
    for j in range(3):
        one = quality.fsim(a[j:j + 1].contiguous(), b[j:j + 1].contiguous())
        for k in range(2):
            assert batch[k][j:j + 1].tobytes() == one[k].tobytes(), (k, j)
    rev = quality.fsim(a.flip(0).contiguous(), b.flip(0).contiguous())      # other neighbours, another slot
    for k in range(2):
        assert rev[k][::-1].tobytes() == batch[k].tobytes(), k
    ys = torch.from_numpy(np.stack([ref.case(kind, 64, 64)[2]["planes_a"][0] for kind in KINDS])).to(DEV)
    pcs = quality.phase_congruency(ys)
    assert quality.phase_congruency(ys.flip(0).contiguous())[::-1].tobytes() == pcs.tobytes()
    assert quality.phase_congruency(ys[1:2].contiguous()).tobytes() == pcs[1:2].tobytes()


@pytest.mark.parametrize("H,W", [(47, 47), (31, 44), (384, 400), (2, 2)])
def test_equal_images_give_exactly_one(H, W):
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    a = ref.case("noise", H, W)[0]
    f, fc = quality.fsim(_up(a), _up(a))
    assert float(f[0]) == 1.0 and float(fc[0]) == 1.0


def test_flat_planes():
    import sgic_amd  # noqa: F401
    from sgic_amd import quality
    grey = torch.full((1, 40, 56, 3), 90, dtype=torch.uint8, device=DEV)
    f, fc = quality.fsim(grey, grey.clone())
    assert float(f[0]) == 1.0 and float(fc[0]) == 1.0                   # sum PCm = 0, equal planes
    f, fc = quality.fsim(grey, torch.full_like(grey, 140))
    assert float(f[0]) == 0.0 and float(fc[0]) == 0.0
    other = grey.clone()                                                # another colour, constant too: only I and Q (and a little Y) differ
    other[..., 0], other[..., 2] = 52, 187
    f, fc = quality.fsim(grey, other)
    assert float(f[0]) == 0.0 and float(fc[0]) == 0.0
    pc = quality.phase_congruency(torch.full((2, 9, 12), 77.25, dtype=torch.float64, device=DEV))
    assert np.array_equal(pc, np.zeros((2, 9, 12)))
    # a flat original against a textured reconstruction: PC1 = 0 everywhere, the pooled values are the restatement's;
    # in one batch with a textured pair, which must not change
    a, b, want = ref.case("noise", 40, 56)
    flat = np.full((40, 56, 3), 90, np.uint8)
    wf = ref.fsim(flat, b)
    f, fc = quality.fsim(torch.from_numpy(np.stack([flat, a])).to(DEV), torch.from_numpy(np.stack([b, b])).to(DEV))
    print(f"flat against texture: {float(f[0])!r}, {float(fc[0])!r} against {wf!r}")
    assert _rel(float(f[0]), wf[0]) <= TOL and _rel(float(fc[0]), wf[1]) <= TOL
    assert _rel(float(f[1]), want["fsim"]) <= TOL and _rel(float(fc[1]), want["fsimc"]) <= TOL


def test_refusals():
    """a ValueError that names the limit from the wrappers, SGIC_EINVAL before any launch from the C entry points"""
    import sgic_amd  # noqa: F401
    from sgic_amd import _lib, quality
    for H, W, what in ((1, 50, r"sides >= 2"), (50, 1, r"sides >= 2"), (300, 2100, r"<= 2048")):
        a = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match=what):
            quality.fsim(a, a)
        m = quality.measure_fsim(a, a)
        assert m == {"fsim": None, "fsimc": None}
    with pytest.raises(ValueError, match=r"sides >= 2"):
        quality.phase_congruency(torch.zeros(1, 1, 12, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match=r"<= 2048"):
        quality.phase_congruency(torch.zeros(1, 2, 2049, dtype=torch.float64, device=DEV))
    img = torch.zeros(1, 300, 2100, 3, dtype=torch.uint8, device=DEV)
    nbytes = ctypes.c_size_t(0)
    _lib.call("sgic_fsim_work_bytes", 1, 16, 16, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    out = torch.full((4, 16, 16), -7.0, dtype=torch.float64, device=DEV)
    size = ctypes.c_size_t
    bad = [("sgic_fsim", (img, img, 1, 1, 50, work, size(nbytes.value), out[0], out[1])),
           ("sgic_fsim", (img, img, 1, 300, 2100, work, size(nbytes.value), out[0], out[1])),
           ("sgic_fsim", (img, img, 0, 16, 16, work, size(nbytes.value), out[0], out[1])),
           ("sgic_fsim", (img, img, 1, 16, 16, work, size(nbytes.value - 1), out[0], out[1])),
           ("sgic_fsim", (img, None, 1, 16, 16, work, size(nbytes.value), out[0], out[1])),
           ("sgic_fsim", (img, img, 1, 16, 16, None, size(nbytes.value), out[0], out[1])),
           ("sgic_fsim", (img, img, 1, 16, 16, work, size(nbytes.value), out[0], None)),
           ("sgic_fsim_phasecong", (out, 1, 1, 16, work, size(nbytes.value), out[1])),
           ("sgic_fsim_phasecong", (out, 1, 16, 2049, work, size(nbytes.value), out[1])),
           ("sgic_fsim_phasecong", (out, 1, 16, 16, work, size(64), out[1])),
           ("sgic_fsim_phasecong", (None, 1, 16, 16, work, size(nbytes.value), out[1])),
           ("sgic_fsim_planes_u8", (img, 1, 1, 50, out)),
           ("sgic_fsim_planes_u8", (None, 1, 16, 16, out))]
    for name, args in bad:
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call(name, *args)
    for name, args in (("sgic_fsim_work_bytes", (1, 1, 50)), ("sgic_fsim_work_bytes", (1, 300, 2100)), ("sgic_fsim_work_bytes", (0, 16, 16)),
                       ("sgic_fsim_phasecong_work_bytes", (1, 1, 12)), ("sgic_fsim_phasecong_work_bytes", (1, 2049, 2))):
        with pytest.raises(_lib.SgicError, match="rc=-1"):
            _lib.call(name, *args, ctypes.byref(nbytes))
    assert bool((out == -7.0).all())
