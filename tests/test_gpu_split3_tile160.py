"""GPU tests of the split GEMM's 160x256 tile (launch mode 32: an odd number of block rows per wave, so the A fragment's register
set alternates with the K slice's parity), of launch mode 26 choosing it by arithmetic, and of the LDS-DMA pieces dealt over the
planes (the 160x256 and the 128x192 tile).  Everything is compared bitwise with the same call on other tiles -- the arithmetic per
output element is fixed by K alone -- and one call per shape against an fp64 product at the bound of
test_gpu_split3.py::test_edge_shapes_every_mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T160 = 32


@pytest.fixture(scope="module")
def ops():
    import sgic_amd  # noqa
    from sgic_amd import ops as O
    return O


def _data(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    r = torch.randn(M, N, device="cuda", generator=g)
    return a, w, bias, r


# K = 32, 64, 96, 160: nk = 1, 2, 3, 5 slices -- both slice parities, the odd tail, the single slice
# M = 160 (one tile), 161 (one row into a second tile), 81 (one row past the seam between the two wave rows), 487 (three tiles + 7 rows)
# N = 256 (one column tile), 264 (a second column tile 8 wide), 1000 (ragged last tile)
@pytest.mark.parametrize("K", [32, 64, 96, 160])
def test_tile160_equals_tiles_1_and_4_on_the_smallest_shapes(ops, K):
    for M in (160, 161, 81, 487):
        for N in (256, 264, 1000):
            a, w, bias, r = _data(M, N, K, M + N + K)
            out = {t: ops.gemm(a, w, bias, residual=r, precision="split3", tile=t) for t in (T160, 1, 4)}
            torch.cuda.synchronize()
            assert torch.equal(out[T160], out[1]), (M, N, K)
            assert torch.equal(out[T160], out[4]), (M, N, K)
            ref = a.double() @ w.double().T + bias.double() + r.double()
            err, bound = float((out[T160].double() - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
            assert err < bound, (M, N, K, err, bound)


@pytest.fixture(scope="module")
def epi(ops):
    M, N, K = 487, 1000 - 8, 96          # N % 32 == 0 (the planes output needs it): 992 = three column tiles + 224
    return (M, N, K) + _data(M, N, K, 77)


def test_tile160_bias_gelu(ops, epi):
    M, N, K, a, w, bias, r = epi
    out = {t: ops.gemm(a, w, bias, act=ops.ACT_GELU, precision="split3", tile=t) for t in (T160, 1, 4)}
    torch.cuda.synchronize()
    assert torch.equal(out[T160], out[1]) and torch.equal(out[T160], out[4])
    ref = torch.nn.functional.gelu(a.double() @ w.double().T + bias.double())
    assert float((out[T160].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))


def test_tile160_residual_in_place(ops, epi):
    M, N, K, a, w, bias, r = epi
    got = {}
    for t in (T160, 1, 4):
        x = r.clone()
        y = ops.gemm(a, w, bias, residual=x, out=x, precision="split3", tile=t)      # out is residual
        torch.cuda.synchronize()
        assert y.data_ptr() == x.data_ptr()
        got[t] = x
    assert torch.equal(got[T160], got[1]) and torch.equal(got[T160], got[4])
    ref = a.double() @ w.double().T + bias.double() + r.double()
    assert float((got[T160].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))


def test_tile160_planes_output(ops, epi):
    M, N, K, a, w, bias, r = epi
    old = ops.PRECISION
    ops.set_precision("split3")
    try:
        for t in (T160, 1, 4):
            pl = ops.gemm(a, w, bias, residual=r, to_gemm=True, tile=t)
            f = ops.gemm(a, w, bias, residual=r, tile=t)
            want = ops.split3_planes(f)
            torch.cuda.synchronize()
            assert isinstance(pl, ops.Planes) and torch.equal(pl.t, want.t), t
    finally:
        ops.set_precision(old)


def test_tile160_c_seg_row_map(ops):
    n, Lt, L, K, N = 3, 163, 200, 96, 264           # 489 logical rows: three tiles + 9 rows; every tile straddles a segment seam
    a, w, bias, _ = _data(n * Lt, N, K, 5)
    got = {}
    for t in (T160, 1, 4):
        out = torch.zeros(n * L, N, device="cuda")
        ops.gemm(a, w, bias, out=out, M=n * Lt, c_seg=(Lt, L), precision="split3", tile=t)
        torch.cuda.synchronize()
        got[t] = out
    assert torch.equal(got[T160], got[1]) and torch.equal(got[T160], got[4])
    o3 = got[T160].reshape(n, L, N)
    ref = (a.double() @ w.double().T + bias.double()).reshape(n, Lt, N)
    assert float((o3[:, :Lt].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
    assert float(o3[:, Lt:].abs().max()) == 0.0


def test_tile160_presplit_planes_operand(ops, epi):
    M, N, K, a, w, bias, r = epi
    ap = ops.split3_planes(a)
    y_pl = ops.gemm(ap, w, bias, residual=r, precision="split3", tile=T160)
    y = ops.gemm(a, w, bias, residual=r, precision="split3", tile=T160)
    y1 = ops.gemm(ap, w, bias, residual=r, precision="split3", tile=1)
    torch.cuda.synchronize()
    assert torch.equal(y_pl, y) and torch.equal(y_pl, y1)


def test_mode26_one_round_of_160_row_tiles_equals_the_two_launch_plan(ops):
    """(9248, 1024): mode 26 is one launch of 160x256 tiles, mode 27 whole rounds of 128x256 + a ring tail at row 8192"""
    M, N, K = 9248, 1024, 96
    a, w, bias, r = _data(M, N, K, 26)
    got = {}
    for t in (26, 1, 27):
        x = r.clone()
        ops.gemm(a, w, bias, residual=x, out=x, precision="split3", tile=t)
        torch.cuda.synchronize()
        got[t] = x
    assert torch.equal(got[26], got[1]) and torch.equal(got[26], got[27])
    # one image's rows computed alone == those rows inside the batch
    x = r[289:578].clone()
    ops.gemm(a[289:578].contiguous(), w, bias, residual=x, out=x, precision="split3", tile=23)
    torch.cuda.synchronize()
    assert torch.equal(x, got[26][289:578])


@pytest.mark.parametrize("M,N,K", [(8192, 768, 96), (300, 200, 160)])
def test_tiles_128x192_with_pieces_dealt_over_the_planes(ops, M, N, K):
    a, w, bias, r = _data(M, N, K, M + N)
    out = {t: ops.gemm(a, w, bias, residual=r, precision="split3", tile=t) for t in (1, 28, 29)}
    torch.cuda.synchronize()
    assert torch.equal(out[28], out[1]) and torch.equal(out[29], out[1])
    ref = a.double() @ w.double().T + bias.double() + r.double()
    assert float((out[28].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
