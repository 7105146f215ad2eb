"""The shape table of tests/test_gpu_wide_operands.py: operands past 2^31 (tier A) and 2^32 (tier B) elements.

A case is a call of one entry point at a wide shape.  Its logical space is `n_units` units (images, batch items, rows); a probe p is
the slab of `span` consecutive units that starts at unit p (span = 1 image; 256 rows of a GEMM; 4096 rows of the search index).
Every operand of the call says where a range of units lives in it, in ELEMENTS from its base:
  Rows    unit u is `rpu` consecutive rows of `ld` elements (plain NHWC rows, a zero-halo NHWC buffer with rpu = (H+2)(W+2), a GEMM
          operand with rpu = 1, the columns [:, :3] of a 4-column buffer with ld = 4);
  Planes  slice-major bf16x3 planes [3][cols / 32][n_units rpu][32] (csrc/split3.h): a slab has one piece in each of the
          3 cols / 32 chunks;
  Seg     a GEMM output written through the row map m -> (m // seg) seg_stride + m % seg into a larger buffer.
The width marks are the byte offsets 2^31 and 2^32 and the element indices 2^31 and 2^32, in every operand.  probes(case) is: slab
0, the last slab, and for every mark an operand crosses the slab that holds it with its neighbours -- the slab before and the slab
itself when the mark is exactly where a piece of the slab begins, else the slab and both neighbours.
footprint(case) is the largest sum of bytes that are live together: the wide operands of a phase, one slab of every operand (the
slab reruns), `extra` (buffers the wrappers cache: the split GEMM's activation planes, GroupNorm's statistics) and SCRATCH (the
comparisons' temporaries).  The GPU tests hold their max_memory_allocated against it."""

MARK_BYTES = (1 << 31, 1 << 32)
MARK_ELEMS = (1 << 31, 1 << 32)
FOOTPRINT_LIMIT = 64 * 10 ** 9          # bytes per test: a quarter of the card
HEADROOM = 8 * 10 ** 9                  # free memory a test wants beyond its footprint
GUARD = 4096                            # sentinel elements at both ends of an output the test allocates
SCRATCH = 3 * 10 ** 9                   # temporaries of the comparisons: contiguous copies of a slab, the regenerated image, bit views

H = W = 1024
C = 128
HW = H * W
HALO = (H + 2) * (W + 2)
B_A, B_B = 17, 33                       # tier A: above 2^31 elements; tier B: above 2^32 (the production batch plus one)
GEMM_M, GEMM_K, GEMM_N, GEMM_SPAN = (1 << 24) + 288, 128, 128, 256
GEMM_SEG, GEMM_SEG_STRIDE = 1 << 20, (1 << 20) + 256
ATT_B, ATT_L, ATT_C = 129, 4096, 512
SEARCH_D, SEARCH_BLOCK, SEARCH_N = 512, 4096, (1 << 23) + 8192
SEARCH_PLANTED = (0, (1 << 22) - 1, 1 << 22, (1 << 23) - 1, 1 << 23, SEARCH_N - 1)
SEARCH_K = 64                           # centroids of assign_codes


class Rows:
    def __init__(self, name, rpu, ld, esize=4):
        self.name, self.rpu, self.ld, self.esize = name, rpu, ld, esize

    def elems(self, n_units):
        return n_units * self.rpu * self.ld

    def pieces(self, u0, u1, n_units):
        return [(u0 * self.rpu * self.ld, u1 * self.rpu * self.ld)]

    def unit_of(self, e, n_units):
        return e // (self.rpu * self.ld)


class Planes:
    def __init__(self, name, rpu, cols):
        self.name, self.rpu, self.cols, self.esize = name, rpu, cols, 2

    def elems(self, n_units):
        return 3 * n_units * self.rpu * self.cols

    def pieces(self, u0, u1, n_units):
        rows = n_units * self.rpu
        return [((c * rows + u0 * self.rpu) * 32, (c * rows + u1 * self.rpu) * 32) for c in range(3 * self.cols // 32)]

    def unit_of(self, e, n_units):
        return ((e // 32) % (n_units * self.rpu)) // self.rpu


class Seg:
    def __init__(self, name, ld, seg, seg_stride, esize=4):
        self.name, self.ld, self.seg, self.seg_stride, self.esize = name, ld, seg, seg_stride, esize

    def row(self, m):
        return (m // self.seg) * self.seg_stride + m % self.seg

    def elems(self, n_units):
        return (self.row(n_units - 1) + 1) * self.ld

    def pieces(self, u0, u1, n_units):
        assert u0 // self.seg == (u1 - 1) // self.seg, "a probe block must not straddle a segment"
        return [(self.row(u0) * self.ld, (self.row(u1 - 1) + 1) * self.ld)]

    def unit_of(self, e, n_units):
        p = e // self.ld
        s, o = divmod(p, self.seg_stride)
        return min(s * self.seg + o if o < self.seg else (s + 1) * self.seg, n_units - 1)


def _case(name, tier, n_units, span, operands, phases, extra=0, what=""):
    return dict(name=name, tier=tier, n_units=n_units, span=span, operands={o.name: o for o in operands}, phases=phases, extra=extra,
                what=what)


def _image_cases():
    x = Rows("x", HW, C)
    xs = Rows("x", HW // 4, C)                 # the 512 x 512 input of the nearest-2x upsample
    y = Rows("y", HW, C)
    yh = Rows("y", HALO, C)                    # zero-halo fp32 NHWC
    yp = Planes("y", HALO, C)                  # zero-halo bf16x3 planes
    r = Rows("r", HW, C)
    o4 = Rows("y", HW, 4)                      # the thin convolution's 4-column output
    gn_ws = lambda B: B * 64 * C * 2 * 8 + B * 32 * 2 * 4      # noqa: E731
    cases = [
        _case("groupnorm_plain", "A", B_A, 1, [x, y], [("x", "y")], gn_ws(B_A), "ops.groupnorm, plain output"),
        _case("groupnorm_halo", "A", B_A, 1, [x, yh], [("x", "y")], gn_ws(B_A), "ops.groupnorm, halo=True fp32 output"),
        _case("halo_copy_plain", "A", B_A, 1, [x, yh], [("x", "y")], 0, "ops.halo_copy"),
        _case("halo_copy_up_f32", "A", B_A, 1, [xs, yh], [("x", "y")], 0, "ops.halo_copy upsample=True, fp32 output"),
        _case("halo_copy_tile16", "A", B_A, 1, [x, yh], [("x", "y")], 0, "ops.halo_copy tile16=True"),
        _case("conv_f32", "A", B_A, 1, [Rows("x", HALO, C), r, y], [("x", "r", "y")], 0, "ops.conv3x3 f32 path with residual"),
        _case("conv_split_res", "A", B_A, 1, [x, Planes("p", HALO, C), r, y], [("x", "p"), ("p", "r", "y")], gn_ws(B_A),
              "ops.conv3x3 split path fed by groupnorm's planes, with residual"),
    ]
    for tier, B in (("A", B_A), ("B", B_B)):
        cases += [
            _case(f"groupnorm_planes_{tier}", tier, B, 1, [x, yp], [("x", "y")], gn_ws(B), "ops.groupnorm to_conv planes output"),
            _case(f"halo_copy_up_planes_{tier}", tier, B, 1, [xs, yp], [("x", "y")], 0, "ops.halo_copy upsample=True, planes output"),
            _case(f"conv_split_{tier}", tier, B, 1, [x, Planes("p", HALO, C), y], [("x", "p"), ("p", "y")], gn_ws(B),
                  "ops.conv3x3 split path fed by groupnorm's planes"),
            _case(f"conv_thin_{tier}", tier, B, 1, [Rows("x", HALO, C), o4], [("x", "y")], 0, "ops.conv3x3 thin kernel, Cout = 3"),
        ]
    return cases


def _gemm_cases():
    M, K, N = GEMM_M, GEMM_K, GEMM_N
    a, c, r = Rows("a", 1, K), Rows("c", 1, N), Rows("r", 1, N)
    ws = 3 * M * K * 2                         # ops._A3_WS: the activation planes of a split GEMM fed with fp32
    return [
        _case("gemm_f32", "A", M, GEMM_SPAN, [a, c], [("a", "c")], 0, "ops.gemm precision=f32"),
        _case("gemm_split3", "A", M, GEMM_SPAN, [a, c], [("a", "c")], ws, "ops.gemm precision=split3"),
        _case("gemm_residual", "A", M, GEMM_SPAN, [a, r, c], [("a", "r", "c")], ws, "ops.gemm with a residual"),
        _case("gemm_c_seg", "A", M, GEMM_SPAN, [a, Seg("c", N, GEMM_SEG, GEMM_SEG_STRIDE)], [("a", "c")], ws,
              "ops.gemm writing through a c_seg row map into a larger buffer"),
        _case("gemm_to_gemm", "A", M, GEMM_SPAN, [a, Planes("c", 1, N)], [("a", "c")], ws, "ops.gemm to_gemm=True planes output"),
        _case("gemm_planes_a", "A", M, GEMM_SPAN, [a, Planes("ap", 1, K), c], [("a", "ap", "c")], 0,
              "ops.gemm fed a pre-split Planes A operand"),
    ]


def _other_cases():
    L, c = ATT_L, ATT_C
    att = _case("vqgan_attention", "A", ATT_B, 1, [Rows("q", L, c), Rows("k", L, c), Rows("s", L, L), Rows("vt", c, L), Rows("o", L, c)],
                [("q", "k", "s", "vt", "o")], 0, "gemm_batched S = Q K^T, softmax_rows in place, gemm_batched P V")
    n = SEARCH_N
    units = n // SEARCH_BLOCK
    # db, r_db, the assignment (int32 ids + int64 M + fp32 score) and the sort of cluster_sums (ids, order, their sorted copies)
    search = _case("search_index", "A", units, 1,
                   [Rows("db", SEARCH_BLOCK, SEARCH_D, 1), Rows("r_db", SEARCH_BLOCK, 1), Rows("assign", SEARCH_BLOCK, 1),
                    Rows("assign_m", SEARCH_BLOCK, 1, 8)], [("db", "r_db", "assign", "assign_m")], n * (4 + 8 + 4 + 8 + 4 + 8),
                   "search_codes / range / rank / assign_codes / cluster_sums over a u8 index above 2^32 bytes")
    # end to end at the SMALL width: 32 channels at resolution 1024 (2^30 elements, 2^32 bytes), its halo planes, the convolution's
    # output and residual, the attention scores at resolution 64, and every cached halo / planes buffer of the lower resolutions
    # (`extra`: an allowance; the decode peaks at 38.2 GB of max_memory_allocated on an MI355X)
    e2e = _case("decode_batch_32x1024", "E", 32, 1, [Rows("h", HW, 32), Planes("hp", HALO, 32), Rows("r", HW, 32), Rows("o", HW, 32)],
                [("h", "hp", "r", "o")], 22 * 10 ** 9, "encode_batch + decode_batch of 32 images of 1024 x 1024, SMALL configuration")
    return [att, search, e2e]


CASES = {c["name"]: c for c in _image_cases() + _gemm_cases() + _other_cases()}


def operand_bytes(case, name):
    op = case["operands"][name]
    return op.elems(case["n_units"]) * op.esize


def marks(op, n_units):
    """the width marks inside the operand, as element indices"""
    total = op.elems(n_units)
    return sorted({m for m in MARK_ELEMS + tuple(b // op.esize for b in MARK_BYTES) if m < total})


def probes(case):
    n, span = case["n_units"], case["span"]
    last = n - span
    out = {0, last}
    for op in case["operands"].values():
        for m in marks(op, n):
            s = min((op.unit_of(m, n) // span) * span, last)
            on_edge = any(a == m for a, _ in op.pieces(s, s + span, n))
            out |= {max(s - span, 0), s} | (set() if on_edge else {min(s + span, last)})
    return sorted(out)


def footprint(case):
    n, span = case["n_units"], case["span"]
    wide = max(sum(operand_bytes(case, o) for o in phase) for phase in case["phases"])
    slab = sum(sum(b - a for a, b in op.pieces(0, span, n)) * op.esize for op in case["operands"].values())
    return wide + slab + case["extra"] + SCRATCH
