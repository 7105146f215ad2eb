"""The shape table of the wide-operand GPU tests (tests/wide_shapes.py) keeps its promises: every tier-A case has an operand above
2^31 elements and every tier-B case one above 2^32, each probe set holds a slab that lies wholly beyond the highest mark an operand
crosses, and no case needs more than the footprint limit.  No GPU."""
import pytest

import wide_shapes as ws


@pytest.mark.parametrize("name", sorted(ws.CASES))
def test_case_is_wide_probed_and_fits(name):
    case = ws.CASES[name]
    n, span = case["n_units"], case["span"]
    widest = max(op.elems(n) for op in case["operands"].values())
    if case["tier"] in ("A", "B"):
        assert widest > 1 << 31, (name, widest)
    if case["tier"] == "B":
        assert widest > 1 << 32, (name, widest)
    pr = ws.probes(case)
    assert pr[0] == 0 and pr[-1] == n - span and all(0 <= p <= n - span for p in pr), (name, pr)
    crossed = 0
    for op in case["operands"].values():
        ms = ws.marks(op, n)
        if not ms:
            continue
        crossed += 1
        top = ms[-1]
        beyond = [p for p in pr if any(a >= top for a, _ in op.pieces(p, p + span, n))]
        assert beyond, (name, op.name, top, pr)
        # the slab that holds each mark, and a slab on either side of it, are probed
        for m in ms:
            s = min((op.unit_of(m, n) // span) * span, n - span)
            assert s in pr and max(s - span, 0) in pr, (name, op.name, m, s, pr)
    assert crossed or case["tier"] == "E", name
    assert ws.footprint(case) <= ws.FOOTPRINT_LIMIT, (name, ws.footprint(case))
    for phase in case["phases"]:
        assert all(o in case["operands"] for o in phase), (name, phase)


def test_the_issue_probe_sets():
    """contiguous fp32 images of 1024 x 1024 x 128: the marks fall at images 4, 8, 16 and 32"""
    assert ws.probes(ws.CASES["groupnorm_plain"]) == [0, 3, 4, 7, 8, 15, 16]
    b = ws.probes(ws.CASES["groupnorm_planes_B"])
    assert {0, 3, 4, 7, 8, 15, 16, 31, 32} <= set(b)
    assert ws.probes(ws.CASES["vqgan_attention"]) == [0, 31, 32, 63, 64, 127, 128]
    g = ws.probes(ws.CASES["gemm_f32"])
    M = ws.GEMM_M
    assert g == [0, (1 << 22) - 256, 1 << 22, (1 << 23) - 256, 1 << 23, (1 << 24) - 256, 1 << 24, M - 256]
    s = ws.probes(ws.CASES["search_index"])
    assert s == [0, 1023, 1024, 2047, 2048, 2049]
    assert all(p // ws.SEARCH_BLOCK in s for p in ws.SEARCH_PLANTED)


def test_marks_inside_halo_and_planes_layouts():
    """in the halo and planes layouts the marks fall inside an image: that image and both neighbours are probed"""
    case = ws.CASES["groupnorm_halo"]
    y = case["operands"]["y"]
    img = ws.HALO * ws.C
    for m in ws.marks(y, case["n_units"]):
        b = m // img
        assert m % img and {b - 1, b, b + 1} <= set(ws.probes(case))
    case = ws.CASES["groupnorm_planes_A"]
    y = case["operands"]["y"]
    assert y.elems(ws.B_A) == 3 * ws.B_A * ws.HALO * ws.C and len(y.pieces(0, 1, ws.B_A)) == 12
    for m in ws.marks(y, ws.B_A):
        b = y.unit_of(m, ws.B_A)
        lo, hi = [(a, e) for a, e in y.pieces(b, b + 1, ws.B_A) if a <= m < e][0]
        assert lo <= m < hi and {max(b - 1, 0), b, min(b + 1, ws.B_A - 1)} <= set(ws.probes(case))


def test_seg_row_map_matches_the_kernels():
    c = ws.CASES["gemm_c_seg"]["operands"]["c"]
    for m in (0, 5, ws.GEMM_SEG - 1, ws.GEMM_SEG, 3 * ws.GEMM_SEG + 7, ws.GEMM_M - 1):
        row = (m // ws.GEMM_SEG) * ws.GEMM_SEG_STRIDE + m % ws.GEMM_SEG
        assert c.row(m) == row and c.unit_of(row * c.ld + 3, ws.GEMM_M) == m
    assert c.unit_of((ws.GEMM_SEG + 5) * c.ld, ws.GEMM_M) == ws.GEMM_SEG           # an element of the gap -> the next segment's first row
    assert c.elems(ws.GEMM_M) > 1 << 31
