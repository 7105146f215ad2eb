"""encoder.swin_rowmap against the textbook construction (no GPU: the map is built on the host; it is the d_rowmap / d_biasvar
argument of every Swin attention launch, tests/test_gpu_attention_rowmap.py covers the kernel side).

The reference block shifts the map cyclically by -win/2 in both directions, cuts it into win x win windows in raster order, tokens
of a window in raster order (blocks/swin_transformer.py:26,77,96,104-106), and adds the upper-lower mask to the LAST ROW of
windows (`dots[:, :, -nw_w:]`, line 116) and the left-right mask to the LAST COLUMN of windows (`dots[:, :, nw_w - 1::nw_w]`,
line 117).  encoder.SwinW stacks the bias as [plain | +UL | +LR | +UL+LR], so bit 0 of a window's variant selects the
upper-lower mask and bit 1 the left-right mask."""
import pytest
import torch

import kernels_ref as kr


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("B,H,W,win", [(2, 32, 48, 16), (1, 16, 16, 16)])
def test_swin_rowmap_vs_roll_and_window_partition(B, H, W, win, shifted):
    import sgic_amd  # noqa
    from sgic_amd.encoder import swin_rowmap
    rowmap, var = swin_rowmap(B, H, W, win, shifted, "cpu")
    nseq = B * (H // win) * (W // win)
    assert rowmap.dtype == torch.int32 and rowmap.shape == (nseq * win * win,) and var.dtype == torch.int32 and var.shape == (nseq,)
    # a permutation of the row space: every position is in exactly one window
    assert torch.equal(torch.sort(rowmap.long()).values, torch.arange(B * H * W))
    # an integer-valued map whose value names its position, stored in 16x16-tile-major rows, indexed with the row map ...
    x = torch.arange(B * H * W * 2, dtype=torch.float32).reshape(B, H, W, 2)
    got = kr.tm16(x)[rowmap.long()].reshape(nseq, win * win, 2)
    # ... is the window partition of the cyclically shifted map, token for token
    s = win // 2 if shifted else 0
    want = kr.window_partition(torch.roll(x, shifts=(-s, -s), dims=(1, 2)), win)
    assert torch.equal(got, want)
    # bias variants: windows are in raster order (b, window row, window column)
    nh, nw = H // win, W // win
    v = var.reshape(B, nh, nw)
    last_row = torch.zeros(B, nh, nw, dtype=torch.bool)
    last_col = torch.zeros(B, nh, nw, dtype=torch.bool)
    if shifted:
        last_row[:, nh - 1, :] = True
        last_col[:, :, nw - 1] = True
    assert torch.equal((v & 1).bool(), last_row) and torch.equal((v & 2).bool(), last_col)
    assert int(v.min()) >= 0 and int(v.max()) <= 3
