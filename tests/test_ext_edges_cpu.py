"""Guards of tests/test_gpu_ext_edges.py that need no GPU: the inputs its disparity-order and smoothness tests are built
from must keep telling a right kernel from a subtly wrong one (`<` for `<=`, the two depth orders exchanged, a tie
resolved in row-major order), whoever changes the generators later."""
import pytest
import torch

from ext_edge_inputs import disp_order_count_strict, disp_order_inputs, first_extrema, swap_orders, tied_disparity
from oracle import midas_oracle as mo

DISP_SHAPES = [(6, 24, 40), (6, 160, 208), (6, 3, 3), (300, 8, 8)]
TIED_SHAPES = [(2, 33, 17), (2, 17, 40)]


@pytest.mark.parametrize("B,H,W", DISP_SHAPES)
def test_disp_order_inputs_discriminate(B, H, W):
    d1, d2, m1, m2, order, ovl = disp_order_inputs(B, H, W, seed=H * W + B)
    assert float((m1 * m2).sum()) > 0                                     # the masks overlap
    assert bool((d1 * 4 == (d1 * 4).round()).all()) and float((d1 == 0).float().mean()) > 0.3
    assert set(order.tolist()) == {0, 1, 2} and set(ovl.tolist()) == {0, 1}
    assert {(int(o), int(v)) for o, v in zip(order, ovl)} == {(o, v) for o in (0, 1, 2) for v in (0, 1)}
    ref = mo.disp_order_count(d1, d2, m1, m2, order, ovl)
    assert ref > 0
    assert disp_order_count_strict(d1, d2, m1, m2, order, ovl) != ref      # `<` for `<=` shows
    if min(H, W) > 3:    # (3 x 3: both erosions are the centre pixel, every comparison is v <= v -- the orders cannot differ)
        assert mo.disp_order_count(d1, d2, m1, m2, swap_orders(order), ovl) != ref


def test_disp_order_masks_touch_three_borders():
    _, _, m1, m2, _, _ = disp_order_inputs(6, 24, 40, seed=1)
    assert bool((m2 == 1).all())
    for b in range(6):
        m = m1[b, 0]
        touched = [bool(m[0].any()), bool(m[-1].any()), bool(m[:, 0].any()), bool(m[:, -1].any())]
        assert sum(touched) == 3, (b, touched)


@pytest.mark.parametrize("B,H,W", TIED_SHAPES)
def test_tied_maps_select_the_column_major_first_extremum(B, H, W):
    disp, _ = tied_disparity(B, H, W, seed=H * 100 + W)
    d = disp.double().requires_grad_(True)
    mn = d.min(2, True)[0].min(3, True)[0]
    mx = d.max(2, True)[0].max(3, True)[0]
    gmn, = torch.autograd.grad(mn.sum(), [d], retain_graph=True)
    gmx, = torch.autograd.grad(mx.sum(), [d])
    for b in range(B):
        ex = first_extrema(disp[b, 0])
        for name, grad in (("min", gmn), ("max", gmx)):
            val = disp[b, 0].min() if name == "min" else disp[b, 0].max()
            assert int((disp[b, 0] == val).sum()) > 1                       # tied
            col_first, row_first = ex[name]
            assert col_first != row_first                                  # the two orders disagree
            # torch's chained min(2).min(3) / max(2).max(3) sends everything to the column-major first one
            assert float(grad[b, 0][col_first]) == 1.0 and float(grad[b, 0].abs().sum()) == 1.0
