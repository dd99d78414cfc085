"""Input builders of tests/test_gpu_ext_edges.py (CPU tensors only), kept importable without a GPU so that
tests/test_ext_edges_cpu.py can assert that they still discriminate: ties at the extrema of the disparity-order count,
and tied minima / maxima whose column-major first element is not the row-major first one for the smoothness loss."""
import torch


# ---- io_disp_order_count ---------------------------------------------------------------------------------------------
def disp_order_inputs(B, H, W, seed):
    """-> d1, d2, m1, m2 [B,1,H,W] fp32, order [B], ovl [B] (int64).
    Disparities are multiples of 0.25 in [0, 1] with a run of exact zeros (rows of d1, columns of d2): the values a ReLU
    head produces, so `<=` and `<` count different pixels.  m2 covers the whole image (its erosion is the interior), m1
    is a band from one border across the image (it touches three borders and lies inside m2).  Every erosion is
    non-empty, so the oracle never meets an empty selection.  depth orders cycle through {0, 1, 2} x is_overlap {0, 1}."""
    g = torch.Generator().manual_seed(seed)
    d1 = torch.randint(0, 5, (B, 1, H, W), generator=g).float() * 0.25
    d2 = torch.randint(0, 5, (B, 1, H, W), generator=g).float() * 0.25
    d1[:, :, :max(H // 3, 1), :] = 0.0
    d2[:, :, :, W - max(W // 3, 1):] = 0.0
    m2 = torch.ones(B, 1, H, W)
    m1 = torch.zeros(B, 1, H, W)
    for b in range(B):
        if min(H, W) == 3:                       # the only masks of a 3-wide image whose erosion is not empty hold the centre cross
            m1[b] = 1.0
            m1[b, 0, H - 1, 0] = m1[b, 0, H - 1, W - 1] = 0.0
        elif b % 2 == 0:
            m1[b, 0, :3 + (3 * b) % (H - 3), :] = 1.0        # top, left and right borders
        else:
            m1[b, 0, :, :3 + (3 * b) % (W - 3)] = 1.0        # left, top and bottom borders
    order = torch.tensor([(b % 3) for b in range(B)], dtype=torch.int64)
    ovl = torch.tensor([((b // 3) % 2) for b in range(B)], dtype=torch.int64)
    return d1, d2, m1, m2, order, ovl


def swap_orders(order):
    """depth orders 0 and 1 exchanged (what le_order = 1 means: `<=` on disp1 for depth order 1)."""
    return torch.where(order == 0, torch.ones_like(order), torch.where(order == 1, torch.zeros_like(order), order))


def disp_order_count_strict(d1, d2, m1, m2, order, ovl):
    """oracle.midas_oracle.disp_order_count with `<` / `>` for `<=` / `>=`: what a kernel with strict comparisons would
    count.  Only for the guard that the inputs tell the two apart."""
    from scipy import ndimage
    total = 0
    for b in range(d1.shape[0]):
        if int(ovl[b]) != 0 or int(order[b]) not in (0, 1):
            continue
        e1 = torch.from_numpy(ndimage.binary_erosion(m1[b, 0].numpy()).astype(bool))
        e2 = torch.from_numpy(ndimage.binary_erosion(m2[b, 0].numpy()).astype(bool))
        a, c = (d1[b, 0], d2[b, 0]) if int(order[b]) == 0 else (d2[b, 0], d1[b, 0])
        total += int((a[e1] < a[e2].max()).sum() + (a[e1].min() < a[e2]).sum())
        total += int((c[e1] > c[e2].max()).sum() + (c[e1].min() > c[e2]).sum())
    return float(total) / float(d1.shape[2] * d1.shape[3])


# ---- io_smooth_loss_* --------------------------------------------------------------------------------------------------
def tied_disparity(B, H, W, seed):
    """-> disp [B,1,H,W], img [B,3,H,W] fp32.  disp = randint(0, 6) * 0.25: exact in fp32, so equal neighbours are equal
    in both precisions and no neighbour difference changes sign between them; its minimum 0 and maximum 1.25 occur many
    times.  For H, W >= 4 a minimum and a maximum are planted in row 0 and in column 0 and taken out of the corner, so
    that the first extremum in column-major order (key w * H + h) is never the first one in row-major order."""
    g = torch.Generator().manual_seed(seed)
    disp = torch.randint(0, 6, (B, 1, H, W), generator=g).float() * 0.25
    img = torch.randn(B, 3, H, W, generator=g)
    if H >= 4 and W >= 4:
        disp[:, :, 0, 0] = 0.5
        disp[:, :, 0, W - 1] = 0.0
        disp[:, :, H - 1, 0] = 0.0
        disp[:, :, 0, W - 2] = 1.25
        disp[:, :, H - 2, 0] = 1.25
    return disp, img


def first_extrema(dmap):
    """dmap [H,W] -> {'min': (col_major_first, row_major_first), 'max': ...} as (h, w) pairs."""
    H, W = dmap.shape
    out = {}
    for name, val in (("min", dmap.min()), ("max", dmap.max())):
        hw = (dmap == val).nonzero().tolist()
        out[name] = (tuple(min(hw, key=lambda p: p[1] * H + p[0])), tuple(min(hw, key=lambda p: p[0] * W + p[1])))
    return out
