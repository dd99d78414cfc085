"""The operator kernels of the MiDaS branch (csrc/ext_ops.hip) on the paths and edges tests/test_gpu_ext_ops.py does not
reach: every dispatch arm of the launchers (ext_ops.hip io_* functions; each case names the condition that routes it),
grid caps and grid-stride loops, degenerate extents, ties, aliasing, and the autograd nodes without a node-level test.

Every reference is plain torch in fp64 on the CPU or oracle/midas_oracle.py; for bf16 it is built from bf16-rounded
inputs.  Every output buffer is NaN-filled and GUARD elements longer than the kernel is told, every workspace is exactly
the size its query returns plus such a tail; the tail must come back untouched.

Bars (the ones the project applies to these kernels): fp32 elementwise / upsample / head out 1e-6, fp32 dw / db 1e-5,
tensors stored as bf16 6e-3 (one output rounding), fp32-accumulated sums of bf16 data 2e-5.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ext_edge_inputs import disp_order_inputs, first_extrema, swap_orders, tied_disparity
from instaorder_amd import _lib
from test_gpu_ops import L, P, ST, nhwc, relerr  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 48
TDT = {0: torch.float32, 1: torch.bfloat16}
DTN = {0: "fp32", 1: "bf16"}
IO_ERR_WORKSPACE = -2


def rounded(t, dt):
    """fp64 copy of t after rounding to the storage type (the reference sees what the kernel sees)"""
    return t.float().to(TDT[dt]).double()


def put(t, dt):
    return t.float().to(TDT[dt]).to(DEV).contiguous()


def guarded(n, dtype=torch.float32):
    """n + GUARD elements of NaN: the kernel is told n"""
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)


def tail_untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# =====================================================================================================================
# 1. io_head1_fwd / io_head1_bwd: every dispatch arm.  nq = pitch * sizeof(T) / 16 (ext_ops.hip io_head1_fwd / _bwd:
#    `nq == 4` -> head1_*_rows_kernel<T,4>, `nq == 8` -> <T,8>, anything else -> the column-lane head1_*_kernel)
# =====================================================================================================================
HEAD_CASES = [
    # dt, pitch, C
    pytest.param(0, 16, 16, id="fp32-rows4-p16c16"),          # nq = 4
    pytest.param(0, 16, 12, id="fp32-rows4-p16c12"),          # nq = 4, one padding chunk
    pytest.param(0, 32, 32, id="fp32-rows8-p32c32"),          # nq = 8
    pytest.param(0, 32, 20, id="fp32-rows8-p32c20"),          # nq = 8, three padding chunks
    pytest.param(0, 64, 32, id="fp32-cols-p64c32"),           # nq = 16: column lanes
    pytest.param(0, 8, 4, id="fp32-cols-p8c4"),               # nq = 2
    pytest.param(0, 20, 20, id="fp32-cols-p20c20"),           # nq = 5
    pytest.param(1, 32, 32, id="bf16-rows4-p32c32"),          # nq = 4
    pytest.param(1, 32, 12, id="bf16-rows4-p32c12"),          # nq = 4, C % 8 == 4: the guard q*VEC+e < C inside a chunk
    pytest.param(1, 32, 4, id="bf16-rows4-p32c4"),            # nq = 4, half a chunk
    pytest.param(1, 64, 32, id="bf16-rows8-p64c32"),          # nq = 8: the production form
    pytest.param(1, 64, 64, id="bf16-rows8-p64c64"),          # nq = 8, no padding
    pytest.param(1, 64, 20, id="bf16-rows8-p64c20"),          # nq = 8, C % 8 == 4
    pytest.param(1, 16, 16, id="bf16-cols-p16c16"),           # nq = 2: column lanes
    pytest.param(1, 40, 36, id="bf16-cols-p40c36"),           # nq = 5
    pytest.param(1, 8, 4, id="bf16-cols-p8c4"),               # nq = 1
]


@pytest.mark.parametrize("M", [1, 257, 70001])       # one row; five 64-row blocks, the last a single row; rpb = 69, nb = 1015, a 35-row tail block
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dt,pitch,C", HEAD_CASES)
def test_head1_every_arm(dt, pitch, C, relu, M):
    """x and w are multiples of 1/8, b = -1/4: every pre-activation is exact in fp32 (and x in bf16), so the ReLU mask of
    the kernel and of the fp64 reference cannot differ by rounding, and exact zeros occur.  Row 0 is x = e_0 with
    w[0] = -b: s == 0 exactly, where the kernel's `out > 0` must agree with torch's ReLU gradient at 0 (0)."""
    g = torch.Generator().manual_seed(1000 * pitch + 10 * C + dt)
    x = torch.randint(-16, 17, (M, pitch), generator=g).double() / 8           # the padding channels hold values too
    w = torch.randint(1, 9, (C,), generator=g).double() / 8 * (torch.randint(0, 2, (C,), generator=g).double() * 2 - 1)
    b = torch.tensor([-0.25], dtype=torch.float64)
    x[0] = 0.0
    x[0, 0] = 1.0
    w[0] = 0.25
    dy = torch.randn(M, generator=g).double()
    w.requires_grad_(True)
    b.requires_grad_(True)
    xr = x[:, :C].clone().requires_grad_(True)
    z = xr @ w + b
    assert float(z.detach()[0]) == 0.0
    if M > 1:
        assert float((z <= 0).double().mean()) >= 1.0 / 3.0 and int((z == 0).sum()) >= 1
    y = torch.relu(z) if relu else z
    gx, gw, gb = torch.autograd.grad(y, [xr, w, b], dy)

    xd, wd, bd, dyd = put(x, dt), put(w.detach(), 0), put(b.detach(), 0), put(dy, 0)
    out = guarded(M)
    _lib.check(L().io_head1_fwd(P(xd), M, pitch, C, P(wd), P(bd), relu, P(out), dt, ST()), "head1 fwd")
    assert tail_untouched(out, M)
    assert relerr(out[:M], y.detach()) < (2e-5 if dt else 1e-6)
    npart = int(L().io_colsum_partial_floats(M, C))
    part = guarded(npart)
    dx = guarded(M * pitch, TDT[dt])
    dw, db = guarded(C), guarded(1)
    _lib.check(L().io_head1_bwd(P(dyd), P(out), P(xd), M, pitch, C, P(wd), relu, P(dx), P(dw), P(db), P(part), npart, dt,
                                ST()), "head1 bwd")
    for buf, n in ((out, M), (dx, M * pitch), (dw, C), (db, 1), (part, npart)):
        assert tail_untouched(buf, n)
    dxv = dx[:M * pitch].view(M, pitch).float()
    assert relerr(dxv[:, :C], gx) < (6e-3 if dt else 1e-6)
    if pitch > C:
        assert float(dxv[:, C:].abs().max()) == 0.0
    assert not bool(torch.isnan(dxv).any())
    assert relerr(dw[:C], gw) < (2e-5 if dt else 1e-5)
    assert relerr(db[:1], gb) < (2e-5 if dt else 1e-5)


# =====================================================================================================================
# 2. io_colsum.  vec = 16 / sizeof(T); `C % vec == 0 && 256 % (C / vec) == 0` -> colsum_partial_rows_kernel, otherwise the
#    element form colsum_partial_kernel.  rows_per_block: rpb = max(64, ceil(M / 1024)).
# =====================================================================================================================
COLSUM_CASES = [pytest.param(0, 1, id="fp32-c1-element"), pytest.param(0, 2, id="fp32-c2-element"),
                pytest.param(0, 4, id="fp32-c4-rows-256lanes"),          # C / vec == 1
                pytest.param(0, 8, id="fp32-c8-rows"), pytest.param(0, 64, id="fp32-c64-rows"),
                pytest.param(0, 256, id="fp32-c256-rows-4lanes"),
                pytest.param(1, 1, id="bf16-c1-element"), pytest.param(1, 2, id="bf16-c2-element"),
                pytest.param(1, 4, id="bf16-c4-element"),
                pytest.param(1, 8, id="bf16-c8-rows-256lanes"),          # C / vec == 1
                pytest.param(1, 16, id="bf16-c16-rows"), pytest.param(1, 256, id="bf16-c256-rows-8lanes")]


def _colsum_input(M, C, dt):
    g = torch.Generator().manual_seed(M + 7 * C + dt)
    return rounded(torch.randn(M, C, generator=g) + 0.5, dt)             # (+ 0.5: no column sum is a cancellation)


# M = 1: one row; 63 / 65: below the 64-row floor / two blocks, the second a single row; 70001: rpb = 69 (off the floor),
# nb = 1015 > 64, so colsum_final_kernel's lanes loop
@pytest.mark.parametrize("M", [1, 63, 65, 70001])
@pytest.mark.parametrize("dt,C", COLSUM_CASES)
def test_colsum_every_form(dt, C, M):
    v = _colsum_input(M, C, dt)
    npart = int(L().io_colsum_partial_floats(M, C))
    part, s = guarded(npart), guarded(C)
    _lib.check(L().io_colsum(P(put(v, dt)), M, C, P(s), P(part), npart, dt, ST()), "colsum")
    assert tail_untouched(s, C) and tail_untouched(part, npart)
    assert relerr(s[:C], v.sum(0)) < (2e-5 if dt else 1e-6)


def test_colsum_short_workspace_is_an_error_and_writes_nothing():
    M, C = 65, 8
    v = _colsum_input(M, C, 0)
    npart = int(L().io_colsum_partial_floats(M, C))
    part, s = guarded(npart), guarded(C)
    rc = L().io_colsum(P(put(v, 0)), M, C, P(s), P(part), npart - 1, 0, ST())
    torch.cuda.synchronize()
    assert rc == IO_ERR_WORKSPACE
    assert bool(torch.isnan(s).all()) and bool(torch.isnan(part).all())


# =====================================================================================================================
# 3. elementwise: io_bias_act, io_relu_bwd, io_add, bit-equal to torch (bf16: computed in fp32, rounded once).
#    ew_blocks(n4) = min(8192, ceil(n4 / 256)): the last count needs more than 8192 blocks, so the grid-stride loops iterate.
# =====================================================================================================================
EW_COUNTS = [pytest.param(4, id="n4-one-vector"), pytest.param(4 * 1003, id="n4012-partial-block"),
             pytest.param(8192 * 256 * 4 + 148, id="over-block-cap")]


@pytest.mark.parametrize("n", EW_COUNTS)
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_add_bits(dt, n):
    g = torch.Generator().manual_seed(n % 1000 + dt)
    a, b = torch.randn(n, generator=g).to(TDT[dt]), torch.randn(n, generator=g).to(TDT[dt])
    ref = (a.float() + b.float()).to(TDT[dt])
    out = guarded(n, TDT[dt])
    _lib.check(L().io_add(P(a.to(DEV)), P(b.to(DEV)), n, P(out), dt, ST()), "add")
    assert tail_untouched(out, n)
    assert torch.equal(bits(out[:n]), bits(ref))


@pytest.mark.parametrize("inplace", [0, 1], ids=["out", "dx-is-dy"])
@pytest.mark.parametrize("n", EW_COUNTS)
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_relu_bwd_bits(dt, n, inplace):
    g = torch.Generator().manual_seed(n % 1000 + dt + 5)
    dy, act = torch.randn(n, generator=g).to(TDT[dt]), torch.randn(n, generator=g).to(TDT[dt])
    act[0::7] = 0.0          # exact +0.0 and -0.0: not active
    act[3::7] = -0.0
    if n == 4:
        act = torch.tensor([0.0, -0.0, -1.5, 2.0]).to(TDT[dt])
    ref = torch.where(act > 0, dy, torch.zeros_like(dy))
    buf = guarded(n, TDT[dt])
    dyd = dy.to(DEV)
    if inplace:
        buf[:n] = dyd
        dyd = buf
    _lib.check(L().io_relu_bwd(P(dyd), P(act.to(DEV)), n, P(buf), dt, ST()), "relu_bwd")
    assert tail_untouched(buf, n)
    assert torch.equal(bits(buf[:n]), bits(ref))


BIAS_CASES = [
    # M, C, bias, relu
    pytest.param(1, 4, 1, 0, id="n4-bias-norelu"),
    pytest.param(1003, 4, 1, 0, id="c4-partial-block-bias-norelu"),
    pytest.param(1003, 4, 0, 1, id="c4-partial-block-nobias-relu"),
    pytest.param(37, 36, 1, 1, id="c36-bias-relu"),
    pytest.param(16385, 512, 1, 0, id="over-block-cap-bias-norelu"),
    pytest.param(16385, 512, 0, 1, id="over-block-cap-nobias-relu"),
]


@pytest.mark.parametrize("inplace", [0, 1], ids=["out", "out-is-x"])
@pytest.mark.parametrize("M,C,bias,relu", BIAS_CASES)
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_bias_act_bits(dt, M, C, bias, relu, inplace):
    g = torch.Generator().manual_seed(M + C + dt)
    x = torch.randn(M, C, generator=g).to(TDT[dt])
    b = torch.randn(C, generator=g) if bias else None
    ref = x.float() + b if bias else x.float()
    ref = (torch.relu(ref) if relu else ref).to(TDT[dt])
    n = M * C
    buf = guarded(n, TDT[dt])
    xd = x.to(DEV)
    if inplace:
        buf[:n] = xd.reshape(-1)
        xd = buf
    _lib.check(L().io_bias_act(P(xd), P(b.to(DEV)) if bias else None, M, C, relu, P(buf), dt, ST()), "bias_act")
    assert tail_untouched(buf, n)
    assert torch.equal(bits(buf[:n].view(M, C)), bits(ref))


# =====================================================================================================================
# 4. io_upsample2x_bilinear_fwd / _bwd.  IO_UPSAMPLE_LAUNCH: bf16 && C % 8 == 0 -> <bf16,8>, bf16 -> <bf16,4>, fp32 -> <float,4>;
#    up_grid clamps x to 64 blocks (rows of more than 64 * 256 chunks stride) and y to 65535 image rows.
# =====================================================================================================================
def _upsample_check(N, H, W, C, align, dt, seed, fp32_align_bar=None):
    """fp32_align_bar: the fp32 bar with align_corners at extents where the arithmetic of the source index, not a bug, sets
    the error (see UP_WIDE)"""
    g = torch.Generator().manual_seed(seed)
    x = rounded(torch.randn(N, C, H, W, generator=g), dt).requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=bool(align))
    dy = rounded(torch.randn(y.shape, generator=g), dt)
    gx, = torch.autograd.grad(y, [x], dy)
    tol = 6e-3 if dt else (fp32_align_bar if (align and fp32_align_bar) else 1e-6)
    x_l, dy_l = x.detach().permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous()
    n_out, n_in = N * 4 * H * W * C, N * H * W * C
    out = guarded(n_out, TDT[dt])
    _lib.check(L().io_upsample2x_bilinear_fwd(P(put(x_l, dt)), N, H, W, C, align, P(out), dt, ST()), "up fwd")
    assert tail_untouched(out, n_out)
    o = out[:n_out].view(N, 2 * H, 2 * W, C).double().cpu()
    assert relerr(o, y.detach().permute(0, 2, 3, 1)) < tol
    dx = guarded(n_in, TDT[dt])
    _lib.check(L().io_upsample2x_bilinear_bwd(P(put(dy_l, dt)), N, H, W, C, align, P(dx), dt, ST()), "up bwd")
    assert tail_untouched(dx, n_in)
    d = dx[:n_in].view(N, H, W, C).double().cpu()
    assert relerr(d, gx.permute(0, 2, 3, 1)) < tol
    # adjointness on the kernel's own outputs: <up(x), dy> == <x, up^T(dy)>.  Every term of either sum carries at most the
    # relative error of the parity bar, so the two agree to tol * sum |terms| (not tol * |sum|: the sum may cancel).
    lhs, rhs = float((o * dy_l).sum()), float((x_l * d).sum())
    assert abs(lhs - rhs) <= tol * float((o.abs() * dy_l.abs()).sum()), (lhs, rhs)


# fp32 -> <float,4>; bf16 C = 8, 24 -> <bf16,8>; bf16 C = 4, 12 -> <bf16,4>
UP_CHANNELS = [(0, 4), (0, 12), (1, 4), (1, 8), (1, 12), (1, 24)]


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("dt,C", UP_CHANNELS, ids=["%s-c%d" % (DTN[d], c) for d, c in UP_CHANNELS])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (2, 2)])      # lerp_of with H == 1: both taps on one source
def test_upsample_degenerate_extents(H, W, dt, C, align):
    _upsample_check(2, H, W, C, align, dt, seed=100 * H + 10 * W + C)


# rows of more than 64 * 256 = 16384 chunks (the x grid-stride of the `j` loop): chunks per row = 2W * C/V forward, W * C/V backward.
# With align_corners the source index dst * (W - 1) / (2W - 1) is formed in the compute type, by the kernel as by PyTorch: in
# fp32 its fraction -- the interpolation weight -- carries half an ulp of an index of up to W (H below), so the 1e-6 bar of the
# small maps cannot hold at these extents.  Bars for fp32 with align_corners = 4 x the distance of a plain fp32 torch
# evaluation (F.interpolate and its autograd on the CPU) from the fp64 reference on the same inputs, the larger of forward
# and backward, measured with relerr():
#   W = 136:    fwd 1.059e-05  bwd 1.101e-05  -> 4.4e-05        H = 16400:  fwd 1.180e-03  bwd 1.219e-03  -> 4.9e-03
#   W = 264:    fwd 1.981e-05  bwd 1.740e-05  -> 7.9e-05        H = 32800:  fwd 1.744e-03  bwd 1.834e-03  -> 7.3e-03
# (without align_corners the index 0.5 * (dst + 0.5) - 0.5 is exact and the same measurement gives 6e-8 .. 2e-7: 1e-6 stays.)
UP_WIDE = [pytest.param(0, 136, 4.4e-5, id="fp32-w136-fwd-17408-chunks"), pytest.param(1, 264, None, id="bf16-w264-fwd-16896-chunks"),
           pytest.param(0, 264, 7.9e-5, id="fp32-w264-bwd-16896-chunks"), pytest.param(1, 520, None, id="bf16-w520-bwd-16640-chunks")]


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("dt,W,bar", UP_WIDE)
def test_upsample_x_grid_stride(dt, W, bar, align):
    _upsample_check(1, 2, W, 256, align, dt, seed=W, fp32_align_bar=bar)


# more than 65535 image rows (the y clamp of up_grid, the `row` loop): forward N * 2H = 65600, backward N * H = 65600
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,bar", [pytest.param(16400, 4.9e-3, id="h16400-fwd-65600-rows"),
                                   pytest.param(32800, 7.3e-3, id="h32800-bwd-65600-rows")])    # (bars: see UP_WIDE)
def test_upsample_y_clamp(H, bar, dt, align):
    _upsample_check(2, H, 1, 4, align, dt, seed=H, fp32_align_bar=bar)


# =====================================================================================================================
# 5. io_disp_order_count
# =====================================================================================================================
def _disp_count_c_abi(d1, d2, m1, m2, order, ovl, le_order, scale):
    B, _, H, W = d1.shape
    nws = int(L().io_disp_order_workspace_floats(B, H, W))
    ws, out = guarded(nws), guarded(1)
    f = lambda t: t.float().to(DEV).contiguous()       # noqa: E731
    _lib.check(L().io_disp_order_count(P(f(d1)), P(f(d2)), P(f(m1)), P(f(m2)), P(order.to(DEV)), P(ovl.to(DEV)), B, H, W,
                                       le_order, scale, P(out), P(ws), nws, ST()), "disp_order_count")
    assert tail_untouched(ws, nws) and tail_untouched(out, 1)
    return float(out[0])


# disp_blocks(N) = ceil(N / 2048): 24 x 40 -> one block per sample, 160 x 208 -> 17, 3 x 3 -> the erosion is the centre pixel;
# B = 300 > 256: the stride loop of disp_order_finalize_kernel
@pytest.mark.parametrize("le_order", [0, 1])
@pytest.mark.parametrize("B,H,W", [(6, 24, 40), (6, 160, 208), (6, 3, 3), (300, 8, 8)])
def test_disp_order_count_ties_overlap_borders(B, H, W, le_order):
    """Quantised, zero-heavy disparities, overlapping masks on the image border, every (depth order, is_overlap) pair;
    le_order = 1 is the oracle with depth orders 0 and 1 exchanged.  tests/test_ext_edges_cpu.py asserts that on these
    inputs `<` for `<=` and exchanged orders give another count."""
    from oracle import midas_oracle as mo
    d1, d2, m1, m2, order, ovl = disp_order_inputs(B, H, W, seed=H * W + B)
    ref = mo.disp_order_count(d1, d2, m1, m2, swap_orders(order) if le_order else order, ovl)
    assert ref > 0
    got = _disp_count_c_abi(d1, d2, m1, m2, order, ovl, le_order, 1.0)
    assert abs(got - ref) < 1e-6 * max(1.0, abs(ref)), (got, ref)


def test_disp_order_count_node_scale_with_le_order_1():
    from instaorder_amd import ops
    from oracle import midas_oracle as mo
    d1, d2, m1, m2, order, ovl = disp_order_inputs(6, 24, 40, seed=24 * 40 + 6)
    ref = mo.disp_order_count(d1, d2, m1, m2, swap_orders(order), ovl)
    a = [t.cuda() for t in (d1, d2, m1, m2, order, ovl)]
    got = ops.disp_order_count(*a, 1, 1.0)
    got2 = ops.disp_order_count(*a, 1, 0.25)
    assert got.shape == () and abs(float(got) - ref) < 1e-6 * max(1.0, abs(ref)), (float(got), ref)
    assert abs(float(got2) - 0.25 * ref) < 1e-6 * max(1.0, abs(ref))


# =====================================================================================================================
# 6. io_smooth_loss_fwd / _bwd through the C ABI.  smooth_blocks(N) = min(512, ceil(N / 1024)).
# =====================================================================================================================
SM_OUT, SM_GRAD = 0.7, 1.5          # out_scale (= the backward's scale) and the incoming gradient


def _smooth_c_abi(disp, img, prefill=None):
    """-> loss, ddisp [B,1,H,W] (cpu).  prefill: ddisp holds it and the backward accumulates."""
    B, _, H, W = disp.shape
    n = B * H * W
    nws = int(L().io_smooth_loss_workspace_floats(B, H, W))
    ws, gbuf, loss, dd = guarded(nws), guarded(n), guarded(1), guarded(n)
    if prefill is not None:
        dd[:n] = prefill.reshape(-1).to(DEV)
    d, im = disp.float().to(DEV).contiguous(), img.float().to(DEV).contiguous()
    _lib.check(L().io_smooth_loss_fwd(P(d), P(im), B, H, W, SM_OUT, P(loss), P(gbuf), P(ws), nws, ST()), "smooth fwd")
    go = torch.tensor([SM_GRAD], device=DEV)
    _lib.check(L().io_smooth_loss_bwd(P(gbuf), P(ws), P(go), SM_OUT, B, H, W, 0 if prefill is None else 1, P(dd), ST()),
               "smooth bwd")
    for buf, k in ((ws, nws), (gbuf, n), (loss, 1), (dd, n)):
        assert tail_untouched(buf, k)
    return float(loss[0]), dd[:n].view(B, 1, H, W).cpu()


def _smooth_oracle(disp, img):
    from oracle import midas_oracle as mo
    d64 = disp.double().requires_grad_(True)
    ref = mo.smooth_loss(d64, img.double()) * SM_OUT
    g, = torch.autograd.grad(ref, [d64], torch.tensor(SM_GRAD, dtype=torch.float64))
    return float(ref.detach()), g


def _smooth_compare(disp, img):
    ref, gref = _smooth_oracle(disp, img)
    got, gg = _smooth_c_abi(disp, img)
    assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    assert not bool(torch.isnan(gg).any() or torch.isinf(gg).any())
    gmax = float(gref.abs().max())
    assert float((gg.double() - gref).abs().max()) <= 2e-4 * gmax, float((gg.double() - gref).abs().max()) / max(gmax, 1e-300)
    return gg, gref


@pytest.mark.parametrize("B,H,W", [(2, 33, 17), (2, 17, 40),        # non-square, tied: the key w * H + h decides
                                   (2, 2, 9), (2, 9, 2)])           # H - 1 == 1 / W - 1 == 1
def test_smooth_loss_tied_maps(B, H, W):
    """Multiples of 0.25: many equal neighbours (|n(p) - n(q)| has gradient sgn(0) = 0 there) and many minima / maxima; the
    two whole-map sums of the backward go to the elements with the smallest w * H + h (tests/test_ext_edges_cpu.py: that
    is what torch's chained min / max selects, and it is not the row-major first one)."""
    disp, img = tied_disparity(B, H, W, seed=H * 100 + W)
    gg, gref = _smooth_compare(disp, img)
    gmax = float(gref.abs().max())
    for b in range(B):
        ex = first_extrema(disp[b, 0])
        for name in ("min", "max"):
            for hw in ex[name]:
                a, r = float(gg[b, 0][hw]), float(gref[b, 0][hw])
                assert abs(a - r) < 2e-4 * gmax + 1e-3 * abs(r), (b, name, hw, a, r)


def test_smooth_loss_zero_map():
    """mn = mx = 0: both reciprocals are 1e7, every difference is sgn(0)"""
    g = torch.Generator().manual_seed(3)
    loss, gg = _smooth_c_abi(torch.zeros(2, 1, 12, 20), torch.randn(2, 3, 12, 20, generator=g))
    assert loss == 0.0 and bool((gg == 0).all())


def test_smooth_loss_constant_map():
    g = torch.Generator().manual_seed(4)
    _smooth_compare(torch.full((2, 1, 12, 20), 0.75), torch.randn(2, 3, 12, 20, generator=g))


def test_smooth_loss_accumulate_adds_the_plain_result():
    g = torch.Generator().manual_seed(5)
    disp, img = torch.rand(2, 1, 24, 40, generator=g) * 3.0 + 0.2, torch.randn(2, 3, 24, 40, generator=g)
    p = torch.randn(2, 1, 24, 40, generator=g)
    _, r = _smooth_c_abi(disp, img)
    _, acc = _smooth_c_abi(disp, img, prefill=p)
    assert torch.equal(bits(acc), bits(p + r))


def test_smooth_loss_block_cap():
    """726 x 724 = 525 624 pixels: ceil(N / 1024) = 514 > 512, the grid-stride loops of smooth_fwd / _bwd iterate"""
    g = torch.Generator().manual_seed(6)
    disp, img = torch.rand(1, 1, 726, 724, generator=g) * 3.0 + 0.2, torch.randn(1, 3, 726, 724, generator=g)
    gg, gref = _smooth_compare(disp, img)
    flat = disp[0, 0].reshape(-1)
    for idx in (int(flat.argmin()), int(flat.argmax())):
        a, r = float(gg.reshape(-1)[idx]), float(gref.reshape(-1)[idx])
        assert abs(a - r) < 2e-4 * float(gref.abs().max()) + 1e-3 * abs(r), (idx, a, r)


# =====================================================================================================================
# 7. io_weights_prepare / io_weights_unpack_grads, direct.  weights_prepare_kernel: T == 1 -> 64 x 64 tiles, T == 9 -> 32 x 32 x 9,
#    anything else -> the generic body with tap tiles of up to 9.
# =====================================================================================================================
WEIGHT_ROWS = [
    # Co, Ci, T, Cop, Cip, transpose
    (32, 128, 9, 64, 128, True),        # T == 9, co_pad: output channels 32..63 are zeros
    (64, 3, 49, 64, 8, False),          # the stem: generic body, ntt = 6, last tap tile of 4, dst_t = -1
    (96, 40, 1, 128, 64, True),         # T == 1: tile edges in both channel directions
    (256, 256, 1, 256, 256, True),      # T == 1, unpadded, 16 tiles
    (48, 33, 9, 64, 64, True),          # T == 9, odd Ci
    (8, 8, 25, 8, 8, True),             # generic body, ntt = 3 (9 + 9 + 7 taps), a quarter tile
    (264, 260, 9, 320, 264, True),      # T == 9, 10 x 9 = 90 tiles > the 64 blocks of a row: a block does a second tile
]


def _weight_table():
    from instaorder_amd.ops import _WeightDesc
    descs, src, op, gk = [], 3, 5, 2
    for Co, Ci, T, Cop, Cip, tr in WEIGHT_ROWS:
        sz = Cop * T * Cip
        descs.append(_WeightDesc(src, op, op + sz + 7 if tr else -1, gk, Co, Ci, T, Cop, Cip))
        src += Co * Ci * T + 5                     # (gaps everywhere: nothing may be written between the slices)
        op += (2 * sz + 14) if tr else (sz + 7)
        gk += sz + 3
    tab = (_WeightDesc * len(descs))(*descs)
    table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    return descs, table, src, op, gk


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_weights_prepare_direct(dt):
    descs, table, n_par, n_op, _ = _weight_table()
    g = torch.Generator().manual_seed(11)
    params = torch.randn(n_par, generator=g)
    ops_buf = guarded(n_op, TDT[dt])
    _lib.check(L().io_weights_prepare(P(table), len(descs), P(params.to(DEV)), P(ops_buf), dt, ST()), "weights_prepare")
    got = ops_buf.cpu()
    written = torch.zeros(n_op + GUARD, dtype=torch.bool)
    for d in descs:
        w = params[d.src:d.src + d.Co * d.Ci * d.T].view(d.Co, d.Ci, d.T)
        ref = torch.zeros(d.Cop, d.T, d.Cip)
        ref[:d.Co, :, :d.Ci] = w.permute(0, 2, 1)
        sz = d.Cop * d.T * d.Cip
        assert torch.equal(bits(got[d.dst_op:d.dst_op + sz]), bits(ref.to(TDT[dt]).reshape(-1))), (d.Co, d.Ci, d.T)
        written[d.dst_op:d.dst_op + sz] = True
        if d.dst_t >= 0:
            reft = ref.permute(2, 1, 0).contiguous()          # [Cip][T][Cop]
            assert torch.equal(bits(got[d.dst_t:d.dst_t + sz]), bits(reft.to(TDT[dt]).reshape(-1))), (d.Co, d.Ci, d.T, "t")
            written[d.dst_t:d.dst_t + sz] = True
    assert bool(torch.isnan(got[~written]).all())             # the gaps, the missing transpose of the stem and the tail


def test_weights_unpack_grads_direct_full_and_sub_range():
    from instaorder_amd.ops import _WeightDesc
    descs, table, n_par, _, n_gk = _weight_table()
    g = torch.Generator().manual_seed(12)
    gk = torch.randn(n_gk, generator=g)                       # (the padding entries hold values: they must not come through)
    gkd = gk.to(DEV)

    def expect(rows):
        ref = torch.full((n_par + GUARD,), float("nan"))
        for d in rows:
            sz = d.Cop * d.T * d.Cip
            v = gk[d.dst_g:d.dst_g + sz].view(d.Cop, d.T, d.Cip)[:d.Co, :, :d.Ci].permute(0, 2, 1)
            ref[d.src:d.src + d.Co * d.Ci * d.T] = v.reshape(-1)
        return ref

    grads = guarded(n_par)
    _lib.check(L().io_weights_unpack_grads(P(table), len(descs), P(gkd), P(grads), ST()), "unpack_grads")
    assert torch.equal(bits(grads), bits(expect(descs)))      # NaN gaps and tail included: bit patterns
    # rows [2, 5) through an offset table pointer, as WeightPlan.unpack_grads(lo, hi) does: the other rows stay untouched
    grads = guarded(n_par)
    sub = C.c_void_p(table.data_ptr() + 2 * C.sizeof(_WeightDesc))
    _lib.check(L().io_weights_unpack_grads(sub, 3, P(gkd), P(grads), ST()), "unpack_grads sub-range")
    assert torch.equal(bits(grads), bits(expect(descs[2:5])))


# =====================================================================================================================
# 8. autograd nodes without a node-level test (through ops.*: the node is what is checked)
# =====================================================================================================================
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_node_add_shared(dt):
    from instaorder_amd import ops
    g = torch.Generator().manual_seed(21)
    a64, b64 = rounded(torch.randn(2, 3, 5, 8, generator=g), dt), rounded(torch.randn(2, 3, 5, 8, generator=g), dt)
    dy = put(torch.randn(2, 3, 5, 8, generator=g), dt)
    a, b = put(a64, dt).requires_grad_(True), put(b64, dt).requires_grad_(True)
    out = ops.add_shared(a, b)
    assert relerr(out.detach().float(), a64 + b64) < (6e-3 if dt else 1e-6)
    ga, gb = torch.autograd.grad(out, [a, b], dy)
    assert torch.equal(ga, dy) and torch.equal(gb, dy)
    assert ga.data_ptr() != gb.data_ptr()           # b gets its OWN copy (the contract of _AddShared's docstring)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_node_avgpool_fc(dt):
    from instaorder_amd import ops
    N, H, W, Cc, K = 3, 5, 7, 128, 3
    g = torch.Generator().manual_seed(22)
    x64 = rounded(torch.randn(N, H, W, Cc, generator=g), dt).requires_grad_(True)
    w64 = torch.randn(K, Cc, generator=g).double().requires_grad_(True)
    b64 = torch.randn(K, generator=g).double().requires_grad_(True)
    ref = x64.mean((1, 2)) @ w64.t() + b64
    dl = torch.randn(K, N, generator=g)
    gx, gw, gb = torch.autograd.grad(ref, [x64, w64, b64], dl.t().double())
    x = put(x64.detach(), dt).requires_grad_(True)
    w, b = put(w64.detach(), 0).requires_grad_(True), put(b64.detach(), 0).requires_grad_(True)
    logits = ops.avgpool_fc(x, w, b)
    assert relerr(logits.detach(), ref.detach()) < (2e-5 if dt else 1e-5)
    dld = dl.to(DEV).t()                             # [N][K] with strides (1, N)
    assert not dld.is_contiguous()
    dx, dw, db = torch.autograd.grad(logits, [x, w, b], dld)
    assert dx.dtype == TDT[dt] and relerr(dx.float(), gx) < (6e-3 if dt else 1e-5)
    assert relerr(dw, gw) < (2e-5 if dt else 1e-5) and relerr(db, gb) < (2e-5 if dt else 1e-5)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_node_bias_act_fewer_bias_entries_than_channels(dt):
    """32 bias entries on 64 stored channels (the co_pad output of the 128 -> 32 convolution): the padded channels stay 0
    through the ReLU, carry no gradient, and db has 32 entries"""
    from instaorder_amd import ops
    g = torch.Generator().manual_seed(23)
    x64 = rounded(torch.randn(2, 3, 5, 64, generator=g), dt)
    x64[..., 32:] = 0.0
    b64 = torch.randn(32, generator=g).double().requires_grad_(True)
    dy64 = rounded(torch.randn(2, 3, 5, 64, generator=g), dt)
    xr = x64.clone().requires_grad_(True)
    ref = torch.relu(xr + torch.cat([b64, torch.zeros(32, dtype=torch.float64)]))
    gx, gb = torch.autograd.grad(ref, [xr, b64], dy64)
    x, b = put(x64, dt).requires_grad_(True), put(b64.detach(), 0).requires_grad_(True)
    y = ops.bias_act(x, b, True)
    assert relerr(y.detach().float(), ref.detach()) < (6e-3 if dt else 1e-6)
    assert float(y.detach()[..., 32:].float().abs().max()) == 0.0
    dx, db = torch.autograd.grad(y, [x, b], put(dy64, dt))
    assert db.shape == (32,) and relerr(db, gb) < (2e-5 if dt else 1e-5)
    assert relerr(dx.float(), gx) < (6e-3 if dt else 1e-6)
    assert float(dx[..., 32:].float().abs().max()) == 0.0


# ops.conv2d(groups=32) -> _GroupedConv: io_gconv_pack, io_gconv2d_fwd / _dgrad / _wgrad, io_gconv_unpack_grad
GCONV_CASES = [pytest.param(0, 8, 1, id="fp32-cg8-s1"), pytest.param(0, 8, 2, id="fp32-cg8-s2"),
               pytest.param(1, 8, 1, id="bf16-cg8-s1"), pytest.param(1, 8, 2, id="bf16-cg8-s2"),
               pytest.param(1, 32, 1, id="bf16-cg32-s1")]


@pytest.mark.parametrize("dt,cg,stride", GCONV_CASES)
def test_node_grouped_conv_non_square(dt, cg, stride):
    from instaorder_amd import ops
    N, H, W, groups = 2, 9, 14, 32
    Cc = cg * groups
    g = torch.Generator().manual_seed(24 + cg + stride)
    x64 = rounded(torch.randn(N, Cc, H, W, generator=g), dt).requires_grad_(True)
    w64 = rounded(torch.randn(Cc, cg, 3, 3, generator=g) / np.sqrt(9 * cg), dt).requires_grad_(True)
    yref = F.conv2d(x64, w64, stride=stride, padding=1, groups=groups)
    dy64 = rounded(torch.randn(yref.shape, generator=g), dt)
    gx, gw = torch.autograd.grad(yref, [x64, w64], dy64)
    x = put(x64.detach().permute(0, 2, 3, 1), dt).requires_grad_(True)
    w = put(w64.detach(), 0).requires_grad_(True)
    y = ops.conv2d(x, w, stride=stride, pad=1, groups=groups)
    assert y.shape == (N, yref.shape[2], yref.shape[3], Cc)
    assert relerr(y.detach().float().permute(0, 3, 1, 2), yref.detach()) < (6e-3 if dt else 2e-6)
    dx, dw = torch.autograd.grad(y, [x, w], put(dy64.permute(0, 2, 3, 1), dt))
    assert relerr(dx.float().permute(0, 3, 1, 2), gx) < (6e-3 if dt else 2e-6)
    assert dw.dtype == torch.float32 and relerr(dw, gw) < (2e-5 if dt else 2e-6)
