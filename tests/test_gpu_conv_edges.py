"""The dense convolution launchers on geometry edges, all three passes: io_conv2d_fwd_dt, io_conv2d_dgrad_dt and
io_conv2d_wgrad_dt (csrc/conv_igemm.hip, with conv_p256.hip / conv_halo3.hip in front of it for bf16) in fp32 and bf16 on
the case table of conv_edge_inputs.py -- odd maps through strided filters, no padding and padding beyond the filter's
reach, one-pixel and one-column maps, partial row tiles of 128-wide output tiles, short last splits and k-tiles of the
split-K filter gradient, non-square and large filters the networks never send, and the Winograd forms at their smallest
-- against F.conv2d and autograd in fp64 on the CPU on the same seeded inputs (bf16: inputs rounded to bf16 first).

Metric and bars are those of test_gpu_ops.py / test_gpu_bf16.py / test_gpu_wino.py: max |got - ref| / max |ref| below 2e-5
(fp32), 4e-5 (Winograd forms), 6e-3 (bf16 forward and data gradient: one output rounding), 2e-5 (bf16 filter gradient:
fp32 accumulation of exact products).  On top of that:
- positions the geometry proves exactly zero (conv_edge_inputs.dx_zero_positions / y_zero_positions) must be bit-equal
  to 0.0, or to `add` where the launch accumulates;
- every output (y, dx, dw, the split-K workspace) is the middle of a larger allocation with 4 KiB of sentinel bytes on
  either side, which must be intact after every call; the workspace has exactly io_conv2d_wgrad_workspace_bytes bytes, and
  outputs are pre-filled with NaN so that an unwritten element shows;
- group B (shapes only the C ABI accepts): the result is right, or the call returns an error with a message and writes
  nothing; DESIGN.md lists which;
- the kernel family the launch went to (io_debug_last_nt_route / io_debug_last_wgrad_route) is the one the restated shape
  conditions predict; the finer template choice is held by tests/test_conv_edges_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_edge_inputs as cei
from conv_edge_inputs import CASES, GROUP, IDS, TDT, reference, worst
from instaorder_amd import _lib
from step_edge_inputs import EPS, MOMENTUM, bn_forward_ref, bn_inputs
from test_gpu_ops import L, P, ST, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
SENT = 0xA5
BAR = {0: 2e-5, 1: 6e-3}           # forward / data gradient, by storage type
BAR_WGRAD = 2e-5
BAR_WINO = 4e-5
DTN = {0: "fp32", 1: "bf16"}
CASE_IDS = [IDS[c] for c in CASES]


@pytest.fixture(autouse=True)
def _switches():
    """every eligible bf16 shape goes to the persistent kernels (the route then depends on the shape alone, not on the CU
    count of the box); Winograd forms on; both restored"""
    lib = L()
    prev_p, prev_w = lib.io_get_bf16_p256(), lib.io_get_winograd()
    lib.io_set_bf16_p256(3)
    lib.io_set_winograd(1)
    yield
    lib.io_set_bf16_p256(prev_p)
    lib.io_set_winograd(prev_w)


class Guarded(object):
    """a device tensor in the middle of a larger allocation: GUARD sentinel bytes in front, at least GUARD behind"""

    def __init__(self, shape, dtype, fill=float("nan"), src=None):
        es = torch.empty((), dtype=dtype).element_size()
        self.nb = int(np.prod(shape)) * es
        self.raw = torch.full((GUARD + (self.nb + 15) // 16 * 16 + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.nb].view(dtype).view(shape)
        if src is not None:
            self.t.copy_(src)
        elif self.nb:
            self.t.fill_(fill)
        self.before = self.raw.clone()

    def p(self):
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.nb:] == SENT).all())

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.raw, self.before)


def dev(t, dt):       # NCHW fp64 CPU -> NHWC device tensor of the storage type
    return t.permute(0, 2, 3, 1).contiguous().to(TDT[dt]).to(DEV)


def nchw(t):          # NHWC device tensor -> NCHW fp64 CPU
    return t.detach().float().permute(0, 3, 1, 2).double().cpu()


def bits32(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def filters(ref, case, dt):
    """the fp32 master [Co][R*S][Ci] and, through io_filter_prepare, the forward operand and the transposed one"""
    N, H, W, Ci, Co, R, S, s, p = case
    wk = ref["w"].permute(0, 2, 3, 1).contiguous().float().to(DEV).view(Co, R * S, Ci)
    wt = torch.empty(Ci, R * S, Co, dtype=TDT[dt], device=DEV)
    if dt:
        wf = torch.empty(Co, R * S, Ci, dtype=TDT[dt], device=DEV)
        _lib.check(L().io_filter_prepare(P(wk), Co, R * S, Ci, P(wf), 0, dt, ST()), "filter cast")
    else:
        wf = wk             # (fp32: the master is the operand; io_filter_prepare refuses the copy as nothing to do)
    _lib.check(L().io_filter_prepare(P(wk), Co, R * S, Ci, P(wt), 1, dt, ST()), "filter transpose")
    assert torch.equal(wf.float(), wk) and torch.equal(wt.float(), wk.permute(2, 1, 0))
    return wk, wf, wt


def refused(rc, case, what, outs):
    """group B: a non-zero return must come with a message and must have written nothing.  -> True when refused"""
    if rc == 0:
        return False
    assert GROUP[case] == "B", "%s %s: rejected (%d): %s" % (IDS[case], what, rc, _lib.last_error())
    assert len(_lib.last_error()) > 0
    for o in outs:
        assert o.untouched(), "%s %s: returned %d after writing" % (IDS[case], what, rc)
    print("REFUSED %s %s: %s" % (IDS[case], what, _lib.last_error()))
    return True


def held(tag, case, got, ref, bound, stride=1):
    """the bar, with the worst element's (n, h, w, c), its lattice class and its 128-row tile on failure"""
    e, (n, h, w, c) = worst(got, ref)
    Hh, Ww = ref.shape[2:]
    hc, wc = len(range(h % stride, Hh, stride)), len(range(w % stride, Ww, stride))
    row = (n * hc + h // stride) * wc + w // stride
    msg = "%s %s: %.3e (bar %.1e) worst (n, h, w, c) = (%d, %d, %d, %d), class (%d, %d), row tile %d" % (
        IDS.get(case, str(case)), tag, e, bound, n, h, w, c, h % stride, w % stride, row // 128)
    print("DIST " + msg)
    assert e < bound, msg


def bit_equal(t_nhwc, pos, want_nhwc=None):
    """the NHWC device tensor at the [H, W] positions: all bits zero, or the bits of want_nhwc"""
    got = bits32(t_nhwc)[:, pos.to(DEV)]
    if want_nhwc is None:
        return bool((got == 0).all())
    return torch.equal(got, bits32(want_nhwc)[:, pos.to(DEV)])


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward(case, dt):
    N, H, W, Ci, Co, R, S, s, p = case
    ref = reference(case, dt)
    Ho, Wo = cei.out_hw(case)
    _, wf, _ = filters(ref, case, dt)
    y = Guarded((N, Ho, Wo, Co), TDT[dt])
    rc = L().io_conv2d_fwd_dt(P(dev(ref["x"], dt)), P(wf), y.p(), N, H, W, Ci, Co, R, S, s, p, dt, dt, ST())
    if refused(rc, case, "forward " + DTN[dt], [y]):
        return
    assert y.intact(), "forward wrote outside y"
    assert L().io_debug_last_nt_route() == (cei.bf16_nt_route(cei.geom_fwd(case)) if dt else 0)
    held("forward " + DTN[dt], case, nchw(y.t), ref["y"], BAR[dt])
    zr = cei.y_zero_positions(case)
    if bool(zr.any()):
        assert bit_equal(y.t, zr), "outputs whose taps all lie in the padding must be exactly 0"


# ---- data gradient ------------------------------------------------------------------------------------------------------------------
def _dgrad(case, dt, dyd, wt, dx, add, mask):
    N, H, W, Ci, Co, R, S, s, p = case
    return L().io_conv2d_dgrad_dt(P(dyd), P(wt), dx.p(), add, P(mask), N, H, W, Ci, Co, R, S, s, p, dt, ST())


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dgrad_four_ways(case, dt):
    """plain into a NaN-filled dx; accumulating in place (add == dx); accumulating from a separate tensor (classes without
    taps must then copy it); the same with the ReLU mask -- and, in bf16 on stride-1 shapes, with the mask also as bits
    (io_conv2d_dgrad_fused_dt)"""
    N, H, W, Ci, Co, R, S, s, p = case
    ref = reference(case, dt)
    _, _, wt = filters(ref, case, dt)
    dyd, addd, actd = dev(ref["dy"], dt), dev(ref["add"], dt), dev(ref["act"], dt)
    zr = cei.dx_zero_positions(case)
    shape = (N, H, W, Ci)
    tag = "dgrad %s " % DTN[dt]
    want_route = max([cei.bf16_nt_route(g) for _, _, g in cei.dgrad_classes(case)]) if dt else 0

    dx = Guarded(shape, TDT[dt])
    if not refused(_dgrad(case, dt, dyd, wt, dx, None, None), case, tag + "plain", [dx]):
        assert dx.intact(), "plain: wrote outside dx"
        assert L().io_debug_last_nt_route() == want_route
        held(tag + "plain", case, nchw(dx.t), ref["gx"], BAR[dt], s)
        assert bit_equal(dx.t, zr), "plain: pixels no window reads must be exactly 0"

    acc = Guarded(shape, TDT[dt], src=addd)
    if not refused(_dgrad(case, dt, dyd, wt, acc, acc.p(), None), case, tag + "in place", [acc]):
        assert acc.intact(), "in place: wrote outside dx"
        held(tag + "in place", case, nchw(acc.t), ref["gx"] + ref["add"], BAR[dt], s)
        assert bit_equal(acc.t, zr, addd), "in place: pixels no window reads must keep `add`"

    sep = Guarded(shape, TDT[dt])
    if not refused(_dgrad(case, dt, dyd, wt, sep, P(addd), None), case, tag + "separate add", [sep]):
        assert sep.intact(), "separate add: wrote outside dx"
        held(tag + "separate add", case, nchw(sep.t), ref["gx"] + ref["add"], BAR[dt], s)
        assert bit_equal(sep.t, zr, addd), "separate add: pixels no window reads must be exactly `add`"

    keep = ref["act"] > 0
    want = (ref["gx"] + ref["add"]) * keep
    msk = Guarded(shape, TDT[dt])
    done = not refused(_dgrad(case, dt, dyd, wt, msk, P(addd), actd), case, tag + "add + mask", [msk])
    if done:
        assert msk.intact(), "add + mask: wrote outside dx"
        held(tag + "add + mask", case, nchw(msk.t), want, BAR[dt], s)
        assert bit_equal(msk.t, zr, torch.where(actd > 0, addd, torch.zeros_like(addd))), "add + mask: pixels no window reads must be `add` or 0"
        assert bool((nchw(msk.t)[~keep] == 0).all())
    if dt == 1 and s == 1 and done:
        words = ((actd.float() > 0).view(-1, 32).to(torch.int64) << torch.arange(32, device=DEV)).sum(-1)
        bits = (words & 0xffffffff).to(torch.int64)
        bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
        opt = _lib.DgradFused()
        opt.add, opt.relu_mask, opt.relu_maskbits = addd.data_ptr(), actd.data_ptr(), bits.data_ptr()
        mb = Guarded(shape, TDT[dt])
        rc = L().io_conv2d_dgrad_fused_dt(P(dyd), P(wt), mb.p(), N, H, W, Ci, Co, R, S, p, 1, C.byref(opt), dt, ST())
        if not refused(rc, case, tag + "add + mask as bits", [mb]):
            assert mb.intact(), "mask as bits: wrote outside dx"
            assert torch.equal(bits32(mb.t), bits32(msk.t)), "the mask as bits must give what the mask tensor gives"


# ---- filter gradient -------------------------------------------------------------------------------------------------------------------
def _wgrad(case, dt, ref, tag, bar):
    N, H, W, Ci, Co, R, S, s, p = case
    nb = L().io_conv2d_wgrad_workspace_bytes(N, H, W, Ci, Co, R, S, s, p)
    ws = Guarded((nb,), torch.uint8, fill=0)
    dw = Guarded((Co, R * S, Ci), torch.float32)
    rc = L().io_conv2d_wgrad_dt(P(dev(ref["x"], dt)), P(dev(ref["dy"], dt)), dw.p(), N, H, W, Ci, Co, R, S, s, p, ws.p(), nb, dt,
                                dt, ST())
    if refused(rc, case, tag, [dw, ws]):
        return
    assert dw.intact() and ws.intact(), "filter gradient wrote outside dw or its workspace"
    assert L().io_debug_last_wgrad_route() == (cei.bf16_wgrad_route(cei.geom_fwd(case)) if dt else 0)
    got = dw.t.view(Co, R, S, Ci).permute(0, 3, 1, 2).double().cpu()
    e, (o, r, q, c) = worst(got, ref["gw"])
    msg = "%s %s: %.3e (bar %.1e) worst (o, r, s, c) = (%d, %d, %d, %d)" % (IDS[case], tag, e, bar, o, r, q, c)
    print("DIST " + msg)
    assert e < bar, msg


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_wgrad(case, dt):
    ref = reference(case, dt)
    g = cei.geom_fwd(case)
    wino = dt == 0 and cei.wgrad_form(g, 0, True).startswith("wino")
    _wgrad(case, dt, ref, "wgrad " + DTN[dt] + (" (Winograd row form)" if wino else ""), BAR_WINO if wino else BAR_WGRAD)
    if wino:              # ... and the direct form of the same shape (for 32 | Wo: the scalar row decode)
        L().io_set_winograd(0)
        _wgrad(case, dt, ref, "wgrad fp32 (direct, %s)" % cei.wgrad_form(g, 0, False), BAR_WGRAD)


def test_wgrad_switch_case_runs_both_forms():
    g = cei.geom_fwd(cei.WGRAD_WINO_SWITCH)
    assert cei.wgrad_form(g, 0, True) == "wino-f43" and cei.wgrad_form(g, 0, False) == "rows-w32"
    assert all(cei.wgrad_form(cei.geom_fwd(c), 0, True).startswith("wino") for c in cei.WINO_WGRAD)


# ---- Winograd forward forms at their smallest ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cei.WINO_FWD, ids=[IDS[c] for c in cei.WINO_FWD])
def test_wino_forward(case):
    """io_conv2d_fwd_wino as tests/test_gpu_wino.py calls it: plain, then with the input transform and the statistics
    epilogue"""
    N, H, W, Ci, Co, R, S, s, p = case
    ref = reference(case, 0)
    lib = L()
    nsc = lib.io_conv2d_wino_scratch_floats(Ci, Co)
    sc = torch.empty(nsc, device=DEV)
    xd = dev(ref["x"], 0)
    wd, _, _ = filters(ref, case, 0)
    y = Guarded((N, H, W, Co), torch.float32)
    _lib.check(lib.io_conv2d_fwd_wino(P(xd), P(wd), y.p(), N, H, W, Ci, Co, 1, None, None, None, None, None, None, None, 0.1,
                                      1e-5, None, None, None, None, None, 0, P(sc), nsc, ST()), "wino plain")
    assert y.intact()
    held("wino forward (%s)" % cei.wino_fwd_form(cei.geom_fwd(case))[0], case, nchw(y.t), ref["y"], BAR_WINO)
    g = torch.Generator().manual_seed(3 + H * W)
    rt = lambda t: t.float().double()      # noqa: E731
    scale = rt(torch.randn(1, Ci, generator=g, dtype=torch.float64) * 0.7 + 0.3)
    shift = rt(torch.randn(1, Ci, generator=g, dtype=torch.float64) * 0.5 + 0.4)
    mean = rt(torch.randn(1, Ci, generator=g, dtype=torch.float64) * 0.3)
    v4 = lambda t: t.view(1, -1, 1, 1)      # noqa: E731
    ref2 = F.conv2d(F.relu((ref["x"] - v4(mean)) * v4(scale) + v4(shift)), ref["w"], padding=1)
    gamma, beta = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g)
    rm, rv = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
    mean2, rstd, sc2, sh2 = (torch.empty(Co, device=DEV) for _ in range(4))
    nws = lib.io_conv2d_bnstats_workspace_floats(N, H, W, Co, 3, 3, 1, 1, 1)
    ws = torch.empty(nws, device=DEV)
    y2 = Guarded((N, H, W, Co), torch.float32)
    f = lambda t: t.float().to(DEV)      # noqa: E731
    _lib.check(lib.io_conv2d_fwd_wino(P(xd), P(wd), y2.p(), N, H, W, Ci, Co, 1, P(f(mean)), P(f(scale)), P(f(shift)),
                                      P(f(gamma)), P(f(beta)), P(rm), P(rv), 0.1, 1e-5, P(mean2), P(rstd), P(sc2), P(sh2), P(ws),
                                      nws, P(sc), nsc, ST()), "wino xf+stats")
    assert y2.intact()
    held("wino forward xf + stats", case, nchw(y2.t), ref2, BAR_WINO)
    yk = nchw(y2.t)                     # statistics of the kernel's own output, test_gpu_wino.py's bars
    assert relerr(mean2, yk.mean((0, 2, 3))) < 2e-5
    assert relerr(rstd, 1.0 / torch.sqrt(yk.var((0, 2, 3), unbiased=False) + 1e-5)) < 2e-5


# ---- fused forms on the smallest maps ------------------------------------------------------------------------------------------------
def _chk(tag, got, ref, bound):
    e = relerr(got, ref)
    print("DIST %-52s %.3e  (bound %.1e)" % (tag, e, bound))
    assert e < bound, (tag, e, bound)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case,G", cei.FUSED, ids=["n128-1x1-g1", "n256-1x1-g2", "n32-2x2-g1"])
def test_fused_forms_on_the_smallest_maps(case, G, dt):
    """io_conv2d_fwd_bnstats_dt and io_conv2d_dgrad_bnbwd_dt where a 128-row tile is 128 (or 32) samples: the references and
    bars of tests/test_gpu_convbn.py (test_fwd_bnstats_dt_grouped, test_dgrad_bnbwd_dt), with BatchNorm inputs that keep
    every pre-activation a margin away from zero (step_edge_inputs.bn_inputs), so that the fp64 reference forms the ReLU
    mask itself and every element is compared"""
    N, H, W, Ci, Co, R, S, s, p = case
    bf = dt == 1
    M = N * H * W
    lib = L()
    f = lambda t: t.detach().float().to(DEV).contiguous()      # noqa: E731
    rd = lambda t: cei.rounded(t, dt)                          # noqa: E731
    # forward + statistics
    ref = reference(case, dt)
    g = torch.Generator().manual_seed(77 + N + G + dt)
    gamma = (torch.rand(Co, generator=g, dtype=torch.float64) + 0.5).float().double()
    beta = torch.randn(Co, generator=g, dtype=torch.float64).float().double()
    rm0 = (torch.randn(Co, generator=g, dtype=torch.float64) * 0.1).float().double()
    rv0 = (torch.rand(Co, generator=g, dtype=torch.float64) + 0.5).float().double()
    yrows = ref["y"].permute(0, 2, 3, 1).reshape(M, Co)
    st = bn_forward_ref(yrows, G, gamma, beta, rm0, rv0)
    _, wf, _ = filters(ref, case, dt)
    y = Guarded((N, H, W, Co), TDT[dt])
    d_rm, d_rv = f(rm0), f(rv0)
    mean, rstd, scale, shift = (torch.full((G * Co,), float("nan"), device=DEV) for _ in range(4))
    nws = lib.io_conv2d_bnstats_workspace_floats(N, H, W, Co, R, S, s, p, G)
    ws = Guarded((nws,), torch.float32)
    _lib.check(lib.io_conv2d_fwd_bnstats_dt(P(dev(ref["x"], dt)), P(wf), y.p(), N, H, W, Ci, Co, R, S, s, p, G, P(f(gamma)),
                                            P(f(beta)), P(d_rm), P(d_rv), MOMENTUM, EPS, P(mean), P(rstd), P(scale), P(shift),
                                            ws.p(), nws, dt, 0, ST()), "conv + stats")
    assert y.intact() and ws.intact()
    assert lib.io_debug_last_nt_route() == 0
    tag = "%s fwd_bnstats %s G=%d" % (IDS.get(case, "n%d-1x1" % N), DTN[dt], G)
    held(tag + " y", case, nchw(y.t), ref["y"], 1.1e-2 if bf else 2e-5)
    _chk(tag + " mean", mean.view(G, Co), st["mean"], 2e-5)
    _chk(tag + " rstd", rstd.view(G, Co), st["rstd"], 1e-4)
    _chk(tag + " scale", scale.view(G, Co), st["scale"], 1e-4)
    assert torch.equal(shift.view(G, Co).cpu(), beta.float().expand(G, Co))
    _chk(tag + " running_mean", d_rm, st["rm"], 2e-5)
    _chk(tag + " running_var", d_rv, st["rv"], 1e-4)
    # data gradient + BatchNorm backward of the producer: autograd through conv(relu(bn(ya))) w.r.t. ya / gamma / beta
    d = bn_inputs(M // G, G, Ci, dt)
    ya = d["y"].clone().requires_grad_(True)                               # [M, Ci], rows in NHWC order
    ga, ba = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    pre = bn_forward_ref(ya, G, ga, ba)["pre"]
    assert float(pre.detach().abs().min()) > d["margin"]
    keep = (pre.detach() > 0)
    a = (pre * keep).view(N, H, W, Ci).permute(0, 3, 1, 2)
    o = F.conv2d(a, ref["w"], stride=1, padding=p)
    do = rd(torch.randn(o.shape, generator=g, dtype=torch.float64))
    gy, gg, gb = torch.autograd.grad(o, [ya, ga, ba], do)
    a2 = a.detach().requires_grad_(True)
    dz_ref = torch.autograd.grad(F.conv2d(a2, ref["w"], stride=1, padding=p), a2, do)[0] * keep.view(N, H, W, Ci).permute(0, 3, 1, 2)
    _, _, wt = filters(ref, case, dt)
    yad = d["y"].view(N, H, W, Ci).to(TDT[dt]).to(DEV).contiguous()
    tmean, trstd, tscale, tshift = (torch.empty(G * Ci, device=DEV) for _ in range(4))
    npart = lib.io_bn_partial_floats(M, Ci, G)
    part = torch.empty(npart, device=DEV)
    _lib.check(lib.io_bn_stats_finalize_dt(P(yad), M, Ci, G, P(f(ga)), P(f(ba)), None, None, MOMENTUM, EPS, P(tmean), P(trstd),
                                           P(tscale), P(tshift), P(part), npart, dt, ST()), "stats")
    tiles = M // 128
    nws2 = 2 * ((tiles + tiles // 64 + G + 2) * Ci) + 2 * G * Ci
    ws2 = Guarded((nws2,), torch.float32)
    dz, dyb = Guarded((N, H, W, Ci), TDT[dt]), Guarded((N, H, W, Ci), TDT[dt])
    dgam, dbet = torch.full((Ci,), float("nan"), device=DEV), torch.full((Ci,), float("nan"), device=DEV)
    _lib.check(lib.io_conv2d_dgrad_bnbwd_dt(P(dev(do, dt)), P(wt), dz.p(), N, H, W, Ci, Co, R, S, p, P(yad), G, P(f(ga)),
                                            P(tmean), P(trstd), P(tscale), P(tshift), P(dgam), P(dbet), dyb.p(), ws2.p(), nws2,
                                            dt, 0, ST()), "dgrad + bnbwd")
    assert dz.intact() and dyb.intact() and ws2.intact()
    assert lib.io_debug_last_nt_route() == 0
    tag = "%s dgrad_bnbwd %s G=%d" % (IDS.get(case, "n%d-1x1" % N), DTN[dt], G)
    held(tag + " dz", case, nchw(dz.t), dz_ref, 8e-3 if bf else 3e-5)
    held(tag + " dyb", case, nchw(dyb.t), gy.view(N, H, W, Ci).permute(0, 3, 1, 2), 1.5e-2 if bf else 3e-5)
    _chk(tag + " dgamma", dgam, gg, 3e-5)
    _chk(tag + " dbeta", dbet, gb, 3e-5)


# ---- io_conv2d_fwd_resid_dt with out_bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [0, 1])
@pytest.mark.parametrize("shape,dt,route", cei.RESID, ids=["fp32", "bf16-p256-declines", "bf16-p256-takes"])
def test_fwd_resid_writes_the_mask_bits_on_every_route(shape, dt, route, two):
    """after IO_OK, out_bits == [out > 0] bit for bit -- on conv_p256 (which writes them next to `out`) and on conv_nt_kernel
    (whose launcher packs them from `out`): the executor's bits_written() relies on it"""
    N, H, W, Ci, Co, G = shape
    M = N * H * W
    lib = L()
    g = torch.Generator().manual_seed(31 + Co + dt + two)
    rd = lambda t: cei.rounded(t, dt)      # noqa: E731
    y3 = rd(torch.randn(M, Ci, generator=g, dtype=torch.float64))
    sec = rd(torch.randn(M, Ci, generator=g, dtype=torch.float64))
    w = rd(torch.randn(Co, Ci, generator=g, dtype=torch.float64) / Ci ** 0.5)
    ta = (torch.rand(G, Ci, generator=g) + 0.5).double()
    tb = (torch.randn(G, Ci, generator=g) * 0.3).double()
    tc = (torch.randn(G, Ci, generator=g) * 0.3).double()
    grp = torch.arange(M) // (M // G)
    A, B_, Cc = ta[grp], tb[grp], tc[grp]
    out_ref = torch.relu((y3 - B_) * A + Cc + sec) if two == 0 else torch.relu(A * y3 + B_ * sec + Cc)
    td = TDT[dt]
    f = lambda t: t.to(td).to(DEV).contiguous()      # noqa: E731
    y = Guarded((M, Co), td)
    out = Guarded((M, Ci), td)
    bits = Guarded((M * Ci // 32,), torch.int32, fill=0x5A5A5A5A)       # a pattern: stale words show
    tabs = [t.float().contiguous().to(DEV) for t in (ta, tb, tc)]
    _lib.check(lib.io_conv2d_fwd_resid_dt(P(f(y3)), P(f(sec)), P(f(w)), y.p(), out.p(), bits.p(), N, H, W, Ci, Co, G, two,
                                          P(tabs[0]), P(tabs[1]), P(tabs[2]), None, None, dt, ST()), "fwd_resid_dt")
    assert y.intact() and out.intact() and bits.intact()
    assert lib.io_debug_last_nt_route() == route
    bar = 6e-3 if dt else 2e-5
    _chk("resid %s two=%d out" % (DTN[dt], two), out.t, out_ref, bar)
    _chk("resid %s two=%d y" % (DTN[dt], two), y.t, out.t.double().cpu() @ w.t(), bar)      # the GEMM multiplies the stored operand
    word = bits.t.cpu().numpy().view(np.uint32)
    got = ((word[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).reshape(M, Ci).astype(bool)
    want = (out.t.float().cpu() > 0).numpy()
    assert 0.2 < want.mean() < 0.8
    assert np.array_equal(got, want), "%d of %d mask bits differ from [out > 0]" % (int((got != want).sum()), want.size)
