"""The autograd layer of the MiDaS-based nets (instaorder_amd.ops.conv_bn / batch_norm, midas_net.Bottleneck,
midas_net.FeatureFusionBlock) one node and one block at a time, against plain torch in fp64 on the CPU, on every route
_ConvBn can take -- and the C entry points only that layer calls (io_conv2d_dgrad_bnbwd_dt, io_conv2d_fwd_bnstats_dt and
io_conv2d_fwd_bias_dt with the grouped window gw = 64, fp32 and bf16).

Reference and tolerance rules:
- ReLU masks come from the HIP forward.  An fp32 pre-activation that rounds to the other side of zero moves upstream
  gradients by O(1) at one element (the "knife-edge" event), so the fp64 reference evaluates every ReLU as z * mask with
  the mask read off the HIP output (out > 0; for the C-ABI cases: the sign of fma(y - mean, scale, shift) on the fp32
  tables, which is what the kernels evaluate).  With that the bounds are element-wise: relerr = max |got - ref| / max |ref|.
- bf16 references round where the HIP path stores bf16: inputs, packed filters (the folded w * scale in eval), conv
  outputs y, BatchNorm / ReLU outputs, and the stored gradients dy / dz (a rounding node whose backward rounds the
  gradient).  Statistics follow the route the case pins: the fused epilogue (io_conv2d_fwd_bnstats_dt) reduces the fp32
  accumulators, io_bn_stats_finalize_dt the stored y.  The block references (midas_oracle._bottleneck / _fusion) take
  their statistics from the stored y on every route and round a sum once, where it is next stored, rather than at the add.
- fp32 bounds: 3e-5 of the largest reference entry, nodes and blocks alike (as for
  test_gpu_ops.test_conv_dgrad_with_fused_bn_backward; the C-ABI forward checks keep that file's 2e-5 / 1e-4).  Measured
  on the MI355X: at most 1.3e-6 anywhere in this file.
- bf16 bounds: about 3x the largest distance measured on the MI355X over the cases of the test, written next to each
  bound -- but never below the fp32 bound of the same quantity (statistics, running estimates and the dgamma / dbeta of
  fp32 reductions sit at fp32 noise in bf16 too).
- Every case asserts the route it means to test (entry points counted by a spy on the loaded library), so a change of
  a route condition in ops.py cannot move a case elsewhere unnoticed.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from instaorder_amd import _lib
from test_gpu_ops import L, P, ST, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
TD = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _chk(tag, got, ref, bound):
    e = relerr(got, ref)
    print("DIST %-44s %.3e  (bound %.1e)" % (tag, e, bound))
    assert e < bound, (tag, e, bound)


def _r(t, bf):
    """the value the HIP path stores: bf16 or fp32, back in fp64"""
    return t.bfloat16().double() if bf else t.float().double()


class _Round(torch.autograd.Function):
    """a stored activation: rounded forward, and its gradient (stored in the same type) rounded backward"""

    @staticmethod
    def forward(ctx, t, bf):
        ctx.bf = bf
        return _r(t, bf)

    @staticmethod
    def backward(ctx, g):
        return _r(g, ctx.bf), None


class _RoundW(torch.autograd.Function):
    """a packed filter: rounded forward, the fp32 filter gradient passes unrounded"""

    @staticmethod
    def forward(ctx, t, bf):
        return _r(t, bf)

    @staticmethod
    def backward(ctx, g):
        return g, None


def _cpu(t):        # NHWC device tensor -> NCHW fp64 CPU
    return t.detach().float().permute(0, 3, 1, 2).double().cpu()


def _dev(t, dt):    # NCHW fp64 CPU -> NHWC device tensor of dt
    return t.detach().permute(0, 2, 3, 1).contiguous().to(dt).to(DEV)


# ---- route spy --------------------------------------------------------------------------------------------------------
SPIED = ["io_conv2d_fwd_bnstats_dt", "io_conv2d_fwd_dt", "io_gconv2d_fwd", "io_bn_stats_finalize_dt", "io_conv2d_fwd_bias_dt",
         "io_bn_bwd_dt", "io_conv2d_dgrad_dt", "io_gconv2d_dgrad", "io_conv2d_dgrad_bnbwd_dt", "io_conv2d_wgrad_dt",
         "io_gconv2d_wgrad", "io_gconv_pack"]
NT_ROUTED = ("io_conv2d_fwd_bnstats_dt", "io_conv2d_fwd_bias_dt", "io_conv2d_dgrad_bnbwd_dt")


class Spy(object):
    """counts the launches of SPIED entry points made through the cached library handle (restored by monkeypatch)"""

    def __init__(self, monkeypatch):
        lib = _lib.lib()
        self.calls = []
        for name in SPIED:
            fn = getattr(lib, name)

            def wrapped(*a, _fn=fn, _name=name):
                rc = _fn(*a)
                self.calls.append((_name, a, lib.io_debug_last_nt_route() if _name in NT_ROUTED else None))
                return rc
            monkeypatch.setattr(lib, name, wrapped)

    def n(self, name):
        return sum(1 for c in self.calls if c[0] == name)

    def gw(self, name):       # the gw argument (second to last) of every call of `name`
        return [c[1][-2] for c in self.calls if c[0] == name]

    def routes(self, name):
        return [c[2] for c in self.calls if c[0] == name]


@pytest.fixture
def spy(monkeypatch):
    return Spy(monkeypatch)


def _tables(yd, M, C, G, gamma, beta, bf):
    """forward BatchNorm tables of a stored y (what the producer's forward left for the fused backward)"""
    mean, rstd, scale, shift = (torch.empty(G * C, device=DEV) for _ in range(4))
    npart = L().io_bn_partial_floats(M, C, G)
    part = torch.empty(npart, device=DEV)
    _lib.check(L().io_bn_stats_finalize_dt(P(yd), M, C, G, P(gamma), P(beta), None, None, 0.1, EPS, P(mean), P(rstd),
                                           P(scale), P(shift), P(part), npart, 1 if bf else 0, ST()), "stats")
    return mean, rstd, scale, shift


def _kernel_mask(yd, mean, scale, shift, G):
    """relu(bn(y)) > 0 exactly as the kernels decide it: fma(y - mean, scale, shift) > 0 with y - mean in fp32 (the
    product of two floats is exact in fp64, so only the sign of the fp32 fma is reproduced)"""
    N, H, W, C = yd.shape
    yv = yd.float().view(G, N // G, H, W, C)
    mu, sc, sh = (t.view(G, 1, 1, 1, C) for t in (mean, scale, shift))
    m = ((yv - mu).double() * sc.double() + sh.double()) > 0
    return m.view(N, H, W, C).permute(0, 3, 1, 2).cpu()


def _gbn(y, gamma, beta, G, y_stat=None):
    """training BatchNorm per statistic group in fp64: normalises y with the batch statistics of y_stat (default y)"""
    y_stat = y if y_stat is None else y_stat
    per = y.shape[0] // G
    outs = []
    for g in range(G):
        sl = slice(g * per, (g + 1) * per)
        ys = y_stat[sl]
        mu = ys.mean((0, 2, 3), keepdim=True)
        var = ys.var((0, 2, 3), unbiased=False, keepdim=True)
        outs.append((y[sl] - mu) / torch.sqrt(var + EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1))
    return torch.cat(outs, 0)


def _running(y_stat, rm, rv, G, R):
    """the running estimates after G sequential module calls on the parts, or R calls on the same input (momentum 0.1,
    unbiased variance): F.batch_norm itself"""
    rm, rv = rm.clone(), rv.clone()
    per = y_stat.shape[0] // G
    for g in range(G):
        for _ in range(R):
            F.batch_norm(y_stat[g * per:(g + 1) * per].detach(), rm, rv, None, None, True, 0.1, EPS)
    return rm, rv


# ---- 1. C-ABI: the _dt / gw = 64 entries -------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("cg", [0, 8, 16, 32, 64])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dgrad_bnbwd_dt(dtype, cg, G):
    """io_conv2d_dgrad_bnbwd_dt: the consumer's data gradient with the producer's BatchNorm backward in its epilogue ==
    autograd through conv(relu(bn(y))) w.r.t. y / gamma / beta.  cg = 0: dense 1x1 (conv3 of a Bottleneck); else the
    grouped 3x3 window form (conv2 of ResNeXt) with cg input channels per group."""
    bf = dtype == "bf16"
    td = TD[dtype]
    N, H = 4, 8
    M = N * H * H
    if cg:
        Cin = Cout = 128
        k, groups = 3, 128 // cg
    else:
        Cin, Cout, k, groups = 128, 256, 1, 1
    g = torch.Generator().manual_seed(100 + cg + G)
    y = _r(torch.randn(N, Cin, H, H, generator=g, dtype=torch.float64) * 0.7 + 0.2, bf).requires_grad_(True)
    gamma = _r(1 + 0.2 * torch.randn(Cin, generator=g, dtype=torch.float64), False).requires_grad_(True)
    beta = _r(0.2 * torch.randn(Cin, generator=g, dtype=torch.float64), False).requires_grad_(True)
    w = _r(torch.randn(Cout, Cin // groups, k, k, generator=g, dtype=torch.float64) / np.sqrt(Cin // groups * k * k), bf)
    do = _r(torch.randn(N, Cout, H, H, generator=g, dtype=torch.float64), bf)
    f = lambda t: t.detach().float().to(DEV).contiguous()      # noqa: E731
    yd = _dev(y, td)
    mean, rstd, scale, shift = _tables(yd, M, Cin, G, f(gamma), f(beta), bf)
    mask = _kernel_mask(yd, mean, scale, shift, G)
    t = _gbn(y, gamma, beta, G)
    o = F.conv2d(t * mask, w, padding=k // 2, groups=groups)
    gy, gg, gb = torch.autograd.grad(o, [y, gamma, beta], do)
    a2 = (t * mask).detach().requires_grad_(True)
    dz_ref = torch.autograd.grad(F.conv2d(a2, w, padding=k // 2, groups=groups), a2, do)[0] * mask
    if cg:
        wc = torch.empty(Cin, k * k, 64, device=DEV, dtype=td)
        wt = torch.empty_like(wc)
        _lib.check(L().io_gconv_pack(P(f(w.reshape(Cout, cg, k * k))), Cin, cg, k * k, P(wc), P(wt), 1 if bf else 0, ST()),
                   "pack")
    else:
        wt = f(w).permute(0, 2, 3, 1).reshape(Cout, k * k, Cin).permute(2, 1, 0).contiguous().to(td)
    tiles = M // 128
    nws = 2 * ((tiles + tiles // 64 + G + 2) * Cin) + 2 * G * Cin
    ws = torch.empty(nws, device=DEV)
    dz = torch.full((N, H, H, Cin), float("nan"), device=DEV, dtype=td)
    dyb = torch.full_like(dz, float("nan"))
    dgam, dbet = torch.full((Cin,), float("nan"), device=DEV), torch.full((Cin,), float("nan"), device=DEV)
    _lib.check(L().io_conv2d_dgrad_bnbwd_dt(P(_dev(do, td)), P(wt), P(dz), N, H, H, Cin, Cout, k, k, k // 2, P(yd), G,
                                            P(f(gamma)), P(mean), P(rstd), P(scale), P(shift), P(dgam), P(dbet), P(dyb),
                                            P(ws), nws, 1 if bf else 0, 64 if cg else 0, ST()), "dgrad+bnbwd")
    if cg:
        assert L().io_debug_last_nt_route() == 0          # the grouped window runs on the 128-row kernel only
    tag = "dgrad_bnbwd %s cg=%d G=%d" % (dtype, cg, G)
    # bf16 measured max: dz 2.6e-3, dyb 4.9e-3, dgamma 2.5e-7, dbeta 1.9e-7 (the reductions see the unrounded dz)
    _chk(tag + " dz", _cpu(dz), dz_ref, 8e-3 if bf else 3e-5)
    _chk(tag + " dyb", _cpu(dyb), gy, 1.5e-2 if bf else 3e-5)
    _chk(tag + " dgamma", dgam, gg, 3e-5)
    _chk(tag + " dbeta", dbet, gb, 3e-5)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("stride,cg", [(1, 8), (2, 32), (1, 64)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fwd_bnstats_dt_grouped(dtype, stride, cg, G):
    """io_conv2d_fwd_bnstats_dt with gw = 64 (ResNeXt conv2 in training): the grouped convolution and the batch
    statistics of its fp32 accumulators per group, the tables, and the running estimates after one call whose momentum
    is that of two folded calls (1 - 0.9^2)."""
    bf = dtype == "bf16"
    td = TD[dtype]
    N, C = 4, 128
    H = 8 * stride
    g = torch.Generator().manual_seed(200 + stride + cg + G)
    x = _r(torch.randn(N, C, H, H, generator=g, dtype=torch.float64), bf)
    w = _r(torch.randn(C, cg, 3, 3, generator=g, dtype=torch.float64) / np.sqrt(9 * cg) + 0.3 / np.sqrt(9 * cg), bf)
    gamma = _r(torch.rand(C, generator=g, dtype=torch.float64) + 0.5, False)
    beta = _r(torch.randn(C, generator=g, dtype=torch.float64), False)
    rm0 = _r(torch.randn(C, generator=g, dtype=torch.float64) * 0.1, False)
    rv0 = _r(torch.rand(C, generator=g, dtype=torch.float64) + 0.5, False)
    ref = F.conv2d(x, w, stride=stride, padding=1, groups=C // cg)
    Ho = ref.shape[2]
    mom = 1.0 - 0.9 ** 2
    per = N // G
    rm, rv = rm0.clone(), rv0.clone()
    means, rstds = [], []
    for gi in range(G):
        yg = ref[gi * per:(gi + 1) * per]
        mu, var = yg.mean((0, 2, 3)), yg.var((0, 2, 3), unbiased=False)
        means.append(mu)
        rstds.append(1.0 / torch.sqrt(var + EPS))
        n = yg.numel() / C
        rm = (1 - mom) * rm + mom * mu
        rv = (1 - mom) * rv + mom * var * n / (n - 1)
    f = lambda t: t.float().to(DEV).contiguous()       # noqa: E731
    wc = torch.empty(C, 9, 64, device=DEV, dtype=td)
    wt = torch.empty_like(wc)
    _lib.check(L().io_gconv_pack(P(f(w.reshape(C, cg, 9))), C, cg, 9, P(wc), P(wt), 1 if bf else 0, ST()), "pack")
    y = torch.full((N, Ho, Ho, C), float("nan"), device=DEV, dtype=td)
    d_rm, d_rv = f(rm0), f(rv0)
    mean, rstd, scale, shift = (torch.full((G * C,), float("nan"), device=DEV) for _ in range(4))
    nws = L().io_conv2d_bnstats_workspace_floats(N, H, H, C, 3, 3, stride, 1, G)
    ws = torch.empty(nws, device=DEV)
    _lib.check(L().io_conv2d_fwd_bnstats_dt(P(_dev(x, td)), P(wc), P(y), N, H, H, C, C, 3, 3, stride, 1, G, P(f(gamma)),
                                            P(f(beta)), P(d_rm), P(d_rv), mom, EPS, P(mean), P(rstd), P(scale), P(shift),
                                            P(ws), nws, 1 if bf else 0, 64, ST()), "gconv+stats")
    assert L().io_debug_last_nt_route() == 0
    tag = "fwd_bnstats gw=64 %s s=%d cg=%d G=%d" % (dtype, stride, cg, G)
    # bf16 measured max: y 3.6e-3 (the output rounding); statistics 2.3e-7 (fp32 accumulators, as in fp32)
    _chk(tag + " y", _cpu(y), ref, 1.1e-2 if bf else 2e-5)
    _chk(tag + " mean", mean.view(G, C), torch.stack(means), 2e-5)
    _chk(tag + " rstd", rstd.view(G, C), torch.stack(rstds), 1e-4)
    _chk(tag + " scale", scale.view(G, C), torch.stack(rstds) * gamma, 1e-4)
    assert torch.equal(shift.view(G, C).cpu(), beta.float().expand(G, C))
    _chk(tag + " running_mean", d_rm, rm, 2e-5)
    _chk(tag + " running_var", d_rv, rv, 1e-4)


@pytest.mark.parametrize("identity,relu", [(False, False), (False, True), (True, True), (True, False)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fwd_bias_dt_grouped(dtype, identity, relu):
    """io_conv2d_fwd_bias_dt with gw = 64: eval-mode ResNeXt conv2 after folding, [relu](gconv(x, w * s) + b (+ add))."""
    bf = dtype == "bf16"
    td = TD[dtype]
    N, H, C = 2, 6, 128
    cg = 8 if relu else 64
    g = torch.Generator().manual_seed(300 + 2 * identity + relu)
    x = _r(torch.randn(N, C, H, H, generator=g, dtype=torch.float64), bf)
    w = _r(torch.randn(C, cg, 3, 3, generator=g, dtype=torch.float64) / np.sqrt(9 * cg), bf)
    bias = _r(torch.randn(C, generator=g, dtype=torch.float64) * 0.5, False)
    add = _r(torch.randn(N, C, H, H, generator=g, dtype=torch.float64), bf) if identity else None
    ref = F.conv2d(x, w, padding=1, groups=C // cg) + bias.view(1, -1, 1, 1)
    if add is not None:
        ref = ref + add
    if relu:
        ref = F.relu(ref)
    wc = torch.empty(C, 9, 64, device=DEV, dtype=td)
    wt = torch.empty_like(wc)
    _lib.check(L().io_gconv_pack(P(w.reshape(C, cg, 9).float().to(DEV).contiguous()), C, cg, 9, P(wc), P(wt), 1 if bf else 0,
                                 ST()), "pack")
    y = torch.full((N, H, H, C), float("nan"), device=DEV, dtype=td)
    _lib.check(L().io_conv2d_fwd_bias_dt(P(_dev(x, td)), P(wc), P(y), N, H, H, C, C, 3, 3, 1, 1, P(bias.float().to(DEV)),
                                         P(_dev(add, td) if add is not None else None), int(relu), 1 if bf else 0, 64, ST()),
               "gconv+bias")
    assert L().io_debug_last_nt_route() == 0
    # bf16 measured max: 3.4e-3 (the output rounding)
    _chk("fwd_bias gw=64 %s id=%d relu=%d" % (dtype, identity, relu), _cpu(y), ref, 1.1e-2 if bf else 2e-5)


# ---- 2. ops.conv_bn / ops.batch_norm through autograd, one node at a time ------------------------------------------------
MODES = [(1, 1), (2, 1), (1, 2)]          # (bn_groups, repeat)


def _node_geom(kind, fused):
    """dense: 3x3 64 -> 128; grouped: 3x3 over 128 channels, cg = 16.  fused: 8 x 8 maps, 4 samples (M = 256, M / 2 = 128:
    statistics in the epilogue); otherwise 5 x 5 (M = 100: a separate statistics pass)."""
    H = 8 if fused else 5
    if kind == "dense":
        return dict(N=4, H=H, Ci=64, Co=128, k=3, stride=1, pad=1, groups=1)
    return dict(N=4, H=H, Ci=128, Co=128, k=3, stride=1, pad=1, groups=8)


def _params(gen, Ci, Co, k, groups, bf):
    w = _r(torch.randn(Co, Ci // groups, k, k, generator=gen, dtype=torch.float64) / np.sqrt(Ci // groups * k * k), False)
    gamma = _r(1 + 0.3 * torch.randn(Co, generator=gen, dtype=torch.float64), False)
    beta = _r(0.3 * torch.randn(Co, generator=gen, dtype=torch.float64), False)
    rm = _r(0.1 * torch.randn(Co, generator=gen, dtype=torch.float64), False)
    rv = _r(torch.rand(Co, generator=gen, dtype=torch.float64) + 0.5, False)
    return w, gamma, beta, rm, rv


def _leaf(t):
    return t.float().to(DEV).requires_grad_(True)


def _ref_node(x, w, gamma, beta, stride, pad, groups, G, bf, fused, identity=None, mask=None):
    """fp64 reference of one training conv_bn node: -> (out, y_stat)"""
    y_acc = F.conv2d(x, _RoundW.apply(w, bf), stride=stride, padding=pad, groups=groups)
    y = _Round.apply(y_acc, bf)
    y_stat = y_acc if fused else y          # the fused epilogue reduces the accumulators, finalize the stored y
    z = _gbn(y, gamma, beta, G, y_stat)
    if identity is not None:
        z = z + identity
    if mask is not None:
        z = z * mask
    return _Round.apply(z, bf), y_stat


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("G,R", MODES)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", ["dense", "grouped"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conv_bn_node(dtype, kind, fused, G, R, relu, spy):
    """One training ops.conv_bn node, no producer offer: forward output, running estimates, and the gradients of x, w,
    gamma, beta (relu: also of `identity`, and x forked -- its second use's gradient rides in the data-gradient launch's
    `add` operand (dense) or is summed in Python (grouped))."""
    from instaorder_amd import ops
    bf = dtype == "bf16"
    td = TD[dtype]
    c = _node_geom(kind, fused)
    N, H, Ci, Co, k, s, pd, grp = c["N"], c["H"], c["Ci"], c["Co"], c["k"], c["stride"], c["pad"], c["groups"]
    gen = torch.Generator().manual_seed(400 + 10 * G + R + 2 * relu + fused)
    x64 = _r(torch.randn(N, Ci, H, H, generator=gen, dtype=torch.float64) + 0.1, bf)
    w64, g64, b64, rm64, rv64 = _params(gen, Ci, Co, k, grp, bf)
    Ho = (H + 2 * pd - k) // s + 1
    id64 = _r(torch.randn(N, Co, Ho, Ho, generator=gen, dtype=torch.float64), bf) if relu else None
    dout = _r(torch.randn(N, Co, Ho, Ho, generator=gen, dtype=torch.float64), bf)
    dfork = _r(torch.randn(N, Ci, H, H, generator=gen, dtype=torch.float64), bf) if relu else None
    x = _dev(x64, td).requires_grad_(True)
    w, gamma, beta = _leaf(w64), _leaf(g64), _leaf(b64)
    rm, rv = rm64.float().to(DEV), rv64.float().to(DEV)
    idt = _dev(id64, td).requires_grad_(True) if relu else None
    res = ops.conv_bn(x, w, gamma, beta, rm, rv, s, pd, grp, True, relu=relu, identity=idt, bn_groups=G, repeat=R,
                      fork=relu)
    out, alias = res if relu else (res, None)
    assert not hasattr(out, "_io_offer")              # (relu with identity: no offer)
    fwd = list(spy.calls)
    if relu:
        torch.autograd.backward([out, alias], [_dev(dout, td), _dev(dfork, td)])
    else:
        out.backward(_dev(dout, td))
    torch.cuda.synchronize()
    # routes
    nf = lambda n: sum(1 for cc in fwd if cc[0] == n)        # noqa: E731
    if fused:
        assert nf("io_conv2d_fwd_bnstats_dt") == 1 and nf("io_bn_stats_finalize_dt") == 0
        assert spy.gw("io_conv2d_fwd_bnstats_dt") == [0 if kind == "dense" else 64]
        if kind == "grouped":
            assert spy.routes("io_conv2d_fwd_bnstats_dt") == [0]
    else:
        assert nf("io_conv2d_fwd_bnstats_dt") == 0 and nf("io_bn_stats_finalize_dt") == 1
        assert nf("io_conv2d_fwd_dt" if kind == "dense" else "io_gconv2d_fwd") == 1
    assert spy.n("io_bn_bwd_dt") == 1 and spy.n("io_conv2d_dgrad_bnbwd_dt") == 0
    if kind == "dense":
        dg = [cc[1] for cc in spy.calls if cc[0] == "io_conv2d_dgrad_dt"]
        assert len(dg) == 1 and spy.n("io_gconv2d_dgrad") == 0
        assert (dg[0][3] is not None) == relu          # the forked gradient as the `add` operand
    else:
        assert spy.n("io_gconv2d_dgrad") == 1 and spy.n("io_conv2d_dgrad_dt") == 0
    # reference
    xr = x64.clone().requires_grad_(True)
    wr, gr, br = (t.clone().requires_grad_(True) for t in (w64, g64, b64))
    ir = id64.clone().requires_grad_(True) if relu else None
    mask = (_cpu(out) > 0) if relu else None
    ref, y_stat = _ref_node(xr, wr, gr, br, s, pd, grp, G, bf, fused, ir, mask)
    rm_ref, rv_ref = _running(y_stat, rm64, rv64, G, R)
    ref.backward(dout)
    gx_ref = xr.grad + dfork if relu else xr.grad
    tag = "node %s %s %s G=%d R=%d relu=%d" % (dtype, kind, "fused" if fused else "unfused", G, R, relu)
    # bf16 measured max: out 2.4e-3, running mean / var 6.6e-5 / 4.3e-5, dx 5.5e-3, dw 2.8e-3, dgamma 4.5e-4,
    # dbeta 3.9e-8, didentity 0 (exact)
    _chk(tag + " out", _cpu(out), ref, 8e-3 if bf else 3e-5)
    _chk(tag + " running_mean", rm, rm_ref, 2e-4 if bf else 3e-5)
    _chk(tag + " running_var", rv, rv_ref, 1.3e-4 if bf else 3e-5)
    _chk(tag + " dx", _cpu(x.grad), gx_ref, 1.7e-2 if bf else 3e-5)
    _chk(tag + " dw", w.grad, wr.grad, 9e-3 if bf else 3e-5)
    _chk(tag + " dgamma", gamma.grad, gr.grad, 1.4e-3 if bf else 3e-5)
    _chk(tag + " dbeta", beta.grad, br.grad, 3e-5)
    if relu:
        _chk(tag + " didentity", _cpu(idt.grad), ir.grad, 1e-6)


@pytest.mark.parametrize("G,R", MODES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("kind", ["dense", "grouped"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conv_bn_sole_chain(dtype, kind, stride, G, R, spy):
    """producer conv_bn(relu) -> consumer conv_bn(sole=True).  Stride 1: the producer's BatchNorm backward runs in the
    consumer's data-gradient launch (io_conv2d_dgrad_bnbwd_dt, gw = 0 / 64) and the producer's own backward skips
    io_bn_bwd_dt; stride 2: the offer is refused and both nodes take the plain backward."""
    from instaorder_amd import ops
    bf = dtype == "bf16"
    td = TD[dtype]
    N, H, Ci, C = 4, 8, 64, 128
    grp = 1 if kind == "dense" else 8
    gen = torch.Generator().manual_seed(500 + 10 * G + R + stride)
    x64 = _r(torch.randn(N, Ci, H, H, generator=gen, dtype=torch.float64), bf)
    pw, pg, pb, prm, prv = _params(gen, Ci, C, 1, 1, bf)
    cw, cgm, cb, crm, crv = _params(gen, C, C, 3, grp, bf)
    Ho = (H + 2 - 3) // stride + 1
    dout = _r(torch.randn(N, C, Ho, Ho, generator=gen, dtype=torch.float64), bf)
    x = _dev(x64, td).requires_grad_(True)
    leaves = [_leaf(t) for t in (pw, pg, pb, cw, cgm, cb)]
    stats = [t.float().to(DEV) for t in (prm, prv, crm, crv)]
    a = ops.conv_bn(x, leaves[0], leaves[1], leaves[2], stats[0], stats[1], 1, 0, 1, True, relu=True, bn_groups=G, repeat=R)
    assert getattr(a, "_io_offer", None) is not None
    out = ops.conv_bn(a, leaves[3], leaves[4], leaves[5], stats[2], stats[3], stride, 1, grp, True, relu=True,
                      bn_groups=G, repeat=R, sole=True)
    out.backward(_dev(dout, td))
    torch.cuda.synchronize()
    if stride == 1:
        assert spy.n("io_conv2d_dgrad_bnbwd_dt") == 1 and spy.gw("io_conv2d_dgrad_bnbwd_dt") == [0 if kind == "dense" else 64]
        if kind == "grouped":
            assert spy.routes("io_conv2d_dgrad_bnbwd_dt") == [0]
        assert spy.n("io_bn_bwd_dt") == 1                 # the consumer's own; the producer's ran in the fused launch
        assert spy.n("io_gconv2d_dgrad") == 0 and spy.n("io_conv2d_dgrad_dt") == 1
    else:
        assert spy.n("io_conv2d_dgrad_bnbwd_dt") == 0 and spy.n("io_bn_bwd_dt") == 2
        assert spy.n("io_conv2d_dgrad_dt") == (2 if kind == "dense" else 1)
        assert spy.n("io_gconv2d_dgrad") == (0 if kind == "dense" else 1)
    # reference chain, both masks from the HIP forward
    xr = x64.clone().requires_grad_(True)
    refs = [t.clone().requires_grad_(True) for t in (pw, pg, pb, cw, cgm, cb)]
    ar, ys_a = _ref_node(xr, refs[0], refs[1], refs[2], 1, 0, 1, G, bf, True, mask=_cpu(a) > 0)
    o_ref, ys_o = _ref_node(ar, refs[3], refs[4], refs[5], stride, 1, grp, G, bf, stride == 1, mask=_cpu(out) > 0)
    o_ref.backward(dout)
    tag = "sole %s %s s=%d G=%d R=%d" % (dtype, kind, stride, G, R)
    # bf16 measured max: out 2.8e-3, dx 5.3e-3; producer dw 4.2e-3, dgamma 4.7e-3, dbeta 4.6e-3 (the fused reductions
    # see the unrounded dz, the reference the stored one: test_dgrad_bnbwd_dt pins them tightly); consumer dw 3.4e-3,
    # dgamma 7.0e-5, dbeta 2.3e-8; running estimates 1.1e-5 (consumer mean), else at most 2.2e-6
    bounds = {"producer dw": 1.3e-2, "producer dgamma": 1.5e-2, "producer dbeta": 1.4e-2, "consumer dw": 1.1e-2,
              "consumer dgamma": 2.1e-4, "consumer dbeta": 3e-5}
    _chk(tag + " out", _cpu(out), o_ref, 9e-3 if bf else 3e-5)
    _chk(tag + " dx", _cpu(x.grad), xr.grad, 1.6e-2 if bf else 3e-5)
    names = ["producer dw", "producer dgamma", "producer dbeta", "consumer dw", "consumer dgamma", "consumer dbeta"]
    for nm, got, rr in zip(names, leaves, refs):
        _chk(tag + " " + nm, got.grad, rr.grad, bounds[nm] if bf else 3e-5)
    for nm, got, (ys, r0, v0) in (("producer", stats[:2], (ys_a, prm, prv)), ("consumer", stats[2:], (ys_o, crm, crv))):
        rm_ref, rv_ref = _running(ys, r0, v0, G, R)
        _chk(tag + " %s running_mean" % nm, got[0], rm_ref, 3.3e-5 if bf else 3e-5)
        _chk(tag + " %s running_var" % nm, got[1], rv_ref, 3e-5)


@pytest.mark.parametrize("identity,relu", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("kind", ["dense", "grouped"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conv_bn_eval_folded(dtype, kind, identity, relu, spy):
    """eval conv_bn: the BatchNorm folded into the filters and a bias (io_conv2d_fwd_bias_dt, gw = 0 / 64); a second call
    takes the folded operands from the `_io_folded` cache and gives the identical output."""
    from instaorder_amd import ops
    bf = dtype == "bf16"
    td = TD[dtype]
    c = _node_geom(kind, False)
    N, H, Ci, Co, k, grp = c["N"], c["H"], c["Ci"], c["Co"], c["k"], c["groups"]
    gen = torch.Generator().manual_seed(600 + 2 * identity + relu)
    x64 = _r(torch.randn(N, Ci, H, H, generator=gen, dtype=torch.float64), bf)
    w64, g64, b64, rm64, rv64 = _params(gen, Ci, Co, k, grp, bf)
    id64 = _r(torch.randn(N, Co, H, H, generator=gen, dtype=torch.float64), bf) if identity else None
    x = _dev(x64, td)
    w, gamma, beta = (nn.Parameter(t.float().to(DEV)) for t in (w64, g64, b64))
    rm, rv = rm64.float().to(DEV), rv64.float().to(DEV)
    idt = _dev(id64, td) if identity else None
    with torch.no_grad():
        out1 = ops.conv_bn(x, w, gamma, beta, rm, rv, 1, 1, grp, False, relu=relu, identity=idt)
        folded = w._io_folded[1]
        out2 = ops.conv_bn(x, w, gamma, beta, rm, rv, 1, 1, grp, False, relu=relu, identity=idt)
    torch.cuda.synchronize()
    assert w._io_folded[1] is folded and torch.equal(out1, out2)
    assert spy.n("io_conv2d_fwd_bias_dt") == 2 and spy.gw("io_conv2d_fwd_bias_dt") == [0 if kind == "dense" else 64] * 2
    assert spy.n("io_gconv_pack") == (0 if kind == "dense" else 1)
    if kind == "grouped":
        assert spy.routes("io_conv2d_fwd_bias_dt") == [0, 0]
    assert torch.equal(rm.cpu(), rm64.float()) and torch.equal(rv.cpu(), rv64.float())
    fscale = (g64.float() / torch.sqrt(rv64.float() + EPS))            # fp32, as ops folds it
    fbias = (b64.float() - rm64.float() * fscale).double()
    wf = _r((w64.float() * fscale.view(-1, 1, 1, 1)).double(), bf)
    ref = F.conv2d(x64, wf, padding=1, groups=grp) + fbias.view(1, -1, 1, 1)
    if identity:
        ref = ref + id64
    if relu:
        ref = F.relu(ref)
    # against the unfolded BatchNorm too (fp32: the fold is exact to rounding)
    ref_bn = F.batch_norm(F.conv2d(x64, w64, padding=1, groups=grp), rm64, rv64, g64, b64, False, 0.1, EPS)
    if identity:
        ref_bn = ref_bn + id64
    if relu:
        ref_bn = F.relu(ref_bn)
    tag = "eval %s %s id=%d relu=%d" % (dtype, kind, identity, relu)
    # bf16 measured max: 2.7e-3 against the folded reference, 3.3e-3 against the unfolded BatchNorm
    _chk(tag + " out", _cpu(out1), ref, 9e-3 if bf else 3e-5)
    _chk(tag + " out vs unfolded", _cpu(out1), ref_bn, 1.1e-2 if bf else 3e-5)


@pytest.mark.parametrize("G,R", MODES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_batch_norm_node(dtype, G, R):
    """ops.batch_norm (training, + identity + ReLU): output, running estimates and gradients under bn_groups / repeat."""
    from instaorder_amd import ops
    bf = dtype == "bf16"
    td = TD[dtype]
    N, H, C = 4, 6, 128
    gen = torch.Generator().manual_seed(700 + 10 * G + R)
    y64 = _r(torch.randn(N, C, H, H, generator=gen, dtype=torch.float64) * 0.6 + 0.3, bf)
    _, g64, b64, rm64, rv64 = _params(gen, C, C, 1, 1, bf)
    id64 = _r(torch.randn(N, C, H, H, generator=gen, dtype=torch.float64), bf)
    dout = _r(torch.randn(N, C, H, H, generator=gen, dtype=torch.float64), bf)
    y = _dev(y64, td).requires_grad_(True)
    gamma, beta = _leaf(g64), _leaf(b64)
    rm, rv = rm64.float().to(DEV), rv64.float().to(DEV)
    idt = _dev(id64, td).requires_grad_(True)
    out = ops.batch_norm(y, gamma, beta, rm, rv, True, relu=True, identity=idt, groups=G, repeat=R)
    out.backward(_dev(dout, td))
    torch.cuda.synchronize()
    yr, gr, br, ir = (t.clone().requires_grad_(True) for t in (y64, g64, b64, id64))
    ref = _Round.apply((_gbn(yr, gr, br, G) + ir) * (_cpu(out) > 0), bf)
    ref.backward(dout)
    rm_ref, rv_ref = _running(y64, rm64, rv64, G, R)
    tag = "batch_norm %s G=%d R=%d" % (dtype, G, R)
    # bf16 measured max: out 9.4e-6 (the reference rounds the same value), dy 3.5e-3, dgamma 1.2e-7, dbeta 0,
    # running estimates 1.3e-7
    _chk(tag + " out", _cpu(out), ref, 3e-5)
    _chk(tag + " running_mean", rm, rm_ref, 3e-5)
    _chk(tag + " running_var", rv, rv_ref, 3e-5)
    _chk(tag + " dy", _cpu(y.grad), yr.grad, 1.1e-2 if bf else 3e-5)
    _chk(tag + " dgamma", gamma.grad, gr.grad, 3e-5)
    _chk(tag + " dbeta", beta.grad, br.grad, 3e-5)
    _chk(tag + " didentity", _cpu(idt.grad), ir.grad, 1e-6)


def test_plan_with_vectors_but_no_filters_clears_the_flat_buffer(monkeypatch):
    """An ops.WeightPlan that holds directly written BatchNorm gradients and NO filter (a module of BatchNorm layers alone):
    its prepare() still clears the flat gradient buffer, and only because it did are gather_grads told ``prezeroed`` -- a
    parameter no loss reaches delivers zero, not what the buffer held before; dgamma / dbeta are the values the autograd +
    gather route (IO_DEPTH_DIRECT_GRADS=0) delivers, bit for bit (the same kernel writing to another destination)."""
    from instaorder_amd import midas_net, ops, optim
    N, H, C = 4, 6, 128
    gen = torch.Generator().manual_seed(731)
    x = _dev(torch.randn(N, C, H, H, generator=gen, dtype=torch.float64) * 0.6 + 0.3, torch.float32)
    dout = _dev(torch.randn(N, C, H, H, generator=gen, dtype=torch.float64), torch.float32)
    g64, b64 = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5, torch.randn(C, generator=gen, dtype=torch.float64)

    def step(mod, opt, plan, record):
        for p in opt._params:
            p.grad = None
        built = []
        with ops.WeightPlan.step(plan, opt if record else None, torch.float32, built.append):
            mod.bn(x).backward(dout)
            opt.gather_grads(**ops.WeightPlan.gather_args())
            if plan is not None:
                plan.unpack_grads()
        return built[0] if record else None

    res = {}
    for direct in ("1", "0"):
        monkeypatch.setenv("IO_DEPTH_DIRECT_GRADS", direct)
        mod = nn.Module()
        mod.bn, mod.unused = midas_net.BatchNorm2d(C), nn.Parameter(torch.ones(70))
        with torch.no_grad():
            mod.bn.weight.copy_(g64)
            mod.bn.bias.copy_(b64)
        mod.to(DEV).train()
        opt = optim.FlatSGD(mod, lr=0.1)
        plan = step(mod, opt, None, True)
        assert plan and plan.n == 0 and len(plan.vecs) == (2 if direct == "1" else 0)
        opt.flat_grads.fill_(7.0)                  # the unused parameter's slice and both BatchNorm slices
        step(mod, opt, plan, False)
        torch.cuda.synchronize()
        res[direct] = [opt.flat_grads[opt.offset_of(p):][:p.numel()].clone() for p in (mod.unused, mod.bn.weight, mod.bn.bias)]
        assert not plan.cleared                    # (the answer of prepare() does not outlive the step's bracket)
    assert torch.equal(res["1"][0], torch.zeros(70, device=DEV)), res["1"][0][:4]
    assert float(res["0"][1].abs().max()) > 0 and float(res["0"][2].abs().max()) > 0
    assert torch.equal(res["1"][1], res["0"][1]) and torch.equal(res["1"][2], res["0"][2])


# ---- 3. midas_net.Bottleneck and FeatureFusionBlock as modules ------------------------------------------------------------
class _RefF(object):
    """torch.nn.functional for midas_oracle, with the HIP forward's ReLU masks (in call order) and rounding to the stored
    type where the HIP path stores: conv outputs, BatchNorm / ReLU outputs, the upsampled map"""

    def __init__(self, masks, bf):
        self.masks, self.bf, self.i, self.sl = masks, bf, 0, slice(None)

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, z):
        m = self.masks[self.i]
        self.i += 1
        return _Round.apply(z * m[self.sl], self.bf)

    def conv2d(self, x, w, b=None, **kw):
        y = _Round.apply(F.conv2d(x, _RoundW.apply(w, self.bf), **kw), self.bf)
        return y if b is None else _Round.apply(y + b.view(1, -1, 1, 1), self.bf)

    def batch_norm(self, *a, **kw):
        return _Round.apply(F.batch_norm(*a, **kw), self.bf)

    def interpolate(self, *a, **kw):
        return _Round.apply(F.interpolate(*a, **kw), self.bf)


def _record_outputs(monkeypatch, mod, names):
    """record what every call of mod.<name> returns (in call order), calling through"""
    rec = []
    for name in names:
        fn = getattr(mod, name)

        def wrapped(*a, _fn=fn, _name=name, **kw):
            r = _fn(*a, **kw)
            rec.append((_name, a, kw, r[0] if isinstance(r, tuple) else r))
            return r
        monkeypatch.setattr(mod, name, wrapped)
    return rec


BLOCKS = {
    # name: (inplanes, planes, stride, groups, base_width, downsample, N, H)
    "layer1": (64, 64, 1, 32, 8, True, 4, 16),          # 64 -> 256 wide, cg = 8, every node fused
    "layer2_first": (128, 64, 2, 16, 16, True, 4, 16),  # stride 2, cg = 16: conv2 refuses the offer, conv3 takes it
    "layer4": (256, 64, 2, 4, 64, True, 4, 6),          # cg = 64 on 6x6 -> 3x3 maps: every node on the unfused routes
    "order_branch": (256, 64, 1, 1, 64, False, 4, 8),   # dense: conv2 and conv3 both fuse the BatchNorm before them
}
FUSED_DGRADS = {"layer1": [0, 64], "layer2_first": [0], "layer4": [], "order_branch": [0, 0]}


def _seed_module(m, gen):
    for name, p in sorted(m.named_parameters()):
        if name.endswith("weight") and p.dim() == 4:
            fan = p[0].numel()
            p.data.copy_(torch.randn(p.shape, generator=gen) / np.sqrt(fan))
        elif name.endswith("weight"):
            p.data.copy_(1 + 0.3 * torch.randn(p.shape, generator=gen))
        else:
            p.data.copy_(0.3 * torch.randn(p.shape, generator=gen))
    for name, b in sorted(m.named_buffers()):
        if name.endswith("running_mean"):
            b.copy_(0.1 * torch.randn(b.shape, generator=gen))
        elif name.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=gen) + 0.5)


def _oracle_state(m, prefix):
    st = {}
    for k, v in m.state_dict().items():
        t = v.detach().cpu()
        if t.is_floating_point():
            t = t.double().clone()
            if k.rsplit(".", 1)[-1] in ("weight", "bias"):
                t.requires_grad_(True)
        st[prefix + k] = t
    return st


@pytest.mark.parametrize("fork", [True, False])
@pytest.mark.parametrize("mode", ["groups2", "repeat2"])
@pytest.mark.parametrize("block", sorted(BLOCKS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bottleneck_module(dtype, block, mode, fork, monkeypatch, spy):
    """midas_net.Bottleneck in training mode under _BnMode(groups=2) (the two mask orders: two sequential reference calls
    on the halves) and _BnMode(repeat=2) (the shared encoder: two reference calls on the same input) against
    midas_oracle._bottleneck in fp64: output, gradients of every parameter and of the input, all running estimates,
    num_batches_tracked; midas_net._FORK on and off."""
    from instaorder_amd import midas_net, ops
    from oracle import midas_oracle
    bf = dtype == "bf16"
    td = TD[dtype]
    inp, planes, stride, groups, bw, ds, N, H = BLOCKS[block]
    monkeypatch.setattr(midas_net, "_FORK", fork)
    gen = torch.Generator().manual_seed(800 + len(block) + 3 * stride)
    downsample = nn.Sequential(midas_net.Conv2d(inp, planes * 4, 1, stride), midas_net.BatchNorm2d(planes * 4)) if ds else None
    blk = midas_net.Bottleneck(inp, planes, stride, downsample, groups, bw)
    _seed_module(blk, gen)
    st = _oracle_state(blk, "blk.")
    blk = blk.to(DEV).train()
    x64 = _r(torch.randn(N, inp, H, H, generator=gen, dtype=torch.float64) + 0.2, bf)
    Ho = (H - 1) // stride + 1
    dout = _r(torch.randn(N, planes * 4, Ho, Ho, generator=gen, dtype=torch.float64), bf)
    x = _dev(x64, td).requires_grad_(True)
    rec = _record_outputs(monkeypatch, ops, ["conv_bn"])
    G, R = (2, 1) if mode == "groups2" else (1, 2)
    with midas_net._BnMode(groups=G, repeat=R):
        out = blk(x)
    out.backward(_dev(dout, td))
    torch.cuda.synchronize()
    assert spy.gw("io_conv2d_dgrad_bnbwd_dt") == FUSED_DGRADS[block]
    if block == "layer4":
        assert spy.n("io_conv2d_fwd_bnstats_dt") == 0
    elif block == "layer1":
        assert spy.n("io_conv2d_fwd_bnstats_dt") == 4 and spy.n("io_bn_stats_finalize_dt") == 0
    assert spy.n("io_bn_bwd_dt") == 4 - len(FUSED_DGRADS[block]) - (0 if ds else 1)
    masks = [_cpu(r) > 0 for (_, a, kw, r) in rec if a[10]]          # conv_bn's `relu` (BatchNorm2d.after passes it 11th)
    assert len(masks) == 3
    # reference: the oracle's own block with the HIP masks
    refF = _RefF(masks, bf)
    monkeypatch.setattr(midas_oracle, "F", refF)
    xr = x64.clone().requires_grad_(True)
    if G == 2:
        outs = []
        for h in range(2):
            refF.i, refF.sl = 0, slice(h * N // 2, (h + 1) * N // 2)
            outs.append(midas_oracle._bottleneck(st, "blk", xr[refF.sl], stride, groups, True))
        ref = torch.cat(outs, 0)
    else:
        ref = midas_oracle._bottleneck(st, "blk", xr, stride, groups, True)
        refF.i = 0
        with torch.no_grad():             # the second of the R identical calls: running estimates only
            midas_oracle._bottleneck(st, "blk", xr, stride, groups, True)
    ref.backward(dout)
    tag = "bottleneck %s %s %s fork=%d" % (dtype, block, mode, fork)
    # bf16 measured max: out 8.7e-3, dx 6.3e-3, parameter gradients 5.8e-3, running mean / var 3.2e-4 / 1.7e-4 (the
    # fused routes reduce the unrounded y, the oracle the stored one)
    _chk(tag + " out", _cpu(out), ref, 2.6e-2 if bf else 3e-5)
    _chk(tag + " dx", _cpu(x.grad), xr.grad, 1.9e-2 if bf else 3e-5)
    for name, p in blk.named_parameters():
        _chk(tag + " d" + name, p.grad, st["blk." + name].grad, 1.8e-2 if bf else 3e-5)
    for name, b in blk.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == 2, name
        else:
            _chk(tag + " " + name, b, st["blk." + name], (1e-3 if "mean" in name else 5.1e-4) if bf else 3e-5)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fusion_block_and_head(dtype, monkeypatch):
    """midas_net.FeatureFusionBlock with two inputs, then the output head of _InstaDepthBase._decode (conv 3x3 + bias,
    upsample2x(align_corners=False), the 128 -> 32 conv stored as 64 channels with bias_act on the padded channels,
    head1 + ReLU) against midas_oracle._fusion and the head lines of midas_oracle.forward in fp64."""
    from instaorder_amd import midas_net, ops
    from oracle import midas_oracle
    bf = dtype == "bf16"
    td = TD[dtype]
    feats, N, H = 64, 2, 6
    gen = torch.Generator().manual_seed(900)
    fb = midas_net.FeatureFusionBlock(feats)
    oc = nn.Sequential(midas_net.Conv2d(feats, 128, 3, 1, 1, bias=True), midas_net._Fn(lambda t: t),
                       midas_net.Conv2d(128, 32, 3, 1, 1, bias=True, co_pad=True), midas_net._Fn(lambda t: t),
                       midas_net.Conv2d(32, 1, 1, 1, 0, bias=True))
    _seed_module(fb, gen)
    _seed_module(oc, gen)
    st = _oracle_state(fb, "rf.")
    st.update(_oracle_state(oc, "scratch.output_conv."))
    fb, oc = fb.to(DEV).train(), oc.to(DEV).train()
    x0 = _r(torch.randn(N, feats, H, H, generator=gen, dtype=torch.float64), bf)
    x1 = _r(torch.randn(N, feats, H, H, generator=gen, dtype=torch.float64), bf)
    dd = torch.randn(N, 4 * H, 4 * H, generator=gen, dtype=torch.float64).float().double()
    xa, xb = _dev(x0, td).requires_grad_(True), _dev(x1, td).requires_grad_(True)
    rec = _record_outputs(monkeypatch, ops, ["relu", "bias_act", "head1"])
    p1 = fb(xa, xb)
    y = oc[0](p1)
    y = ops.upsample2x(y, False)
    y = oc[2](y, relu=True)
    disp = ops.head1(y, oc[4].weight, oc[4].bias, True)
    assert y.shape[-1] == 64 and float(y[..., 32:].abs().max()) == 0.0      # padded channels stay exactly zero
    disp.backward(dd.float().to(DEV))
    torch.cuda.synchronize()
    masks = []
    for name, a, kw, r in rec:
        if name == "relu" or (name == "bias_act" and a[2]):
            c = a[1].numel() if name == "bias_act" else r.shape[-1]         # (the padded channels carry no bias)
            masks.append(_cpu(r)[:, :c] > 0)
        elif name == "head1":
            masks.append((r.detach().double().cpu() > 0).unsqueeze(1))
    assert len(masks) == 6
    refF = _RefF(masks, bf)
    monkeypatch.setattr(midas_oracle, "F", refF)
    r0, r1 = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
    pr = midas_oracle._fusion(st, "rf", r0, r1)
    # the head lines of midas_oracle.forward
    yr = refF.conv2d(pr, st["scratch.output_conv.0.weight"], st["scratch.output_conv.0.bias"], padding=1)
    yr = refF.interpolate(yr, scale_factor=2, mode="bilinear", align_corners=False)
    yr = refF.relu(refF.conv2d(yr, st["scratch.output_conv.2.weight"], st["scratch.output_conv.2.bias"], padding=1))
    yr = F.conv2d(yr, st["scratch.output_conv.4.weight"], st["scratch.output_conv.4.bias"])
    dr = torch.squeeze(yr * masks[5], dim=1)          # head1's ReLU (its output stays fp32)
    dr.backward(dd)
    tag = "fusion+head %s" % dtype
    # bf16 measured max: path1 8.7e-3, disp 1.15e-2, input gradients 5.5e-3, parameter gradients 3.4e-3
    _chk(tag + " path1", _cpu(p1), pr, 2.7e-2 if bf else 3e-5)
    _chk(tag + " disp", disp, dr, 3.5e-2 if bf else 3e-5)
    _chk(tag + " dx0", _cpu(xa.grad), r0.grad, 1.7e-2 if bf else 3e-5)
    _chk(tag + " dx1", _cpu(xb.grad), r1.grad, 1.7e-2 if bf else 3e-5)
    for name, p in list(fb.named_parameters()):
        _chk(tag + " d" + name, p.grad, st["rf." + name].grad, 1.1e-2 if bf else 3e-5)
    for name, p in list(oc.named_parameters()):
        _chk(tag + " doutput_conv." + name, p.grad, st["scratch.output_conv." + name].grad, 1.1e-2 if bf else 3e-5)
