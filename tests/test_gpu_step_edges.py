"""The operators every training step of both branches runs -- csrc/bn.hip and the pooling, head, loss, packing and SGD
parts of csrc/misc.hip -- on the launcher arms and block geometries the older op tests (round channel counts, full blocks,
one-trip loops) never reach.  Each case's id or comment names the condition that routes it to its kernel form.

Every reference is plain torch in fp64 on the CPU (tests/step_edge_inputs.py holds the by-hand ones that stand in where
torch refuses the shape); for bf16 it is built from bf16-rounded inputs.  Every output buffer is NaN-filled and GUARD
elements longer than the kernel is told, every workspace is exactly the size its query returns plus such a tail; the tail
must come back untouched.  No comparison leaves elements out: the BatchNorm inputs keep every pre-activation off zero
(tests/test_step_edges_cpu.py), so the ReLU mask of the kernel and of the reference cannot differ by rounding.

Bars (the ones the project applies to these kernels): fp32 BatchNorm tables / output / running estimates 1e-5, fp32 dy /
dgamma / dbeta 2e-5 (at |mean| = 1000 sigma: output 2e-3, dy / dgamma 1e-3), fp32 dz 1e-6, tensors stored as bf16 6e-3 (one
output rounding), fp32-accumulated sums of bf16 data 2e-5, pooled values 1e-6, logits / dw / db 1e-5.
"""
import pytest
import torch
import torch.nn.functional as F

import step_edge_inputs as sei
from instaorder_amd import _lib, engine
from test_gpu_ext_edges import DTN, GUARD, TDT, bits, guarded, put, tail_untouched
from test_gpu_ops import L, P, ST, _ref_losses, relerr  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(name, got, ref, bar):
    """relerr(got, ref) < bar, the figure printed first (pytest shows it when the assertion fails, -s always)"""
    e = relerr(got, ref)
    print("%-28s %.3e (bar %.1e)" % (name, e, bar))
    assert e < bar, (name, e, bar)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f32(t):
    return t.detach().float().to(DEV).contiguous()


def bn_params(shapes, with_shifted=True):
    out = [pytest.param(Mg, G, Cc, dt, False, id="%s-%s" % (DTN[dt], name)) for Mg, G, Cc, dts, name in shapes for dt in dts]
    if with_shifted:
        out.append(pytest.param(*sei.SHIFTED, 0, True, id="fp32-mg100-c1024-mean-1000-sigma"))
    return out


# =====================================================================================================================
# 1. BatchNorm forward: io_bn_stats_finalize_dt (bn_stats_kernel + bn_finalize_kernel), io_bn_eval_prepare, io_bn_apply_dt
# =====================================================================================================================
def _stats(d, M, Cc, G, dt, running):
    """-> dict of the guarded device buffers io_bn_stats_finalize_dt filled (running: with the running estimates)"""
    t = dict(y=put(d["y"], dt), npart=int(L().io_bn_partial_floats(M, Cc, G)))
    t["part"] = guarded(t["npart"])
    for k in ("mean", "rstd", "scale", "shift"):
        t[k] = guarded(G * Cc)
    t["gamma"], t["beta"] = f32(d["gamma"]), f32(d["beta"])
    if running:
        t["rm"], t["rv"] = guarded(Cc), guarded(Cc)
        t["rm"][:Cc], t["rv"][:Cc] = f32(d["rm0"]), f32(d["rv0"])
    _lib.check(L().io_bn_stats_finalize_dt(P(t["y"]), M, Cc, G, P(t["gamma"]), P(t["beta"]), P(t.get("rm")), P(t.get("rv")),
                                           sei.MOMENTUM, sei.EPS, P(t["mean"]), P(t["rstd"]), P(t["scale"]), P(t["shift"]),
                                           P(t["part"]), t["npart"], dt, ST()), "bn_stats")
    for k in ("mean", "rstd", "scale", "shift"):
        assert tail_untouched(t[k], G * Cc), k
    assert tail_untouched(t["part"], t["npart"])
    return t


@pytest.mark.parametrize("Mg,G,Cc,dt,shifted", bn_params(sei.BN_SHAPES))
def test_bn_statistics(Mg, G, Cc, dt, shifted):
    d = sei.bn_inputs(Mg, G, Cc, dt, shifted)
    M = G * Mg
    ref = sei.bn_forward_ref(d["y"], G, d["gamma"], d["beta"], d["rm0"], d["rv0"])
    t = _stats(d, M, Cc, G, dt, True)
    bar = 2e-5 if dt else 1e-5
    for k in ("mean", "rstd", "scale"):
        close(k, t[k][:G * Cc].view(G, Cc), ref[k], bar)
        assert bool(torch.isfinite(t[k][:G * Cc]).all())
    assert torch.equal(t["shift"][:G * Cc].view(G, Cc).cpu(), d["beta"].float().expand(G, Cc))
    assert tail_untouched(t["rm"], Cc) and tail_untouched(t["rv"], Cc)
    close("running_mean", t["rm"][:Cc], ref["rm"], bar)
    close("running_var", t["rv"][:Cc], ref["rv"], bar)
    # without the running estimates: the same tables, bit for bit
    u = _stats(d, M, Cc, G, dt, False)
    for k in ("mean", "rstd", "scale", "shift"):
        assert same_bits(t[k], u[k]), k


@pytest.mark.parametrize("Mg,G,Cc,dt,shifted", bn_params(sei.BN_SHAPES + sei.APPLY_ONLY_SHAPES))
def test_bn_apply_modes(Mg, G, Cc, dt, shifted):
    """plain, + identity, + second BatchNorm, each with and without ReLU; on the G > 1 rows also per_group_tables = 0 with
    the eval tables of io_bn_eval_prepare (one table set for every group)"""
    d = sei.bn_inputs(Mg, G, Cc, dt, shifted)
    M = G * Mg
    ref = sei.bn_forward_ref(d["y"], G, d["gamma"], d["beta"])
    t = _stats(d, M, Cc, G, dt, False)
    idt, yd = put(d["idt"], dt), put(d["yd"], dt)
    grp = torch.arange(M) // Mg
    bar = 6e-3 if dt else (2e-3 if shifted else 1e-5)         # (shifted: y itself is only 24-bit at 300)
    for per_group in ((1, 0) if G > 1 else (1,)):
        if per_group:
            tabs = [t["mean"], t["scale"], t["shift"]]
            tabs2 = [f32(d[k]) for k in ("mean2", "scale2", "shift2")]
            base = ref["pre"]
            second = (d["yd"] - d["mean2"][grp]) * d["scale2"][grp] + d["shift2"][grp]
        else:
            tabs = [guarded(Cc) for _ in range(3)]
            _lib.check(L().io_bn_eval_prepare(Cc, P(t["gamma"]), P(t["beta"]), P(f32(d["rm0"])), P(f32(d["rv0"])), sei.EPS,
                                              P(tabs[0]), P(tabs[1]), P(tabs[2]), ST()), "bn_eval_prepare")
            assert all(tail_untouched(b, Cc) for b in tabs)
            tabs2 = [f32(d[k][0]) for k in ("mean2", "scale2", "shift2")]
            base = (d["y"] - d["rm0"]) * d["gamma"] / torch.sqrt(d["rv0"] + sei.EPS) + d["beta"]
            second = (d["yd"] - d["mean2"][0]) * d["scale2"][0] + d["shift2"][0]
        for mode in (0, 1, 2):
            for relu in (0, 1):
                want = base + (d["idt"] if mode == 1 else second if mode == 2 else 0.0)
                want = F.relu(want) if relu else want
                out = guarded(M * Cc, TDT[dt])
                _lib.check(L().io_bn_apply_dt(P(t["y"]), M, Cc, G, per_group, P(tabs[0]), P(tabs[1]), P(tabs[2]),
                                              P(idt) if mode == 1 else P(yd) if mode == 2 else None,
                                              P(tabs2[0]) if mode == 2 else None, P(tabs2[1]) if mode == 2 else None,
                                              P(tabs2[2]) if mode == 2 else None, relu, P(out), dt, ST()), "bn_apply")
                assert tail_untouched(out, M * Cc)
                close("apply pg%d mode%d relu%d" % (per_group, mode, relu), out[:M * Cc].view(M, Cc).float(), want, bar)


# =====================================================================================================================
# 2. BatchNorm backward: io_bn_bwd_dt (bn_bwd_reduce_kernel + bn_bwd_finalize_kernel + bn_bwd_apply_kernel),
#    io_bn_bwd_coefs_dt, io_bn_bwd_coefs_from_tile_partials, and the tile merges behind io_conv2d_fwd_bnstats
# =====================================================================================================================
def _bn_bwd(t, d, M, Cc, G, dt, src, dzmode, act):
    """src: 'none' | 'act' | 'tables' (where the ReLU mask comes from); dzmode: 'null' | 'own' | 'alias' (dz_out == dout)
    -> dy, dgamma, dbeta, dz (None for 'null'), each without its guard"""
    n = M * Cc
    dout = guarded(n, TDT[dt])
    dout[:n] = put(d["dout"], dt).reshape(-1)
    dy, dgam, dbet, coef, part = guarded(n, TDT[dt]), guarded(Cc), guarded(Cc), guarded(2 * G * Cc), guarded(t["npart"])
    dz = guarded(n, TDT[dt]) if dzmode == "own" else dout if dzmode == "alias" else None
    _lib.check(L().io_bn_bwd_dt(P(dout), P(act) if src == "act" else None, P(t["scale"]) if src == "tables" else None,
                                P(t["shift"]) if src == "tables" else None, P(t["y"]), M, Cc, G, P(t["gamma"]), P(t["mean"]),
                                P(t["rstd"]), P(dgam), P(dbet), P(dy), P(dz), P(part), t["npart"], P(coef), dt, ST()),
               "bn_bwd %s %s" % (src, dzmode))
    for b, k in ((dout, n), (dy, n), (dgam, Cc), (dbet, Cc), (coef, 2 * G * Cc), (part, t["npart"])) + (((dz, n),) if dz is not None else ()):
        assert tail_untouched(b, k)
    if dzmode != "alias":
        assert same_bits(dout[:n], put(d["dout"], dt).reshape(-1))          # the input gradient is read only
    return dy[:n].view(M, Cc), dgam[:Cc], dbet[:Cc], (dz[:n].view(M, Cc) if dz is not None else None)


def _bn_bwd_check(Mg, G, Cc, dt, shifted):
    d = sei.bn_inputs(Mg, G, Cc, dt, shifted)
    M = G * Mg
    t = _stats(d, M, Cc, G, dt, False)
    act = guarded(M * Cc, TDT[dt])
    _lib.check(L().io_bn_apply_dt(P(t["y"]), M, Cc, G, 1, P(t["mean"]), P(t["scale"]), P(t["shift"]), None, None, None, None, 1,
                                  P(act), dt, ST()), "bn_apply")
    bar_dy = 6e-3 if dt else (1e-3 if shifted else 2e-5)
    bar_dg = 2e-5 if dt else (1e-3 if shifted else 2e-5)
    res = {}
    for src in ("none", "act", "tables"):
        gy, gg, gb, gz = sei.bn_backward_ref(d, G, src != "none")
        own = res[src] = _bn_bwd(t, d, M, Cc, G, dt, src, "own", act)
        if Mg == 2 and not dt:
            # two rows: xhat = +-1 up to eps / var, so dy = gamma * rstd * (dz - mean(dz) - xhat * mean(dz * xhat)) is what
            # is left of terms 1e3 .. 1e5 times its size, and a channel whose two rows are close has rstd ~ 170 in front of
            # the half ulp of its fp32 mean.  An fp32 evaluation is itself a good part of 2e-5 away here: PyTorch-CPU fp32
            # (the same by-hand BatchNorm and its autograd on the same inputs) is 7.5e-6 (no mask) / 4.6e-6 (masked) from the
            # fp64 reference; the bar is 3 x that distance, measured on the spot, plus the project's 2e-5
            d32 = {k: (v.float() if torch.is_tensor(v) else v) for k, v in d.items()}
            anchor = relerr(sei.bn_backward_ref(d32, G, src != "none")[0], gy)
            print("anchor dy %s %.3e" % (src, anchor))
            bar_dy = 2e-5 + 3 * anchor
        close("dy " + src, own[0].float(), gy, bar_dy)
        close("dgamma " + src, own[1], gg, bar_dg)
        close("dbeta " + src, own[2], gb, 2e-5)
        close("dz " + src, own[3].float(), gz, 6e-3 if dt else 1e-6)
        for dzmode in ("null", "alias"):
            other = _bn_bwd(t, d, M, Cc, G, dt, src, dzmode, act)
            assert all(same_bits(a, b) for a, b in zip(own[:3], other[:3])), (src, dzmode)
            assert other[3] is None or same_bits(own[3], other[3]), (src, dzmode)
    # the mask recomputed from y with the forward's tables is the stored activation's mask, bit for bit
    assert all(same_bits(a, b) for a, b in zip(res["act"], res["tables"]))
    return d, t, res


@pytest.mark.parametrize("Mg,G,Cc,dt,shifted", bn_params(sei.BN_SHAPES))
def test_bn_backward_mask_sources_and_dz_aliasing(Mg, G, Cc, dt, shifted):
    _bn_bwd_check(Mg, G, Cc, dt, shifted)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_bn_backward_nine_groups(dt):
    """G = 9 > 8: bn_bwd_finalize_kernel once stopped at eight groups (coefficients of the ninth unwritten, dgamma / dbeta
    without it).  Through the C ABI, and through ops.batch_norm(groups=9) against fp64 autograd of nine F.batch_norm calls."""
    from instaorder_amd import ops
    Mg, G, Cc = sei.G9
    d, t, _ = _bn_bwd_check(Mg, G, Cc, dt, False)
    # the node: x [G, Mg, 1, C] NHWC, one sample per group
    y64 = d["y"].clone().requires_grad_(True)
    gam64, bet64 = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    rm, rv = d["rm0"].clone(), d["rv0"].clone()
    xg = y64.view(G, Mg, 1, Cc).permute(0, 3, 1, 2)                           # NCHW view of the same rows
    ref = F.relu(torch.cat([F.batch_norm(xg[g:g + 1], rm, rv, gam64, bet64, True, sei.MOMENTUM, sei.EPS) for g in range(G)]))
    dout = d["dout"].view(G, Mg, 1, Cc).permute(0, 3, 1, 2)
    gy, gg, gb = torch.autograd.grad(ref, [y64, gam64, bet64], dout)
    x = put(d["y"], dt).view(G, Mg, 1, Cc).requires_grad_(True)
    gamma, beta = f32(d["gamma"]).requires_grad_(True), f32(d["beta"]).requires_grad_(True)
    drm, drv = f32(d["rm0"]), f32(d["rv0"])
    out = ops.batch_norm(x, gamma, beta, drm, drv, True, relu=True, groups=G)
    close("node out", out.detach().float().view(G * Mg, Cc), ref.detach().permute(0, 2, 3, 1).reshape(G * Mg, Cc), 6e-3 if dt else 1e-5)
    close("node running_mean", drm, rm, 2e-5 if dt else 1e-5)
    close("node running_var", drv, rv, 2e-5 if dt else 1e-5)
    dx, dg, db = torch.autograd.grad(out, [x, gamma, beta], put(d["dout"], dt).view(G, Mg, 1, Cc))
    close("node dx", dx.float().view(G * Mg, Cc), gy, 6e-3 if dt else 2e-5)
    close("node dgamma", dg, gg, 2e-5)
    close("node dbeta", db, gb, 2e-5)


@pytest.mark.parametrize("Mg,G,Cc,dt,shifted", bn_params(sei.BN_SHAPES) + bn_params([sei.G9 + ((0, 1), "mg65-g9-nine-groups")], False))
def test_bn_backward_coefficient_tables(Mg, G, Cc, dt, shifted):
    """io_bn_bwd_coefs_dt: dgamma / dbeta and the tables A | B | Cc of dy = A * dz + B * y + Cc against the formula of
    bn_bwd_finalize_kernel's comment in fp64"""
    d = sei.bn_inputs(Mg, G, Cc, dt, shifted)
    M = G * Mg
    t = _stats(d, M, Cc, G, dt, False)
    gy, gg, gb, gz = sei.bn_backward_ref(d, G, True)
    gz = sei.rounded(gz, dt)                                  # (a mask: representable already)
    A, B, Cq = sei.bn_coefs_ref(d["y"], gz, G, d["gamma"])
    dgam, dbet, coef, part = guarded(Cc), guarded(Cc), guarded(3 * G * Cc), guarded(t["npart"])
    _lib.check(L().io_bn_bwd_coefs_dt(P(put(gz, dt)), P(t["y"]), M, Cc, G, P(t["gamma"]), P(t["mean"]), P(t["rstd"]), P(dgam),
                                      P(dbet), P(coef), P(part), t["npart"], dt, ST()), "bn_bwd_coefs")
    for b, k in ((dgam, Cc), (dbet, Cc), (coef, 3 * G * Cc), (part, t["npart"])):
        assert tail_untouched(b, k)
    bar = 2e-5 if dt else (1e-3 if shifted else 2e-5)
    got = coef[:3 * G * Cc].view(3, G, Cc)
    close("dgamma", dgam[:Cc], gg, bar)
    close("dbeta", dbet[:Cc], gb, 2e-5)
    close("A", got[0], A, bar)
    close("B", got[1], B, bar)
    close("Cc", got[2], Cq, bar)


# nt tiles of 128 rows per group: 1 and 64 -> bn_bwd_finalize_kernel straight on the tile partials; 65 -> bn_sum_tiles_kernel
# with chunks of 64 + 1; 130 -> 64 + 64 + 2.  C = 40: the last 32-channel block of bn_sum_tiles_kernel and the last 8-channel
# block of bn_bwd_finalize_kernel are partial / exactly full
@pytest.mark.parametrize("Cc", [8, 40, 2048])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("nt", [1, 64, 65, 130])
def test_bn_coefs_from_synthetic_tile_partials(nt, G, Cc):
    g = torch.Generator().manual_seed(nt + 10 * G + Cc)
    Mg = nt * 128
    p = [torch.randn(G, nt, Cc, generator=g, dtype=torch.float64).float().double() * 3 for _ in range(2)]
    gamma = (1 + 0.2 * torch.randn(Cc, generator=g, dtype=torch.float64)).float().double()
    mean = (torch.randn(G, Cc, generator=g, dtype=torch.float64) * 0.5).float().double()
    rstd = (torch.rand(G, Cc, generator=g, dtype=torch.float64) + 0.5).float().double()
    n_in = G * nt * Cc
    n_all = (G * nt + (G * nt) // 64 + G) * Cc
    nch = -(-nt // 64) if nt > 64 else 0                     # level-1 outputs per group, written behind the tile partials
    bufs = []
    for q in p:
        b = guarded(n_all)
        b[:n_in] = f32(q).reshape(-1)
        bufs.append(b)
    dgam, dbet, coef = guarded(Cc), guarded(Cc), guarded(3 * G * Cc)
    _lib.check(L().io_bn_bwd_coefs_from_tile_partials(P(bufs[0]), P(bufs[1]), G * Mg, Cc, G, P(f32(gamma)), P(f32(mean)),
                                                      P(f32(rstd)), P(dgam), P(dbet), P(coef), ST()), "coefs_from_tiles")
    for b, q in zip(bufs, p):
        assert same_bits(b[:n_in], f32(q).reshape(-1))                        # the tile partials are read only
        assert bool(torch.isfinite(b[n_in:n_in + G * nch * Cc]).all())
        assert bool(torch.isnan(b[n_in + G * nch * Cc:]).all())               # nothing past the level-1 sums, guard included
    for b, k in ((dgam, Cc), (dbet, Cc), (coef, 3 * G * Cc)):
        assert tail_untouched(b, k)
    s1, s2 = p[0].sum(1), p[1].sum(1)                                          # [G, C]
    A = gamma * rstd
    B = -A * rstd * (s2 / Mg)
    got = coef[:3 * G * Cc].view(3, G, Cc)
    close("dbeta", dbet[:Cc], s1.sum(0), 2e-5)
    close("dgamma", dgam[:Cc], s2.sum(0), 2e-5)
    close("A", got[0], A, 2e-5)
    close("B", got[1], B, 2e-5)
    close("Cc", got[2], -A * (s1 / Mg) - B * mean, 2e-5)


# io_bn_finalize_tiles behind io_conv2d_fwd_bnstats: nt = 128 -> bn_finalize_kernel on the tile partials (no merge);
# 129 -> bn_merge_tiles_kernel with chunks of 64 + 64 + 1, bn_finalize_kernel then weighs a last partial of 128 rows
# against two of 8192; 130 -> 64 + 64 + 2
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("nt", [128, 129, 130])
def test_conv_bnstats_tile_merges(nt, G):
    N, H, W, Cc = nt * G, 16, 8, 64
    g = torch.Generator().manual_seed(nt + G)
    x = torch.randn(N, H, W, Cc, generator=g).double()
    x = x + torch.randn(N, 1, 1, 1, generator=g).double()                      # tile means differ: the merge has work to do
    w = (torch.randn(Cc, Cc, generator=g) / 8.0 + 0.05).double()               # [Cout][Cin], biased: outputs with a mean
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).double(), torch.randn(Cc, generator=g).double()
    rm0, rv0 = (torch.randn(Cc, generator=g) * 0.1).double(), (torch.rand(Cc, generator=g) + 0.5).double()
    yref = (x.view(-1, Cc) @ w.t()).view(G, -1, Cc)
    rm, rv = rm0.clone(), rv0.clone()
    for gi in range(G):
        F.batch_norm(yref[gi], rm, rv, None, None, True, sei.MOMENTUM, sei.EPS)
    mref, vref = yref.mean(1), yref.var(1, unbiased=False)
    y = guarded(N * H * W * Cc)
    nws = int(L().io_conv2d_bnstats_workspace_floats(N, H, W, Cc, 1, 1, 1, 0, G))
    ws = guarded(nws)
    tabs = [guarded(G * Cc) for _ in range(4)]
    drm, drv = guarded(Cc), guarded(Cc)
    drm[:Cc], drv[:Cc] = f32(rm0), f32(rv0)
    _lib.check(L().io_conv2d_fwd_bnstats(P(f32(x)), P(f32(w).view(Cc, 1, Cc)), P(y), N, H, W, Cc, Cc, 1, 1, 1, 0, G, P(f32(gamma)),
                                         P(f32(beta)), P(drm), P(drv), sei.MOMENTUM, sei.EPS, P(tabs[0]), P(tabs[1]), P(tabs[2]),
                                         P(tabs[3]), P(ws), nws, ST()), "conv+stats")
    assert tail_untouched(y, N * H * W * Cc) and tail_untouched(ws, nws) and tail_untouched(drm, Cc) and tail_untouched(drv, Cc)
    assert all(tail_untouched(b, G * Cc) for b in tabs)
    close("y", y[:N * H * W * Cc].view(G, -1, Cc), yref, 2e-5)
    close("mean", tabs[0][:G * Cc].view(G, Cc), mref, 1e-5)
    close("rstd", tabs[1][:G * Cc].view(G, Cc), 1.0 / torch.sqrt(vref + sei.EPS), 1e-5)
    close("running_mean", drm[:Cc], rm, 1e-5)
    close("running_var", drv[:Cc], rv, 1e-5)


# =====================================================================================================================
# 3. max-pool: io_maxpool_fwd_dt / io_maxpool_fwd_xf_dt / io_maxpool_bwd_dt (forms: step_edge_inputs.POOL_FORMS)
# =====================================================================================================================
IDX_FILL = -1


def _nhwc(t, dt):
    return put(t.permute(0, 2, 3, 1), dt)


def _pool_fwd(x, dt, xf=None, want_idx=True):
    """x [N,C,H,W] fp64 -> out [N,C,Ho,Wo] (cpu, fp32 values), idx (guarded device words).  xf = (G, mean | None, scale, shift)"""
    N, Cc, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    n_out = N * Ho * Wo * Cc
    out = guarded(n_out, TDT[dt])
    idx = torch.full((n_out // 4 + GUARD,), IDX_FILL, dtype=torch.int32, device=DEV) if want_idx else None
    if xf is None:
        _lib.check(L().io_maxpool_fwd_dt(P(_nhwc(x, dt)), N, H, W, Cc, P(out), P(idx), dt, ST()), "maxpool_fwd")
    else:
        G, mean, scale, shift = xf
        _lib.check(L().io_maxpool_fwd_xf_dt(P(_nhwc(x, dt)), N, H, W, Cc, P(out), P(idx), G, P(f32(mean)) if mean is not None else None,
                                            P(f32(scale)), P(f32(shift)), dt, ST()), "maxpool_fwd_xf")
    assert tail_untouched(out, n_out)
    if want_idx:
        assert bool((idx[n_out // 4:] == IDX_FILL).all())
    return out[:n_out].view(N, Ho, Wo, Cc).permute(0, 3, 1, 2).float().cpu(), idx


def _pool_bwd(dy, idx, shape, dt):
    N, Cc, H, W = shape
    dx = guarded(N * H * W * Cc, TDT[dt])
    _lib.check(L().io_maxpool_bwd_dt(P(_nhwc(dy, dt)), P(idx), N, H, W, Cc, P(dx), dt, ST()), "maxpool_bwd")
    assert tail_untouched(dx, N * H * W * Cc)
    return dx[:N * H * W * Cc].view(N, H, W, Cc).permute(0, 3, 1, 2).float().cpu()


def _pool_check(x, dt, seed, xf=None):
    """forward exact (with and without idx), backward element by element against autograd of F.max_pool2d, ties included"""
    xa = (sei.pool_xf_apply(x, *xf) if xf is not None else x).clone().requires_grad_(True)
    ref = F.max_pool2d(xa, 3, 2, 1)
    g = torch.Generator().manual_seed(seed)
    dy = sei.rounded(torch.randn(ref.shape, generator=g, dtype=torch.float64), dt)
    gref, = torch.autograd.grad(ref, [xa], dy)
    out, idx = _pool_fwd(x, dt, xf)
    assert torch.equal(out.double(), ref.detach())
    out2, _ = _pool_fwd(x, dt, xf, want_idx=False)               # the eval forward: idx == NULL
    assert torch.equal(out2, out)
    dx = _pool_bwd(dy, idx, x.shape, dt)
    close("dx", dx, gref, 6e-3 if dt else 1e-6)
    assert torch.equal(dx == 0, gref == 0)                       # not one element receives a gradient it should not


@pytest.mark.parametrize("relu", [0, 1], ids=["three-values", "relu-two-values"])
@pytest.mark.parametrize("dt,Cc,H,W", [pytest.param(*c[:4], id=c[4]) for c in sei.pool_cases()])
def test_maxpool_tied_windows_every_form(dt, Cc, H, W, relu):
    x = sei.tied_pool_input(sei.POOL_N, Cc, H, W, relu, seed=100 * H + W + Cc)
    _pool_check(x, dt, seed=H + W)


# the transform form (relu(bn1(x)) evaluated on the fly): rows kernels at C = 64 (shift) and fp32 C = 12 (divide), the
# element-indexed kernel at bf16 C = 12; G = 3 -> one sample per table group; scales of either sign (the arg-max is taken
# over the transformed values); in_mean NULL / a table
@pytest.mark.parametrize("with_mean", [0, 1], ids=["mean-null", "mean-table"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("dt,Cc", [pytest.param(0, 64, id="fp32-c64-rows"), pytest.param(0, 12, id="fp32-c12-rows-divide"),
                                   pytest.param(1, 64, id="bf16-c64-rows"), pytest.param(1, 12, id="bf16-c12-element")])
def test_maxpool_input_transform_forms(dt, Cc, G, with_mean):
    x = sei.tied_pool_input(sei.POOL_N, Cc, 9, 13, 0, seed=Cc + G)
    mean, scale, shift = sei.pool_xf_tables(G, Cc, seed=G + Cc)
    _pool_check(x, dt, seed=G, xf=(G, mean if with_mean else None, scale, shift))


POOL_EDGE_FORMS = [pytest.param(0, 4, id="fp32-c4-rows"), pytest.param(1, 8, id="bf16-c8-rows"), pytest.param(1, 4, id="bf16-c4-element")]


@pytest.mark.parametrize("dt,Cc", POOL_EDGE_FORMS)
def test_maxpool_one_nan_input(dt, Cc):
    """exactly the windows that hold the NaN are NaN, and the backward routes their gradients to it: the routing of the same
    map with +inf in its place"""
    N, H, W = 2, 9, 13
    x = sei.tied_pool_input(N, Cc, H, W, 0, seed=3)
    g = torch.Generator().manual_seed(4)
    dy = sei.rounded(torch.randn(N, Cc, 5, 7, generator=g, dtype=torch.float64), dt)
    xi = x.clone()
    xi[1, Cc - 1, 3, 5] = float("inf")                    # an odd row and column: in the windows (1..2, 2..3)
    xi.requires_grad_(True)
    ref = F.max_pool2d(xi, 3, 2, 1)
    gref, = torch.autograd.grad(ref, [xi], dy)
    assert int((ref == float("inf")).sum()) == 4
    xn = x.clone()
    xn[1, Cc - 1, 3, 5] = float("nan")
    out, idx = _pool_fwd(xn, dt)
    assert torch.equal(torch.isnan(out), ref.detach() == float("inf"))
    keep = ~torch.isnan(out)
    assert torch.equal(out[keep].double(), ref.detach()[keep])
    dx = _pool_bwd(dy, idx, x.shape, dt)
    close("dx", dx, gref, 6e-3 if dt else 1e-6)
    assert torch.equal(dx == 0, gref == 0)


@pytest.mark.parametrize("dt,Cc", POOL_EDGE_FORMS)
def test_maxpool_all_minus_infinity(dt, Cc):
    """A window of nothing but -inf keeps -inf and sends its gradient to its first in-bounds tap, as PyTorch does
    (tests/test_step_edges_cpu.py) -- the tap index once stayed at 0, which lies in the padding for the first output row and
    column, and the backward dropped the gradient"""
    x = torch.full((1, Cc, 4, 4), float("-inf"), dtype=torch.float64)
    dy = sei.rounded(torch.arange(1.0, 4 * Cc + 1.0, dtype=torch.float64).view(1, Cc, 2, 2) / 8, dt)
    out, idx = _pool_fwd(x, dt)
    assert bool((out == float("-inf")).all())
    dx = _pool_bwd(dy, idx, x.shape, dt)
    want = torch.zeros(1, Cc, 4, 4, dtype=torch.float64)
    want[:, :, :2, :2] = dy                               # (0,0), (0,1), (1,0), (1,1)
    assert torch.equal(dx.double(), want)


# =====================================================================================================================
# 4. average pool + heads: io_avgpool_fc_fwd_dt / io_avgpool_fc_bwd_dt (avgpool_fc_kernel, avgpool_fc_bwd_data_kernel,
#    fc_bwd_weight_kernel)
# =====================================================================================================================
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,HW,Cc,K0,K1", [pytest.param(*s[:5], id=s[5]) for s in sei.HEAD_SHAPES])
def test_avgpool_heads_small_and_ragged(N, HW, Cc, K0, K1, dt):
    g = torch.Generator().manual_seed(N + HW + Cc + K0)
    heads = [K0] + ([K1] if K1 else [])
    x = sei.rounded(torch.randn(N, HW, Cc, generator=g, dtype=torch.float64), dt).requires_grad_(True)
    ws = [(torch.randn(k, Cc, generator=g, dtype=torch.float64) / Cc ** 0.5).float().double().requires_grad_(True) for k in heads]
    bs = [torch.randn(k, generator=g, dtype=torch.float64).float().double().requires_grad_(True) for k in heads]
    pooled = x.mean(1)
    ref = torch.cat([F.linear(pooled, w, b) for w, b in zip(ws, bs)], 1)
    K = K0 + K1
    dl = torch.randn(N, K, generator=g, dtype=torch.float64).float().double()
    grads = torch.autograd.grad(ref, [x] + ws + bs, dl)
    xd, dw, db = put(x.detach(), dt), [f32(w) for w in ws], [f32(b) for b in bs]
    pl, lg = guarded(N * Cc), guarded(N * K)
    _lib.check(L().io_avgpool_fc_fwd_dt(P(xd), N, HW, Cc, P(dw[0]), P(db[0]), K0, P(dw[1]) if K1 else None,
                                        P(db[1]) if K1 else None, K1, P(pl), P(lg), dt, ST()), "avgpool_fc_fwd")
    assert tail_untouched(pl, N * Cc) and tail_untouched(lg, N * K)
    close("pooled", pl[:N * Cc].view(N, Cc), pooled.detach(), 2e-5 if dt else 1e-6)
    close("logits", lg[:N * K].view(N, K), ref.detach(), 2e-5 if dt else 1e-5)
    msk = sei.rounded(torch.randn(N, HW, Cc, generator=g, dtype=torch.float64), dt)
    n = N * HW * Cc
    res = []
    for mask in (None, msk):
        dx = guarded(n, TDT[dt])
        gw, gb = [guarded(k * Cc) for k in heads], [guarded(k) for k in heads]
        _lib.check(L().io_avgpool_fc_bwd_dt(P(f32(dl)), P(pl), N, HW, Cc, P(dw[0]), K0, P(dw[1]) if K1 else None, K1,
                                            P(put(mask, dt)) if mask is not None else None, P(dx), P(gw[0]), P(gb[0]),
                                            P(gw[1]) if K1 else None, P(gb[1]) if K1 else None, dt, ST()), "avgpool_fc_bwd")
        assert tail_untouched(dx, n)
        want = grads[0] if mask is None else grads[0] * (mask > 0)
        close("dx", dx[:n].view(N, HW, Cc).float(), want, 6e-3 if dt else 1e-5)
        res.append(dx[:n].view(N, HW, Cc))
        for i, k in enumerate(heads):
            assert tail_untouched(gw[i], k * Cc) and tail_untouched(gb[i], k)
            close("dw%d" % i, gw[i][:k * Cc].view(k, Cc), grads[1 + i], 2e-5 if dt else 1e-5)
            close("db%d" % i, gb[i][:k], grads[1 + len(heads) + i], 2e-5 if dt else 1e-5)
    assert torch.equal(res[1], res[0] * (put(msk, dt) > 0))       # the mask selects, it changes no value


# =====================================================================================================================
# 5. order loss, SGD, packing (through instaorder_amd.engine)
# =====================================================================================================================
# B = 257: one thread past the block, a second trip of every row loop for thread 0 only
@pytest.mark.parametrize("Kocc,Kdep,ndir,weighted", [
    pytest.param(2, 1, 1, True, id="kdep1-one-direction-weighted"), pytest.param(0, 1, 3, False, id="kdep1-three-directions-plain"),
    pytest.param(2, 2, 3, True, id="kdep2-three-directions-weighted"), pytest.param(0, 2, 1, True, id="kdep2-one-direction-weighted"),
    pytest.param(2, 2, 1, False, id="kdep2-one-direction-plain")])
def test_order_loss_small_heads_and_outside_rows(Kocc, Kdep, ndir, weighted):
    B = 257
    z, occ_t, dep_t, ov = sei.order_loss_inputs(Kocc, Kdep, ndir, B, weighted, seed=Kocc + 10 * Kdep + ndir)
    tot, lo, ld, dz = _ref_losses(z, B, Kocc, Kdep, occ_t, dep_t, ov, 0.1, 0.9, 0.5)
    args = (z.float().to(DEV), B, Kocc, Kdep, occ_t.float().to(DEV), dep_t.to(DEV), ov.to(DEV) if weighted else None, 0.1, 0.9, 0.5)
    losses, dl = engine.order_loss(*args, True)
    got = losses.cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(dl).all())
    for name, a, r in (("total", got[0], tot), ("occ", got[1], lo), ("depth", got[2], ld)):
        print(name, float(a), float(r))
        assert abs(a - r) < 2e-6 * max(1, abs(float(r))), name
    close("dlogits", dl, dz, 1e-5)
    if weighted:          # the rows in neither subset carry no gradient in their depth columns
        outside = ((ov != 0) & (ov != 1)).repeat(ndir)
        assert float(dl.cpu()[outside][:, Kocc:].abs().max()) == 0.0
    losses2, none = engine.order_loss(*args, False)              # dlogits == NULL
    assert none is None and same_bits(losses2, losses)


@pytest.mark.parametrize("n", [4, 1028])           # one float4; 257 float4: one past a block
def test_sgd_momentum_small_counts(n):
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([par], lr=1e-2, momentum=0.9, weight_decay=1e-3)
    dp, buf = guarded(n), guarded(n)
    dp[:n], buf[:n] = p0.to(DEV), 0.0
    for _ in range(3):
        gr = torch.randn(n, generator=g)
        par.grad = gr.clone()
        opt.step()
        engine.sgd_momentum(dp[:n], gr.to(DEV), buf[:n], 1e-2, 0.9, 1e-3)
    assert tail_untouched(dp, n) and tail_untouched(buf, n)
    close("params", dp[:n], par.detach(), 1e-6)
    close("momentum", buf[:n], opt.state[par]["momentum_buffer"], 1e-6)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nplanes", [1, 2, 3, 5])
def test_pack_planes_strides_offsets_and_zero_channels(nplanes, dt):
    """N * H * W = 105 pixels (not a multiple of 256); every plane has its own sample stride, plane 1 (0 when alone) starts
    at an element offset inside a larger tensor; channels nplanes..7 are exactly 0"""
    N, H, W = 3, 5, 7
    HW = H * W
    g = torch.Generator().manual_seed(nplanes)
    store, planes, strides, want = [], [], [], torch.zeros(N, H, W, 8)
    for c in range(nplanes):
        stride, off = HW + 3 * c + (5 if c % 2 else 0), (11 if c == min(1, nplanes - 1) else 0)
        s = torch.randn(off + N * stride, generator=g)
        for n in range(N):
            want[n, :, :, c] = s[off + n * stride: off + n * stride + HW].view(H, W)
        store.append(s.to(DEV))
        planes.append((store[-1], off))
        strides.append(stride)
    buf = guarded(N * HW * 8, TDT[dt])
    engine.pack_planes(planes, strides, N, H, W, buf[:N * HW * 8].view(N, H, W, 8))
    torch.cuda.synchronize()
    assert tail_untouched(buf, N * HW * 8)
    got = buf[:N * HW * 8].view(N, H, W, 8)
    assert same_bits(got, want.to(TDT[dt]))
    assert float(got[..., nplanes:].float().abs().max()) == 0.0
