"""Guards of tests/test_gpu_step_edges.py that need no GPU: its generators must keep telling a right kernel from a subtly
wrong one (no BatchNorm pre-activation near zero, so no element is left out of a comparison; pooling windows full of
ties, where the first and the last maximum route differently), its by-hand references must agree with torch wherever
torch accepts the shape, and the launchers must refuse an empty batch on the host instead of dividing by zero."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import step_edge_inputs as sei

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN_ROWS = [(Mg, G, C, dt, False) for Mg, G, C, dts, _ in sei.BN_SHAPES + sei.APPLY_ONLY_SHAPES for dt in dts] + \
          [sei.G9 + (0, False), sei.G9 + (1, False), sei.SHIFTED + (0, True)]


@pytest.mark.parametrize("Mg,G,C,dt,shifted", BN_ROWS)
def test_bn_inputs_keep_every_pre_activation_off_zero(Mg, G, C, dt, shifted):
    d = sei.bn_inputs(Mg, G, C, dt, shifted)
    assert d["margin"] >= sei.MASK_MARGIN[dt]
    assert torch.equal(d["y"], sei.rounded(d["y"], dt))                      # representable in the storage type
    ref = sei.bn_forward_ref(d["y"], G, d["gamma"], d["beta"], d["rm0"], d["rv0"])
    assert float(ref["pre"].abs().min()) > d["margin"]
    frac = float((ref["pre"] > 0).double().mean())
    assert Mg * C < 64 or 0.2 < frac < 0.8                                   # both sides of the ReLU occur
    if shifted:
        assert float((ref["mean"].abs() / ref["var"].sqrt()).min()) > 700.0       # 1000 sigma, with the sample sigma of 100 rows
    if Mg == 1:
        assert float(ref["var"].abs().max()) == 0.0 and torch.equal(ref["pre"], d["beta"].expand(G, C))
        assert bool(torch.isfinite(ref["rstd"]).all()) and torch.allclose(ref["rv"], 0.9 * d["rv0"])
        return
    # the by-hand reference is F.batch_norm wherever torch accepts the shape
    rm, rv = d["rm0"].clone(), d["rv0"].clone()
    outs = [F.batch_norm(d["y"][g * Mg:(g + 1) * Mg], rm, rv, d["gamma"], d["beta"], True, sei.MOMENTUM, sei.EPS) for g in range(G)]
    tol = dict(rtol=1e-9, atol=1e-6 if shifted else 1e-11)      # (at mean = 1000 sigma torch's own fp64 pre-activation is good to 1e-8)
    assert torch.allclose(torch.cat(outs), ref["pre"], **tol)
    assert torch.allclose(rm, ref["rm"], rtol=1e-12, atol=1e-12) and torch.allclose(rv, ref["rv"], rtol=1e-9, atol=1e-12)


def test_bn_shapes_reach_the_block_geometries_their_ids_name():
    def rows_per_block(Mg, G):               # bn.hip bn_rows_per_block
        want = max(1024 // G, 1)
        rpb = -(-Mg // want)
        if rpb < 64:
            rpb = min(Mg, 64)
        return rpb, -(-Mg // rpb)
    geo = {(Mg, G): rows_per_block(Mg, G) for Mg, G, _, _, _ in sei.BN_SHAPES}
    assert geo[(65, 2)] == (64, 2) and geo[(100, 1)] == (64, 2) and geo[(130, 1)] == (64, 3)
    assert geo[(8200, 8)] == (65, 127) and geo[(70001, 1)] == (69, 1015) and 70001 - 1014 * 69 == 35
    assert geo[(63, 1)] == (63, 1) and geo[(1, 1)] == (1, 1) and rows_per_block(*sei.G9[:2]) == (64, 2)
    assert 1015 > 64 and 1015 > 512          # more than one trip of bn_finalize_kernel / bn_bwd_finalize_kernel


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dt,C,H,W,name", sei.pool_cases(), ids=[c[4] for c in sei.pool_cases()])
def test_pool_inputs_are_tied_and_the_tie_rule_shows(dt, C, H, W, name, relu):
    x = sei.tied_pool_input(sei.POOL_N, C, H, W, relu, seed=100 * H + W + C)
    assert torch.equal(x, sei.rounded(x, 1))
    g = torch.Generator().manual_seed(H + W)
    dy = torch.randn(sei.POOL_N, C, (H + 1) // 2, (W + 1) // 2, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    gref, = torch.autograd.grad(F.max_pool2d(xr, 3, 2, 1), [xr], dy)
    first = sei.maxpool_bwd_by_hand(x, dy)
    assert torch.equal(first, gref)                    # torch sends a tie to the first maximum in (kh, kw) order
    if (H, W) == (1, 1):
        return                                         # one tap per window: nothing can tie
    frac = sei.tied_window_fraction(x)
    # the maps with many nine-tap windows are tied more often than not; a single row (two- and three-tap windows) and the
    # one four-tap window of a 2 x 2 map, a few dozen windows in all, at least a fifth of the time
    assert frac > (0.5 if H * W >= 100 else 0.2), frac
    assert not torch.equal(sei.maxpool_bwd_by_hand(x, dy, last=True), gref)


def test_pool_of_minus_infinity_routes_to_the_first_in_bounds_tap():
    x = torch.full((1, 4, 4, 4), float("-inf"), dtype=torch.float64, requires_grad=True)
    out = F.max_pool2d(x, 3, 2, 1)
    assert bool((out == float("-inf")).all())
    dy = torch.arange(1.0, 17.0, dtype=torch.float64).view(1, 4, 2, 2)
    gref, = torch.autograd.grad(out, [x], dy)
    want = torch.zeros(1, 4, 4, 4, dtype=torch.float64)
    want[:, :, :2, :2] = dy
    assert torch.equal(gref, want) and torch.equal(sei.maxpool_bwd_by_hand(x.detach(), dy), want)


def test_pool_transform_tables_keep_the_values_exact_and_flip_signs():
    for G in (1, 3):
        mean, scale, shift = sei.pool_xf_tables(G, 64, seed=G)
        assert bool((scale < 0).any()) and bool((scale > 0).any())
        x = sei.tied_pool_input(3, 64, 9, 13, 0, seed=5)
        xa = sei.pool_xf_apply(x, G, mean, scale, shift)
        assert torch.equal(xa, sei.rounded(xa, 1)) and sei.tied_window_fraction(xa) > 0.5


def test_order_loss_inputs_carry_rows_outside_both_subsets():
    z, occ_t, dep_t, ov = sei.order_loss_inputs(2, 2, 3, 257, True, seed=1)
    assert {2, -1, 0, 1} == set(ov.tolist())
    out = (ov != 0) & (ov != 1)
    for d in range(3):
        lab = dep_t[d * 257:(d + 1) * 257]
        assert bool(((lab < 0) | (lab >= 2))[out].any()) and not bool(((lab < 0) | (lab >= 2))[~out].any())


_CHILD = r"""
import ctypes as C, importlib.util, sys
spec = importlib.util.spec_from_file_location("io_lib", sys.argv[1])
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
L = m.lib()
bad = []
def chk(name, rc):
    if not (rc < 0 and len(L.io_last_error_string()) > 0):
        bad.append((name, rc))
N = None
for M in (0, -64):
    chk("stats %d" % M, L.io_bn_stats_finalize(N, M, 64, 1, N, N, N, N, 0.1, 1e-5, N, N, N, N, N, 0, N))
    chk("bwd %d" % M, L.io_bn_bwd(N, N, N, N, N, M, 64, 1, N, N, N, N, N, N, N, N, 0, N, N))
    chk("coefs %d" % M, L.io_bn_bwd_coefs_dt(N, N, M, 64, 1, N, N, N, N, N, N, N, 0, 0, N))
chk("bwd bf16 c4", L.io_bn_bwd_dt(N, N, N, N, N, 64, 4, 1, N, N, N, N, N, N, N, N, 1 << 20, N, 1, N))
chk("coefs bf16 c4", L.io_bn_bwd_coefs_dt(N, N, 64, 4, 1, N, N, N, N, N, N, N, 1 << 20, 1, N))
print("BAD", bad)
sys.exit(1 if bad else 0)
"""


def test_bn_launchers_refuse_an_empty_batch_on_the_host():
    """M = 0 once reached an integer division by zero in bn_rows_per_block, M < 0 a launch with a negative row count, bf16
    with C = 4 a launch with zero chunks per row.  All are refused before the first HIP call, so this runs without a GPU
    -- in a child process: a regression is a signal, not an exception."""
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "instaorder_amd", "_lib.py")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
