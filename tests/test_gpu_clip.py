"""Gradient clipping on the MI355X: io_grad_norm against fp64 NumPy on the same bits, the clipping record, the clipped
SGD / Adam updates against the plain kernels on a pre-scaled gradient, the non-finite guard, hipGraph capture, the four
flat optimisers inside the ResNet and MiDaS models, and checkpoints between clipped and unclipped models."""
import numpy as np
import pytest
import torch

from helpers import ALGO_CLASSES, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS64 = 2.0 ** -52
N_BIG = (1 << 20) + 12


def _ch():
    from instaorder_amd import engine
    return engine.grad_norm_chunk()


def _state():
    from instaorder_amd import engine
    return engine.new_clip_state(DEV)


def _read(state):
    from instaorder_amd import engine
    return engine.read_clip_state(state)


def _f32_bits(x):
    return np.float32(x).view(np.uint32)


def _within_ulps(got, ref32, k=1):
    ref32 = np.float32(ref32)
    return abs(float(np.float32(got)) - float(ref32)) <= k * float(np.spacing(np.abs(ref32)))


def _scaled_randn(n, seed):
    """randn times per-position scales from 1e-3 to 1e3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    scale = 10.0 ** ((torch.arange(n) % 61).double() / 10.0 - 3.0)
    return (x.double() * scale).float()


def _segmentations(n, ch):
    q = n // 4
    a, b = 4 * (q * 3 // 10), 4 * (q * 7 // 10)
    out = {"one": [0, n], "uneven": [0, a, b, n], "empty": [0, a, a, n], "sixteen": [4 * (q * i // 16) for i in range(17)]}
    if n > 2 * ch:      # more boundaries that are no multiple of the chunk: just below one, just above it
        assert a % ch and b % ch
        out["uneven_chunks"] = [0, ch - 4, ch + 8, n]
    return out


# ---- 1. the norm kernel against fp64 NumPy on the same bits -----------------------------------------------------------
@pytest.mark.parametrize("which", ["4", "252", "CH-4", "CH", "CH+4", "3CH+12", "2^20+12"])
def test_grad_norm_matches_fp64_numpy(which):
    from instaorder_amd import engine
    ch = _ch()
    n = {"4": 4, "252": 252, "CH-4": ch - 4, "CH": ch, "CH+4": ch + 4, "3CH+12": 3 * ch + 12, "2^20+12": N_BIG}[which]
    x = _scaled_randn(n, 11 + n % 97)
    x64 = x.numpy().astype(np.float64)
    g = x.to(DEV)
    assert engine.grad_norm_workspace_bytes(n, 1) == 8 * ((n + ch - 1) // ch + 1)
    for name, offs in _segmentations(n, ch).items():
        runs = []
        for _ in range(2):
            st = _state()
            seg = engine.grad_norm(g, float("inf"), st, offs)
            runs.append((seg.cpu().numpy().copy(), _read(st)))
        (seg, rec), (seg2, rec2) = runs
        ref = np.array([np.sum(x64[lo:hi] ** 2) for lo, hi in zip(offs[:-1], offs[1:])])
        err = np.abs(seg - ref)
        print(which, name, "max rel err of the segment sums %.2e (bound %.2e)" % (float((err / np.maximum(ref, 1e-300)).max()),
                                                                               n * EPS64))
        # each value is squared exactly in fp64 (24-bit significands) and the <= n additions round once each
        assert np.all(err <= n * EPS64 * ref), (which, name, seg, ref)
        want = np.float32(np.sqrt(ref.sum()))
        assert _within_ulps(rec["norm"], want), (which, name, rec["norm"], want)
        assert rec["coef"] == 1.0 and rec["nonfinite"] == 0 and (rec["steps"], rec["clipped"], rec["skipped"]) == (1, 0, 0)
        # bitwise repeatable
        assert seg.tobytes() == seg2.tobytes() and _f32_bits(rec["norm"]) == _f32_bits(rec2["norm"]), (which, name)


def test_grad_norm_refuses_a_short_workspace():
    from instaorder_amd import engine
    n = 3 * _ch()
    g = torch.zeros(n, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        engine.grad_norm(g, 1.0, _state(), None, torch.empty(16, dtype=torch.uint8, device=DEV))


# ---- 2. tiny and huge magnitudes ------------------------------------------------------------------------------------
def test_grad_norm_tiny_and_huge_values():
    from instaorder_amd import engine
    n = N_BIG
    tiny = torch.full((n,), 1e-30)
    # fp32 squares underflow: torch's own norm of these gradients is 0 (on the CPU, the same arithmetic as on the device)
    assert float(torch.linalg.vector_norm(tiny)) == 0.0
    st = _state()
    engine.grad_norm(tiny.to(DEV), 1.0, st)
    rec = _read(st)
    want = np.float32(float(np.float32(1e-30)) * np.sqrt(float(n)))
    print("1e-30 x %d: norm %.9e, expected %.9e" % (n, rec["norm"], want))
    assert rec["norm"] > 0 and _within_ulps(rec["norm"], want) and rec["nonfinite"] == 0 and rec["coef"] == 1.0
    st = _state()
    engine.grad_norm(torch.full((n,), 1e18, device=DEV), float("inf"), st)     # fp32 sum of squares: inf at 1e36 x 2^20
    rec = _read(st)
    want = np.float32(float(np.float32(1e18)) * np.sqrt(float(n)))
    print("1e18 x %d: norm %.9e, expected %.9e" % (n, rec["norm"], want))
    assert np.isfinite(rec["norm"]) and _within_ulps(rec["norm"], want) and rec["nonfinite"] == 0 and rec["skipped"] == 0


# ---- 3. the coefficient ---------------------------------------------------------------------------------------------
def test_clip_coefficient():
    from instaorder_amd import engine
    n = 3 * _ch() + 12
    g = _scaled_randn(n, 5).to(DEV)
    st = _state()
    engine.grad_norm(g, float("inf"), st)
    r0 = _read(st)
    norm = np.float32(r0["norm"])
    assert r0["coef"] == 1.0 and r0["clipped"] == 0
    half = float(norm) / 2
    engine.grad_norm(g, half, st)
    r1 = _read(st)
    want = np.float32(half) / (norm + np.float32(1e-6))            # fp32, IEEE division
    assert _f32_bits(r1["norm"]) == _f32_bits(norm) and _f32_bits(r1["coef"]) == _f32_bits(want), (r1, want)
    assert r1["coef"] < 1.0 and (r1["steps"], r1["clipped"], r1["skipped"]) == (2, 1, 0)
    engine.grad_norm(g, 2 * float(norm), st)
    r2 = _read(st)
    assert r2["coef"] == 1.0 and (r2["steps"], r2["clipped"]) == (3, 1)
    zero = torch.zeros(n, device=DEV)
    st = _state()
    seg = engine.grad_norm(zero, 1.0, st, [0, 4 * (n // 8), n])
    rz = _read(st)
    assert rz["norm"] == 0.0 and rz["coef"] == 1.0 and rz["nonfinite"] == 0 and rz["clipped"] == 0
    assert seg.cpu().tolist() == [0.0, 0.0]


def test_clip_against_torch_clip_grad_norm():
    """The fused path against torch.nn.utils.clip_grad_norm_ on a copy of the same gradients, cut into parameters."""
    from instaorder_amd import engine
    n = 3 * _ch() + 12
    g = _scaled_randn(n, 7).to(DEV)
    cuts = [0, 1000, 1004, n // 3, n // 2 + 4, n]
    params = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        p = torch.nn.Parameter(torch.zeros(hi - lo, device=DEV))
        p.grad = g[lo:hi].clone()
        params.append(p)
    st = _state()
    engine.grad_norm(g, float("inf"), st)
    # a third of the norm: at exactly half, coef is exactly 0.5 whichever way it is formed and nothing is compared
    max_norm = _read(st)["norm"] / 3
    engine.grad_norm(g, max_norm, st)
    rec = _read(st)
    tnorm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    mine = torch.mul(g, rec["coef"]).double()
    theirs = torch.cat([p.grad for p in params]).double()
    dn = abs(rec["norm"] - tnorm) / tnorm
    dg = float((mine - theirs).abs().max() / theirs.abs().max())
    print("against clip_grad_norm_: total norm rel diff %.3e, clipped gradients rel diff %.3e" % (dn, dg))
    # torch sums the squares in fp32 and multiplies by a reciprocal where this path divides: last-bits differences.
    # The norm: half the relative error of torch's fp32 sum of n squares (worst case n * 2^-24) plus its two roundings.
    assert dn <= n * 2.0 ** -25 + 2.0 ** -23, dn
    assert dg <= 4 * CLIP_TORCH_MEASURED, dg


# First run on an MI355X (max_norm at half and at a third of the norm alike): total norm rel diff 0, clipped gradients rel
# diff 0 (max |a - b| / max |b|) -- torch's fp32 norm of these 49164 gradients rounds to the same float as the fp64 one, and
# its reciprocal-and-multiply gives the same coefficient as the division here.  Four times the measured value is 0: the
# clipped gradients are held to bitwise equality with torch's.
CLIP_TORCH_MEASURED = 0.0


# ---- 4. the clipped update is the unclipped update on a scaled gradient ------------------------------------------------
def _clip_record_for(g, coef_below_one):
    from instaorder_amd import engine
    st = _state()
    engine.grad_norm(g, float("inf"), st)
    if coef_below_one:
        engine.grad_norm(g, _read(st)["norm"] / 3, st)
    rec = _read(st)
    assert (rec["coef"] < 1.0) == coef_below_one and rec["nonfinite"] == 0
    return st, rec["coef"]


@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_clipped_sgd_is_plain_sgd_on_the_scaled_gradient(wd, scaled):
    from instaorder_amd import engine
    torch.manual_seed(2)
    n = N_BIG
    g = torch.randn(n, device=DEV) * 3
    st, coef = _clip_record_for(g, scaled)
    gs = torch.mul(g, coef) if scaled else g
    p0, b0 = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    p1, b1, p2, b2 = p0.clone(), b0.clone(), p0.clone(), b0.clone()
    for _ in range(2):
        engine.sgd_momentum(p1, g, b1, 0.05, 0.9, wd, clip_state=st)
        engine.sgd_momentum(p2, gs, b2, 0.05, 0.9, wd)
    assert torch.equal(p1, p2) and torch.equal(b1, b2) and not torch.equal(p1, p0)


@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_clipped_adam_is_plain_adam_on_the_scaled_gradient(wd, scaled):
    from instaorder_amd import engine
    torch.manual_seed(3)
    n = N_BIG
    g = torch.randn(n, device=DEV) * 3
    st, coef = _clip_record_for(g, scaled)
    gs = torch.mul(g, coef) if scaled else g
    p0, m0, v0 = torch.randn(n, device=DEV), torch.randn(n, device=DEV) * 0.1, torch.rand(n, device=DEV) * 0.01
    a, b = [t.clone() for t in (p0, m0, v0)], [t.clone() for t in (p0, m0, v0)]
    for step in (3, 4):
        engine.adam_step(a[0], g, a[1], a[2], 1e-3, 0.5, 0.999, 1e-8, wd, step, clip_state=st)
        engine.adam_step(b[0], gs, b[1], b[2], 1e-3, 0.5, 0.999, 1e-8, wd, step)
    for x, y, what in zip(a, b, ("p", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), what
    assert not torch.equal(a[0], p0)
    # a sub-range, as FusedAdam's runs launch it
    engine.adam_step(a[0], g, a[1], a[2], 1e-3, 0.5, 0.999, 1e-8, wd, 5, 1024, n - 2048, clip_state=st)
    engine.adam_step(b[0], gs, b[1], b[2], 1e-3, 0.5, 0.999, 1e-8, wd, 5, 1024, n - 2048)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def test_clipped_updates_need_a_record():
    from instaorder_amd import engine
    t = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match="clip_state"):
        engine.sgd_momentum(t, t.clone(), t.clone(), 0.1, 0.9, 0.0, clip_state=torch.zeros(8, device=DEV))


# ---- 5. the guard -----------------------------------------------------------------------------------------------------
def test_non_finite_gradient_skips_the_step():
    from instaorder_amd import engine
    ch = _ch()
    n = 2 * ch + 252
    offs = [0, ch + 100, n]              # segment 0 ends in a partial block [ch, ch + 100); so does segment 1
    torch.manual_seed(4)
    clean = torch.randn(n, device=DEV)
    p, buf = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    ap, am, av = torch.randn(n, device=DEV), torch.randn(n, device=DEV), torch.rand(n, device=DEV)
    keep = [t.clone() for t in (p, buf, ap, am, av)]
    st = _state()
    skipped = 0
    for pos in (0, n - 1, ch + 50):
        for val in (float("inf"), float("-inf"), float("nan")):
            g = clean.clone()
            g[pos] = val                                   # a value in a gradient tensor: nothing faults
            engine.grad_norm(g, 1.0, st, offs)
            engine.sgd_momentum(p, g, buf, 0.1, 0.9, 1e-4, clip_state=st)
            engine.adam_step(ap, g, am, av, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 2, clip_state=st)
            rec = _read(st)
            skipped += 1
            assert rec["nonfinite"] == 1 and rec["skipped"] == skipped and rec["steps"] == skipped, (pos, val, rec)
            for t, k, what in zip((p, buf, ap, am, av), keep, ("p", "buf", "adam p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(t, k), (pos, val, what)
    # a clean step afterwards updates as usual
    engine.grad_norm(clean, float("inf"), st, offs)
    engine.sgd_momentum(p, clean, buf, 0.1, 0.9, 1e-4, clip_state=st)
    engine.adam_step(ap, clean, am, av, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 2, clip_state=st)
    rec = _read(st)
    assert rec["nonfinite"] == 0 and rec["skipped"] == skipped and rec["steps"] == skipped + 1 and rec["clipped"] == 0
    engine.sgd_momentum(keep[0], clean, keep[1], 0.1, 0.9, 1e-4)
    engine.adam_step(keep[2], clean, keep[3], keep[4], 1e-3, 0.9, 0.999, 1e-8, 1e-2, 2)
    for t, k in zip((p, buf, ap, am, av), keep):
        assert torch.equal(t, k)
    assert bool(torch.isfinite(p).all())


# ---- 6. capturable ----------------------------------------------------------------------------------------------------
def test_norm_and_clipped_update_replay_in_a_graph():
    from instaorder_amd import engine
    ch = _ch()
    n = 5 * ch + 36
    offs = [0, 2 * ch + 8, n]
    torch.manual_seed(6)
    contents = [torch.randn(n, device=DEV), torch.randn(n, device=DEV) * 7]
    p0, b0 = torch.randn(n, device=DEV), torch.randn(n, device=DEV)

    def buffers():
        return (_state(), torch.zeros(2, dtype=torch.float64, device=DEV),
                torch.empty(engine.grad_norm_workspace_bytes(n, 2), dtype=torch.uint8, device=DEV))

    def run(g, p, b, st, seg, ws):
        engine.grad_norm(g, 40.0, st, offs, ws, seg)
        engine.sgd_momentum(p, g, b, 0.05, 0.9, 1e-4, clip_state=st)

    eager = []
    g, p, b = torch.empty(n, device=DEV), p0.clone(), b0.clone()
    st, seg, ws = buffers()
    for c in contents:
        g.copy_(c)
        run(g, p, b, st, seg, ws)
        eager.append((p.clone(), b.clone(), seg.clone(), _read(st)))
    assert eager[0][3]["coef"] < 1.0 and eager[1][3]["coef"] < eager[0][3]["coef"]
    g, p, b = torch.zeros(n, device=DEV), p0.clone(), b0.clone()
    st, seg, ws = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(g, p, b, st, seg, ws)
    for c, (pe, be, sege, rece) in zip(contents, eager):
        g.copy_(c)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(p, pe) and torch.equal(b, be) and torch.equal(seg, sege)
        assert _read(st) == rece


# ---- 7. whole model, ResNet -----------------------------------------------------------------------------------------
ALGO, SEED, S, B = "InstaOrderNet_o", 23, 64, 4


def _order_model(optim, dtype, clip="absent", seed=SEED, lr=1e-3):
    import instaorder_amd as ia
    cfg = dict(algo=ALGO, lr=lr, weight_decay=1e-4, optim=optim, beta1=0.5, backbone_arch="resnet50_cls",
               backbone_param=dict(in_channels=5, num_classes=ALGO_CLASSES[ALGO]), use_rgb=True, dtype=dtype)
    if clip != "absent":
        cfg["clip_grad_norm"] = clip
    m = ia.InstaOrderNet_o(cfg, dist_model=False)
    sd = synthetic.make_state_dict(seed, 5, ALGO_CLASSES[ALGO], prefix="module.", style="kaiming")
    m.model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m.switch_to("train")
    return m


def _feed_order(m, it):
    t = {k: torch.from_numpy(v.copy()) for k, v in synthetic.make_pair_batch(SEED + 300 + it, B, S).items()}
    m.set_input(t["rgb"], t["modal1"], t["modal2"], t["occ_order"])


def _views_norm(views):
    """fp64 norm over per-parameter gradient views (logical elements only: no storage padding), rounded to fp32"""
    tot = torch.zeros((), dtype=torch.float64, device=DEV)
    for v in views:
        tot += (v.detach().double() ** 2).sum()
    return np.float32(np.sqrt(float(tot)))


def _check_stats(stats, views, names):
    want = _views_norm(views)
    print("norm %.9e, fp64 over the parameter views %.9e, stages %s" % (stats["norm"], want, stats["stage_norms"]))
    assert stats["norm"] > 0 and _within_ulps(stats["norm"], want), (stats["norm"], want)
    assert sorted(stats["stage_norms"]) == sorted(names)
    # the segment sums add up to the total in fp64; norm is that total's root rounded to fp32 (2^-24), squared (2^-23)
    ssq = sum(v * v for v in stats["stage_norms"].values())
    assert abs(ssq - stats["norm"] ** 2) <= 2.0 ** -22 * stats["norm"] ** 2
    assert all(v > 0 for v in stats["stage_norms"].values())


@pytest.mark.parametrize("optim", ["SGD", "Adam"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_resnet_model_with_clipping(dtype, optim):
    from instaorder_amd.optim import FusedAdam, FusedSGD
    from instaorder_amd.single_stage_model import SingleStageModel
    plain, inf = _order_model(optim, dtype), _order_model(optim, dtype, float("inf"))
    assert isinstance(inf.optim, FusedAdam if optim == "Adam" else FusedSGD) and plain.optim.max_grad_norm is None
    norm0 = None
    for it in range(3):                                   # eager, capture, replay
        for m in (plain, inf):
            _feed_order(m, it)
            m.step()
        assert torch.equal(plain.net.flat_params, inf.net.flat_params), it
        stats = inf.optim.grad_stats()
        _check_stats(stats, [p.grad for p in inf.net.parameters()], SingleStageModel.RESNET_STAGE_NAMES)
        assert stats["coef"] == 1.0 and stats["nonfinite"] == 0 and stats["steps"] == it + 1 and stats["skipped"] == 0
        norm0 = stats["norm"] if it == 0 else norm0
    assert inf._graph is not None and plain._graph is not None
    assert inf.optim.clip_state.is_cuda and plain.optim.clip_state is None
    del plain, inf
    # clipping at half of step 0's norm == the existing optimiser on the views' gradients scaled by the reported coef
    half, ref = _order_model(optim, dtype, norm0 / 2), _order_model(optim, dtype)
    start = half.net.flat_params.clone()
    _feed_order(half, 0)
    half.step()
    stats = half.optim.grad_stats()
    assert _f32_bits(stats["norm"]) == _f32_bits(norm0) and 0.49 < stats["coef"] < 0.51 and stats["clipped"] == 1
    with torch.no_grad():
        for dst, src in zip(ref.net._grad_views, half.net._grad_views):
            dst.copy_(torch.mul(src, stats["coef"]))
    ref.net.attach_grads()
    ref.optim.step()
    assert torch.equal(half.net.flat_params, ref.net.flat_params)
    assert not torch.equal(half.net.flat_params, start)


# ---- 8. whole model, MiDaS --------------------------------------------------------------------------------------------
def _depth_model(optim, clip="absent", seed=31, lr=1e-4):
    import instaorder_amd as ia
    torch.manual_seed(seed)
    cfg = dict(algo="InstaDepthNet_od", lr=lr, weight_decay=1e-4, optim=optim, beta1=0.5, pretrained_weight=None,
               use_rgb=True, dtype="fp32", overlap_weight=0.1, distinct_weight=0.9, dorder_weight=1.0, smooth_weight=0.1,
               occ_order_weight=1.0)
    if clip != "absent":
        cfg["clip_grad_norm"] = clip
    m = ia.InstaDepthNet_od(cfg, dist_model=False)
    m.switch_to("train")
    return m


def _feed_depth(m, seed=131):
    t = {k: torch.from_numpy(v.copy()) for k, v in synthetic.make_depth_batch(seed, 2, 64).items()}
    m.set_input(t["rgb"], t["modal1"], t["modal2"], t["depth_order"], t["count"], t["is_overlap"], t["occ_order"])


def _flat_views(opt, buf):
    return [buf[off:off + k].view(p.shape) for p, (off, k) in zip(opt._params, opt._spans)]


@pytest.mark.parametrize("optim", ["SGD", "Adam"])
def test_midas_model_with_clipping(optim):
    from instaorder_amd.optim import FlatAdam, FlatSGD
    plain, inf = _depth_model(optim), _depth_model(optim, float("inf"))
    assert isinstance(inf.optim, FlatAdam if optim == "Adam" else FlatSGD)
    assert torch.equal(plain.optim.flat_params, inf.optim.flat_params)
    for m in (plain, inf):
        _feed_depth(m)
        m.step()
    assert torch.equal(plain.optim.flat_params, inf.optim.flat_params)
    stats = inf.optim.grad_stats()
    _check_stats(stats, _flat_views(inf.optim, inf.optim.flat_grads), inf.STAGE_NAMES)
    assert stats["coef"] == 1.0 and stats["nonfinite"] == 0
    norm0 = stats["norm"]
    # a poisoned gradient element: the step leaves every parameter (and the optimiser state) as it is
    before = inf.optim.flat_params.clone()
    state_before = [t.clone() for t in ((inf.optim._buf,) if optim == "SGD" else (inf.optim._exp_avg, inf.optim._exp_avg_sq))]
    off, k = inf.optim._spans[len(inf.optim._spans) // 2]
    inf.optim.flat_grads[off + k - 1] = float("nan")
    inf.optim.step(gathered=True)
    stats = inf.optim.grad_stats()
    assert stats["nonfinite"] == 1 and stats["skipped"] == 1 and stats["steps"] == 2
    assert torch.equal(inf.optim.flat_params, before)
    for t, k0 in zip((inf.optim._buf,) if optim == "SGD" else (inf.optim._exp_avg, inf.optim._exp_avg_sq), state_before):
        assert torch.equal(t, k0)
    del plain, inf, before, state_before
    torch.cuda.empty_cache()
    half, ref = _depth_model(optim, norm0 / 2), _depth_model(optim)
    _feed_depth(half)
    half.step()
    stats = half.optim.grad_stats()
    assert _f32_bits(stats["norm"]) == _f32_bits(norm0) and 0.49 < stats["coef"] < 0.51 and stats["clipped"] == 1
    with torch.no_grad():
        for dst, src in zip(_flat_views(ref.optim, ref.optim.flat_grads), _flat_views(half.optim, half.optim.flat_grads)):
            dst.copy_(torch.mul(src, stats["coef"]))
    if optim == "Adam":
        ref.optim._live = list(half.optim._live)
    ref.optim.step(gathered=True)
    assert torch.equal(half.optim.flat_params, ref.optim.flat_params)


# ---- 9. checkpoints -----------------------------------------------------------------------------------------------------
def _run(m, its):
    for it in its:
        _feed_order(m, it)
        m.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize("optim", ["SGD", "Adam"])
def test_checkpoints_interchange_between_clipped_and_unclipped(optim, tmp_path):
    """clip_grad_norm=inf never scales, so a run that changes from a clipped to an unclipped model (or back) at a
    checkpoint ends on the bits of the uninterrupted unclipped run; the optimiser state dict is torch's either way."""
    inf = float("inf")
    whole = _order_model(optim, "fp32")
    _run(whole, range(3))
    for first, second, tag in ((inf, "absent", "a"), ("absent", inf, "b")):
        d = tmp_path / tag
        d.mkdir()
        a = _order_model(optim, "fp32", first)
        _run(a, range(2))
        a.save_state(str(d), 2)
        b = _order_model(optim, "fp32", second, seed=SEED + 1)       # other weights: everything comes from the file
        b.load_state(str(d), 2, resume=True)
        _run(b, range(2, 3))
        assert torch.equal(whole.net.flat_params, b.net.flat_params), (first, second)
        assert (b.optim.max_grad_norm == inf) == (second == inf)
    # torch's own optimiser: its state dict loads into the clipped optimiser and the clipped one's into torch's
    clipped = _order_model(optim, "fp32", 0.5)
    _run(clipped, range(2))
    params = list(clipped.net.parameters())
    kw = dict(momentum=0.9, weight_decay=1e-4) if optim == "SGD" else dict(betas=(0.5, 0.999))
    topt = getattr(torch.optim, optim)(params, lr=1e-3, **kw)
    sd = clipped.optim.state_dict()
    topt.load_state_dict(sd)
    key = "momentum_buffer" if optim == "SGD" else "exp_avg"
    for i, p in enumerate(params):
        assert torch.equal(topt.state[p][key], sd["state"][i][key])
    back = topt.state_dict()
    assert "max_grad_norm" not in back["param_groups"][0] and "clip_grad_norm" not in back["param_groups"][0]
    other = _order_model(optim, "fp32", 0.25, seed=SEED + 1)
    other.optim.load_state_dict(back)
    assert other.optim.max_grad_norm == 0.25
    out = other.optim.state_dict()
    for i in sd["state"]:
        assert torch.equal(out["state"][i][key], sd["state"][i][key])
    if optim == "Adam":
        assert other.optim._steps == [2] * len(params)
