"""optim: Adam on the MI355X: the io_adam_step kernel against torch.optim.Adam, the reference's own Adam runs
(tests/golden/adam_*.npz, tests/golden/make_golden_adam.py), FusedAdam / FlatAdam against the torch.optim.Adam path they
replace, checkpoints and the learning-rate schedule."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import ALGO_CLASSES, load_golden, norms_and_samples, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = float(np.finfo(np.float32).eps)


# ---- 1. the kernel against torch.optim.Adam on the same tensors ----------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_kernel_matches_torch_adam(wd):
    from instaorder_amd import engine
    torch.manual_seed(3)
    n = (1 << 20) + 12
    p0 = torch.randn(n, device=DEV)
    grads = [torch.randn(n, device=DEV) * (10.0 ** -(s % 3)) for s in range(5)]
    ref = nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(0.5, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    lrs = [1e-3, 1e-3, 4e-4, 4e-4, 2e-3]
    for s in range(5):
        opt.param_groups[0]["lr"] = lrs[s]
        ref.grad = grads[s].clone()
        opt.step()
        engine.adam_step(p, grads[s], m, v, lrs[s], 0.5, 0.999, 1e-8, wd, s + 1)
    torch.cuda.synchronize()
    st = opt.state[ref]
    # exp_avg can cancel (g + wd*p against m): its rounding is held to the size of the terms it is formed from
    g_last = grads[-1].abs() + wd * ref.detach().abs()
    for mine, theirs, scale, what in ((m, st["exp_avg"], st["exp_avg"].abs() + g_last, "exp_avg"),
                                      (v, st["exp_avg_sq"], st["exp_avg_sq"].abs(), "exp_avg_sq")):
        ulps = ((mine - theirs).abs() / (scale * EPS32 + 1e-30)).max().item()
        print(what, "max ulp", ulps)
        assert ulps <= 8, (what, ulps)        # measured: 0 / 4.4 (wd 0), 1.0 / 4.4 (wd 1e-2)
    dp = (p - ref.detach()).abs()
    bound = 1e-6 * max(lrs) + 2 * EPS32 * ref.detach().abs()
    print("max |dp| %.3e" % dp.max().item())
    assert bool((dp <= bound).all()), float(dp.max())


def test_adam_kernel_rejects_unaligned_length():
    from instaorder_amd import engine
    t = torch.zeros(10, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        engine.adam_step(t, t.clone(), t.clone(), t.clone(), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 6)


# ---- 2. the reference's own Adam runs ------------------------------------------------------------------------------
def _order_cfg(algo, lr, beta1, dtype="fp32"):
    return dict(algo=algo, lr=lr, weight_decay=1e-4, optim="Adam", beta1=beta1, backbone_arch="resnet50_cls",
                backbone_param=dict(in_channels=5, num_classes=ALGO_CLASSES[algo]), use_rgb=True, overlap_weight=0.1,
                distinct_weight=0.9, dtype=dtype)


def _order_model(algo, seed, lr, beta1, dtype="fp32", style="xavier"):
    import instaorder_amd as ia
    m = getattr(ia, algo)(_order_cfg(algo, lr, beta1, dtype), dist_model=False)
    sd = synthetic.make_state_dict(seed, 5, ALGO_CLASSES[algo], prefix="module.", style=style)
    m.model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m


def _feed_order(m, algo, batch):
    t = {k: torch.from_numpy(v.copy()) for k, v in batch.items()}
    if algo == "InstaOrderNet_od":
        m.set_input(t["rgb"], t["modal1"], t["modal2"], t["depth_order"], t["count"], t["is_overlap"], t["occ_order"])
    else:
        m.set_input(t["rgb"], t["modal1"], t["modal2"], t["occ_order"])


@pytest.mark.parametrize("tag,algo", [("adam_o_S64_B4", "InstaOrderNet_o"), ("adam_od_S64_B4", "InstaOrderNet_od")])
def test_adam_golden(tag, algo):
    """Three steps of the reference with optim: Adam, beta1 0.5.  Post-step parameters: Adam's first update is
    lr * m_hat / sqrt(v_hat) = lr * sign(g) per element, whatever |g| is -- so an element whose gradient is within
    rounding of zero (where two fp32 implementations disagree on the sign) moves by up to 2 lr relative to the reference,
    while every other element agrees to rounding.  Hence: >= 99 % of the samples within 1e-3 lr, all within 2.5 lr."""
    from instaorder_amd.optim import FusedAdam
    g = load_golden(tag)
    S, B, seed, steps = [int(v) for v in g["meta"]]
    lr, beta1 = float(g["lr"]), float(g["beta1"])
    m = _order_model(algo, seed, lr, beta1)
    assert isinstance(m.optim, FusedAdam)
    m.switch_to("train")
    params = list(m.net.parameters())
    for it in range(steps):
        _feed_order(m, algo, synthetic.make_pair_batch(seed + 100 + it, B, S))
        ret = m.step()
        out = {k: float(v) for k, v in ret[0].items()} if isinstance(ret, tuple) else {}
        out["loss"] = float((ret[1] if isinstance(ret, tuple) else ret)["loss"])
        # step 0 from identical weights: 1e-5.  Later steps start from weights in which ~1 % of the elements sit 2 lr
        # away from the reference's (the sign flips above): the losses then differ by a few percent (measured, _o / _od:
        # 1.1e-2 / 1.3e-3 at step 1, 5.2e-2 / 2.8e-2 at step 2), the amplification of rounding that makes the SGD goldens
        # chaotic after step 0 (tests/test_gpu_net.py).  They are held to 1e-1; the optimiser itself is pinned to
        # torch.optim.Adam to rounding by the tests below.
        tol = 1e-5 if it == 0 else 1e-1
        for k, v in out.items():
            ref = float(g["step%d_%s" % (it, k)])
            print(tag, "step", it, k, v, ref, abs(v - ref) / abs(ref))
            assert abs(v - ref) <= tol * abs(ref), (it, k, v, ref)
        if it == 0:
            gn, _ = norms_and_samples([p.grad for p in params])
            gerr = np.abs(gn - g["grad_norms"]) / np.maximum(g["grad_norms"], 1e-30)
            print(tag, "grad-norm rel diff: median %.2e max %.2e" % (np.median(gerr), gerr.max()))
            assert np.median(gerr) < 0.02 and gerr.max() < 0.15
        if it in (0, steps - 1):
            _, ps = norms_and_samples(params)
            d = np.abs(ps.astype(np.float64) - g["step%d_param_samples" % it])
            frac = float((d <= 1e-3 * lr).mean())
            print(tag, "step", it, "param samples within 1e-3 lr: %.4f, max |dp| / lr %.3f" % (frac, d.max() / lr))
            if it == 0:
                assert frac >= 0.99 and d.max() <= 2.5 * lr, (frac, d.max() / lr)
            else:      # three updates of about lr each, after the divergence described above (measured: 6.0 lr)
                assert d.max() <= 2 * 3.5 * lr, (frac, d.max() / lr)


# ---- 3. fused / flat Adam against the torch.optim.Adam path they replace --------------------------------------------
# Both paths see bit-identical gradients in the first step (same kernels up to the optimiser), so the parameters after it
# agree to rounding.  Later steps are computed on weights that differ by rounding, and these tiny-batch steps amplify
# that (see test_adam_golden), so for three steps the fused optimiser is checked against torch.optim.Adam SHADOWING it:
# a copy of the parameters updated by torch from the gradients the fused step consumed (hipGraph replay included).
def _close(a, b, what, lr, steps):
    d = (a - b).abs()
    bound = 16 * EPS32 * torch.maximum(a.abs(), b.abs()) + 1e-5 * lr * steps
    bad = int((d > bound).sum())
    print(what, "max |dp| %.3e, elements beyond fp32 rounding: %d" % (float(d.max()), bad))
    assert bad == 0, (what, bad, float(d.max()))


def _flat_grad_views(opt, buf):
    return [buf[off:off + k].view(p.shape) for p, (off, k) in zip(opt._params, opt._spans)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fused_adam_equals_torch_adam_resnet(dtype):
    from instaorder_amd.optim import FusedAdam
    algo, seed, S, B, lr = "InstaOrderNet_od", 23, 64, 4, 1e-4
    first = []
    for fused in (True, False):
        m = _order_model(algo, seed, lr, 0.5, dtype, style="kaiming")
        params = list(m.net.parameters())
        if fused:
            assert isinstance(m.optim, FusedAdam)
            shadow = [p.detach().clone().requires_grad_() for p in params]
            sh = torch.optim.Adam(shadow, lr=lr, betas=(0.5, 0.999))
        else:
            m.optim = torch.optim.Adam(m.model.parameters(), lr=lr, betas=(0.5, 0.999))
        m.switch_to("train")
        for it in range(3 if fused else 1):
            _feed_order(m, algo, synthetic.make_pair_batch(seed + 300 + it, B, S))
            m.step()
            if fused:
                for q, p in zip(shadow, params):
                    q.grad = p.grad.detach().clone()
                sh.step()
            if it == 0:
                first.append(m.net.flat_params.clone())
        torch.cuda.synchronize()
        if fused:
            assert m._graph is not None         # steps 2 and 3: captured forward + backward, replayed
            st = m.optim.state_dict()["state"]
            assert len(st) == len(params) and all(float(s["step"]) == 3.0 for s in st.values())
            _close(torch.cat([p.detach().reshape(-1) for p in params]), torch.cat([q.detach().reshape(-1) for q in shadow]),
                   "ResNet %s, 3 steps vs torch.optim.Adam shadow" % dtype, lr, 3)
    _close(first[0], first[1], "ResNet %s, first step vs the torch.optim.Adam path" % dtype, lr, 1)


def _depth_model(seed, lr, beta1=0.5, dtype="fp32"):
    import instaorder_amd as ia
    torch.manual_seed(seed)
    cfg = dict(algo="InstaDepthNet_od", lr=lr, weight_decay=1e-4, optim="Adam", beta1=beta1, pretrained_weight=None,
               use_rgb=True, dtype=dtype, overlap_weight=0.1, distinct_weight=0.9, dorder_weight=1.0, smooth_weight=0.1,
               occ_order_weight=1.0)
    return ia.InstaDepthNet_od(cfg, dist_model=False)


def _feed_depth(m, seed, B, S):
    t = {k: torch.from_numpy(v.copy()) for k, v in synthetic.make_depth_batch(seed, B, S).items()}
    m.set_input(t["rgb"], t["modal1"], t["modal2"], t["depth_order"], t["count"], t["is_overlap"], t["occ_order"])


DEAD = "scratch.refinenet4.resConfUnit1.conv1.weight"     # single-input fusion block: never in the graph


def test_flat_adam_equals_torch_adam_midas():
    from instaorder_amd.optim import FlatAdam
    S, B, seed, lr = 64, 2, 31, 1e-4
    first, no_grad = [], []
    for flat in (True, False):
        m = _depth_model(seed, lr)
        names = [n for n, _ in m.net.named_parameters()]
        params = list(m.net.parameters())
        i = names.index(DEAD)
        dead0 = params[i].detach().clone()
        if flat:
            assert isinstance(m.optim, FlatAdam) and all(a is b for a, b in zip(m.optim._params, params))
            shadow = [p.detach().clone().requires_grad_() for p in params]
            sh = torch.optim.Adam(shadow, lr=lr, betas=(0.5, 0.999))
        else:
            m.optim = torch.optim.Adam(m.model.parameters(), lr=lr, betas=(0.5, 0.999))
        m.switch_to("train")
        for it in range(3 if flat else 1):
            _feed_depth(m, seed + 100 + it, B, S)
            m.step()
            if flat:
                for q, g, live in zip(shadow, _flat_grad_views(m.optim, m.optim.flat_grads), m.optim._live):
                    q.grad = g.detach().clone() if live else None
                sh.step()
                if it == 0:
                    no_grad.append([not live for live in m.optim._live])
            else:
                no_grad.append([p.grad is None for p in params])
            if it == 0:
                first.append(torch.cat([p.detach().reshape(-1) for p in params]))
        torch.cuda.synchronize()
        assert torch.equal(params[i].detach(), dead0)
        if flat:
            assert m._graph is not None and m._wplan and m._wplan.n > 150     # third step replayed, filters planned
            st = m.optim.state_dict()["state"]
            assert i not in st and float(st[0]["step"]) == 3.0 and m.optim._steps[i] == 0
            _close(torch.cat([p.detach().reshape(-1) for p in params]), torch.cat([q.detach().reshape(-1) for q in shadow]),
                   "InstaDepthNet_od, 3 steps vs torch.optim.Adam shadow", lr, 3)
        else:
            assert params[i] not in m.optim.state
    assert no_grad[0] == no_grad[1] and no_grad[0][i] and sum(no_grad[0]) < len(no_grad[0]) // 2
    _close(first[0], first[1], "InstaDepthNet_od, first step vs the torch.optim.Adam path", lr, 1)


# ---- 4. checkpoints and the learning-rate schedule -------------------------------------------------------------------
def test_adam_checkpoint_resume_equals_uninterrupted(tmp_path):
    algo, seed, S, B, lr = "InstaOrderNet_o", 27, 64, 4, 1e-3

    def run(m, its):
        m.switch_to("train")
        for it in its:
            _feed_order(m, algo, synthetic.make_pair_batch(seed + 400 + it, B, S))
            m.step()
        torch.cuda.synchronize()

    a = _order_model(algo, seed, lr, 0.5, style="kaiming")
    run(a, range(4))
    b = _order_model(algo, seed, lr, 0.5, style="kaiming")
    run(b, range(2))
    b.save_state(str(tmp_path), 2)
    c = _order_model(algo, seed + 1, lr, 0.5, style="kaiming")     # different weights: everything must come from the file
    c.load_state(str(tmp_path), 2, resume=True)
    assert c.optim._steps == [2] * len(c.optim._steps)
    run(c, range(2, 4))
    assert torch.equal(a.net.flat_params, c.net.flat_params)


def test_torch_adam_checkpoint_loads_into_fused_adam(tmp_path):
    """A checkpoint whose optimiser state torch.optim.Adam wrote (the path before this optimiser existed) resumes in
    FusedAdam: same parameters after the next step (step count 3) as torch.optim.Adam continuing from the same file."""
    from instaorder_amd.optim import FusedAdam
    algo, seed, S, B, lr = "InstaOrderNet_o", 29, 64, 4, 1e-3
    t = _order_model(algo, seed, lr, 0.5, style="kaiming")
    t.optim = torch.optim.Adam(t.model.parameters(), lr=lr, betas=(0.5, 0.999))
    t.switch_to("train")
    for it in range(2):
        _feed_order(t, algo, synthetic.make_pair_batch(seed + 600 + it, B, S))
        t.step()
    t.save_state(str(tmp_path), 2)
    ends = []
    for fused in (True, False):
        m = _order_model(algo, seed + 1, lr, 0.5, style="kaiming")
        if not fused:
            m.optim = torch.optim.Adam(m.model.parameters(), lr=lr, betas=(0.5, 0.999))
        m.load_state(str(tmp_path), 2, resume=True)
        if fused:
            assert isinstance(m.optim, FusedAdam) and m.optim._steps[0] == 2
        m.switch_to("train")
        _feed_order(m, algo, synthetic.make_pair_batch(seed + 602, B, S))
        m.step()
        torch.cuda.synchronize()
        ends.append(m.net.flat_params.clone())
    _close(ends[0], ends[1], "resumed from a torch.optim.Adam checkpoint", lr, 3)


def test_scheduler_lr_and_gradient_less_steps_reach_the_kernel():
    """StepLRScheduler rewrites param_groups[0]['lr'] between steps and FlatAdam's launches use it; parameters without a
    gradient in a step keep value, moments and step count (per-parameter step counts then differ, as in torch)."""
    from instaorder_amd.optim import FlatAdam
    from instaorder_amd.scheduler import StepLRScheduler
    torch.manual_seed(5)
    mods = [nn.Sequential(nn.Linear(33, 17), nn.Linear(17, 9), nn.Linear(9, 5)).to(DEV) for _ in range(2)]
    mods[1].load_state_dict(mods[0].state_dict())
    opts = [FlatAdam(mods[0], lr=1e-2, betas=(0.5, 0.999)),
            torch.optim.Adam(mods[1].parameters(), lr=1e-2, betas=(0.5, 0.999), foreach=False)]
    scheds = [StepLRScheduler(o, [2, 4], [0.1, 0.5], 1e-2, [], []) for o in opts]
    for it in range(6):
        grads = [torch.randn_like(p) for p in mods[0].parameters()]
        for mod, opt, sch in zip(mods, opts, scheds):
            sch.step(it)
            for j, (p, gr) in enumerate(zip(mod.parameters(), grads)):
                p.grad = None if (j // 2 == 1 and it in (1, 2)) or (j // 2 == 2 and it == 0) else gr.clone()
            opt.step()
        assert opts[0].param_groups[0]["lr"] == opts[1].param_groups[0]["lr"]
    torch.cuda.synchronize()
    assert opts[0]._steps == [6, 6, 4, 4, 5, 5]
    for a, b in zip(mods[0].parameters(), mods[1].parameters()):
        _close(a.detach(), b.detach(), "scheduled Adam", 1e-2, 6)
    sd = opts[0].state_dict()["state"]
    for i, p in enumerate(mods[1].parameters()):
        assert float(sd[i]["step"]) == float(opts[1].state[p]["step"])
        _close(sd[i]["exp_avg"], opts[1].state[p]["exp_avg"], "exp_avg", 0.0, 1)
