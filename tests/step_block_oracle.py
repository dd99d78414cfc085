"""A teacher-forced fp64 oracle of the ResNet-50 training step, unit by unit (test-only, plain torch on the CPU).

The step under test keeps the stem conv output, the max-pool output and every Bottleneck output in its workspace
(io_net_activation_offset).  `run` recomputes each unit -- stem conv, bn1 + relu + max-pool, each Bottleneck, avgpool +
heads -- in float64 FROM THE STORED INPUT of that unit, so a forward error stays in the unit that made it instead of
growing ~1.2x per block.  The backward is one autograd graph in which block i's input VALUE is the stored tensor while
its gradient flows on to block i-1's computed output (x_i = prev + (stored - prev).detach()); the ReLU mask of a block
output is taken from the stored output (what the kernels use, as a tensor or as bits), the inner masks from the
recomputation (where that cannot decide one within fp32 rounding, resolve_undecided takes an fp32 step's own decision).  BatchNorm uses batch statistics over G contiguous sample groups and updates the running estimates once per
group in group order (oracle/resnet_oracle.py: two calls on the two halves of a pair batch); strides and the downsample
branch are those of resnet_cls.py (stride on the 3x3, downsample on the first block of every layer).

Without `stored` the same code is a free-running step; with `rnd` it rounds every tensor the bf16 plan stores (y1, a1,
y2, a2, y3, yd, block / stem / pool outputs) on the way forward and the gradient crossing it on the way back, parameters,
statistics, pooled features and logits staying exact.  As in the step, a convolution reads its filter as a GEMM operand of
the storage type (the fp32 master cast once per forward; the filter GRADIENT is an fp32 sum) and its BatchNorm statistics
are those of its fp32 accumulators or of the rounded tensor it stored, by route (both are emulated).  That emulated run
exists only to measure the noise floor `ec` of the comparison (floors / bar below); `fault` builds one named defect into
one block, for the tests that show the bars are not vacuous.  tests/test_step_blocks_cpu.py holds all of this to
oracle/resnet_oracle.py."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

LAYERS = (3, 4, 6, 3)
BLOCKS = [(li, bi) for li, n in enumerate(LAYERS) for bi in range(n)]      # 16 x (layer, index in layer)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
NUNITS = 19                                  # stem conv, pool, 16 blocks, logits: the order of `stored`
UNIT_NAMES = ["stem", "pool"] + ["layer%d.%d" % (li + 1, bi) for li, bi in BLOCKS] + ["logits"]

# (dtype, N, S, G, io_set_bf16_p256 mode, io_set_bf16_p256_xop) of tests/test_gpu_step_blocks.py; fp32 takes neither switch
# (left at the defaults).  tests/test_step_blocks_cpu.py asserts that on 256 CUs this list reaches every route.
CASES = [("fp32", 3, 96, 1, 1, 1), ("fp32", 8, 64, 1, 1, 1), ("fp32", 8, 64, 2, 1, 1), ("fp32", 32, 64, 1, 1, 1),
         ("bf16", 3, 96, 1, 1, 1), ("bf16", 4, 64, 1, 0, 0), ("bf16", 4, 64, 1, 1, 1), ("bf16", 4, 64, 1, 3, 1),
         ("bf16", 4, 64, 2, 3, 1), ("bf16", 16, 64, 1, 3, 1), ("bf16", 16, 64, 2, 3, 1), ("bf16", 16, 64, 1, 3, 0),
         ("bf16", 64, 64, 1, 3, 1)]
CASE_NCU = 256


def case_id(case):
    return "%s-n%d-s%d-g%d-p256_%d-xop%d" % case


# ---- bars ----------------------------------------------------------------------------------------------------------
# floors of the existing suite (tests/test_gpu_bf16.py): one bf16 output rounding; fp32 tensors and fp32-accumulated sums
# (parameter gradients, BatchNorm running estimates); logits
FLOOR_BF16, FLOOR_F32, FLOOR_LOGITS = 6e-3, 2e-5, 1e-5
FACTOR = 3.0                                 # tests/test_gpu_net.py: e < max(1e-3, 3 * ec)


# An inner pre-activation z = (y - mean) * s + beta, s = gamma * rstd, of an fp32 step: y is an fp32 sum of products (a
# few roundings of relative size 2^-24 against sum |x||w|, stored rounded once more), mean * s and beta meet in the shift
# table (one rounding each) and the multiply-add rounds once: |dz| <~ 2^-24 (s (sum |x||w| + |mean|) + |beta|) per
# rounding; 8 of them is the bound inside which the sign of z counts as undecided.
UNDECIDED = 8 * 2.0 ** -24


def floor_fwd(dtype, unit):
    """floor of the forward error of unit 0 .. 18 (18 = logits, fp32 in either dtype)"""
    if unit == NUNITS - 1:
        return FLOOR_LOGITS
    return FLOOR_BF16 if dtype == "bf16" else FLOOR_F32


def bar(ec, floor):
    """the bar of a unit / tensor whose reference noise floor is `ec`: fused routes round less often than the emulation,
    never more, so a correct kernel sits at or below ec"""
    return FACTOR * ec + floor


def round_fn(dtype):
    if dtype == "bf16":
        return lambda t: t.float().bfloat16().double()
    return lambda t: t.float().double()


class _RoundBoth(torch.autograd.Function):
    """rounds the tensor on the way forward and the gradient that crosses it on the way back"""

    @staticmethod
    def forward(ctx, t, rnd):
        ctx.rnd = rnd
        return rnd(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.rnd(g), None


def _store(t, rnd):
    return t if rnd is None else _RoundBoth.apply(t, rnd)


def _operand(w, rnd):
    """a filter as the GEMM reads it: the fp32 master cast to the storage type (io_filter_prepare; the whole flat buffer
    once per bf16 forward), its gradient accumulated in fp32 and left alone"""
    return w if rnd is None else w + (rnd(w.detach()) - w.detach())


# ---- errors --------------------------------------------------------------------------------------------------------
def err_max(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def err_l2(got, ref):
    return float((got.double() - ref).norm()) / max(float(ref.norm()), 1e-300)


# ---- the step ------------------------------------------------------------------------------------------------------
def state64(sd, prefix=""):
    """state dict (ndarray or tensor values) -> OrderedDict name -> float64 tensor (counters dropped)"""
    out = OrderedDict()
    for k, v in sd.items():
        if k.startswith(prefix):
            k = k[len(prefix):]
        if k.endswith("num_batches_tracked"):
            continue
        out[k] = torch.as_tensor(v).detach().double().clone()
    return out


def param_names(state):
    return [k for k in state if not (k.endswith("running_mean") or k.endswith("running_var"))]


def block_of(name):
    """parameter / buffer name -> unit index whose computation owns it (0 stem conv, 1 bn1, 2 + i block i, 18 heads)"""
    if name.startswith("conv1."):
        return 0
    if name.startswith("bn1."):
        return 1
    if name.startswith("layer"):
        li, bi = int(name[5]) - 1, int(name.split(".")[1])
        return 2 + BLOCKS.index((li, bi))
    return NUNITS - 1


class _Step(object):
    def __init__(self, state, G, rnd, fault, acc_stats=True, track=False, toggle=None):
        self.acc_stats = acc_stats
        self.track, self.toggle, self.inner = track, toggle or {}, OrderedDict()
        self.w = {k: state[k].clone().requires_grad_(True) for k in param_names(state)}
        self.running = {k: state[k].clone() for k in state if k not in self.w}
        self.G, self.rnd, self.fault = G, rnd, fault

    def conv(self, x, name, **kw):
        return F.conv2d(x, _operand(self.w[name], self.rnd), **kw)

    def bn(self, x, name, swap_groups=False, unmasked_gamma=None, stats_of=None):
        """batch statistics over G contiguous sample groups; running estimates once per group, in group order.
        stats_of: the convolution output before it was rounded for storage.  The step has both forms: a convolution with
        the BatchNorm-statistics epilogue reduces its fp32 accumulators (acc_stats), a statistics pass of its own reads the
        rounded tensor it finds in memory"""
        N, C, H, W = x.shape
        G = self.G
        xg = x.reshape(G, N // G, C, H, W)
        sg = xg if (stats_of is None or not self.acc_stats) else stats_of.reshape(G, N // G, C, H, W)
        mean = sg.mean(dim=(1, 3, 4), keepdim=True)
        var = ((sg - mean) ** 2).mean(dim=(1, 3, 4), keepdim=True)
        n = (N // G) * H * W
        rm, rv = self.running[name + ".running_mean"], self.running[name + ".running_var"]
        for g in range(G):
            rm.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean[g].detach().reshape(C))
            rv.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * var[g].detach().reshape(C) * (n / max(n - 1, 1)))
        if swap_groups:                          # fault: group 1's statistics used for group 0
            mean = torch.cat([mean[1:2], mean[1:]], 0)
            var = torch.cat([var[1:2], var[1:]], 0)
        xhat = ((xg - mean) / torch.sqrt(var + BN_EPS)).reshape(N, C, H, W)
        w, b = self.w[name + ".weight"].view(1, C, 1, 1), self.w[name + ".bias"].view(1, C, 1, 1)
        if unmasked_gamma is not None:           # fault: see bottleneck
            unmasked_gamma.append(xhat.detach() * (w - w.detach()))
            w = w.detach()
        self.last_stats = (mean.detach(), 1.0 / torch.sqrt(var.detach() + BN_EPS))
        return xhat * w + b

    def inner_relu(self, pre, name, x, wname, **kw):
        """relu of an inner BatchNorm output `pre` = bn(conv(x, w[wname])) (bn1 / bn2, the stem's bn1): its mask is the
        recomputation's own.  track: also finds the elements whose sign fp32 arithmetic cannot decide (UNDECIDED below) and
        keeps the activation, so that run() can return the gradient arriving at them; toggle[name]: flat indices whose
        mask is taken the other way"""
        mask = pre.detach() > 0
        if name in self.toggle and len(self.toggle[name]):
            mask.view(-1)[self.toggle[name]] ^= True
        a = pre * mask.to(pre.dtype)
        if self.track:
            N, C, H, W = pre.shape
            G = self.G
            mean, rstd = self.last_stats
            s = self.w[name + ".weight"].detach().abs().view(1, 1, C, 1, 1) * rstd
            amp = F.conv2d(x.detach().abs(), self.w[wname].detach().abs(), **kw).reshape(G, N // G, C, H, W)
            tau = UNDECIDED * (s * (amp + mean.abs()) + self.w[name + ".bias"].detach().abs().view(1, 1, C, 1, 1))
            idx = (pre.detach().abs() < tau.reshape(N, C, H, W)).flatten().nonzero().flatten()
            self.inner[name] = (a, idx, (idx // (H * W)) % C, mask.flatten()[idx])
        return a

    def bottleneck(self, i, x, stored_out):
        li, bi = BLOCKS[i]
        p = "layer%d.%d" % (li + 1, bi)
        stride = 2 if (bi == 0 and li > 0) else 1
        rnd, w = self.rnd, self.w
        fault = self.fault[0] if self.fault is not None and self.fault[1] == i else None
        y1 = self.conv(x, p + ".conv1.weight")
        a1 = _store(self.inner_relu(self.bn(_store(y1, rnd), p + ".bn1", stats_of=y1), p + ".bn1", x, p + ".conv1.weight"),
                    rnd)
        y2 = self.conv(a1, p + ".conv2.weight", stride=stride, padding=1)
        a2 = _store(self.inner_relu(self.bn(_store(y2, rnd), p + ".bn2", stats_of=y2), p + ".bn2", a1,
                                    p + ".conv2.weight", stride=stride, padding=1), rnd)
        y3 = self.conv(a2, p + ".conv3.weight")
        extra = [] if fault == "dgamma3_unmasked" else None
        z3 = self.bn(_store(y3, rnd), p + ".bn3", swap_groups=fault == "swap_group_stats", unmasked_gamma=extra,
                     stats_of=y3)
        xi = x.detach() if fault == "drop_residual_grad" else x
        if bi == 0:
            yd = self.conv(xi, p + ".downsample.0.weight", stride=stride)
            idt = self.bn(_store(yd, rnd), p + ".downsample.1", stats_of=yd)
        else:
            idt = xi
        pre = z3 if fault == "no_identity" else z3 + idt
        ref = pre.detach() if fault == "no_relu" else F.relu(pre).detach()
        # the mask of the backward: the stored output's (teacher forcing), else the recomputation's own
        mask = (stored_out > 0) if stored_out is not None else (pre.detach() > 0)
        if fault == "shift_mask":
            mask = torch.roll(mask, 1, dims=1)
        out = pre * mask.to(pre.dtype)
        if fault == "no_relu" and stored_out is None:
            out = pre
        if extra:
            out = out + extra[0]                 # value 0; gives bn3.weight the gradient sum without the mask
        return out, ref


def run(state, x, dlogits, G, stored=None, rnd=None, fault=None, backward=True, acc_stats=True, track=False, toggle=None):
    """One training step in float64.

    state: name -> float64 tensor (state64); x[N,C,S,S] the network input as the step sees it (the packed x8, real
    channels); dlogits[N,K]; stored: None (free run) or the NUNITS kept tensors, NCHW float64, in the order stem conv,
    pool, 16 block outputs, logits; rnd: None or round_fn(dtype); fault: None or (name, block index); acc_stats: which of
    the two statistics forms the emulation takes (see _Step.bn; no effect without rnd); track / toggle: see
    resolve_undecided.
    -> dict(ref = the NUNITS unit outputs recomputed from the unit's (stored) input, acts = what this run would store (ref
    after rounding), grads = name -> gradient, running = name -> running estimate after the step; with track also
    undecided = BatchNorm name -> (flat indices, their channels, the oracle's mask there, the gradient arriving there))"""
    st = _Step(state, G, rnd, fault, acc_stats, track, toggle)
    w = st.w
    refs, acts = [], []

    def unit(out, ref=None):
        """records the unit's output, hands on the next unit's input: the stored value, the computed gradient path"""
        refs.append((out if ref is None else ref).detach())
        acts.append(refs[-1] if rnd is None else rnd(refs[-1]))
        out = _store(out, rnd)
        if stored is None:
            return out
        return out + (stored[len(refs) - 1] - out).detach()

    y0 = st.conv(x, "conv1.weight", stride=2, padding=3)
    h = unit(y0)
    h = unit(F.max_pool2d(st.inner_relu(st.bn(h, "bn1", stats_of=y0 if stored is None else None), "bn1", x,
                                        "conv1.weight", stride=2, padding=3), kernel_size=3, stride=2, padding=1))
    for i in range(len(BLOCKS)):
        out, ref = st.bottleneck(i, h, None if stored is None else stored[2 + i])
        h = unit(out, ref)
    feat = torch.flatten(F.adaptive_avg_pool2d(h, 1), 1)
    if "fc_occ.weight" in w:
        logits = torch.cat([F.linear(feat, w["fc_occ.weight"], w["fc_occ.bias"]),
                            F.linear(feat, w["fc_depth.weight"], w["fc_depth.bias"])], 1)
    else:
        logits = F.linear(feat, w["fc.weight"], w["fc.bias"])
    refs.append(logits.detach())
    acts.append(logits.detach())
    res = dict(ref=refs, acts=acts, running=st.running, grads=None)
    if backward:
        names = list(w)
        inner = list(st.inner.items())
        gl = torch.autograd.grad(logits, [w[k] for k in names] + [v[0] for _, v in inner], dlogits)
        res["grads"] = OrderedDict((k, g.detach()) for k, g in zip(names, gl))
        res["undecided"] = OrderedDict((k, (idx, ch, m, g.flatten()[idx])) for (k, (_, idx, ch, m)), g
                                       in zip(inner, gl[len(names):]))
        if fault is not None and fault[0] == "wgrad_over_G":     # one stage's filter gradients scaled by 1 / G
            li = BLOCKS[fault[1]][0]
            for k in names:
                if k.startswith("layer%d." % (li + 1)) and (".conv" in k or "downsample.0" in k):
                    res["grads"][k] = res["grads"][k] / G
    return res


# ---- comparing a step (the kernels', the emulation's, a faulty one's) with the oracle on ITS stored tensors ------------
def errors(got_acts, got_grads, got_running, oracle):
    """-> (fwd[NUNITS] max-norm relative, grads name -> L2 relative, running name -> max-norm relative); any of the
    three inputs may be None"""
    fwd = None if got_acts is None else [err_max(a, r) for a, r in zip(got_acts, oracle["ref"])]
    grads = None if got_grads is None else OrderedDict((k, err_l2(got_grads[k], r)) for k, r in oracle["grads"].items())
    running = None if got_running is None else OrderedDict((k, err_max(got_running[k], r))
                                                           for k, r in oracle["running"].items())
    return fwd, grads, running


def resolve_undecided(oracle, got_grads, rerun):
    """The inner masks are the recomputation's own, and where |bn(y)| lies within fp32 rounding of zero (UNDECIDED) either
    sign is a correct fp32 result: the oracle cannot know which one an fp32 step took, and one such element moves every
    gradient upstream of it by ~1e-3.  It can read the decision off the step's own output, as it reads the block-output
    masks off the stored outputs: the gradient of that BatchNorm's bias is the sum of the masked incoming gradient over the
    channel, so taking element u the other way changes it by exactly +-g_u, the gradient arriving at u (which the oracle
    has).  Per BatchNorm and channel with undecided elements, the subset whose toggling brings the oracle's bias gradient
    closest to got_grads' is toggled; rerun(toggle) is the oracle with those masks.  The BatchNorms are visited in the
    order of the backward pass and the oracle is rerun after each that toggled, so a decision is never read through the
    ~1e-3 a decision behind it would add.  Nothing else is read from got_grads, and no element outside the fp32 rounding
    bound can be toggled.
    -> (oracle, number of undecided elements, number toggled)"""
    toggle = {}
    nund = sum(len(v[0]) for v in oracle["undecided"].values())
    for name in reversed(list(oracle["undecided"])):
        idx, ch, mask, g = oracle["undecided"][name]
        if not len(idx):
            continue
        diff = got_grads[name + ".bias"].double() - oracle["grads"][name + ".bias"]
        delta = torch.where(mask, -g, g)                       # effect on the bias gradient of toggling the element
        picked = []
        for c in ch.unique().tolist():
            sel = (ch == c).nonzero().flatten()[:12].tolist()  # (12: a bound on the enumeration; a channel has 0 or 1)
            best, best_set = abs(float(diff[c])), []
            for bits in range(1, 1 << len(sel)):
                sub = [u for j, u in enumerate(sel) if bits >> j & 1]
                e = abs(float(diff[c]) - float(delta[sub].sum()))
                if e < best:
                    best, best_set = e, sub
            picked += best_set
        if picked:
            toggle[name] = idx[picked]
            oracle = rerun(dict(toggle))
    return oracle, nund, sum(len(v) for v in toggle.values())


def noise_floor(state, x, dlogits, G, dtype):
    """ec of every unit, parameter gradient and running estimate: the emulated step in `dtype` held to the exact oracle
    on the emulation's own stored tensors -- the code under test plays no part in it.  Which of the two statistics forms
    a BatchNorm of the step takes is a matter of its route, so the floor is the larger of the two emulations'."""
    out = None
    for acc_stats in (True, False):
        emu = run(state, x, dlogits, G, rnd=round_fn(dtype), acc_stats=acc_stats)
        exact = run(state, x, dlogits, G, stored=emu["acts"])
        f, g, r = errors(emu["acts"], emu["grads"], emu["running"], exact)
        if out is None:
            out = (f, g, r)
        else:
            out = ([max(a, b) for a, b in zip(out[0], f)], OrderedDict((k, max(v, g[k])) for k, v in out[1].items()),
                   OrderedDict((k, max(v, r[k])) for k, v in out[2].items()))
    return out


def worst_ratio(err, ec, floor_of):
    """-> (max err / bar, key, err, bar) over a list or dict of errors; floor_of(key) -> floor"""
    keys = range(len(err)) if isinstance(err, list) else list(err)
    worst = (0.0, None, 0.0, 0.0)
    for k in keys:
        b = bar(ec[k], floor_of(k))
        if err[k] / b > worst[0] or not err[k] == err[k]:
            worst = (err[k] / b if err[k] == err[k] else float("inf"), k, err[k], b)
    return worst
