"""Fused momentum-SGD over the network's flat parameter buffer.

Behaves as ``torch.optim.SGD(model.parameters(), lr, momentum=0.9, weight_decay=wd)`` does in the
reference (models/single_stage_model.py:35-38): ONE parameter group (BN affine terms and biases are
decayed too), coupled L2, dampening 0, no Nesterov, momentum buffer = first decayed gradient.  It IS
a ``torch.optim.Optimizer`` (utils/scheduler.py:7-9 type-checks it and rewrites
``param_groups[i]['lr']``), and its ``state_dict`` has torch.optim.SGD's layout (one
``momentum_buffer`` per parameter) so checkpoints interchange with the reference
(single_stage_model.py:66-72).  The update itself is one HIP launch over 23.5 M floats.

FusedAdam / FlatAdam do the same for ``optim: Adam`` (single_stage_model.py:39-42, torch.optim.Adam with
betas=(beta1, 0.999)) over the same two flat layouts: torch.optim.Adam's state_dict layout, per-parameter step counts,
parameters without a gradient skipped as torch skips them.

All four take ``max_grad_norm`` (default None: off, everything as without it): global-norm gradient clipping with a
non-finite step guard (_GradClip below; DESIGN.md "Gradient clipping and the non-finite guard").
"""
import math

import torch

from . import engine


def _check_max_grad_norm(v):
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or not v > 0:
        raise ValueError("max_grad_norm must be a positive number or float('inf') (None: no clipping), got %r" % (v,))
    return float(v)


class _GradClip(object):
    """Global-norm clipping of the flat gradient buffer and the non-finite guard, mixed into the four flat optimisers.

    With ``max_grad_norm`` set, ``step()`` first runs io_grad_norm over ``flat_grads`` (fp64 sums of squares per segment
    and in total, two launches, no host synchronisation) and then the clipped update, which reads the device record
    io_grad_norm left: gradients scaled by coef = min(1, max_grad_norm / (norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s
    arithmetic -- or, when the norm is inf / NaN, NO update at all (parameters and optimiser state keep their bits, the
    record's ``skipped`` count goes up).  ``float('inf')`` measures and guards without ever scaling.

    ``step()`` is what the model wrappers call AFTER the data-parallel gradient exchange (every path of _OrderBase.step /
    _DepthBase.step, the staged ones after their last bucket has arrived), so the clip acts on the summed gradient, the
    same on every rank.  The norm is defined over parameter elements: the storage padding of the flat buffers (the stem
    filter's channels 5..7, the 64-float span padding of _FlatLayout) holds zero gradients and contributes nothing.

    The setting is an attribute, not a param-group key: state_dict() stays in torch's layout and checkpoints written with
    and without clipping interchange.  Known limit: on a skipped step Adam's host-side per-parameter step counts still
    advance (keeping them would need a host synchronisation); moments and parameters do not change."""

    def _clip_init(self, max_grad_norm):
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        self._seg_names = ("all",)
        self._seg_offsets = None        # None: one segment over the whole buffer
        self._clip_bufs = None          # (state record, fp64 segment sums, workspace)

    def set_grad_segments(self, slices, names=None):
        """``slices``: [lo, hi) float ranges that tile the flat gradient buffer (any order, e.g. the backward stages of
        grad_stage_slices(); at most 16, boundaries multiples of 4); grad_stats() reports one norm per range under
        ``names``."""
        slices = [(int(lo), int(hi)) for lo, hi in slices]
        names = tuple(names) if names is not None else tuple("stage%d" % i for i in range(len(slices)))
        if not 1 <= len(slices) <= 16 or len(names) != len(slices) or len(set(names)) != len(names):
            raise ValueError("gradient segments: 1..16 ranges with one distinct name each")
        order = sorted(range(len(slices)), key=lambda i: slices[i])
        offs = [slices[order[0]][0]]
        for i in order:
            lo, hi = slices[i]
            if lo != offs[-1] or hi < lo or lo % 4 or hi % 4:
                raise ValueError("gradient segments must tile the buffer with boundaries that are multiples of 4: %r"
                                 % (slices,))
            offs.append(hi)
        if offs[0] != 0:
            raise ValueError("gradient segments must start at 0: %r" % (slices,))
        self._seg_offsets = offs
        self._seg_names = tuple(names[i] for i in order)
        self._clip_bufs = None

    def _clip_buffers(self, flat_grads):
        n = flat_grads.numel()
        offs = self._seg_offsets if self._seg_offsets is not None else [0, n]
        if offs[-1] != n:
            raise ValueError("gradient segments end at %d, the flat gradient buffer has %d floats" % (offs[-1], n))
        b = self._clip_bufs
        if b is None or b[0].device != flat_grads.device:
            dev = flat_grads.device
            state = engine.new_clip_state(dev)
            if b is not None:
                state.copy_(b[0])       # the counters move with the model
            b = (state, torch.zeros(len(offs) - 1, dtype=torch.float64, device=dev),
                 torch.empty(max(8, engine.grad_norm_workspace_bytes(n, len(offs) - 1)), dtype=torch.uint8, device=dev))
            self._clip_bufs = b
        return offs, b

    def _measure(self, flat_grads):
        """io_grad_norm over the flat gradients when clipping is on; returns the device record (None: clipping off)"""
        max_norm = _check_max_grad_norm(getattr(self, "max_grad_norm", None))
        if max_norm is None:
            return None
        offs, (state, seg, ws) = self._clip_buffers(flat_grads)
        engine.grad_norm(flat_grads, max_norm, state, offs, ws, seg)
        return state

    @property
    def clip_state(self):
        """The io_clip_state record on the device (64 bytes, uint8; engine.read_clip_state decodes it); no
        synchronisation.  None while clipping is off or before the first step."""
        return self._clip_bufs[0] if self._clip_bufs is not None else None

    def grad_stats(self):
        """What the last step measured (synchronises): norm, coef, nonfinite, the cumulative steps / clipped / skipped
        counts, and stage_norms {segment name: norm of that slice of the flat gradient buffer}."""
        if self._clip_bufs is None:
            raise RuntimeError("grad_stats(): no clipped step has run (max_grad_norm=%r)" % (self.max_grad_norm,))
        state, seg, _ = self._clip_bufs
        out = engine.read_clip_state(state)
        sums = seg.cpu().tolist()
        out["stage_norms"] = {name: math.sqrt(v) if v >= 0 else float("nan") for name, v in zip(self._seg_names, sums)}
        return out


class FusedSGD(_GradClip, torch.optim.Optimizer):
    def __init__(self, module, lr, momentum=0.9, weight_decay=0.0, max_grad_norm=None):
        self._clip_init(max_grad_norm)
        net = getattr(module, "module", module)     # DistModule / FixModule wrap the ResNet
        if not hasattr(net, "flat_params"):
            raise TypeError("FusedSGD needs an instaorder_amd ResNet (flat parameter buffer)")
        self._net = net
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False)
        super(FusedSGD, self).__init__(list(net.parameters()), defaults)
        if len(self.param_groups) != 1:
            raise ValueError("FusedSGD supports exactly one parameter group")
        self._buf = None
        self._views = None

    def _ensure_buf(self):
        flat = self._net.flat_params
        if self._buf is None or self._buf.device != flat.device:
            old = self._buf
            self._buf = torch.zeros_like(flat)
            if old is not None:
                self._buf.copy_(old)
            self._views = [self._net._view(self._buf, t) for t, _ in self._net._param_list]
        return self._buf

    def zero_grad(self, set_to_none=True):
        # gradients are rewritten in full by every backward of the engine; nothing to clear
        for p in self.param_groups[0]["params"]:
            if set_to_none:
                p.grad = None

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        if g.get("nesterov") or g.get("dampening", 0) != 0:
            raise ValueError("FusedSGD: nesterov / dampening are not supported")
        buf = self._ensure_buf()
        engine.sgd_momentum(self._net.flat_params, self._net.flat_grads, buf, g["lr"], g["momentum"],
                            g["weight_decay"], clip_state=self._measure(self._net.flat_grads))
        return None

    # ---- checkpoint interchange with torch.optim.SGD ------------------------------------------------
    def state_dict(self):
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        n = len(self.param_groups[0]["params"])
        group["params"] = list(range(n))
        state = {}
        if self._buf is not None:
            for i, v in enumerate(self._views):
                state[i] = {"momentum_buffer": v.detach().clone().contiguous()}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        grp = sd["param_groups"][0]
        for k, v in grp.items():
            if k != "params":
                self.param_groups[0][k] = v
        if sd["state"]:
            self._ensure_buf()
            with torch.no_grad():
                self._buf.zero_()
                for i, st in sd["state"].items():
                    mb = st.get("momentum_buffer")
                    if mb is not None:
                        self._views[int(i)].copy_(mb)


def _trainable(module):
    params = []
    seen = set()
    for p in module.parameters():
        if id(p) not in seen and p.requires_grad:
            seen.add(id(p))
            params.append(p)
    return params


class _FlatLayout(torch.optim.Optimizer):
    """An ordinary module tree (the MiDaS branch) moved into ONE flat fp32 buffer: each ``nn.Parameter`` becomes a view
    of it (spans padded to 64 floats), so an optimiser update is one HIP launch; the gradients autograd produced per
    tensor are gathered into a flat buffer first (that buffer is also what the data-parallel all-reduce runs on)."""

    def __init__(self, params, defaults):
        super(_FlatLayout, self).__init__(params, defaults)
        self._params = params
        n = sum(((p.numel() + 63) // 64) * 64 for p in params)
        dev = params[0].device
        self.flat_params = torch.zeros(n, device=dev)
        self.flat_grads = torch.zeros(n, device=dev)
        self._spans = []
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                self.flat_params[off:off + k].copy_(p.reshape(-1))
                p.data = self.flat_params[off:off + k].view(p.shape)
                self._spans.append((off, k))
                off += ((k + 63) // 64) * 64

    def gather_grads(self, skip=None, prezeroed=False):
        """Per-tensor autograd gradients -> the flat gradient buffer (missing gradients count as zero).  ``skip``: ids of
        parameters whose slice somebody else fills (ops.WeightPlan: filters unpacked right afterwards, BatchNorm gradients
        written in place by their kernels).  ``prezeroed``: the buffer was cleared before the backward pass (WeightPlan.prepare):
        gradient-less parameters need no fill of their own."""
        with torch.no_grad():
            dst, src = [], []
            for p, (off, k) in zip(self._params, self._spans):
                if p.grad is None:
                    if not prezeroed and (skip is None or id(p) not in skip):
                        self.flat_grads[off:off + k].zero_()
                else:
                    dst.append(self.flat_grads[off:off + k].view(p.shape))
                    src.append(p.grad)
            if dst:
                # one multi-tensor copy instead of a launch per parameter (680 tensors in InstaDepthNet_od)
                torch._foreach_copy_(dst, src)
        return self.flat_grads

    def gather_stage(self, idx, grads, skip=None, attach=False, prezeroed=False):
        """The gradients of the parameters ``idx`` (indices into the flat layout, one stage of a staged backward pass) ->
        their slices of the flat gradient buffer; ``grads``: what torch.autograd.grad returned for them (None = no
        gradient: zeros, unless the parameter is in ``skip`` -- ops.WeightPlan fills those).  attach: ``p.grad`` = the view."""
        with torch.no_grad():
            dst, src = [], []
            for i, g in zip(idx, grads):
                p = self._params[i]
                off, k = self._spans[i]
                view = self.flat_grads[off:off + k].view(p.shape)
                if g is None:
                    if not prezeroed and (skip is None or id(p) not in skip):
                        view.zero_()
                else:
                    dst.append(view)
                    src.append(g)
                if attach:
                    p.grad = view
            if dst:
                torch._foreach_copy_(dst, src)

    def offset_of(self, param):
        for p, (off, _) in zip(self._params, self._spans):
            if p is param:
                return off
        raise KeyError("parameter is not in the flat buffer")


class FlatSGD(_GradClip, _FlatLayout):
    """Momentum-SGD over the flat layout of _FlatLayout: the update is the same single HIP launch as FusedSGD.
    torch.optim.SGD semantics / state_dict layout as above."""

    def __init__(self, module, lr, momentum=0.9, weight_decay=0.0, max_grad_norm=None):
        self._clip_init(max_grad_norm)
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False)
        super(FlatSGD, self).__init__(_trainable(module), defaults)
        self._buf = torch.zeros_like(self.flat_params)

    @torch.no_grad()
    def step(self, closure=None, gathered=False):
        g = self.param_groups[0]
        if not gathered:
            self.gather_grads()
        engine.sgd_momentum(self.flat_params, self.flat_grads, self._buf, g["lr"], g["momentum"], g["weight_decay"],
                            clip_state=self._measure(self.flat_grads))
        from . import ops
        ops.WEIGHTS_EPOCH[0] += 1          # parameters changed in place, invisibly to torch's version counters
        return None

    def state_dict(self):
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._params)))
        state = {i: {"momentum_buffer": self._buf[off:off + k].view(p.shape).detach().clone()}
                 for i, (p, (off, k)) in enumerate(zip(self._params, self._spans))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        for k, v in sd["param_groups"][0].items():
            if k != "params":
                self.param_groups[0][k] = v
        with torch.no_grad():
            for i, st in sd["state"].items():
                mb = st.get("momentum_buffer")
                if mb is not None:
                    off, k = self._spans[int(i)]
                    self._buf[off:off + k].copy_(mb.reshape(-1))


# ---- Adam ----------------------------------------------------------------------------------------------------------
# param-group keys torch.optim.Adam may carry that change nothing here, and those that must keep torch's default
_ADAM_INERT = ("foreach", "fused", "capturable", "differentiable", "initial_lr")
_ADAM_OFF = ("amsgrad", "maximize", "decoupled_weight_decay")


def _adam_defaults(lr, betas, eps, weight_decay):
    """The installed torch's Adam param group (same key set as its state_dict writes), with these hyper-parameters;
    torch's own constructor validates them."""
    probe = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=lr, betas=betas, eps=eps,
                             weight_decay=weight_decay)
    return {k: v for k, v in probe.param_groups[0].items() if k != "params"}


class _AdamFlat(_GradClip):
    """torch.optim.Adam (amsgrad / maximize off, coupled L2) over a flat fp32 parameter buffer; mixed into a
    torch.optim.Optimizer.  The subclass provides ``_params`` (group order), ``_begin[i]`` (float offset of parameter i's
    storage, 16-byte aligned, increasing with i), ``_flat()`` -> (params, grads) and ``_state_view(buf, i)``.

    State per parameter as torch keeps it: ``step`` (an int here), ``exp_avg`` / ``exp_avg_sq`` (slices of two flat
    buffers).  A parameter without a gradient in a step (``_live[i]`` False) is skipped: value, moments and step count
    stay, and it has no state entry before its first gradient.  The launches cover runs of consecutive parameters that
    take the update with one step count; a parameter that never had a gradient joins any run when weight_decay is 0 --
    its gradient slice, exp_avg and exp_avg_sq are all zero, so the update leaves all three bit-identical
    (m = lerp(0, 0) = 0, v = 0, p -= step_size * 0 / eps).  Hence the usual step is ONE launch over the whole buffer."""

    def _adam_layout(self):
        n = len(self._params)
        self._steps = [0] * n
        self._live = [True] * n
        self._exp_avg = None
        self._exp_avg_sq = None
        if any(b % 4 for b in self._begin) or any(a >= b for a, b in zip(self._begin, self._begin[1:])):
            raise ValueError("flat Adam: parameter storage must be 16-byte aligned and in buffer order")

    def _ensure_state(self):
        flat, _ = self._flat()
        if self._exp_avg is None or self._exp_avg.device != flat.device:
            old = (self._exp_avg, self._exp_avg_sq)
            self._exp_avg, self._exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
            if old[0] is not None:
                self._exp_avg.copy_(old[0])
                self._exp_avg_sq.copy_(old[1])
        return self._exp_avg, self._exp_avg_sq

    @staticmethod
    def _check_group(group):
        bad = [k for k in _ADAM_OFF if group.get(k)]
        if bad:
            raise ValueError("flat Adam supports torch.optim.Adam with %s off (got %s)"
                             % (" / ".join(_ADAM_OFF), ", ".join("%s=%r" % (k, group[k]) for k in bad)))
        unknown = set(group) - set(("params", "lr", "betas", "eps", "weight_decay") + _ADAM_OFF + _ADAM_INERT)
        if unknown:
            raise ValueError("flat Adam: param-group keys it cannot honour: %s" % sorted(unknown))

    def _runs(self, weight_decay):
        """[(first, last, step)] over the parameters in group order: parameters first..last take this update with step
        count ``step`` (after it)."""
        n = len(self._params)
        live, steps = self._live, self._steps
        if all(live) and steps.count(steps[0]) == n:
            return [(0, n - 1, steps[0] + 1)]
        runs = []
        cur, pend = None, None          # cur = [first, last, step]; pend: first of a streak of never-stepped, gradient-less
        for i in range(n):
            if live[i]:
                t = steps[i] + 1
                if cur is not None and cur[2] == t:
                    cur[1] = i
                else:
                    if cur is not None:
                        runs.append(tuple(cur))
                    cur = [i if pend is None else pend, i, t]
                pend = None
            elif steps[i] == 0 and weight_decay == 0:
                if pend is None:
                    pend = i
            else:
                if cur is not None:
                    runs.append(tuple(cur))
                cur, pend = None, None
        if cur is not None:
            runs.append(tuple(cur))
        return runs

    def _adam_update(self):
        g = self.param_groups[0]
        self._check_group(g)
        flat_p, flat_g = self._flat()
        m, v = self._ensure_state()
        b1, b2 = g["betas"]
        n = len(self._params)
        clip = self._measure(flat_g)            # one record for every launch below (None: clipping off)
        for first, last, t in self._runs(g["weight_decay"]):
            end = self._begin[last + 1] if last + 1 < n else flat_p.numel()
            engine.adam_step(flat_p, flat_g, m, v, g["lr"], b1, b2, g["eps"], g["weight_decay"], t,
                             self._begin[first], end, clip_state=clip)
        self._steps = [s + 1 if l else s for s, l in zip(self._steps, self._live)]

    # ---- checkpoint interchange with torch.optim.Adam --------------------------------------------------------------
    def state_dict(self):
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._params)))
        state = {}
        for i, s in enumerate(self._steps):
            if s > 0:
                state[i] = {"step": torch.tensor(float(s)),
                            "exp_avg": self._state_view(self._exp_avg, i).detach().clone().contiguous(),
                            "exp_avg_sq": self._state_view(self._exp_avg_sq, i).detach().clone().contiguous()}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """A state_dict of torch.optim.Adam (any torch since 1.7: ``step`` an int or a 0-d tensor) or of this class."""
        if len(sd["param_groups"]) != 1:
            raise ValueError("flat Adam has one parameter group, the checkpoint has %d" % len(sd["param_groups"]))
        grp = sd["param_groups"][0]
        self._check_group(grp)
        ids = list(grp["params"])
        if len(ids) != len(self._params):
            raise ValueError("checkpoint optimiser holds %d parameters, this model %d" % (len(ids), len(self._params)))
        where = {pid: i for i, pid in enumerate(ids)}
        m, v = self._ensure_state()
        steps = [0] * len(self._params)
        with torch.no_grad():
            m.zero_()
            v.zero_()
            for pid, st in sd["state"].items():
                i = where[pid]
                s = st["step"]
                steps[i] = int(s.item()) if torch.is_tensor(s) else int(s)
                self._state_view(m, i).copy_(st["exp_avg"])
                self._state_view(v, i).copy_(st["exp_avg_sq"])
        self._steps = steps
        for k, val in grp.items():
            if k != "params":
                self.param_groups[0][k] = tuple(val) if k == "betas" else val


class FusedAdam(_AdamFlat, torch.optim.Optimizer):
    """torch.optim.Adam(model.parameters(), lr, betas, eps, weight_decay) for the instaorder_amd ResNet: the update runs
    over its flat fp32 master buffers (``flat_params`` / ``flat_grads``, in fp32 and bf16 mode alike)."""

    def __init__(self, module, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None):
        self._clip_init(max_grad_norm)
        net = getattr(module, "module", module)     # DistModule / FixModule wrap the ResNet
        if not hasattr(net, "flat_params"):
            raise TypeError("FusedAdam needs an instaorder_amd ResNet (flat parameter buffer)")
        self._net = net
        params = list(net.parameters())
        super(FusedAdam, self).__init__(params, _adam_defaults(lr, betas, eps, weight_decay))
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdam supports exactly one parameter group")
        info = {id(p): t for t, p in net._param_list}
        self._params = params
        self._info = [info[id(p)] for p in params]
        self._begin = [t["offset"] for t in self._info]
        self._adam_layout()

    def _flat(self):
        return self._net.flat_params, self._net.flat_grads

    def _state_view(self, buf, i):
        return self._net._view(buf, self._info[i])

    def zero_grad(self, set_to_none=True):
        # gradients are rewritten in full by every backward of the engine; nothing to clear
        for p in self.param_groups[0]["params"]:
            if set_to_none:
                p.grad = None

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdam: closures are not supported")
        self._live = [p.grad is not None for p in self._params]
        self._adam_update()
        return None


class FlatAdam(_AdamFlat, _FlatLayout):
    """torch.optim.Adam for an ordinary module tree (the MiDaS nets) over the flat layout FlatSGD uses, so ops.WeightPlan,
    the hipGraph step and the staged data-parallel step take it as they take FlatSGD.  Which parameters had a gradient
    is what the last gather_grads / gather_stage saw (a parameter ops.WeightPlan fills counts as having one); a replayed
    hipGraph keeps what its capture saw."""

    def __init__(self, module, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None):
        self._clip_init(max_grad_norm)
        super(FlatAdam, self).__init__(_trainable(module), _adam_defaults(lr, betas, eps, weight_decay))
        self._begin = [off for off, _ in self._spans]
        self._adam_layout()
        self._ensure_state()

    def _flat(self):
        return self.flat_params, self.flat_grads

    def _state_view(self, buf, i):
        off, k = self._spans[i]
        return buf[off:off + k].view(self._params[i].shape)

    def gather_grads(self, skip=None, prezeroed=False):
        self._live = [p.grad is not None or (skip is not None and id(p) in skip) for p in self._params]
        return super(FlatAdam, self).gather_grads(skip=skip, prezeroed=prezeroed)

    def gather_stage(self, idx, grads, skip=None, attach=False, prezeroed=False):
        for i, g in zip(idx, grads):
            self._live[i] = g is not None or (skip is not None and id(self._params[i]) in skip)
        return super(FlatAdam, self).gather_stage(idx, grads, skip=skip, attach=attach, prezeroed=prezeroed)

    @torch.no_grad()
    def step(self, closure=None, gathered=False):
        if closure is not None:
            raise ValueError("FlatAdam: closures are not supported")
        if not gathered:
            self.gather_grads()
        self._adam_update()
        from . import ops
        ops.WEIGHTS_EPOCH[0] += 1          # parameters changed in place, invisibly to torch's version counters
        return None
