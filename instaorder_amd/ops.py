"""Operator layer for graphs the fixed ResNet-50 executor (io_net_*) does not cover -- today the MiDaS branch
(InstaDepthNet_od / _d, midas/midas_net.py:116-212) and the training step of PCNet-M's UNet (unet.py).  Every function is a ``torch.autograd.Function`` whose forward
and backward are launches of libinstaorder_hip.so on **NHWC** tensors, fp32 or bf16 (the element type of the input
selects the kernels; parameters and their gradients are always fp32); torch supplies memory, streams and the autograd
tape only.  Filters are taken in the reference's OIHW layout (what ``state_dict`` holds) and re-laid out to the
kernels' [Cout][taps][Cin] (in the activation type) once per call.

There is no CPU path: inputs must live on an MI355X.
"""
import contextlib
import ctypes as C
import os
from collections import namedtuple

import torch

from . import _lib

__all__ = ["conv2d", "conv_bn", "batch_norm", "max_pool_3x3s2", "avgpool_fc", "upsample2x", "bias_act", "relu", "add", "head1",
           "max_pool_2x2", "up2x_concat", "unet_head_loss", "nhwc_from_nchw", "nchw_from_nhwc"]


# bumped by whoever changes parameters behind torch's back (the HIP optimiser kernels update them in place without
# touching torch's version counters): invalidates the folded inference operands cached on the parameters
WEIGHTS_EPOCH = [0]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _WeightDesc(C.Structure):        # io_weight_desc of include/instaorder_hip.h
    _fields_ = [("src", C.c_long), ("dst_op", C.c_long), ("dst_t", C.c_long), ("dst_g", C.c_long), ("Co", C.c_int),
                ("Ci", C.c_int), ("T", C.c_int), ("Cop", C.c_int), ("Cip", C.c_int)]


# A planned filter: stored channel counts, operand [Cop][taps][Cip], its transpose for the data gradient (None for the packed
# 8-channel stems), the staging view its filter-gradient launch writes.
PlanEntry = namedtuple("PlanEntry", "Cip Cop op op_t grad")
# What a conv_bn with ReLU offers the sole consumer of its output (``out._io_offer``), whose data-gradient launch can then run
# this BatchNorm's backward.  ``link``: the dict both nodes hold -- "_gamma" / "_beta" (the parameters) and, once the consumer
# has run the backward, "dy" / "dgamma" / "dbeta" (the latter two as autograd gets them); G / M / C: groups, rows, channels of y.
BnOffer = namedtuple("BnOffer", "link y mean rstd scale shift gamma G M C")
Folded = namedtuple("Folded", "key wop bias")      # ``w._io_folded``: BatchNorm folded into the filters and a bias (inference)


class WeightPlan(object):
    """Every dense filter of a module tree re-laid out in ONE launch per training step, instead of three to six tiny
    launches per convolution (OIHW master -> [Cout'][taps][Cin'] operand + its transpose for the data gradient; filter
    gradient back to OIHW): ``prepare()`` before the forward, ``unpack_grads()`` after the backward, and in between
    ``_Conv`` / ``_ConvBn`` pick their operands up as views of the plan's buffers (the filter gradient is written into
    the plan's staging buffer and the node returns no gradient for ``w``).

    Built from a RECORDING of one eager training step (which filters are used, with which stored channel counts), so
    it needs no knowledge of the module tree; a filter used more than once per step stays on the per-call path (its
    gradients must accumulate).  Only for parameters that live in a flat buffer (optim.FlatSGD, optim.FlatAdam)."""
    active = None          # the plan convolutions consult (set for the duration of a training step)
    _recording = None      # id(w) -> [w, Cip, Cop, uses] while a step is being recorded

    @classmethod
    def start_recording(cls):
        cls._recording = {}

    @classmethod
    def note(cls, w, Cip, Cop):
        if cls._recording is not None:
            r = cls._recording.setdefault(id(w), [w, Cip, Cop, 0])
            r[3] += 1
            if (r[1], r[2]) != (Cip, Cop):
                r[3] += 100        # used with two layouts: never plan it

    @classmethod
    def note_vec(cls, *ps):
        """the 1-D parameters a node consumes (BatchNorm weight / bias): recorded like the filters -- used exactly once per
        step, their gradient kernels may write straight into the flat gradient buffer (``grad_target``)"""
        if cls._recording is not None:
            for q in ps:
                if q is not None:
                    cls._recording.setdefault(id(q), [q, -1, -1, 0])[3] += 1

    @classmethod
    def grad_target(cls, q):
        """where the gradient of the 1-D parameter ``q`` goes in the step in flight: its slice of optim.flat_grads (the node
        then returns no gradient for it), or None = an ordinary autograd gradient"""
        plan = cls.active
        return plan.vecs.get(id(q)) if (plan is not None and q is not None) else None

    @classmethod
    def stop_recording(cls):
        recs, cls._recording = cls._recording, None
        return [r for r in (recs or {}).values() if r[3] == 1]

    @classmethod
    @contextlib.contextmanager
    def step(cls, plan, record_for=None, dtype=None, built=None, prepare=True):
        """The bracket around one training step (forward, backward, gradient gathering): under ``plan`` (or None) and, with
        ``record_for`` = the flat optimiser, recorded: ``built`` then gets the plan of ``dtype`` operands made from the
        recording (False: nothing to plan).  prepare=False: the caller runs ``plan.prepare()`` inside the block (a staged
        capture wants it in its first graph)."""
        if record_for is not None:
            cls.start_recording()
        if plan is not None and prepare:
            plan.prepare()
        cls.active = plan
        try:
            yield plan
        finally:
            cls.active = None
            if plan is not None:
                plan.cleared = False
            recs = cls.stop_recording() if record_for is not None else None
        if record_for is not None:           # (not after an exception: half a step is no recording)
            built(cls(record_for, recs, dtype) if recs else False)

    @classmethod
    def gather_args(cls):
        """inside the bracket, for optim.gather_grads / gather_stage: what the plan fills, and whether ITS prepare() cleared the buffer"""
        plan = cls.active
        return dict(skip=plan.skip if plan is not None else None, prezeroed=plan is not None and plan.cleared)

    def __init__(self, optim, recs, dtype):
        spans = {id(p): off for p, (off, k) in zip(optim._params, optim._spans)}
        dev = optim.flat_params.device
        self.optim, self.dtype = optim, dtype
        self.entries = {}
        rows, n_op, n_g = [], 0, 0
        # rows in the order of the flat parameter buffer: a contiguous slice of that buffer (one stage of a staged,
        # data-parallel backward pass) is then a contiguous range of rows (unpack_grads(lo, hi))
        for w, Cip, Cop, _ in sorted((r for r in recs if id(r[0]) in spans), key=lambda r: spans[id(r[0])]):
            if id(w) not in spans or w.dim() != 4:
                continue
            Co, Ci, R, S = w.shape
            T = R * S
            sz = Cop * T * Cip
            need_t = Cip != 8                       # the packed 8-channel stems have no data gradient
            rows.append((w, _WeightDesc(spans[id(w)], n_op, n_op + sz if need_t else -1, n_g, Co, Ci, T, Cop, Cip)))
            n_op += sz * (2 if need_t else 1)
            n_g += sz
        # BatchNorm weights / biases used once per step: BatchNorm-backward launches write dgamma / dbeta into these views of
        # the flat gradient buffer -- no per-tensor gradient, no copy into the flat buffer (gather_grads made 286 of them
        # per InstaDepthNet_od step: torch._foreach_copy_ decomposes into one hipMemcpyAsync per tensor)
        self.vecs = {}
        direct = os.environ.get("IO_DEPTH_DIRECT_GRADS", "1") != "0"      # (0: every BatchNorm gradient through autograd + gather -- A/B runs)
        for q, Cip, _, _ in recs:
            if direct and Cip == -1 and id(q) in spans and q.dim() == 1:
                off = spans[id(q)]
                self.vecs[id(q)] = optim.flat_grads[off:off + q.numel()]
        self.skip_ids = None
        self.cleared = False       # prepare() has cleared optim.flat_grads for the step in flight (reset by the step bracket)
        self.n = len(rows)
        self._row_off = [d.src for _, d in rows]
        self.ops = torch.zeros(max(n_op, 1), device=dev, dtype=dtype)
        self.gk = torch.zeros(max(n_g, 1), device=dev, dtype=torch.float32)
        tab = (_WeightDesc * max(self.n, 1))(*[d for _, d in rows])
        self.table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        for w, d in rows:
            sz = d.Cop * d.T * d.Cip
            self.entries[id(w)] = PlanEntry(d.Cip, d.Cop,
                                            self.ops[d.dst_op:d.dst_op + sz].view(d.Cop, d.T, d.Cip),
                                            self.ops[d.dst_t:d.dst_t + sz].view(d.Cip, d.T, d.Cop) if d.dst_t >= 0 else None,
                                            self.gk[d.dst_g:d.dst_g + sz].view(d.Cop, d.T, d.Cip))

    @property
    def skip(self):
        """ids of the parameters whose slice of the flat gradient buffer this plan fills (optim.gather_grads leaves them alone)"""
        if self.skip_ids is None:
            self.skip_ids = set(self.entries) | set(self.vecs)
        return self.skip_ids

    def lookup(self, w, Cip, Cop, dtype):
        e = self.entries.get(id(w))
        return e if (e is not None and e.Cip == Cip and e.Cop == Cop and dtype == self.dtype) else None

    def prepare(self):
        """-> whether it cleared optim.flat_grads: kept in ``cleared`` until the step's bracket closes (= gather's ``prezeroed``)"""
        if self.n:
            # A planned filter whose gradient kernel does not run in this step (a loss weight switched to 0 after the plan
            # was recorded) must deliver zero, not the previous step's gradient: unpack_grads() copies every entry of gk.
            self.gk.zero_()
        if self.vecs:
            # ... and so must a directly written BatchNorm gradient, and every parameter no loss reaches (the occlusion
            # branch of the reference's InstaDepthNet_od recipe: occ_order_weight 0) -- ONE fill of the flat buffer
            # instead of one per gradient-less parameter in gather_grads (129 per step); whether or not a filter is planned
            self.optim.flat_grads.zero_()
            self.cleared = True
        if self.n:
            _lib.check(_L().io_weights_prepare(_p(self.table), self.n, _p(self.optim.flat_params), _p(self.ops),
                                               1 if self.dtype == torch.bfloat16 else 0, _st()), "io_weights_prepare")
        return self.cleared

    def unpack_grads(self, lo=None, hi=None):
        """after optim.gather_grads(): the planned filters' gradients into their OIHW places in the flat buffer; with
        (lo, hi) only those of the filters that live in [lo, hi) of the flat buffer (rows are in flat order)"""
        if not self.n:
            return
        r0, r1 = 0, self.n
        if lo is not None:
            r0 = next((i for i, o in enumerate(self._row_off) if o >= lo), self.n)
            r1 = next((i for i, o in enumerate(self._row_off) if o >= hi), self.n)
        if r1 > r0:
            tab = C.c_void_p(self.table.data_ptr() + r0 * C.sizeof(_WeightDesc))
            _lib.check(_L().io_weights_unpack_grads(tab, r1 - r0, _p(self.gk), _p(self.optim.flat_grads), _st()),
                       "io_weights_unpack_grads")


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L():
    _lib.require_gpu()
    return _lib.lib()


def _chk(t, name):
    if not (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous()):
        raise RuntimeError("instaorder_amd.ops: %s must be a contiguous fp32 / bf16 tensor on the GPU (no CPU fallback)"
                           % name)


def _dt(t):
    return 1 if t.dtype == torch.bfloat16 else 0


def nhwc_from_nchw(x, pad_to=None, dtype=None):
    """[N,C,H,W] -> contiguous [N,H,W,C'] (C' = pad_to, zero filled, for the 8-channel stems) of ``dtype``."""
    N, Cc, H, W = x.shape
    dtype = dtype or x.dtype
    if pad_to is not None and pad_to != Cc:
        out = torch.zeros((N, H, W, pad_to), device=x.device, dtype=dtype)
        out[..., :Cc] = x.permute(0, 2, 3, 1)
        return out
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


def nchw_from_nhwc(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---- launch blocks the convolution / BatchNorm nodes are composed of ------------------------------------------------------
# one convolution as its launches take it; Cs / Co are the STORED channel counts of input and output
_Geom = namedtuple("_Geom", "N H W Cs Co R S stride pad")


def _geom(x, w, stride, pad, Cop):
    N, H, W_, Cs = x.shape
    return _Geom(N, H, W_, Cs, Cop, w.shape[2], w.shape[3], stride, pad)


def _grouped(g):
    """the geometry as the grouped launches take it (Cin == Cout: one channel count)"""
    return g.N, g.H, g.W, g.Co, g.R, g.S, g.stride, g.pad


def _conv_out(x, g):
    Ho, Wo = (g.H + 2 * g.pad - g.R) // g.stride + 1, (g.W + 2 * g.pad - g.S) // g.stride + 1
    return torch.empty((g.N, Ho, Wo, g.Co), device=x.device, dtype=x.dtype)


def _conv_operands(x, w, wsrc, g, dense, planned=True):
    """OIHW ``wsrc`` (values of the parameter ``w``) -> (operand of the forward, operand the data gradient starts from,
    PlanEntry or None).  Dense: [Co'][taps][Cs]; planned: the use is noted for a recording, and the operand is the active
    plan's if that holds the filter in this layout.  Grouped: 64-channel windows and their twin for the data gradient."""
    Co, Ci, R, S = w.shape
    if not dense:
        wc = torch.empty((Co, R * S, 64), device=x.device, dtype=x.dtype)
        wtc = torch.empty_like(wc)
        _lib.check(_L().io_gconv_pack(_p(wsrc.contiguous()), Co, Ci, R * S, _p(wc), _p(wtc), _dt(x), _st()), "io_gconv_pack")
        return wc, wtc, None
    ent = None
    if planned:
        WeightPlan.note(w, g.Cs, g.Co)
        ent = WeightPlan.active.lookup(w, g.Cs, g.Co, x.dtype) if WeightPlan.active is not None else None
    if ent is not None:
        return ent.op, ent.op, ent
    wk = torch.zeros((g.Co, R * S, g.Cs), device=x.device, dtype=x.dtype)
    wk[:Co, :, :Ci] = wsrc.permute(0, 2, 3, 1).reshape(Co, R * S, Ci)
    return wk, wk, None


def _conv_fwd(x, wop, y, g, dense):
    if dense:
        _lib.check(_L().io_conv2d_fwd_dt(_p(x), _p(wop), _p(y), *g, _dt(x), _dt(x), _st()), "io_conv2d_fwd_dt")
    else:
        _lib.check(_L().io_gconv2d_fwd(_p(x), _p(wop), _p(y), *_grouped(g), _dt(x), _st()), "io_gconv2d_fwd")


def _conv_dgrad(who, g, x, dy, wback, ent, dense, add=None, prev=None):
    """-> (data gradient, what is left of ``add``): the dense launch sums ``add`` onto it, the others have no such operand.
    ``prev``: the BnOffer of x's producer, whose BatchNorm backward then runs in this launch (_fused_dgrad)."""
    if dense:
        if g.Cs == 8:
            raise RuntimeError("ops.%s: no data gradient for the packed 8-channel stem input" % who)
        wback = ent.op_t if ent is not None else wback.permute(2, 1, 0).contiguous()     # [Cin][taps][Cout]
    if prev is not None:
        return _fused_dgrad(g, x, dy, wback, 0 if dense else 64, prev), add
    dx = torch.empty_like(x)
    if dense:
        _lib.check(_L().io_conv2d_dgrad_dt(_p(dy), _p(wback), _p(dx), _p(add), None, *g, _dt(x), _st()), "io_conv2d_dgrad_dt")
        return dx, None
    _lib.check(_L().io_gconv2d_dgrad(_p(dy), _p(wback), _p(dx), *_grouped(g), _dt(x), _st()), "io_gconv2d_dgrad")
    return dx, add


def _fused_dgrad(g, x, dy, wt_op, gw, prev):
    """data gradient + the PRODUCER's BatchNorm backward: ReLU mask recomputed from its y, its two reductions in
    the epilogue of this launch, then only the apply pass -- the producer node finds its results in the link"""
    dev = x.device
    tiles = prev.M // 128
    nws = 2 * ((tiles + tiles // 64 + prev.G + 2) * prev.C) + 2 * prev.G * prev.C
    wsf = torch.empty(nws, device=dev, dtype=torch.float32)
    dz = torch.empty_like(x)
    dyb = torch.empty_like(x)
    link = prev.link
    dg, link["dgamma"] = _grad_dest(link.get("_gamma"), prev.C, dev)
    db, link["dbeta"] = _grad_dest(link.get("_beta"), prev.C, dev)
    _lib.check(_L().io_conv2d_dgrad_bnbwd_dt(_p(dy), _p(wt_op), _p(dz), g.N, g.H, g.W, g.Cs, g.Co, g.R, g.S, g.pad,
                                             _p(prev.y), prev.G, _p(prev.gamma), _p(prev.mean), _p(prev.rstd),
                                             _p(prev.scale), _p(prev.shift), _p(dg), _p(db), _p(dyb), _p(wsf), nws, _dt(x),
                                             gw, _st()), "io_conv2d_dgrad_bnbwd_dt")
    link["dy"] = dyb
    return dz


def _conv_wgrad(g, x, dy, ent, Co, Ci, dense):
    """-> the filter gradient, OIHW [Co,Ci,R,S]; None for a planned filter (WeightPlan.unpack_grads delivers it)"""
    L, dev = _L(), x.device
    if dense:
        nb = int(L.io_conv2d_wgrad_workspace_bytes(*g))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        dwk = ent.grad if ent is not None else torch.empty((g.Co, g.R * g.S, g.Cs), device=dev, dtype=torch.float32)
        _lib.check(L.io_conv2d_wgrad_dt(_p(x), _p(dy), _p(dwk), *g, _p(ws), nb, _dt(x), _dt(x), _st()), "io_conv2d_wgrad_dt")
        return None if ent is not None else dwk[:Co, :, :Ci].reshape(Co, g.R, g.S, Ci).permute(0, 3, 1, 2).contiguous()
    nb = int(L.io_gconv2d_wgrad_workspace_bytes(*_grouped(g)))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    dwc = torch.empty((Co, g.R * g.S, 64), device=dev, dtype=torch.float32)
    _lib.check(L.io_gconv2d_wgrad(_p(x), _p(dy), _p(dwc), *_grouped(g), _p(ws), nb, _dt(x), _st()), "io_gconv2d_wgrad")
    dw = torch.empty((Co, Ci, g.R, g.S), device=dev, dtype=torch.float32)
    _lib.check(L.io_gconv_unpack_grad(_p(dwc), Co, Ci, g.R * g.S, _p(dw), _st()), "io_gconv_unpack_grad")
    return dw


def _momentum(repeat):
    """R identical module calls advance a running estimate R times with the same statistic:
    r <- (1-m)^R r + (1 - (1-m)^R) s, i.e. ONE update with momentum 1 - (1-m)^R (m = 0.1)."""
    return 1.0 - 0.9 ** int(repeat)


def _bn_partials(M, Cc, G, dev):
    npart = int(_L().io_bn_partial_floats(M, Cc, G))
    return torch.empty(npart, device=dev, dtype=torch.float32), npart


def _bn_stats(t, M, Cc, G, gamma, beta, running_mean, running_var, repeat, coeffs):
    """training: batch statistics of t[M, Cc] in G groups -> ``coeffs``; running estimates advanced in place"""
    mean, rstd, scale, shift = coeffs
    part, npart = _bn_partials(M, Cc, G, t.device)
    _lib.check(_L().io_bn_stats_finalize_dt(_p(t), M, Cc, G, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                            _momentum(repeat), 1e-5, _p(mean), _p(rstd), _p(scale), _p(shift), _p(part),
                                            npart, _dt(t), _st()), "io_bn_stats_finalize_dt")


def _bn_eval_prepare(Cc, gamma, beta, running_mean, running_var, coeffs):
    """eval: ``coeffs`` from the running estimates -> rstd"""
    mean, _, scale, shift = coeffs
    _lib.check(_L().io_bn_eval_prepare(Cc, _p(gamma), _p(beta), _p(running_mean), _p(running_var), 1e-5, _p(mean),
                                       _p(scale), _p(shift), _st()), "io_bn_eval_prepare")
    return scale / gamma


def _bn_apply(t, M, Cc, G, batch_stats, mean, scale, shift, identity, relu):
    out = torch.empty_like(t)
    _lib.check(_L().io_bn_apply_dt(_p(t), M, Cc, G, 1 if batch_stats else 0, _p(mean), _p(scale), _p(shift), _p(identity),
                                   None, None, None, int(relu), _p(out), _dt(t), _st()), "io_bn_apply_dt")
    return out


def _grad_dest(q, n, dev):
    """gradient of the 1-D parameter ``q`` -> (the tensor its kernel writes, what autograd gets for q): the plan's view of the
    flat buffer and None, or one fresh tensor for both"""
    t = WeightPlan.grad_target(q)
    if t is not None:
        return t, None
    t = torch.empty(n, device=dev)
    return t, t


def _bn_backward(dout, relu_out, t, M, Cc, G, has_id, gamma, beta, mean, rstd, link=None):
    """backward of [relu](bn(t) [+ identity]); ``relu_out``: the node's output if it ends in a ReLU
    -> dt, didentity (None without one), dgamma, dbeta (the latter two as autograd gets them)"""
    dev = t.device
    part, npart = _bn_partials(M, Cc, G, dev)
    coef = torch.empty(2 * G * Cc, device=dev, dtype=torch.float32)
    if link is not None and "dy" in link:
        # the sole consumer of the node's output already ran this backward in its data-gradient launch (_fused_dgrad); the
        # query and the buffers above stay ahead of this test: the step's call sequence and pool layout are what they were
        return link.pop("dy"), None, link.pop("dgamma"), link.pop("dbeta")
    dgamma, ret_g = _grad_dest(gamma, Cc, dev)
    dbeta, ret_b = _grad_dest(beta, Cc, dev)
    dx = torch.empty_like(t)
    dz = torch.empty_like(t) if has_id else None          # gradient of the pre-ReLU sum = gradient of `identity`
    _lib.check(_L().io_bn_bwd_dt(_p(dout), _p(relu_out), None, None, _p(t), M, Cc, G, _p(gamma.detach()), _p(mean),
                                 _p(rstd), _p(dgamma), _p(dbeta), _p(dx), _p(dz), _p(part), npart, _p(coef), _dt(t), _st()),
               "io_bn_bwd_dt")
    return dx, dz, ret_g, ret_b


# ---- convolution -------------------------------------------------------------------------------------------------------
class _Conv(torch.autograd.Function):
    """Dense convolution (models/backbone/resnet_cls.py:23-31, midas/blocks.py:27-38, 133-139).  x[N,H,W,Ci'] where
    Ci' >= Ci is the stored channel count (8 for the 3- / 2-channel stems); w OIHW [Co,Ci,R,S].  Output channels are
    padded to a multiple of 64 when `co_pad` (the 128 -> 32 convolution of output_conv): the extra channels are 0."""
    dense = True

    @classmethod
    def forward(cls, ctx, x, w, stride, pad, co_pad=False):
        _chk(x, "x")
        Co, Ci = w.shape[:2]
        if not cls.dense and Co != x.shape[-1]:
            raise ValueError("grouped conv: Cin must equal Cout")
        g = _geom(x, w, stride, pad, ((Co + 63) // 64) * 64 if co_pad else Co)
        wk, wback, ent = _conv_operands(x, w, w.detach(), g, cls.dense)
        y = _conv_out(x, g)
        _conv_fwd(x, wk, y, g, cls.dense)
        ctx.save_for_backward(x, wback)
        ctx.ent, ctx.geom, ctx.wshape = ent, g, (Co, Ci)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wk = ctx.saved_tensors
        g, ent = ctx.geom, ctx.ent
        dy = dy.contiguous()
        dx = _conv_dgrad("conv2d", g, x, dy, wk, ent, True)[0] if ctx.needs_input_grad[0] else None
        dw = _conv_wgrad(g, x, dy, ent, *ctx.wshape, True) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None


class _GroupedConv(_Conv):
    """Grouped 3x3 convolution of ResNeXt (resnet_cls.py:23-26 with groups=32): w OIHW [C, C/groups, R, S]."""
    dense = False

    @staticmethod
    def backward(ctx, dy):
        x, wtc = ctx.saved_tensors
        dy = dy.contiguous()
        dx, _ = _conv_dgrad("conv2d", ctx.geom, x, dy, wtc, None, False)
        return dx, _conv_wgrad(ctx.geom, x, dy, None, *ctx.wshape, False), None, None


def conv2d(x, w, stride=1, pad=0, groups=1, co_pad=False):
    if groups == 1:
        return _Conv.apply(x, w, stride, pad, co_pad)
    if w.shape[0] // groups != w.shape[1]:
        raise ValueError("grouped conv: expected [C, C/groups, R, S] filters")
    return _GroupedConv.apply(x, w, stride, pad)


# ---- BatchNorm (+ residual add) (+ ReLU) ---------------------------------------------------------------------------------
class _BatchNorm(torch.autograd.Function):
    """nn.BatchNorm2d (+ `out += identity`) (+ nn.ReLU) of resnet_cls.py:96-116.  Training: batch statistics, running
    estimates advanced in place (momentum 0.1, unbiased variance); eval: running estimates.
    groups = G: the batch is G consecutive equal parts normalised with separate statistics, running estimates advanced
    part by part -- exactly G sequential module calls on the parts (the two mask orders of a pair batch).
    repeat = R: the module call is accounted R times (running estimates advanced R times with the same statistics):
    the reference runs the shared encoder once per mask order on identical input."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, relu, identity, groups, repeat):
        _chk(x, "x")
        if training:
            WEIGHTS_EPOCH[0] += 1      # running statistics move (behind torch's version counters): folded operands are stale
        Cc = x.shape[-1]
        M = x.numel() // Cc
        G = int(groups) if training else 1
        coeffs = mean, rstd, scale, shift = tuple(torch.empty(G * Cc, device=x.device, dtype=torch.float32) for _ in range(4))
        gd, bd = gamma.detach(), beta.detach()
        if training:
            WeightPlan.note_vec(gamma, beta)
            _bn_stats(x, M, Cc, G, gd, bd, running_mean, running_var, repeat, coeffs)
        else:
            rstd = _bn_eval_prepare(Cc, gd, bd, running_mean, running_var, coeffs)
        out = _bn_apply(x, M, Cc, G, training, mean, scale, shift, identity, relu)
        ctx.save_for_backward(x, out, gamma, mean, rstd)
        ctx.beta = beta
        ctx.cfg = (M, Cc, bool(relu), identity is not None, bool(training), G)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, gamma, mean, rstd = ctx.saved_tensors
        M, Cc, relu, has_id, training, G = ctx.cfg
        if not training:
            raise RuntimeError("ops.batch_norm: backward through eval-mode BatchNorm is not implemented")
        dx, dz, dgamma, dbeta = _bn_backward(dout.contiguous(), out if relu else None, x, M, Cc, G, has_id, gamma, ctx.beta,
                                             mean, rstd)
        return dx, dgamma, dbeta, None, None, None, None, dz, None, None


def batch_norm(x, gamma, beta, running_mean, running_var, training, relu=False, identity=None, groups=1, repeat=1):
    if repeat > 1 and groups > 1:
        raise ValueError("batch_norm: repeat and groups are exclusive")
    return _BatchNorm.apply(x, gamma, beta, running_mean, running_var, training, relu, identity, groups, repeat)


def _conv_bn_infer(x, w, gamma, beta, running_mean, running_var, stride, pad, groups, relu, identity):
    """inference: the BatchNorm is folded into the filters (scaled per output channel) and a bias; the convolution's
    epilogue adds bias (+ identity) (+ ReLU) -- no pass over the conv output.  The folded operands are kept on the
    parameter until the weights change (torch version counters + WEIGHTS_EPOCH, which the HIP-side optimiser bumps): an
    inference loop re-packs nothing."""
    dense = groups == 1
    g = _geom(x, w, stride, pad, w.shape[0])
    key = (x.dtype, g.Cs, WEIGHTS_EPOCH[0], w._version, gamma._version, beta._version, running_mean._version,
           running_var._version)
    hit = getattr(w, "_io_folded", None)
    if hit is None or hit.key != key:
        fscale = gamma.detach() / torch.sqrt(running_var + 1e-5)
        fbias = (beta.detach() - running_mean * fscale).contiguous()
        wsrc = w.detach() * fscale.view(-1, 1, 1, 1)
        hit = w._io_folded = Folded(key, _conv_operands(x, w, wsrc, g, dense, planned=False)[0], fbias)
    y = _conv_out(x, g)
    _lib.check(_L().io_conv2d_fwd_bias_dt(_p(x), _p(hit.wop), _p(y), *g, _p(hit.bias), _p(identity), int(relu), _dt(x),
                                          0 if dense else 64, _st()), "io_conv2d_fwd_bias_dt")
    return y


def _conv_bn_train(ctx, x, w, gamma, beta, running_mean, running_var, stride, pad, groups, relu, identity, bn_groups,
                   repeat, prev):
    """training: batch statistics in the convolution's epilogue where the rows per statistics group are whole 128-row
    tiles, else convolution + statistics pass; then the apply pass.  Fills ``ctx`` for _ConvBn.backward."""
    WEIGHTS_EPOCH[0] += 1      # running statistics move (behind torch's version counters): folded operands are stale
    L = _L()
    Co, Cig = w.shape[:2]
    dense = groups == 1
    g = _geom(x, w, stride, pad, Co)
    wop, wback, ent = _conv_operands(x, w, w.detach(), g, dense)
    y = _conv_out(x, g)
    M, G = y.numel() // Co, int(bn_groups)
    coeffs = mean, rstd, scale, shift = tuple(torch.empty(G * Co, device=x.device, dtype=torch.float32) for _ in range(4))
    gd, bd = gamma.detach(), beta.detach()
    WeightPlan.note_vec(gamma, beta)
    tiled = M % G == 0 and (M // G) % 128 == 0
    if tiled:
        nws = int(L.io_conv2d_bnstats_workspace_floats(g.N, g.H, g.W, Co, g.R, g.S, stride, pad, G))
        ws = torch.empty(nws, device=x.device, dtype=torch.float32)
        _lib.check(L.io_conv2d_fwd_bnstats_dt(_p(x), _p(wop), _p(y), *g, G, _p(gd), _p(bd), _p(running_mean),
                                              _p(running_var), _momentum(repeat), 1e-5, _p(mean), _p(rstd), _p(scale),
                                              _p(shift), _p(ws), nws, _dt(x), 0 if dense else 64, _st()),
                   "io_conv2d_fwd_bnstats_dt")
    else:
        _conv_fwd(x, wop, y, g, dense)
        _bn_stats(y, M, Co, G, gd, bd, running_mean, running_var, repeat, coeffs)
    out = _bn_apply(y, M, Co, G, True, mean, scale, shift, identity, relu)
    ctx.save_for_backward(x, wback, y, out, gamma, mean, rstd)
    ctx.beta, ctx.ent, ctx.geom = beta, ent, g
    ctx.cfg = (Cig, dense, M, G, bool(relu), identity is not None)
    # Cross-node fusion of the BatchNorm backward (see conv_bn's `sole`): as PRODUCER of relu(bn(y)) this node offers
    # what a consumer's data-gradient epilogue needs; as CONSUMER of such a tensor it keeps the producer's offer.
    if relu and identity is None and tiled and Co % 64 == 0:
        ctx.link = {"_gamma": gamma, "_beta": beta}
        _ConvBn.last_offer = BnOffer(ctx.link, y, mean, rstd, scale, shift, gd, G, M, Co)
    if prev is not None and stride == 1 and prev.M == g.N * g.H * g.W and prev.C == g.Cs and (dense or Co == g.Cs):
        ctx.prev = prev
    return out


class _ConvBn(torch.autograd.Function):
    """conv (dense or grouped) -> BatchNorm (+ identity) (+ ReLU) as ONE node: in training mode the batch statistics are
    accumulated in the convolution's epilogue (per 128-row tile, merged with Chan's update) whenever the rows per
    statistics group are a multiple of 128 -- no separate pass over the conv output (resnet_cls.py:99-114)."""
    last_offer = None      # the BnOffer of the forward that just ran, handed over to conv_bn (which hangs it on the output)

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, stride, pad, groups, training, relu, identity,
                bn_groups, repeat, prev, fork):
        _chk(x, "x")
        if groups != 1 and (w.shape[0] != x.shape[-1] or w.shape[0] // groups != w.shape[1]):
            raise ValueError("grouped conv: expected [C, C/groups, R, S] filters on C input channels")
        ctx.prev = ctx.link = _ConvBn.last_offer = None
        ctx.training = bool(training)
        if training:
            out = _conv_bn_train(ctx, x, w, gamma, beta, running_mean, running_var, stride, pad, groups, relu, identity,
                                 bn_groups, repeat, prev)
        else:
            out = _conv_bn_infer(x, w, gamma, beta, running_mean, running_var, stride, pad, groups, relu, identity)
        # fork: x comes back as a second output (an alias) -- for the residual connection of the Bottleneck this convolution
        # opens -- so that the gradient of that path arrives HERE and rides in the `add` operand of the data-gradient
        # launch instead of being summed onto dx by a separate ATen kernel of the autograd engine
        return (out, x) if fork else out

    @staticmethod
    def backward(ctx, dout, dfork=None):
        if not ctx.training:
            raise RuntimeError("ops.conv_bn: backward through eval-mode BatchNorm is not implemented")
        Cig, dense, M, G, relu, has_id = ctx.cfg
        g, ent, prev, link = ctx.geom, ctx.ent, ctx.prev, ctx.link
        if dfork is not None:
            dfork = dfork.contiguous()
        x, wback, y, out, gamma, mean, rstd = ctx.saved_tensors
        dy, dz, dgamma, dbeta = _bn_backward(dout.contiguous(), out if relu else None, y, M, g.Co, G, has_id, gamma, ctx.beta,
                                             mean, rstd, link)
        dx = None
        if ctx.needs_input_grad[0] or not dense:
            dx, dfork = _conv_dgrad("conv_bn", g, x, dy, wback, ent, dense, dfork, prev)
        dw = _conv_wgrad(g, x, dy, ent, g.Co, Cig, dense)
        if dfork is not None:                    # (forms whose data gradient has no add operand: summed here)
            dx = dfork if dx is None else dx + dfork
        return (dx, dw, dgamma, dbeta, None, None, None, None, None, None, None, dz, None, None, None, None)


def conv_bn(x, w, gamma, beta, running_mean, running_var, stride, pad, groups, training, relu=False, identity=None,
            bn_groups=1, repeat=1, sole=False, fork=False):
    """``sole=True``: the caller promises that THIS call is the only consumer of ``x`` (as conv2 / conv3 of a Bottleneck
    are of relu(bn1(.)) / relu(bn2(.)), resnet_cls.py:99-111).  If ``x`` came out of a conv_bn with ReLU, the backward of
    that BatchNorm then runs inside this node's data-gradient launch (mask recomputed from the producer's conv output,
    reductions in the epilogue, io_conv2d_dgrad_bnbwd_dt) instead of as separate reduce + apply passes.
    ``fork=True`` (training, x requires a gradient): returns ``(out, x_alias)``; the caller routes every OTHER use of x (the
    residual connection / the downsample branch of resnet_cls.py:96-114) through ``x_alias``, whose gradient then enters this
    node and is added inside its data-gradient launch (io_conv2d_dgrad_dt's `add`) -- one launch instead of the data gradient
    plus the autograd engine's accumulation kernel (65 of them per InstaDepthNet_od step).  Otherwise returns ``out`` alone."""
    if repeat > 1 and bn_groups > 1:
        raise ValueError("conv_bn: repeat and bn_groups are exclusive")
    prev = getattr(x, "_io_offer", None) if (sole and training) else None
    if prev is not None and prev.G != int(bn_groups):
        prev = None
    fork = bool(fork and training and torch.is_grad_enabled() and x.requires_grad)
    out = _ConvBn.apply(x, w, gamma, beta, running_mean, running_var, stride, pad, groups, training, relu, identity,
                        bn_groups, repeat, prev, fork)
    alias = None
    if fork:
        out, alias = out
    if _ConvBn.last_offer is not None:
        out._io_offer, _ConvBn.last_offer = _ConvBn.last_offer, None
    return (out, alias) if fork else out


# ---- pooling / heads --------------------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x, "x")
        N, H, W_, Cc = x.shape
        Ho, Wo = (H + 1) // 2, (W_ + 1) // 2
        out = torch.empty((N, Ho, Wo, Cc), device=x.device, dtype=x.dtype)
        idx = torch.empty((N, Ho, Wo, Cc // 4), dtype=torch.int32, device=x.device)
        _lib.check(_L().io_maxpool_fwd_dt(_p(x), N, H, W_, Cc, _p(out), _p(idx), _dt(x), _st()), "io_maxpool_fwd_dt")
        ctx.save_for_backward(idx)
        ctx.geom = (N, H, W_, Cc)
        return out

    @staticmethod
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        N, H, W_, Cc = ctx.geom
        dx = torch.empty((N, H, W_, Cc), device=dy.device, dtype=dy.dtype)
        _lib.check(_L().io_maxpool_bwd_dt(_p(dy.contiguous()), _p(idx), N, H, W_, Cc, _p(dx), _dt(dy), _st()),
                   "io_maxpool_bwd_dt")
        return dx


def max_pool_3x3s2(x):
    """nn.MaxPool2d(3, 2, 1) (resnet_cls.py:144)."""
    return _MaxPool.apply(x)


class _AvgPoolFc(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) + flatten + nn.Linear (midas_net.py:195-197, 205-207)."""

    @staticmethod
    def forward(ctx, x, w, b):
        _chk(x, "x")
        N, H, W_, Cc = x.shape
        K = w.shape[0]
        pooled = torch.empty((N, Cc), device=x.device, dtype=torch.float32)
        logits = torch.empty((N, K), device=x.device, dtype=torch.float32)
        wd, bd = w.detach().contiguous(), b.detach().contiguous()
        _lib.check(_L().io_avgpool_fc_fwd_dt(_p(x), N, H * W_, Cc, _p(wd), _p(bd), K, None, None, 0, _p(pooled), _p(logits),
                                             _dt(x), _st()), "io_avgpool_fc_fwd_dt")
        ctx.save_for_backward(pooled, wd)
        ctx.geom = (N, H, W_, Cc, K, x.dtype)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        pooled, wd = ctx.saved_tensors
        N, H, W_, Cc, K, xdt = ctx.geom
        dx = torch.empty((N, H, W_, Cc), device=pooled.device, dtype=xdt)
        dw, db = torch.empty((K, Cc), device=pooled.device), torch.empty(K, device=pooled.device)
        _lib.check(_L().io_avgpool_fc_bwd_dt(_p(dlogits.float().contiguous()), _p(pooled), N, H * W_, Cc, _p(wd), K, None, 0,
                                             None, _p(dx), _p(dw), _p(db), None, None, _dt(dx), _st()),
                   "io_avgpool_fc_bwd_dt")
        return dx, dw, db


def avgpool_fc(x, w, b):
    return _AvgPoolFc.apply(x, w, b)


# ---- decoder pieces -----------------------------------------------------------------------------------------------------
class _Upsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, align):
        _chk(x, "x")
        N, H, W_, Cc = x.shape
        out = torch.empty((N, 2 * H, 2 * W_, Cc), device=x.device, dtype=x.dtype)
        _lib.check(_L().io_upsample2x_bilinear_fwd(_p(x), N, H, W_, Cc, int(align), _p(out), _dt(x), _st()),
                   "io_upsample2x_fwd")
        ctx.geom = (N, H, W_, Cc, int(align))
        return out

    @staticmethod
    def backward(ctx, dy):
        N, H, W_, Cc, align = ctx.geom
        dx = torch.empty((N, H, W_, Cc), device=dy.device, dtype=dy.dtype)
        _lib.check(_L().io_upsample2x_bilinear_bwd(_p(dy.contiguous()), N, H, W_, Cc, align, _p(dx), _dt(dy), _st()),
                   "io_upsample2x_bwd")
        return dx, None


def upsample2x(x, align_corners):
    """nn.functional.interpolate(scale_factor=2, mode='bilinear', align_corners=...) (midas/blocks.py:111-113, 186-188)."""
    return _Upsample.apply(x, align_corners)


class _BiasAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, relu):
        _chk(x, "x")
        Cc = x.shape[-1]
        M = x.numel() // Cc
        out = torch.empty_like(x)
        bd = None
        if bias is not None:
            bd = bias.detach()
            if bd.numel() != Cc:                       # padded output channels carry no bias
                bd = torch.cat([bd, torch.zeros(Cc - bd.numel(), device=x.device)])
        _lib.check(_L().io_bias_act(_p(x), _p(bd), M, Cc, int(relu), _p(out), _dt(x), _st()), "io_bias_act")
        ctx.save_for_backward(out)
        ctx.cfg = (M, Cc, bool(relu), None if bias is None else bias.numel())
        return out

    @staticmethod
    def backward(ctx, dy):
        out, = ctx.saved_tensors
        M, Cc, relu, nbias = ctx.cfg
        L = _L()
        dy = dy.contiguous()
        dx = dy
        if relu:
            dx = torch.empty_like(dy)
            _lib.check(L.io_relu_bwd(_p(dy), _p(out), dy.numel(), _p(dx), _dt(dy), _st()), "io_relu_bwd")
        db = None
        if nbias is not None:
            npart = int(L.io_colsum_partial_floats(M, Cc))
            part = torch.empty(npart, device=dy.device, dtype=torch.float32)
            dbf = torch.empty(Cc, device=dy.device, dtype=torch.float32)
            _lib.check(L.io_colsum(_p(dx), M, Cc, _p(dbf), _p(part), npart, _dt(dx), _st()), "io_colsum")
            db = dbf[:nbias].clone()
        return dx, db, None


def bias_act(x, bias=None, relu=False):
    """[relu](x + bias): the bias of a biased nn.Conv2d and / or nn.ReLU (midas/blocks.py:133-160)."""
    return _BiasAct.apply(x, bias, relu)


def relu(x):
    return _BiasAct.apply(x, None, True)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, "a")
        _chk(b, "b")
        out = torch.empty_like(a)
        _lib.check(_L().io_add(_p(a), _p(b), a.numel(), _p(out), _dt(a), _st()), "io_add")
        return out

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return _Add.apply(a, b)


class _AddShared(_Add):
    """a + b where b is a tensor OTHER STREAMS consume too (the encoder features injected into an order branch that runs on a
    side stream, midas/midas_net.py:190-197).  The backward hands b its OWN copy of the gradient.  With `return dy, dy`
    (what _Add does, and torch's own AddBackward) the branch's next backward node and the node behind b -- on the main
    stream, where the contributions of both order branches meet in one autograd input buffer -- hold the SAME tensor; the
    engine accumulates the second contribution IN PLACE as soon as nobody else references the first (use_count == 1), and
    kernels of the branch that are still queued on the side stream hold no reference: they then read a gradient that
    already contains the other branch's.  Found in round 5 (two processes sharing a GPU: one branch's layers below the
    injection point and the encoder stage under it got gradients 10 % off, run to run; tools/depth_eager_race.py)."""

    @staticmethod
    def backward(ctx, dy):
        return dy, dy.clone()


def add_shared(a, b):
    return _AddShared.apply(a, b)


class _Head1(torch.autograd.Function):
    """nn.Conv2d(C, 1, 1) [+ nn.ReLU] on an input that may carry padding channels (midas_net.py:139-140)."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        _chk(x, "x")
        N, H, W_, pitch = x.shape
        Cc = w.numel()
        M = N * H * W_
        out = torch.empty((N, H, W_), device=x.device, dtype=torch.float32)
        wd, bd = w.detach().reshape(-1).contiguous(), b.detach().reshape(-1).contiguous()
        _lib.check(_L().io_head1_fwd(_p(x), M, pitch, Cc, _p(wd), _p(bd), int(relu), _p(out), _dt(x), _st()), "io_head1_fwd")
        ctx.save_for_backward(x, out, wd)
        ctx.cfg = (M, pitch, Cc, int(relu), tuple(w.shape))
        return out

    @staticmethod
    def backward(ctx, dy):
        x, out, wd = ctx.saved_tensors
        M, pitch, Cc, relu, wshape = ctx.cfg
        L = _L()
        npart = int(L.io_colsum_partial_floats(M, Cc))
        part = torch.empty(npart, device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x)
        dw, db = torch.empty(Cc, device=x.device), torch.empty(1, device=x.device)
        _lib.check(L.io_head1_bwd(_p(dy.float().contiguous()), _p(out), _p(x), M, pitch, Cc, _p(wd), relu, _p(dx), _p(dw),
                                  _p(db), _p(part), npart, _dt(x), _st()), "io_head1_bwd")
        return dx, dw.view(wshape), db, None


def head1(x, w, b, relu):
    return _Head1.apply(x, w, b, relu)


# ---- the UNet-only operators of PCNet-M (models/backbone/unet/unet_parts.py), fp32 ------------------------------------------
def _chk32(t, name):
    _chk(t, name)
    if t.dtype != torch.float32:
        raise NotImplementedError("instaorder_amd.ops: %s must be fp32 (the UNet operators have no bf16 form)" % name)


class _MaxPool2x2(torch.autograd.Function):
    """nn.MaxPool2d(2) (unet_parts.py:36).  fork: x comes back as a second output (an alias), as in _ConvBn: the pooled tensor
    of a ``down`` block is also the skip tensor of an ``up`` block, and with the skip routed through the alias its gradient
    arrives HERE and rides in the `add` operand of io_maxpool2x2_bwd instead of an accumulation pass of the autograd engine
    over a full-resolution tensor."""

    @staticmethod
    def forward(ctx, x, fork):
        _chk32(x, "x")
        N, H, W_, Cc = x.shape
        out = torch.empty((N, H // 2, W_ // 2, Cc), device=x.device, dtype=x.dtype)
        _lib.check(_L().io_maxpool2x2_fwd(_p(x), N, H, W_, Cc, _p(out), _st()), "io_maxpool2x2_fwd")
        ctx.save_for_backward(x)
        return (out, x) if fork else out

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, = ctx.saved_tensors
        N, H, W_, Cc = x.shape
        if dy is None:                    # (only the skip path was used)
            return dskip, None
        dx = torch.empty_like(x)
        add = dskip.contiguous() if dskip is not None else None
        _lib.check(_L().io_maxpool2x2_bwd(_p(dy.contiguous()), _p(x), _p(add), N, H, W_, Cc, _p(dx), _st()),
                   "io_maxpool2x2_bwd")
        return dx, None


def max_pool_2x2(x, fork=False):
    """nn.MaxPool2d(2) on [N,H,W,C] (H, W even).  ``fork=True`` (x requires a gradient): returns ``(pooled, x_alias)``; route
    every other use of x through ``x_alias`` (see _MaxPool2x2)."""
    fork = bool(fork and torch.is_grad_enabled() and x.requires_grad)
    return _MaxPool2x2.apply(x, fork)


class _Up2xConcat(torch.autograd.Function):
    """cat([x2, upsample x2 (bilinear, align_corners=True) of x1], channel) (unet_parts.py:54-71, sizes that meet without F.pad)"""

    @staticmethod
    def forward(ctx, x2, x1):
        _chk32(x2, "x2")
        _chk32(x1, "x1")
        n, h, w, c1 = x1.shape
        c2 = x2.shape[3]
        if tuple(x2.shape[:3]) != (n, 2 * h, 2 * w):
            raise ValueError("up2x_concat: x2 %s is not twice x1 %s" % (tuple(x2.shape), tuple(x1.shape)))
        cat = torch.empty((n, 2 * h, 2 * w, c2 + c1), device=x1.device)
        _lib.check(_L().io_up2x_concat_fwd(_p(x2), _p(x1), n, h, w, c2, c1, _p(cat), _st()), "io_up2x_concat_fwd")
        ctx.geom = (n, h, w, c2, c1)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        n, h, w, c2, c1 = ctx.geom
        dx2 = torch.empty((n, 2 * h, 2 * w, c2), device=dcat.device)
        dx1 = torch.empty((n, h, w, c1), device=dcat.device)
        _lib.check(_L().io_up2x_concat_bwd(_p(dcat.contiguous()), n, h, w, c2, c1, _p(dx2), _p(dx1), _st()), "io_up2x_concat_bwd")
        return dx2, dx1


def up2x_concat(x2, x1):
    return _Up2xConcat.apply(x2, x1)


class _UnetHeadLoss(torch.autograd.Function):
    """The 1x1 head (outconv, unet_parts.py:74-81) and MaskWeightedCrossEntropyLoss (models/losses.py:60-88) over
    ``world_size`` as ONE node on the last activation x[N,H,W,Cs]: forward = io_unet_head in loss mode (no logits in memory),
    backward = io_unet_head_bwd, the incoming scalar gradient read on the device.  w [2,C,1,1] with the C real channels
    stored first; the gradients come back in the parameters' shapes."""

    @staticmethod
    def forward(ctx, x, w, b, mask, eraser, target, inmask_weight, world_size):
        _chk32(x, "x")
        N, H, W_, Cs = x.shape
        Cr = w.shape[1]
        wo = torch.zeros((2, Cs), device=x.device)
        wo[:, :Cr] = w.detach().reshape(2, Cr)
        bo = b.detach().float().contiguous()
        L = _L()
        nf = int(L.io_unet_head_partial_floats(N, H * W_))
        partials, sums = torch.empty(nf, device=x.device), torch.empty(2, device=x.device)
        _lib.check(L.io_unet_head(_p(x), _p(wo), _p(bo), _p(mask), _p(eraser), _p(target), N, H * W_, Cs, 0.5, None, None, None,
                                  _p(partials), nf, _p(sums), _st()), "io_unet_head")
        ctx.save_for_backward(x, wo, bo, eraser, target)
        ctx.cfg = (float(inmask_weight), 1.0 / (N * H * W_ * world_size), tuple(w.shape))
        return (float(inmask_weight) * sums[0] + 1.0 * sums[1]) / (N * H * W_) / world_size

    @staticmethod
    def backward(ctx, dl):
        x, wo, bo, eraser, target = ctx.saved_tensors
        iw, scale, wshape = ctx.cfg
        N, H, W_, Cs = x.shape
        L = _L()
        nf = int(L.io_unet_head_bwd_partial_floats(N, H * W_))
        partials = torch.empty(nf, device=x.device)
        dx = torch.empty_like(x)
        dwo, dbo = torch.empty((2, Cs), device=x.device), torch.empty(2, device=x.device)
        _lib.check(L.io_unet_head_bwd(_p(x), _p(wo), _p(bo), _p(target), _p(eraser), N, H * W_, Cs, iw, scale,
                                      _p(dl.float().contiguous()), _p(dx), _p(dwo), _p(dbo), None, _p(partials), nf, _st()),
                   "io_unet_head_bwd")
        return dx, dwo[:, :wshape[1]].reshape(wshape).contiguous(), dbo, None, None, None, None, None


def unet_head_loss(x, w, b, mask, eraser, target, inmask_weight, world_size=1):
    """-> the 0-d loss.  mask, eraser: fp32 [N,H,W]; target: uint8 [N,H,W] in {0, 1}; all contiguous, on the device."""
    return _UnetHeadLoss.apply(x, w, b, mask, eraser, target, inmask_weight, world_size)


class _SmoothLoss(torch.autograd.Function):
    """Edge-aware smoothness loss (models/supervised_order.py:214-235) of a disparity map disp[B,1,H,W] against the image
    img[B,3,H,W]: three launches forward, one backward (io_smooth_loss_*), the incoming scalar gradient read on the device.
    ``times``: the loss evaluated that many times on the same map (pair mode: both mask orders share the disparity)."""

    @staticmethod
    def forward(ctx, disp, img, times):
        if not (disp.is_cuda and disp.dtype == torch.float32 and img.dtype == torch.float32):
            raise RuntimeError("instaorder_amd.ops.smooth_loss: fp32 tensors on the GPU (no CPU fallback)")
        B, _, H, W_ = disp.shape
        d, im = disp.detach().contiguous(), img.detach().contiguous()
        L = _L()
        nws = int(L.io_smooth_loss_workspace_floats(B, H, W_))
        ws = torch.empty(nws, device=d.device, dtype=torch.float32)
        g = torch.empty((B, H, W_), device=d.device, dtype=torch.float32)
        loss = torch.empty((), device=d.device, dtype=torch.float32)
        _lib.check(L.io_smooth_loss_fwd(_p(d), _p(im), B, H, W_, float(times), _p(loss), _p(g), _p(ws), nws, _st()),
                   "io_smooth_loss_fwd")
        ctx.save_for_backward(g, ws)
        ctx.cfg = (B, H, W_, float(times), tuple(disp.shape))
        return loss

    @staticmethod
    def backward(ctx, dl):
        g, ws = ctx.saved_tensors
        B, H, W_, times, shape = ctx.cfg
        dd = torch.empty((B, H, W_), device=g.device, dtype=torch.float32)
        _lib.check(_L().io_smooth_loss_bwd(_p(g), _p(ws), _p(dl.float().contiguous()), times, B, H, W_, 0, _p(dd), _st()),
                   "io_smooth_loss_bwd")
        return dd.view(shape), None, None


def smooth_loss(disp, img, times=1):
    return _SmoothLoss.apply(disp, img, times)


def disp_order_count(disp1, disp2, modal1, modal2, depth_order1, is_overlap, le_order=0, scale=1.0):
    """supervised_order.py:152-173 for the whole batch in three launches (io_disp_order_count): erosion, masked max / min,
    comparisons and counts on the device, no host round trip; returns a 0-dim tensor = scale * total / (H * W)."""
    B, _, H, W_ = disp1.shape
    dev = disp1.device
    out = torch.empty((), device=dev, dtype=torch.float32)
    nws = int(_L().io_disp_order_workspace_floats(B, H, W_))
    ws = torch.empty(max(nws, 1), device=dev, dtype=torch.float32)
    f = lambda t: t.detach().float().contiguous()       # noqa: E731
    _lib.check(_L().io_disp_order_count(_p(f(disp1)), _p(f(disp2)), _p(f(modal1)), _p(f(modal2)),
                                        _p(depth_order1.long().contiguous()), _p(is_overlap.long().contiguous()), B, H, W_,
                                        int(le_order), float(scale), _p(out), _p(ws), nws, _st()), "io_disp_order_count")
    return out
