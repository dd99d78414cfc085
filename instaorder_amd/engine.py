"""Thin object layer over the C ABI: the ResNet-50 plan (`Net`) and the stand-alone ops.

Tensors are torch tensors used purely as device memory; every call is enqueued on torch's
current HIP stream and returns without synchronising.
"""
import ctypes as C

import torch

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_f32(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 tensor on the GPU" % name)
    return t


class Net(object):
    """Plan of resnet50_cls(in_channels, num_classes) -- mirrors models/backbone/resnet_cls.py:259-268.
    Creating it needs no GPU (it only lays out the flat parameter buffer)."""

    DTYPES = {"fp32": 0, "f32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}

    def __init__(self, in_channels=5, num_classes=2, dtype="fp32"):
        self.lib = _lib.lib()
        if dtype not in self.DTYPES:
            raise ValueError("dtype must be 'fp32' or 'bf16', got %r" % (dtype,))
        self.dtype = "bf16" if self.DTYPES[dtype] else "fp32"
        heads = list(num_classes) if isinstance(num_classes, (list, tuple)) else [int(num_classes)]
        self.head_dims = heads
        arr = (C.c_int * len(heads))(*heads)
        self.handle = self.lib.io_net_create(int(in_channels), len(heads), arr)
        if not self.handle:
            raise RuntimeError("io_net_create failed: " + _lib.last_error())
        _lib.check(self.lib.io_net_set_dtype(self.handle, self.DTYPES[dtype]), "io_net_set_dtype")
        self.in_channels = int(in_channels)
        self.param_floats = int(self.lib.io_net_param_floats(self.handle))
        self.running_floats = int(self.lib.io_net_running_floats(self.handle))
        self.num_logits = int(self.lib.io_net_num_logits(self.handle))
        self.tensors = []
        info = _lib.TensorInfo()
        for i in range(self.lib.io_net_num_tensors(self.handle)):
            _lib.check(self.lib.io_net_tensor_info(self.handle, i, C.byref(info)), "io_net_tensor_info")
            self.tensors.append(dict(name=info.name.decode(), kind=info.kind,
                                     shape=tuple(info.shape[k] for k in range(info.ndim)),
                                     offset=int(info.offset), numel_storage=int(info.numel_storage),
                                     cin_storage=int(info.cin_storage), bn_index=int(info.bn_index),
                                     running_offset=int(info.running_offset)))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.io_net_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def workspace_bytes(self, N, S, training):
        n = int(self.lib.io_net_workspace_bytes(self.handle, int(N), int(S), int(bool(training))))
        if n == 0:
            raise RuntimeError("io_net_workspace_bytes: " + _lib.last_error())
        return n

    def activation_offset(self, N, S, which):
        off = int(self.lib.io_net_activation_offset(self.handle, int(N), int(S), int(which)))
        if off < 0:
            raise RuntimeError("io_net_activation_offset: " + _lib.last_error())
        return off

    def forward(self, params, running, x8, N, S, G, training, ws, logits):
        _lib.require_gpu()
        _lib.check(self.lib.io_net_forward(self.handle, _ptr(params), _ptr(running), _ptr(x8), int(N), int(S),
                                           int(G), int(bool(training)), _ptr(ws), ws.numel() * ws.element_size(),
                                           _ptr(logits), _stream()), "io_net_forward")

    def workspace_bytes_hw(self, N, H, W):
        n = int(self.lib.io_net_workspace_bytes_hw(self.handle, int(N), int(H), int(W)))
        if n == 0:
            raise RuntimeError("io_net_workspace_bytes_hw: " + _lib.last_error())
        return n

    def forward_eval_hw(self, params, running, x8, N, H, W, ws, logits):
        """inference forward on H x W inputs (multiples of 32): the 'orig' mode of the reference's inference.py"""
        _lib.require_gpu()
        _lib.check(self.lib.io_net_forward_eval_hw(self.handle, _ptr(params), _ptr(running), _ptr(x8), int(N), int(H),
                                                   int(W), _ptr(ws), ws.numel() * ws.element_size(), _ptr(logits),
                                                   _stream()), "io_net_forward_eval_hw")

    EVAL_UNITS = 54          # stem, max-pool, per bottleneck a1, a2, (yd), out
    EVAL_CONVS = 53

    def eval_taps_bytes(self, N, H, W):
        n = int(self.lib.io_net_eval_taps_bytes(self.handle, int(N), int(H), int(W)))
        if n == 0:
            raise RuntimeError("io_net_eval_taps_bytes: " + _lib.last_error())
        return n

    def eval_tap_offset(self, N, H, W, which):
        off = int(self.lib.io_net_eval_tap_offset(self.handle, int(N), int(H), int(W), int(which)))
        if off < 0:
            raise RuntimeError("io_net_eval_tap_offset: " + _lib.last_error())
        return off

    def forward_eval_taps(self, params, running, x8, N, H, W, ws, logits, taps=None, routes=False):
        """forward_eval_hw with every unit copied into ``taps`` (uint8, eval_taps_bytes; layout: eval_tap_offset) --
        for unit-wise parity checks.  routes=True: returns the kernel family of each of the 53 convolution launches
        (io_debug_last_nt_route), else None"""
        _lib.require_gpu()
        r = (C.c_int32 * self.EVAL_CONVS)(*([-1] * self.EVAL_CONVS)) if routes else None
        _lib.check(self.lib.io_net_forward_eval_taps(
            self.handle, _ptr(params), _ptr(running), _ptr(x8), int(N), int(H), int(W), _ptr(ws),
            ws.numel() * ws.element_size(), _ptr(logits), None if taps is None else _ptr(taps),
            0 if taps is None else taps.numel() * taps.element_size(), r, self.EVAL_CONVS if routes else 0, _stream()),
            "io_net_forward_eval_taps")
        return [int(v) for v in r] if routes else None

    def backward(self, params, grads, x8, dlogits, N, S, G, ws, stages=None):
        """stages = (lo, hi): only the backward stages [lo, hi) of io_net_backward_stages (0 = heads + layer4 .. 3 =
        layer1 + stem); None = the whole pass"""
        _lib.require_gpu()
        if stages is None:
            _lib.check(self.lib.io_net_backward(self.handle, _ptr(params), _ptr(grads), _ptr(x8), _ptr(dlogits),
                                                int(N), int(S), int(G), _ptr(ws), ws.numel() * ws.element_size(),
                                                _stream()), "io_net_backward")
        else:
            _lib.check(self.lib.io_net_backward_stages(self.handle, _ptr(params), _ptr(grads), _ptr(x8), _ptr(dlogits),
                                                       int(N), int(S), int(G), _ptr(ws), ws.numel() * ws.element_size(),
                                                       int(stages[0]), int(stages[1]), _stream()),
                       "io_net_backward_stages")

    @property
    def backward_stages(self):
        return int(self.lib.io_net_backward_num_stages(self.handle))


TORCH_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16}


def pack_planes(planes, strides, N, H, W, out):
    """planes: list of (fp32 tensor, element offset) giving channel 0.. of sample 0; strides: floats between
    samples.  Writes out[N,H,W,8] (torch.cat + NCHW->NHWC + pad, supervised_order.py:537); ``out`` is fp32 or
    bf16 -- the storage type of the network that will read it."""
    _lib.require_gpu()
    n = len(planes)
    pa = (C.c_void_p * n)(*[t.data_ptr() + 4 * off for t, off in planes])
    sa = (C.c_long * n)(*[int(s) for s in strides])
    if out.dtype not in (torch.float32, torch.bfloat16) or not out.is_contiguous():
        raise ValueError("pack_planes: out must be a contiguous fp32 or bf16 tensor")
    _lib.check(_lib.lib().io_pack_planes_nhwc8_dt(pa, sa, n, int(N), int(H), int(W), _ptr(out),
                                                  1 if out.dtype == torch.bfloat16 else 0, _stream()),
               "io_pack_planes_nhwc8_dt")


def pack_nchw(x, out=None, dtype="fp32"):
    """x[N,C<=5,H,W] (NCHW fp32) -> [N,H,W,8] of ``dtype``."""
    _dev_f32(x, "x")
    N, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((N, H, W, 8), device=x.device, dtype=TORCH_DTYPE[dtype])
    pack_planes([(x, c * H * W) for c in range(Cc)], [Cc * H * W] * Cc, N, H, W, out)
    return out


def pack_pair_directions(rgb, modal1, modal2, out=None, dtype="fp32"):
    """Both mask orders of a pair batch in one buffer: rows [0,B) = (modal1, modal2, rgb), rows
    [B,2B) = (modal2, modal1, rgb) -- the two model calls of supervised_order.py:537-538.  ``rgb=None``
    is the reference's ``use_rgb=False`` form (masks only)."""
    for t, nme in ((rgb, "rgb"), (modal1, "modal1"), (modal2, "modal2")):
        if t is not None:
            _dev_f32(t, nme)
    B, _, H, W = modal1.shape
    if out is None:
        out = torch.empty((2 * B, H, W, 8), device=modal1.device, dtype=TORCH_DTYPE[dtype])
    HW = H * W
    rgbp = [(rgb, c * HW) for c in range(3)] if rgb is not None else []
    st = [HW, HW] + [3 * HW] * len(rgbp)
    pack_planes([(modal1, 0), (modal2, 0)] + rgbp, st, B, H, W, out[:B])
    pack_planes([(modal2, 0), (modal1, 0)] + rgbp, st, B, H, W, out[B:])
    return out


def order_loss(logits, B, Kocc, Kdep, occ_target=None, depth_target=None, is_overlap=None,
               overlap_weight=0.0, distinct_weight=0.0, inv_world=1.0, want_grad=True):
    """losses[3] = (total/world, occlusion, depth) and d(total/world)/dlogits."""
    _lib.require_gpu()
    N = logits.shape[0]
    losses = torch.empty(3, device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits) if want_grad else None
    _lib.check(_lib.lib().io_order_loss(_ptr(logits), int(N), int(B), int(Kocc), int(Kdep), _ptr(occ_target),
                                        _ptr(depth_target), _ptr(is_overlap), float(overlap_weight),
                                        float(distinct_weight), float(inv_world), _ptr(losses), _ptr(dlogits),
                                        _stream()), "io_order_loss")
    return losses, dlogits


def sgd_momentum(params, grads, buf, lr, momentum, weight_decay, clip_state=None):
    """clip_state: the record of the grad_norm() call enqueued before this one -- the update runs on grads * coef, or
    not at all when the norm was not finite (io_sgd_momentum_clipped); None: the plain update."""
    _lib.require_gpu()
    if clip_state is None:
        _lib.check(_lib.lib().io_sgd_momentum(_ptr(params), _ptr(grads), _ptr(buf), params.numel(), float(lr),
                                              float(momentum), float(weight_decay), _stream()), "io_sgd_momentum")
    else:
        _lib.check(_lib.lib().io_sgd_momentum_clipped(_ptr(params), _ptr(grads), _ptr(buf), params.numel(), float(lr),
                                                      float(momentum), float(weight_decay), _ptr(_clip_record(clip_state)),
                                                      _stream()), "io_sgd_momentum_clipped")


def adam_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, begin=0, end=None,
              clip_state=None):
    """torch.optim.Adam's update of the elements [begin, end) of the flat fp32 buffers, all at step count ``step``
    (>= 1, the count after this update); the bias corrections are computed here in double, as torch does.  clip_state: as
    in sgd_momentum (io_adam_step_clipped)."""
    _lib.require_gpu()
    end = params.numel() if end is None else end
    for t in (grads, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == params.numel()
    assert params.dtype == torch.float32 and params.is_contiguous() and 0 <= begin <= end <= params.numel()
    assert begin % 4 == 0, "adam_step: begin must keep 16-byte alignment"
    bc1 = 1.0 - float(beta1) ** int(step)
    bc2 = 1.0 - float(beta2) ** int(step)

    def at(t):
        return C.c_void_p(t.data_ptr() + 4 * begin)
    if clip_state is None:
        _lib.check(_lib.lib().io_adam_step(at(params), at(grads), at(exp_avg), at(exp_avg_sq), end - begin, float(lr),
                                           float(beta1), float(beta2), float(eps), float(weight_decay), bc1, bc2, _stream()),
                                           "io_adam_step")
    else:
        _lib.check(_lib.lib().io_adam_step_clipped(at(params), at(grads), at(exp_avg), at(exp_avg_sq), end - begin,
                                                   float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                                   bc1, bc2, _ptr(_clip_record(clip_state)), _stream()),
                   "io_adam_step_clipped")


# ---- global gradient norm / clipping record (io_grad_norm) ---------------------------------------------------------
CLIP_STATE_BYTES = C.sizeof(_lib.ClipState)          # 64


def _clip_record(t):
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == CLIP_STATE_BYTES):
        raise ValueError("clip_state must be the %d-byte uint8 device record of new_clip_state()" % CLIP_STATE_BYTES)
    return t


def new_clip_state(device):
    """A zeroed io_clip_state record on ``device`` (a uint8 tensor of 64 bytes; read_clip_state decodes it)."""
    return torch.zeros(CLIP_STATE_BYTES, dtype=torch.uint8, device=device)


def read_clip_state(state):
    """The record as a dict (synchronises: one 64-byte copy to the host)."""
    raw = _lib.ClipState.from_buffer_copy(bytes(state.cpu().numpy().tobytes()))
    return dict(norm=float(raw.norm), coef=float(raw.coef), nonfinite=int(raw.nonfinite),
                steps=int(raw.steps), clipped=int(raw.clipped), skipped=int(raw.skipped))


def grad_norm_chunk():
    """floats one block of io_grad_norm sums"""
    return int(_lib.lib().io_grad_norm_chunk_floats())


def grad_norm_workspace_bytes(n, nseg=1):
    return int(_lib.lib().io_grad_norm_workspace_bytes(int(n), int(nseg)))


def grad_norm(grads, max_norm, state, seg_offsets=None, workspace=None, seg_sumsq=None):
    """Sum of squares of the flat fp32 buffer ``grads`` in fp64, per segment (``seg_offsets``: nseg + 1 increasing float
    offsets from 0 to grads.numel(), multiples of 4; None: one segment) and in total, and the clipping record for
    ``max_norm`` (> 0; inf: measure only) in ``state`` (new_clip_state).  Two launches, nothing allocated when
    ``workspace`` (uint8, grad_norm_workspace_bytes) and ``seg_sumsq`` (float64[nseg]) are given -- capturable.  Returns
    seg_sumsq (device float64)."""
    _lib.require_gpu()
    _dev_f32(grads, "grads")
    n = grads.numel()
    offs = [0, n] if seg_offsets is None else [int(o) for o in seg_offsets]
    nseg = len(offs) - 1
    need = grad_norm_workspace_bytes(n, nseg)
    if workspace is None:
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=grads.device)
    if seg_sumsq is None:
        seg_sumsq = torch.empty(max(nseg, 1), dtype=torch.float64, device=grads.device)
    if not (seg_sumsq.is_cuda and seg_sumsq.dtype == torch.float64 and seg_sumsq.is_contiguous()
            and seg_sumsq.numel() >= nseg):
        raise ValueError("seg_sumsq must be a contiguous float64 device tensor of at least %d elements" % nseg)
    if not (workspace.is_cuda and workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous device tensor")
    arr = (C.c_size_t * len(offs))(*offs)
    _lib.check(_lib.lib().io_grad_norm(_ptr(grads), n, arr, nseg, float(max_norm), _ptr(workspace),
                                       workspace.numel() * workspace.element_size(), _ptr(seg_sumsq),
                                       _ptr(_clip_record(state)), _stream()), "io_grad_norm")
    return seg_sumsq


_prof_on = False


def set_winograd(on):
    """Product form of the fp32 3x3 stride-1 layers: True = Winograd row forms where the shape allows (default; env
    IO_WINOGRAD=0 starts a process with them off), False = the direct implicit GEMM everywhere.  Returns the previous
    setting.  A captured hipGraph keeps the form it was captured with."""
    return bool(_lib.lib().io_set_winograd(1 if on else 0))


def get_winograd():
    return bool(_lib.lib().io_get_winograd())


def prof_active():
    return _prof_on


def prof_begin(share_events=True):
    """Start HIP-event timing of every library launch (per kernel class, on the launch stream).  share_events=False:
    own start event per launch group -- for op-by-op graphs (instaorder_amd.ops), where torch kernels and host gaps sit
    between the library's launches and must not be charged to them."""
    global _prof_on
    _lib.check(_lib.lib().io_prof_begin_ex(1 if share_events else 0), "io_prof_begin_ex")
    _prof_on = True


def prof_launches(max_entries=8192):
    """Per-launch records of the running profile, in launch order: [(class, ms, flops, bytes)] (synchronises)."""
    arr = (_lib.ProfEntry * max_entries)()
    n = _lib.lib().io_prof_launches(arr, max_entries)
    return [(arr[i].name.decode(), float(arr[i].total_ms), float(arr[i].flops), float(arr[i].bytes)) for i in range(n)]


def prof_end():
    """Stop and return {class name: dict(launches, total_ms, flops, bytes, flops_executed)} (synchronises); flops = the
    algorithmic count of the direct convolution, flops_executed = what the matrix pipes multiplied (Winograd forms: less)."""
    global _prof_on
    _prof_on = False
    arr = (_lib.ProfEntry * 32)()
    n = _lib.lib().io_prof_end(arr, 32)
    return {arr[i].name.decode(): dict(launches=int(arr[i].launches), total_ms=float(arr[i].total_ms),
                                       flops=float(arr[i].flops), bytes=float(arr[i].bytes),
                                       flops_executed=float(arr[i].flops_executed)) for i in range(n)}
