"""The UNet of PCNet-M (models/backbone/unet/unet_model.py:51-91, unet_parts.py): the folded eval-mode plan and the
train-mode plan of autograd nodes ("Training" at the end of this text).

``UNet(in_channels, w, n_classes=2)`` is an ``nn.Module`` whose ``state_dict()`` has exactly the reference's keys, shapes
and dtypes (``inc.conv.conv.{0,1,3,4}.*``, ``down{1..4}.mpconv.1.conv.*``, ``up{1..4}.conv.conv.*``,
``outc.conv.{weight,bias}``; convolution biases and ``num_batches_tracked`` kept), so a checkpoint the reference wrote
loads unchanged.  The eval-mode forward runs the plan

    inc -> down1..4 (io_maxpool2x2_fwd + double conv) -> up1..4 (io_up2x_concat_fwd + double conv) -> io_unet_head

on NHWC fp32 buffers.  Every conv + BatchNorm + ReLU is ONE launch: the BatchNorm and the convolution's bias are folded
(in fp64, rounded once) into scaled filters and a bias, rebuilt only when a weight changes.  Layers with at most 32 output
channels run io_conv3x3_co32_fwd, the others the dense launcher io_conv2d_fwd_bias_dt; with the route switch off
(``set_co32(False)``) the narrow layers run the dense launcher too, with their output channels padded to 64.

Channel padding.  A tensor of C real channels is STORED with ``stored(C)`` channels: 32 for C <= 32 on the 32-channel
route, else C rounded up to 64 (the widths of this family are powers of two, so that is "rounded up to 32" wherever the
32-channel kernel runs).  The padding filters and their bias are zero, so after bias + ReLU the padding channels hold
exactly 0, and max-pooling / interpolation keep them 0.  The concatenation of an ``up`` block joins the STORED tensors:
[x2 real | x2 padding | x1 real | x1 padding] -- a gap in the middle -- so a tensor carries its layout as a list of
(real, stored) segments and the next filter's input channels are scattered to the stored positions of that list
(``_stored_index``): real channel c of segment k sits at sum(stored of the segments before k) + (c - sum(real before k)).
unet1 (16-channel tensors stored as 32) exercises the gap; unet2's tensors have none.  The network input (2 planes) is
stored as 8 channels in front of the 32-channel kernel and as 32 in front of the dense launcher.

Training.  In ``train()`` mode ``forward(x)`` returns logits that carry autograd, and ``loss_train`` (what
``PartialCompletionMask.step`` calls) the loss through the fused head node.  The plan is the same network strung from
``ops.*`` nodes on the module's own parameters and BatchNorm buffers: ops.conv_bn / ops.conv2d + ops.batch_norm (chosen by
``bn_route``, by shape, in one place), ops.max_pool_2x2, ops.up2x_concat, ops.unet_head_loss.  The route switch does not
apply: every tensor, the network input included, is stored at its real width rounded up to 64 (``plan(False, cin=64)``),
where the dense launchers serve forward, data gradient and filter gradient.  ``_TrainFilter`` scatters a filter to that
layout (zero padding filters; the concatenation keeps ``_stored_index``'s segments) and slices its gradient back; gamma and
beta are zero-padded, so a padding channel is 0 * rstd + 0 = exactly 0 forward and gets exactly 0 gradient.
The reference's 3x3 convolutions carry a bias in front of a batch-statistics BatchNorm: it cancels in the output and
shifts only the batch mean.  It is not added; ``running_mean`` advances by momentum * bias on top of what the statistics
node wrote (the mean of conv + bias); and the bias gets a gradient of exact zeros (the reference's is rounding noise),
so weight decay and momentum move it as they do there.  The statistics nodes bump ops.WEIGHTS_EPOCH: the eval plan
re-folds after training.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops

_CO32_INPUTS = (8, 32, 64, 128)          # stored input widths io_conv3x3_co32_fwd takes
TRAIN_INPUT = 64                         # stored width of the network input on the training route


def set_co32(on):
    """Route switch of the layers with at most 32 output channels (see the module text); returns the previous value."""
    return bool(_lib.lib().io_set_unet_co32(1 if on else 0))


def get_co32():
    return bool(_lib.lib().io_get_unet_co32())


class double_conv(nn.Module):
    def __init__(self, in_ch, out_ch):
        super(double_conv, self).__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True),
                                  nn.Conv2d(out_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True))


class inconv(nn.Module):
    def __init__(self, in_ch, out_ch):
        super(inconv, self).__init__()
        self.conv = double_conv(in_ch, out_ch)


class down(nn.Module):
    def __init__(self, in_ch, out_ch):
        super(down, self).__init__()
        self.mpconv = nn.Sequential(nn.MaxPool2d(2), double_conv(in_ch, out_ch))


class up(nn.Module):
    def __init__(self, in_ch, out_ch):
        super(up, self).__init__()
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.conv = double_conv(in_ch, out_ch)


class outconv(nn.Module):
    def __init__(self, in_ch, out_ch):
        super(outconv, self).__init__()
        self.conv = nn.Conv2d(in_ch, out_ch, 1)


def stored(c, co32):
    """stored width of a tensor with c real channels"""
    return 32 if (co32 and c <= 32) else (c + 63) // 64 * 64


def _stored_index(segments):
    """segments: [(real, stored), ...] of a (concatenated) tensor -> (stored position of every real channel, stored width)"""
    idx, off = [], 0
    for real, st in segments:
        idx.extend(range(off, off + real))
        off += st
    return np.asarray(idx, np.int64), off


def fold_conv_bn(conv, bn):
    """eval-mode bn(conv(x)) == conv'(x) + b': (w' [Co,Ci,3,3], b' [Co]) in fp64"""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = conv.weight.detach().double() * scale.view(-1, 1, 1, 1)
    b = bn.bias.detach().double() + (conv.bias.detach().double() - bn.running_mean.detach().double()) * scale
    return w, b


def pack_filter(w, b, segments, co_stored, co32):
    """folded (w [Co,Ci,3,3], b [Co]) fp64 -> fp32 (operand, bias [co_stored]) for an input of layout ``segments``:
    co32: [9][Ci_stored][32] (io_conv3x3_co32_fwd); else [co_stored][9][Ci_stored] (the dense launcher)."""
    Co, Ci = w.shape[:2]
    idx, ci_stored = _stored_index(segments)
    assert len(idx) == Ci, (len(idx), Ci)
    idx = torch.from_numpy(idx).to(w.device)
    wk = torch.zeros((co_stored, 9, ci_stored), dtype=torch.float64, device=w.device)
    wk[:Co, :, idx] = w.permute(0, 2, 3, 1).reshape(Co, 9, Ci)
    bias = torch.zeros(co_stored, dtype=torch.float64, device=w.device)
    bias[:Co] = b
    if co32:
        wk = wk.permute(1, 2, 0)
    return wk.contiguous().float(), bias.float()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _TrainFilter(torch.autograd.Function):
    """The training operand of a 3x3 convolution in front of a batch-statistics BatchNorm: OIHW [Co,Ci,3,3] scattered to
    [co_st, ci_st, 3, 3] (zero padding filters, input channels at the stored positions ``idx``).  The gradient comes back
    sliced to the parameter's shape.  The convolution's bias is an input only to receive its gradient: exact zeros -- it
    cancels under batch statistics (module text, "Training")."""

    @staticmethod
    def forward(ctx, w, bias, idx, co_st, ci_st):
        co = w.shape[0]
        out = w.new_zeros((co_st, ci_st, 3, 3))
        out[:co, idx] = w.detach()
        ctx.idx, ctx.co = idx, co
        ctx.bias_like = bias.detach()
        return out

    @staticmethod
    def backward(ctx, dw):
        return dw[:ctx.co, ctx.idx].contiguous(), torch.zeros_like(ctx.bias_like), None, None, None


class HipTrainOps(object):
    """the operators UNet.features_train strings together, as launches (NHWC fp32 on the GPU)"""

    @staticmethod
    def pack_input(m1, m2, cs):
        N, H, W = m1.shape
        x = torch.empty((N, H, W, cs), device=m1.device)
        _lib.check(_lib.lib().io_unet_pack_input(_p(m1), _p(m2), None, N, H * W, cs, 0, _p(x), ops._st()), "io_unet_pack_input")
        return x

    @staticmethod
    def conv_bn_relu(x, w, gamma, beta, rm, rv, route):
        if route == "fused":
            return ops.conv_bn(x, w, gamma, beta, rm, rv, 1, 1, 1, True, relu=True)
        return ops.batch_norm(ops.conv2d(x, w, 1, 1), gamma, beta, rm, rv, True, relu=True)

    @staticmethod
    def max_pool_2x2(x):
        return ops.max_pool_2x2(x, fork=True)

    @staticmethod
    def up2x_concat(x2, x1):
        return ops.up2x_concat(x2, x1)


class UNet(nn.Module):
    def __init__(self, in_channels=3, w=4, n_classes=2, dtype="fp32"):
        super(UNet, self).__init__()
        if n_classes != 2:
            raise NotImplementedError("UNet: the head kernel (io_unet_head) is written for n_classes=2")
        c = [int(16 * w), int(32 * w), int(64 * w), int(128 * w)]
        self.inc = inconv(in_channels, c[0])
        self.down1 = down(c[0], c[1])
        self.down2 = down(c[1], c[2])
        self.down3 = down(c[2], c[3])
        self.down4 = down(c[3], c[3])
        self.up1 = up(2 * c[3], c[2])
        self.up2 = up(2 * c[2], c[1])
        self.up3 = up(2 * c[1], c[0])
        self.up4 = up(2 * c[0], c[0])
        self.outc = outconv(c[0], n_classes)
        self.in_channels, self.width, self.dtype = in_channels, c, dtype
        self._packed = {}

    # ---- folded operands, rebuilt when a weight, a running statistic or the route changes -----------------------------
    def _blocks(self):
        return [self.inc.conv] + [d.mpconv[1] for d in (self.down1, self.down2, self.down3, self.down4)] + \
               [u.conv for u in (self.up1, self.up2, self.up3, self.up4)]

    def input_stored(self, co32):
        return 8 if (co32 and self.width[0] <= 32) else 32

    def plan(self, co32, cin=None):
        """[(block index, conv index, segments of the input, real Co, stored Co, runs the 32-channel kernel)] of the 18
        3x3 convolutions, then the layout of the head's input.  ``cin``: stored width of the network input (default: what
        the eval route of ``co32`` packs)."""
        c = self.width
        out_real = [c[0], c[1], c[2], c[3], c[3], c[2], c[1], c[0], c[0]]
        seg = lambda r: (r, stored(r, co32))     # noqa: E731
        skips = [seg(c[0]), seg(c[1]), seg(c[2]), seg(c[3])]              # x1 .. x4
        first = [[(self.in_channels, cin or self.input_stored(co32))], [seg(c[0])], [seg(c[1])], [seg(c[2])], [seg(c[3])],
                 [skips[3], seg(c[3])], [skips[2], seg(c[2])], [skips[1], seg(c[1])], [skips[0], seg(c[0])]]
        steps = []
        for b in range(9):
            co = out_real[b]
            narrow = co32 and co <= 32
            for k, segs in enumerate((first[b], [seg(co)])):
                ci_stored = sum(s for _, s in segs)
                if narrow and ci_stored not in _CO32_INPUTS:
                    raise RuntimeError("UNet: no kernel for a 3x3 convolution of %d stored input channels to %d outputs"
                                       % (ci_stored, co))
                steps.append((b, 3 * k, segs, co, stored(co, co32), narrow))
        return steps, [seg(c[0])]

    def operands(self, co32):
        """the folded, packed operands of ``plan(co32)`` on the weights' device (no launch, no library call):
        ([(filter operand, bias, stored Ci, stored Co, runs the 32-channel kernel)] x 18, (wo [2][Cs], bo [2], Cs))"""
        steps, head_segs = self.plan(co32)
        blocks = self._blocks()
        layers = []
        with torch.no_grad():
            for b, k, segs, co, co_st, narrow in steps:
                seq = blocks[b].conv
                wop, bias = pack_filter(*fold_conv_bn(seq[k], seq[k + 1]), segs, co_st, narrow)
                layers.append((wop, bias, sum(s for _, s in segs), co_st, narrow))
            idx, cs = _stored_index(head_segs)
            wo = torch.zeros((2, cs), device=self.outc.conv.weight.device)
            wo[:, torch.from_numpy(idx).to(wo.device)] = self.outc.conv.weight.detach().reshape(2, -1).float()
            bo = self.outc.conv.bias.detach().float().contiguous()
        return layers, (wo.contiguous(), bo, cs)

    def packed(self):
        """the operands of the current route; one set is kept per route, so switching routes back and forth re-packs
        nothing while the weights stand"""
        co32 = get_co32()
        key = (ops.WEIGHTS_EPOCH[0], str(self.outc.conv.weight.device)) + \
            tuple(t._version for t in list(self.parameters()) + list(self.buffers()))
        hit = self._packed.get(co32)
        if hit is None or hit[0] != key:
            hit = self._packed[co32] = (key,) + self.operands(co32) + (co32,)
        return hit

    # ---- launches ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _conv(x, layer):
        wop, bias, ci_st, co_st, narrow = layer
        N, H, W, Cs = x.shape
        assert Cs == ci_st, (Cs, ci_st)
        y = torch.empty((N, H, W, co_st), device=x.device)
        L, st = _lib.lib(), ops._st()
        if narrow:
            _lib.check(L.io_conv3x3_co32_fwd(_p(x), _p(wop), _p(bias), _p(y), N, H, W, Cs, co_st, 1, st), "io_conv3x3_co32_fwd")
        else:
            _lib.check(L.io_conv2d_fwd_bias_dt(_p(x), _p(wop), _p(y), N, H, W, Cs, co_st, 3, 3, 1, 1, _p(bias), None, 1, 0, 0, st),
                       "io_conv2d_fwd_bias_dt")
        return y

    def _check(self, training=False):
        if self.training != training:
            raise RuntimeError("UNet: this path runs in %s mode, the module is in %s mode"
                               % (("eval", "train")[training], ("eval", "train")[self.training]))
        if self.dtype != "fp32":
            raise NotImplementedError("UNet: dtype=%r is not in the package yet (fp32 only)." % (self.dtype,))
        if self.in_channels != 2:
            raise NotImplementedError("UNet: the packed input is written for in_channels=2 (target and eraser planes).")

    def features(self, m1, m2, scale=None, erase=False):
        """m1, m2: [N,S,S] fp32 planes on the GPU (target, eraser) -> the last activation [N,S,S,Cs] and the head's operands.
        ``scale`` [N] multiplies the first plane; ``erase`` zeroes it where the second is 1 (inference.py:669, 674)."""
        self._check()
        _lib.require_gpu()
        N, H, W = m1.shape
        if H % 16 or W % 16:
            raise ValueError("UNet: the patch is %d x %d; both sides must be multiples of 16 (four 2x poolings whose skip "
                             "tensors meet the upsampled ones without the reference's F.pad)" % (H, W))
        _, layers, head, co32 = self.packed()
        L, st = _lib.lib(), ops._st()
        cin = self.input_stored(co32)
        x = torch.empty((N, H, W, cin), device=m1.device)
        _lib.check(L.io_unet_pack_input(_p(m1), _p(m2), _p(scale), N, H * W, cin, int(bool(erase)), _p(x), st),
                   "io_unet_pack_input")
        x = self._conv(self._conv(x, layers[0]), layers[1])
        skips = [x]
        for b in range(1, 5):
            n, h, w, cs = x.shape
            pooled = torch.empty((n, h // 2, w // 2, cs), device=x.device)
            _lib.check(L.io_maxpool2x2_fwd(_p(x), n, h, w, cs, _p(pooled), st), "io_maxpool2x2_fwd")
            x = self._conv(self._conv(pooled, layers[2 * b]), layers[2 * b + 1])
            skips.append(x)
        x = skips.pop()
        for b in range(5, 9):
            x2 = skips.pop()
            n, h, w, c1 = x.shape
            c2 = x2.shape[3]
            cat = torch.empty((n, 2 * h, 2 * w, c2 + c1), device=x.device)
            _lib.check(L.io_up2x_concat_fwd(_p(x2), _p(x), n, h, w, c2, c1, _p(cat), st), "io_up2x_concat_fwd")
            x = self._conv(self._conv(cat, layers[2 * b]), layers[2 * b + 1])
        return x, head

    def run(self, m1, m2, scale=None, erase=False, th=0.5, want_logits=False, target=None):
        """The whole forward with the head: dict(comp uint8 [N,S,S], counts int32 [N], logits [N,S,S,2] | None,
        loss_sums fp32 [2] (inside, outside the eraser) | None)"""
        m1, m2 = m1.contiguous().float(), m2.contiguous().float()
        x, (wo, bo, cs) = self.features(m1, m2, scale, erase)
        N, H, W = m1.shape
        L, st = _lib.lib(), ops._st()
        comp = torch.empty((N, H, W), dtype=torch.uint8, device=x.device)
        counts = torch.empty(N, dtype=torch.int32, device=x.device)
        logits = torch.empty((N, H, W, 2), device=x.device) if want_logits else None
        partials = sums = None
        nf = 0
        if target is not None:
            nf = L.io_unet_head_partial_floats(N, H * W)
            partials, sums = torch.empty(nf, device=x.device), torch.empty(2, device=x.device)
        _lib.check(L.io_unet_head(_p(x), _p(wo), _p(bo), _p(m1), _p(m2), _p(target), N, H * W, cs, float(th), _p(comp),
                                  _p(counts), _p(logits), _p(partials), nf, _p(sums), st), "io_unet_head")
        return dict(comp=comp, counts=counts, logits=logits, loss_sums=sums)

    # ---- training: the same network composed from autograd nodes of ops.py (module text, "Training") --------------------------
    @staticmethod
    def bn_route(rows):
        """how a conv -> BatchNorm -> ReLU unit runs in training, by its rows per BatchNorm group -- THE place that decides:
        'fused' = ops.conv_bn (statistics in the convolution's epilogue; its contract: whole 128-row tiles),
        'split' = ops.conv2d, then ops.batch_norm"""
        return "fused" if rows % 128 == 0 else "split"

    def _unit_train(self, x, conv, bn, segs, co_st, impl):
        """relu(bn(conv(x))) with batch statistics on the stored layout; the module's running estimates advanced as the
        reference's are"""
        co = conv.weight.shape[0]
        idx, ci_st = _stored_index(segs)
        assert x.shape[3] == ci_st, (tuple(x.shape), ci_st)
        w = _TrainFilter.apply(conv.weight, conv.bias, torch.from_numpy(idx).to(x.device), co_st, ci_st)
        gamma, beta = (nn.functional.pad(t, (0, co_st - co)) for t in (bn.weight, bn.bias))
        # the statistics nodes advance these in place; the padding channels (mean 0, variance 0) are dropped below
        rm, rv = x.new_zeros(co_st), x.new_ones(co_st)
        rm[:co], rv[:co] = bn.running_mean, bn.running_var
        out = impl.conv_bn_relu(x, w, gamma, beta, rm, rv, self.bn_route(x.shape[0] * x.shape[1] * x.shape[2]))
        with torch.no_grad():
            # the node saw conv(x) without the bias: the mean of conv(x) + bias is that mean + bias
            bn.running_mean.copy_(rm[:co]).add_(conv.bias, alpha=bn.momentum)
            bn.running_var.copy_(rv[:co])
            bn.num_batches_tracked += 1
        return out

    def features_train(self, m1, m2, impl=None):
        """m1, m2: [N,S,S] fp32 planes on the GPU -> the last activation [N,S,S,64] with its autograd graph.  ``impl``: the
        four operators the plan is strung from (default: HipTrainOps, the launches; the CPU tests pass torch functions of
        the same signatures to check the stored-layout algebra without a GPU)."""
        self._check(training=True)
        if impl is None:
            _lib.require_gpu()
            impl = HipTrainOps
        N, H, W = m1.shape
        if H % 16 or W % 16:
            raise ValueError("UNet: the patch is %d x %d; both sides must be multiples of 16" % (H, W))
        for blk in self._blocks():
            for k in (1, 4):
                if blk.conv[k].momentum is None or not blk.conv[k].track_running_stats:
                    raise NotImplementedError("UNet: BatchNorm with momentum=None / without running statistics")
        steps, head_segs = self.plan(False, cin=TRAIN_INPUT)
        blocks = self._blocks()
        x = impl.pack_input(m1, m2, TRAIN_INPUT)

        def double(x, b):
            for k in (0, 1):
                _, ck, segs, _, co_st, _ = steps[2 * b + k]
                x = self._unit_train(x, blocks[b].conv[ck], blocks[b].conv[ck + 1], segs, co_st, impl)
            return x

        x = double(x, 0)
        skips = []
        for b in range(1, 5):
            pooled, skip = impl.max_pool_2x2(x)       # (the skip's gradient rides in the pool backward's `add`)
            skips.append(skip)
            x = double(pooled, b)
        for b in range(5, 9):
            x = double(impl.up2x_concat(skips.pop(), x), b)
        assert head_segs[0][1] == x.shape[3]
        return x

    def loss_train(self, mask, eraser, target, inmask_weight, world_size=1):
        """training forward + MaskWeightedCrossEntropyLoss / world_size as the fused head node (no logits in memory):
        mask, eraser [N,1,S,S] fp32, target [N,S,S] in {0, 1} -> the 0-d loss, carrying autograd"""
        m1, m2 = mask[:, 0].contiguous().float(), eraser[:, 0].contiguous().float()
        x = self.features_train(m1, m2)
        return ops.unet_head_loss(x, self.outc.conv.weight, self.outc.conv.bias, m1, m2, target.to(torch.uint8).contiguous(),
                                  inmask_weight, world_size)

    def _forward_train(self, x):
        feat = self.features_train(x[:, 0].contiguous().float(), x[:, 1].contiguous().float())
        w = self.outc.conv.weight
        wp = nn.functional.pad(w, (0, 0, 0, 0, 0, feat.shape[3] - w.shape[1]))       # [2, 64, 1, 1]: real channels first
        logits = ops.bias_act(ops.conv2d(feat, wp, 1, 0, co_pad=True), self.outc.conv.bias)
        return logits[..., :2].permute(0, 3, 1, 2).contiguous()

    def forward(self, x):
        """[N,2,S,S] -> logits [N,2,S,S] (the reference's ``UNet.forward(x)``; it takes no image).  In train() mode the
        logits carry autograd and the BatchNorm buffers advance."""
        self._check(training=self.training)
        if self.training and not x.is_cuda:
            raise NotImplementedError("UNet.forward in training mode is written for the GPU only: the input must be a "
                                      "cuda tensor (there is no CPU fallback).")
        if not x.is_cuda:
            raise RuntimeError("instaorder_amd.unet: the input must be on the GPU (there is no CPU fallback)")
        if self.training:
            return self._forward_train(x)
        out = self.run(x[:, 0], x[:, 1], want_logits=True)
        return out["logits"].permute(0, 3, 1, 2).contiguous()


def unet025(in_channels, **kwargs):
    return UNet(in_channels, w=0.25, **kwargs)


def unet05(in_channels, **kwargs):
    return UNet(in_channels, w=0.5, **kwargs)


def unet1(in_channels, **kwargs):
    return UNet(in_channels, w=1, **kwargs)


def unet2(in_channels, **kwargs):
    return UNet(in_channels, w=2, **kwargs)


def unet4(in_channels, **kwargs):
    return UNet(in_channels, w=4, **kwargs)
