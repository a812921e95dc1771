"""torchvision-style ResNet feature extractors (BasicBlock: ResNet-18 / ResNet-34; Bottleneck: ResNet-50) on the MI355X kernels —
SURVEY.md §8 f4.

The reference builds ``nn.Sequential(*list(resnet34(...).children())[:-2])`` for the frames and
``nn.Sequential(*list(resnet18(...).children())[:-1])`` for the sketch (backbone.py:133-152) and turns the frame feature
maps into tokens (backbone.py:72-89).  This module keeps that Sequential's child indices — ``0`` conv1, ``1`` bn1, ``4``-``7``
layer1-4 — so the ``backbone.{video,sketch}_backbone.*`` keys of a reference checkpoint load unchanged, and uses
``nn.Conv2d`` / ``nn.BatchNorm2d`` purely as parameter containers.  Arithmetic (svol_amd/csrc/resnet.hip + the GEMMs):

  conv + eval-mode BatchNorm (+ identity) (+ ReLU)  =  svol_conv_nhwc (implicit GEMM: the tile kernel gathers its A operand from
  the NHWC activation, no im2col matrix; the stem and odd widths: svol_im2col -> svol_gemm_nt) with the BatchNorm scale folded into the
  weights ([Cout, kh*kw*Cin], (ky,kx,c) order, K padded to 32), the BatchNorm shift as bias and the ReLU — for a block's second
  convolution the ReLU AFTER the identity add (SVOL_ACT_RELU_RES) — in the GEMM epilogue; 3x3 s2 max pooling and the sketch
  branch's global average pooling are their own kernels; activations are NHWC from the stem to the tokens.

Two modes.  Frozen / eval (the default; BatchNorm uses its running statistics, folded into the weights as above, no backward).
``trainable=True`` and ``.train()``: what the reference's training step runs (train.py:72 puts EVERY parameter of build_model(args)
into the optimiser, and ``model.train()`` puts torchvision's BatchNorm into batch-statistics mode): every conv -> BatchNorm (-> +identity)
(-> ReLU) unit is one autograd Function (``_ConvBnFn``) over csrc/resnet_train.hip —

  forward   z = conv(x) (svol_conv_nhwc / im2col + GEMM, no bias) ; batch mean / biased variance per channel (two column passes) ;
            y = relu?(z * gamma * rstd + (beta - mean * gamma * rstd) + identity) ; running statistics updated with the UNBIASED variance
  backward  g = dy * [y > 0] ; dbeta = sum g, dgamma = sum g * xhat ; dz = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)) ; d identity = g ;
            dW = dz^T im2col(x) (svol_gemm_tn) ; dx = col2im(dz W) (svol_gemm_nt + svol_col2im_nhwc)

— plus max pooling with its argmax and the sketch branch's average pooling as Functions.  Activations bf16 / fp16 NHWC, statistics,
parameters and parameter gradients fp32.

Bottleneck (ResNet-50, backbone.py:143-147: frames ``[:-2]``, sketch ``[:-1]``, 2048-wide features): three units per block —
conv1 1x1, conv2 3x3 CARRYING the stride (torchvision's v1.5 layout), conv3 1x1 to 4 * planes with the ReLU after the identity add — and
a downsample in the first block of every stage (stage 4 too: 64 -> 256 at stride 1).  The same units in both modes; the 1x1 stride-1
data gradients go through the same-size-convolution branch of ``_ConvBnFn.backward``, the stride-2 3x3 and the stride-2 1x1 downsample
through GEMM + col2im.  ``nn.Sequential(*list(torchvision.models.resnet50().children())[:-2])`` state dicts load as they are.

compute_dtype: 'bf16' (default), 'fp16' (what the reference's apex amp runs; both modes) or 'fp32' (frozen mode only, explicit
im2col + fp32 GEMM).  fp16 runs the same kernels with fp16 operands (v_mfma_*_f16 at bf16's rate, three more mantissa bits, five
exponent bits).  Nothing clamps a forward activation: every convolution output before its BatchNorm, every unit's output and the
loss-scaled dz must fit 65504 — they do by orders of magnitude on ImageNet-normalised pixels (profiles/resnet_fp16.md) — and the
frozen path's folded weights are checked by refold().  Gradients reach the fp32 parameters through the same buckets as the head's,
so FlatAdamW.loss_scale / DynamicLossScaler cover the backbone with nothing added.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops, params, wgrad
from ..ingest import FrameIngest, is_raw_frames, sketch_frames

_DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32,
           torch.bfloat16: torch.bfloat16, torch.float16: torch.float16, torch.float32: torch.float32}
_H16 = (torch.bfloat16, torch.float16)
_NHWC_OUT = {torch.bfloat16: 'nhwc_bf16', torch.float16: 'nhwc_f16'}


class BasicBlock(nn.Module):
    """torchvision.models.resnet.BasicBlock parameter layout: conv1, bn1, conv2, bn2, downsample.{0,1}."""

    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        self.stride = stride


class Bottleneck(nn.Module):
    """torchvision.models.resnet.Bottleneck parameter layout: conv1/bn1 (1x1), conv2/bn2 (3x3, carries the stride), conv3/bn3 (1x1 to
    4 * planes), downsample.{0,1}."""
    expansion = 4

    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, 1, 0, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, 1, 0, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.downsample = None
        if stride != 1 or inplanes != planes * self.expansion:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * self.expansion, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes * self.expansion))
        self.stride = stride


def _fold(conv: nn.Conv2d, bn: nn.BatchNorm2d, dtype):
    """(W' [Cout, Kp] in `dtype`, shift [Cout] fp32): eval-mode BatchNorm folded into the convolution, K = kh*kw*Cin in
    (ky, kx, c) order, zero-padded to a multiple of 32.  The product W * gamma / sqrt(var + eps) is formed in fp32 and rounded once."""
    w = conv.weight.detach().float()
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    w = (w * scale[:, None, None, None]).permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    K = w.shape[1]
    Kp = (K + 31) // 32 * 32
    if Kp != K:
        w = torch.cat([w, torch.zeros((w.shape[0], Kp - K), dtype=w.dtype, device=w.device)], dim=1)
    return w.to(dtype).contiguous(), shift.contiguous()


def _w16(weight, dtype):
    """[Cout, Cin, kh, kw] fp32 -> [Cout, Kp] compute dtype, (ky, kx, c) order, K padded to a multiple of 32 (the GEMMs' layout)."""
    return ops.conv_weight_pack(weight, dtype)


def _bn_forward(z, bn, gamma, beta, residual, relu, sync=False):
    """train-mode BatchNorm of the conv output z [M, C] (+ identity) (+ ReLU); updates bn's running statistics as nn.BatchNorm2d does."""
    if bn.momentum is None:
        raise NotImplementedError('BatchNorm2d(momentum=None) (cumulative average) is not on the reference path')
    track = bn.track_running_stats and bn.running_mean is not None
    mean, rstd, scale, shift = ops.bn_train_stats(z, gamma.detach(), beta.detach(), bn.running_mean if track else None,
                                                  bn.running_var if track else None, bn.momentum, bn.eps, sync)
    if track:
        with torch.no_grad():
            bn.num_batches_tracked += 1
    return ops.bn_apply(z, scale, shift, residual, relu), mean, rstd


def _weight_grad(dz, make_dwp, weight, sink, keep):
    """dW of a convolution in the parameter's own layout: make_dwp() -> dz^T im2col(x) as [Cout, Kp] fp32 (svol_conv_wgrad_nhwc: the im2col
    view gathered inside the weight-gradient GEMM; the stem: svol_gemm_tn on its kept im2col matrix), folded back by one kernel.
    With a gradient sink (the parameter's .grad is a view of a BucketedGradAllReduce bucket) the three launches go to the
    weight-gradient stream (svol_amd.wgrad: nobody needs dW before the optimiser; the dx chain behind
    it is the backward's critical path) and add straight into the bucket: returns None.  `keep`: tensors the side stream reads."""
    def run(ws):
        with torch.cuda.stream(ws):
            ops.conv_weight_unpack_add(make_dwp(), sink.view.view(weight.shape))

    # (the backbone's weight gradients are never queued behind an attention backward and stay in line under any stream capture)
    if sink is not None and wgrad.issue(run, keep, torch.cuda.current_stream(dz.device), defer=False, capture_ok=False):
        return None
    dW = torch.zeros_like(weight, dtype=torch.float32, memory_format=torch.contiguous_format)
    ops.conv_weight_unpack_add(make_dwp(), dW)
    if sink is not None:
        sink.view.view(weight.shape).add_(dW)
        return None
    return dW


class _ConvBnFn(torch.autograd.Function):
    """y [n*ho*wo, Cout] = relu?(BatchNorm_train(conv(x)) + identity) on NHWC activations; see the module docstring."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, identity, geom, relu, bn, dt, sync=False):
        n, H, W, C, kh, kw, stride, pad = geom
        w16 = _w16(weight, dt)
        z, Ho, Wo = ops.conv_nhwc(x, w16, None, ops.ACT_NONE, n, H, W, C, kh, kw, stride, pad)
        y, mean, rstd = _bn_forward(z, bn, gamma, beta, identity, relu, sync)
        ctx.geom, ctx.relu, ctx.has_id, ctx.out_hw, ctx.sync = geom, relu, identity is not None, (Ho, Wo), sync
        ctx.sink = params.claim(weight, ctx.needs_input_grad[1])
        ctx.save_for_backward(x, weight, w16, z, y if relu else None, mean, rstd, gamma.detach())
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, w16, z, y, mean, rstd, gamma = ctx.saved_tensors
        n, H, W, C, kh, kw, stride, pad = ctx.geom
        Ho, Wo = ctx.out_hw
        dz, did, dgamma, dbeta = ops.bn_bwd(dy.contiguous(), y, z, mean, rstd, gamma, ctx.has_id and ctx.needs_input_grad[4], ctx.sync)
        Cout = weight.shape[0]
        dW = None
        if ctx.needs_input_grad[1]:
            def dwp():
                d = ops.conv_wgrad_nhwc(dz, x, n, H, W, C, kh, kw, stride, pad, w16.shape[1])
                if d is None:   # a shape the gathering kernel does not take: the explicit matrix
                    d = ops.gemm_tn(dz, ops.im2col(x, n, H, W, C, kh, kw, stride, pad, x.dtype, ldcols=w16.shape[1])[0])
                return d
            dW = _weight_grad(dz, dwp, weight, ctx.sink, (x, dz))
        dx = None
        if ctx.needs_input_grad[0]:
            if stride == 1 and 2 * pad == kh - 1 and kh == kw:
                # the data gradient of a "same" stride-1 convolution is the convolution of dz with the reversed taps and swapped channels:
                # the implicit-GEMM kernel again, no [M, 9 C] matrix
                dx = ops.conv_nhwc(dz, ops.conv_weight_pack(weight, x.dtype, flip=True), None, ops.ACT_NONE, n, Ho, Wo, Cout, kh, kw, 1, pad)[0]
            else:
                dx = ops.col2im_nhwc(ops.gemm_nt(dz, w16.t().contiguous()), n, H, W, C, kh, kw, stride, pad)
        return dx, dW, dgamma if ctx.needs_input_grad[2] else None, dbeta if ctx.needs_input_grad[3] else None, did, None, None, None, None, None


def _pixel_geom(pix, nhwc):
    """(n, c, H, W, element strides (sn, sh, sw, sc)) of the stem's input: NCHW pixels, or the NHWC image FrameIngest writes"""
    if nhwc:
        n, H, W, c = pix.shape
        return n, c, H, W, (H * W * c, W * c, c, 1)
    n, c, H, W = pix.shape
    return n, c, H, W, (c * H * W, W, 1, H * W)


class _StemFn(torch.autograd.Function):
    """pixels [n,3,H,W] fp32 (nhwc: [n,H,W,3] in the compute dtype, what FrameIngest writes) -> relu(BatchNorm_train(conv7x7 s2 p3)) as
    NHWC [n*ho*wo, C]; no gradient for the pixels."""

    @staticmethod
    def forward(ctx, pix, weight, gamma, beta, bn, dt, sync=False, nhwc=False):
        n, c, H, W, strides = _pixel_geom(pix, nhwc)
        w16 = _w16(weight, dt)
        kh, kw = weight.shape[2], weight.shape[3]
        cols, Ho, Wo = ops.im2col(pix, n, H, W, c, kh, kw, 2, 3, dt, strides=strides, ldcols=w16.shape[1])
        z = ops.gemm_nt(cols, w16)
        y, mean, rstd = _bn_forward(z, bn, gamma, beta, None, True, sync)
        ctx.sync = sync
        ctx.sink = params.claim(weight, ctx.needs_input_grad[1])
        # the stem's im2col matrix is KEPT for the weight gradient (1 GB at 256 frames of 224 x 224 — 0.4 % of this part's HBM; building
        # it again from the NCHW fp32 pixels costs 0.6 ms) — unless the stem's weight takes no gradient
        ctx.save_for_backward(cols if ctx.needs_input_grad[1] else None, weight, z, y, mean, rstd, gamma.detach())
        return y

    @staticmethod
    def backward(ctx, dy):
        cols, weight, z, y, mean, rstd, gamma = ctx.saved_tensors
        if not any(ctx.needs_input_grad[1:4]):   # a frozen stem: the pixels take no gradient either, nothing to compute
            return None, None, None, None, None, None, None, None
        dz, _, dgamma, dbeta = ops.bn_bwd(dy.contiguous(), y, z, mean, rstd, gamma, False, ctx.sync)
        dW = _weight_grad(dz, lambda: ops.gemm_tn(dz, cols), weight, ctx.sink, (cols, dz)) if ctx.needs_input_grad[1] else None
        return None, dW, dgamma if ctx.needs_input_grad[2] else None, dbeta if ctx.needs_input_grad[3] else None, None, None, None, None


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, geom):
        n, H, W, C, k, stride, pad = geom
        y, idx, Ho, Wo = ops.maxpool_idx_nhwc(x, n, H, W, C, k, stride, pad)
        ctx.geom = geom
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, H, W, C, k, stride, pad = ctx.geom
        return ops.maxpool_bwd_nhwc(dy.contiguous(), ctx.saved_tensors[0], n, H, W, C, k, stride, pad), None


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n, HW, C):
        ctx.shape, ctx.dt = (n, HW, C), x.dtype
        return ops.avgpool_nhwc(x, n, HW, C)

    @staticmethod
    def backward(ctx, dy):
        n, HW, C = ctx.shape
        return (dy.float() / HW).to(ctx.dt).view(n, 1, C).expand(n, HW, C).reshape(n * HW, C).contiguous(), None, None, None


class ResNetExtractor(nn.Module):
    def __init__(self, depths=(2, 2, 2, 2), widths=(64, 128, 256, 512), stem=64, avgpool=False, compute_dtype='bf16', trainable=False,
                 sync_bn=False, block='basic'):
        super().__init__()
        if block not in ('basic', 'bottleneck'):
            raise ValueError(f"block must be 'basic' or 'bottleneck', got {block!r}")
        self.block = block   # 'bottleneck': widths are the blocks' planes, a stage's output has 4 x as many channels
        expansion = Bottleneck.expansion if block == 'bottleneck' else 1
        # --sync_bn (apex.parallel.convert_syncbn_model, train.py:65-68 / test.py:61): train-mode BatchNorm statistics over the
        # GLOBAL batch of all ranks of the default process group; no effect at world size 1 or on the frozen extractor
        self.sync_bn = bool(sync_bn)
        self.add_module('0', nn.Conv2d(3, stem, 7, 2, 3, bias=False))
        self.add_module('1', nn.BatchNorm2d(stem))
        inplanes = stem
        for li, (n, planes) in enumerate(zip(depths, widths)):
            blocks = []
            for bi in range(n):
                blocks.append((Bottleneck if block == 'bottleneck' else BasicBlock)(inplanes, planes, (1 if li == 0 else 2) if bi == 0 else 1))
                inplanes = planes * expansion
            self.add_module(str(4 + li), nn.Sequential(*blocks))
        self.n_layers = len(depths)
        self.out_channels = inplanes
        self.avgpool = avgpool
        self.compute_dtype = _DTYPES[compute_dtype]
        self._folded = None
        self.register_load_state_dict_post_hook(lambda m, _k: setattr(m, '_folded', None))
        self.trainable = bool(trainable)
        for p in self.parameters():
            p.requires_grad_(self.trainable)

    def _apply(self, fn, *a, **kw):  # .to() / .cuda() move the parameters: fold again on the new device
        self._folded = None
        return super()._apply(fn, *a, **kw)

    def refold(self):
        """(re)build the folded compute-dtype weights; call after editing parameters in place.  fp16: a folded weight that is not finite
        after the cast (a BatchNorm channel with a tiny running variance scales its filter past 65504; bf16 has fp32's range and cannot
        overflow there) raises a ValueError that names the unit — checked here, once per fold, not per step."""
        dt = self.compute_dtype
        units = []

        def fold(name, conv, bn):
            w, b = _fold(conv, bn, dt)
            units.append((name, w))
            return w, b
        f = {'stem': fold('0', getattr(self, '0'), getattr(self, '1')), 'blocks': []}
        for li in range(self.n_layers):
            for bi, blk in enumerate(getattr(self, str(4 + li))):
                pre = f'{4 + li}.{bi}.'
                convs = [fold(pre + 'conv1', blk.conv1, blk.bn1), fold(pre + 'conv2', blk.conv2, blk.bn2)]
                if self.block == 'bottleneck':
                    convs.append(fold(pre + 'conv3', blk.conv3, blk.bn3))
                f['blocks'].append((blk.stride, blk.conv1.out_channels, *convs,
                                    fold(pre + 'downsample.0', blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None))
        if dt == torch.float16:
            finite = torch.stack([torch.isfinite(w).all() for _, w in units]).tolist()   # one host read for the whole fold
            bad = [name for (name, _), ok in zip(units, finite) if not ok]
            if bad:
                raise ValueError(f'ResNetExtractor(compute_dtype="fp16"): the BatchNorm-folded weights of {", ".join(bad)} exceed fp16\'s range '
                                 '(65504): a channel with a tiny running variance; use compute_dtype="bf16" for this checkpoint')
        self._folded = f
        return f

    def forward(self, pixel_values, nhwc=False):
        """pixel_values [n,3,H,W] fp32 (normalised as for torchvision's ImageNet weights) -> tokens [n, h*w, C] in the compute
        dtype (row-major over (h, w): the order backbone.py:85-87 flattens to), or [n, C] fp32 with ``avgpool``.
        ``nhwc=True``: pixel_values is [n,H,W,3], contiguous, already in the compute dtype — what FrameIngest(out='nhwc_bf16' /
        'nhwc_f16') writes; the stem reads it through svol_im2col's strides, and its im2col matrix has the bits of the fp32 route
        (one rounding to the 16-bit type either way)."""
        if not pixel_values.is_cuda:
            raise RuntimeError('svol_amd ResNetExtractor runs on the MI355X HIP kernels only (no CPU path)')
        if nhwc and (pixel_values.dtype != self.compute_dtype or not pixel_values.is_contiguous()):
            raise ValueError(f'nhwc pixels must be contiguous {self.compute_dtype}, got {pixel_values.dtype}')
        if self.training and self.trainable:
            return self._forward_train(pixel_values, nhwc)
        if self.training and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('parameters that require gradients need ResNetExtractor(trainable=True): the frozen path folds '
                                      'the running statistics into the weights and has no backward')
        with torch.no_grad():
            return self._forward_frozen(pixel_values, nhwc)

    def _forward_train(self, pixel_values, nhwc=False):
        """batch-statistics BatchNorm, autograd through every unit (module docstring); folded weights are invalidated."""
        dt = self.compute_dtype
        if dt not in _H16:
            raise NotImplementedError('the training path of the ResNet extractor keeps its activations in a 16-bit type '
                                      '(compute_dtype="bf16" or "fp16")')
        self._folded = None
        x = pixel_values if nhwc else pixel_values.float().contiguous()
        n, c, H, W, _ = _pixel_geom(x, nhwc)
        conv0, bn0 = getattr(self, '0'), getattr(self, '1')
        sync = self.sync_bn
        y = _StemFn.apply(x, conv0.weight, bn0.weight, bn0.bias, bn0, dt, sync, nhwc)
        H, W, C = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1, conv0.out_channels
        y = _MaxPoolFn.apply(y, (n, H, W, C, 3, 2, 1))
        H, W = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        for li in range(self.n_layers):
            for blk in getattr(self, str(4 + li)):
                s_, planes = blk.stride, blk.conv1.out_channels
                Ho, Wo = (H + 2 - 3) // s_ + 1, (W + 2 - 3) // s_ + 1
                if self.block == 'bottleneck':
                    t = _ConvBnFn.apply(y, blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, None, (n, H, W, C, 1, 1, 1, 0), True, blk.bn1, dt, sync)
                    t = _ConvBnFn.apply(t, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias, None, (n, H, W, planes, 3, 3, s_, 1), True, blk.bn2, dt, sync)
                    idt = y
                    if blk.downsample is not None:
                        idt = _ConvBnFn.apply(y, blk.downsample[0].weight, blk.downsample[1].weight, blk.downsample[1].bias, None,
                                              (n, H, W, C, 1, 1, s_, 0), False, blk.downsample[1], dt, sync)
                    y = _ConvBnFn.apply(t, blk.conv3.weight, blk.bn3.weight, blk.bn3.bias, idt, (n, Ho, Wo, planes, 1, 1, 1, 0), True, blk.bn3, dt, sync)
                    H, W, C = Ho, Wo, blk.conv3.out_channels
                    continue
                t = _ConvBnFn.apply(y, blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, None, (n, H, W, C, 3, 3, s_, 1), True, blk.bn1, dt, sync)
                idt = y
                if blk.downsample is not None:
                    idt = _ConvBnFn.apply(y, blk.downsample[0].weight, blk.downsample[1].weight, blk.downsample[1].bias, None,
                                          (n, H, W, C, 1, 1, s_, 0), False, blk.downsample[1], dt, sync)
                y = _ConvBnFn.apply(t, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias, idt, (n, Ho, Wo, planes, 3, 3, 1, 1), True, blk.bn2, dt, sync)
                H, W, C = Ho, Wo, planes
        if self.avgpool:
            return _AvgPoolFn.apply(y, n, H * W, C)
        return y.view(n, H * W, C)

    def _forward_frozen(self, pixel_values, nhwc=False):
        dt = self.compute_dtype
        f = self._folded or self.refold()
        x = pixel_values if nhwc else pixel_values.float().contiguous()
        n, c, H, W, strides = _pixel_geom(x, nhwc)
        w0, b0 = f['stem']
        cols, H, W = ops.im2col(x, n, H, W, c, 7, 7, 2, 3, dt, strides=strides, ldcols=w0.shape[1])
        y = ops.gemm_nt(cols, w0, b0, ops.ACT_RELU)
        del cols
        C = w0.shape[0]
        y, H, W = ops.maxpool_nhwc(y, n, H, W, C, 3, 2, 1)
        for stride, planes, (w1, b1), (w2, b2), *rest in f['blocks']:
            down = rest[-1]
            if self.block == 'bottleneck':
                w3, b3 = rest[0]
                t = ops.conv_nhwc(y, w1, b1, ops.ACT_RELU, n, H, W, C, 1, 1, 1, 0)[0]
                t, Ho, Wo = ops.conv_nhwc(t, w2, b2, ops.ACT_RELU, n, H, W, planes, 3, 3, stride, 1)
                idt = ops.conv_nhwc(y, down[0], down[1], ops.ACT_NONE, n, H, W, C, 1, 1, stride, 0)[0] if down is not None else y
                y = ops.conv_nhwc(t, w3, b3, ops.ACT_RELU_RES, n, Ho, Wo, planes, 1, 1, 1, 0, residual=idt)[0]
                H, W, C = Ho, Wo, w3.shape[0]
                continue
            t, Ho, Wo = ops.conv_nhwc(y, w1, b1, ops.ACT_RELU, n, H, W, C, 3, 3, stride, 1)
            idt = ops.conv_nhwc(y, down[0], down[1], ops.ACT_NONE, n, H, W, C, 1, 1, stride, 0)[0] if down is not None else y
            y, _, _ = ops.conv_nhwc(t, w2, b2, ops.ACT_RELU_RES, n, Ho, Wo, planes, 3, 3, 1, 1, residual=idt)
            H, W, C = Ho, Wo, planes
        if self.avgpool:
            return ops.avgpool_nhwc(y, n, H * W, C)
        return y.view(n, H * W, C)


def resnet18(avgpool=False, compute_dtype='bf16', trainable=False, sync_bn=False):
    return ResNetExtractor((2, 2, 2, 2), avgpool=avgpool, compute_dtype=compute_dtype, trainable=trainable, sync_bn=sync_bn)


def resnet34(avgpool=False, compute_dtype='bf16', trainable=False, sync_bn=False):
    return ResNetExtractor((3, 4, 6, 3), avgpool=avgpool, compute_dtype=compute_dtype, trainable=trainable, sync_bn=sync_bn)


def resnet50(avgpool=False, compute_dtype='bf16', trainable=False, sync_bn=False):
    """torchvision's ResNet-50 without its classifier (and, for the frames, without its average pool): 2048-wide features"""
    return ResNetExtractor((3, 4, 6, 3), avgpool=avgpool, compute_dtype=compute_dtype, trainable=trainable, sync_bn=sync_bn, block='bottleneck')


class ResNetBackbone(nn.Module):
    """backbone.py:65-89: sketch [N,1,3,H,W] -> [N,1,C] (global average pooled), frames [N,T,3,H,W] -> [N, T*h*w, C].

    Raw frames — uint8 [N,T,H,W,3] (sketch [N,1,H,W,3]), or a list of N tensors [T,H_b,W_b,3] of any sizes — go through the
    FrameIngest this backbone owns (svol_dataset.py:218-229: Resize((224,224)) + ToTensor(); ``pixel_preset`` overrides
    'totensor'): with two extractors of one 16-bit type (bf16 or fp16) it writes the NHWC image in that type, which the stem's
    im2col reads directly.  ``sketch_filter`` / ``sketch_invert`` give the sketch an ingest of its own, with another of Pillow's
    filters and / or inverted source bytes (preprocess/quickdraw_array_to_pil.py:36 is sketch_filter='bicubic', sketch_invert=True
    on the 28 x 28 bitmaps); a raw sketch may be grey, uint8 [N,1,H,W] or [N,1,H,W,1] (what .convert('RGB') replicates,
    svol_dataset.py:212-229).  With both unset the sketch goes through the frames' ingest.  Float inputs take exactly the path
    they always took."""

    def __init__(self, video_backbone, sketch_backbone, pixel_preset=None, sketch_filter=None, sketch_invert=False):
        super().__init__()
        self.video_backbone = video_backbone
        self.sketch_backbone = sketch_backbone
        self.nhwc = video_backbone.compute_dtype in _H16 and sketch_backbone.compute_dtype == video_backbone.compute_dtype
        out = _NHWC_OUT[video_backbone.compute_dtype] if self.nhwc else 'nchw_f32'
        self.ingest = FrameIngest((224, 224), pixel_preset or 'totensor', out=out)
        self.sketch_ingest = self.ingest
        if sketch_filter is not None or sketch_invert:
            self.sketch_ingest = FrameIngest((224, 224), pixel_preset or 'totensor', out=out, filter=sketch_filter or 'bilinear', invert=sketch_invert)

    def forward(self, sketch_batch, video_batch):
        if is_raw_frames(sketch_batch) or is_raw_frames(video_batch):
            return self._forward_raw(sketch_batch, video_batch)
        N, T = video_batch.shape[:2]
        src_sketch = self.sketch_backbone(sketch_batch.flatten(0, 1)).view(N, -1, self.sketch_backbone.out_channels)
        tok = self.video_backbone(video_batch.flatten(0, 1))                  # [N*T, h*w, C]
        return src_sketch, tok.reshape(N, T * tok.shape[1], tok.shape[2])

    def _forward_raw(self, sketch_batch, video_batch):
        N = len(video_batch)

        def run(extractor, x, ingest):
            if is_raw_frames(x):
                pix = ingest(x)
                return extractor(pix.flatten(0, 1) if pix.dim() == 5 else pix, nhwc=self.nhwc)
            return extractor(x.flatten(0, 1))
        src_sketch = run(self.sketch_backbone, sketch_frames(sketch_batch), self.sketch_ingest).view(N, -1, self.sketch_backbone.out_channels)
        tok = run(self.video_backbone, video_batch, self.ingest)                         # [N*T, h*w, C]
        return src_sketch, tok.reshape(N, -1, tok.shape[2])
