"""Sketch-ViT classification fine-tuning on the HIP kernels (reference preprocess/sketch_vit_finetune.py).

The reference makes its sketch features in two steps.  ``finetune_sketch_vit`` (:88-159) puts a classifier on the [CLS] state of
``transformers.ViTForImageClassification`` (19 / 21 / 24 sketch categories), freezes the embeddings and the first 12 - K layers
(``SketchViT``, :43-77) and trains the last K layers, the final LayerNorm and the classifier with ``nn.CrossEntropyLoss`` on
``outputs[:, 0, :]`` (:140-143, AdamW).  ``extract_sketch_features`` (:162-206) then saves four tensors per sketch, ``before_norm`` and
``after_norm`` each as the class token and as the mean of the patch tokens, which the head consumes as pre-extracted input.

``SketchViTClassifier`` is that model: ``self.vit`` a ``ViTExtractor(trainable=True, train_layers=K)``, ``self.classifier`` a Linear, the
state-dict keys of ``ViTForImageClassification`` (``vit.*``, ``classifier.*``).  Two paths:

    forward(pixel_values)     (before_norm, after_norm, logits) as SketchViT.forward (:79-85), every block on all tokens: feature
                              extraction and evaluation
    cls_logits(pixel_values)  the TRAINING path.  The loss reads one row per image, so in the LAST block only the [CLS] query, its
                              out-projection, its MLP row and its LayerNorm row reach it; K and V are still needed for all tokens:

        LN_before (all rows) -> K | V GEMMs (all rows), Q GEMM (n rows) -> svol_attn_cls_fwd[_h16] (one query per (image, head), fp32
        arithmetic) -> out-proj + fp32 residual (n rows) -> LN_after -> fc1 + GELU -> fc2 + residual (n rows) -> final LN (n rows)
        -> fp32 classifier GEMM

                              which drops 196/197 of that block's Q / out-projection / MLP GEMMs, of its [n 197, 3072] hidden tensor
                              and of the matching data-gradient GEMMs.  Earlier trained blocks (K >= 2) run on all tokens as in
                              ViTExtractor; their stream gradient is the [CLS] rows' scattered into zeros.
    loss(pixel_values, targets)  (mean cross-entropy, top-1 hits) through svol_softmax_xent.

Not here: the script's host-side data loop (ImageFolder, albumentations, file writing); hand over ``pixel_values``, or uint8 frames
through ``svol_amd.ingest.FrameIngest``: ``FrameIngest((224, 224), 'vit', filter=..., invert=...)`` takes grey sketches
(``[n,H,W]`` uint8, what ``ImageFolder``'s ``.convert('RGB')`` replicates) and any of Pillow's filters, so QuickDraw's raw 28 x 28
bitmaps enter as ``filter='bicubic', invert=True`` (preprocess/quickdraw_array_to_pil.py:36).
"""
from __future__ import annotations

import re
from collections import OrderedDict

import torch
from torch import nn

from .. import layers, ops, params
from .backbone import ViTExtractor, hf_rename, vit_base_config


class _ViTClsAttnFn(torch.autograd.Function):
    """x32[cls rows] + o_proj(attention(q_proj(y[cls rows]), k_proj(y), v_proj(y))) -> [n, d] fp32: the attention half of the last
    block for the [CLS] query alone (y = LN_before(x32) on all rows, bf16 or fp16: the dtype of everything 16-bit here).  wc as
    _ViTAttnFn's."""

    @staticmethod
    def forward(ctx, x32, y, Wq, bq, Wk, bk, Wv, bv, Wo, bo, wc, dims):
        n, L, H = dims
        d = Wq.shape[0]
        Wqkv, WqkvT, Woc, WoT = wc
        kv = torch.empty((n * L, 2 * d), dtype=y.dtype, device=y.device)
        ops.gemm_nt(y, Wqkv[d:2 * d], bk, out=kv[:, :d])
        ops.gemm_nt(y, Wqkv[2 * d:], bv, out=kv[:, d:])
        q = ops.gemm_nt(y.view(n, L, d)[:, 0], Wqkv[:d], bq)
        o, lse2 = ops.attn_cls_fwd(q, kv[:, :d], kv[:, d:], n, H, L, d // H)
        out = ops.gemm_nt(o, Woc, bo, residual=x32.view(n, L, d)[:, 0], out_f32=True)
        ctx.save_for_backward(y, kv, q, o, lse2)
        ctx.dims, ctx.WqkvT, ctx.WoT = dims, WqkvT, WoT
        nig = ctx.needs_input_grad
        ctx.sinks = tuple(params.claim(t, nig[i]) for i, t in enumerate((Wq, bq, Wk, bk, Wv, bv, Wo, bo), start=2))
        return out

    @staticmethod
    def backward(ctx, dout32):
        y, kv, q, o, lse2 = ctx.saved_tensors
        n, L, H = ctx.dims
        d = o.shape[1]
        dev = y.device
        dout32 = dout32 if dout32.is_contiguous() else dout32.contiguous()
        ds = ops.cast(dout32, y.dtype)
        sk = ctx.sinks
        grads = params.GradGroup(((sk[6], (d, d)), (sk[7], (d,))), dev)
        grads.tn(ds, o, 0, 1)
        dWo, dbo = grads.finish()
        do = ops.gemm_nt(ds, ctx.WoT)
        dq = torch.empty((n, d), dtype=y.dtype, device=dev)
        dkv = torch.empty((n * L, 2 * d), dtype=y.dtype, device=dev)
        ops.attn_cls_bwd(q, kv[:, :d], kv[:, d:], o, do, lse2, n, H, L, d // H, dq, dkv[:, :d], dkv[:, d:])
        ycls = y.view(n, L, d)[:, 0]
        grads = params.GradGroup(((sk[0], (d, d)), (sk[1], (d,))), dev)
        grads.tn(dq, ycls, 0, 1)
        dWq, dbq = grads.finish()
        grads = params.GradGroup(((sk[2], (d, d)), (sk[4], (d, d)), (sk[3], (d,)), (sk[5], (d,))), dev)
        if grads.direct:
            grads.tn(dkv[:, :d], y, 0, 2)
            grads.tn(dkv[:, d:], y, 1, 3)
        else:   # one launch for both projections: dW_k | dW_v and db_k | db_v are contiguous in the buffer
            ops.gemm_tn(dkv, y, out=grads.buf[:2 * d * d].view(2 * d, d), colsum=grads.buf[2 * d * d:])
        dWk, dWv, dbk, dbv = grads.finish()
        dy = None
        if ctx.needs_input_grad[1]:
            dy = ops.gemm_nt(dkv, ctx.WqkvT[:, d:])                                # [dk | dv] [W_k; W_v]
            dyc = dy.view(n, L, d)[:, 0]
            dyc.copy_(ops.gemm_nt(dq, ctx.WqkvT[:, :d], residual=dyc))             # + dq W_q on the [CLS] rows
        dx32 = None
        if ctx.needs_input_grad[0]:   # (finetune_layers >= 2) the residual reaches the [CLS] rows only
            dx32 = torch.zeros((n * L, d), dtype=torch.float32, device=dev)
            dx32.view(n, L, d)[:, 0] = dout32
        return (dx32, dy, dWq, dbq, dWk, dbk, dWv, dbv, dWo, dbo, None, None)


def _pad4(t, cols):
    """[r, c] fp32 -> a zero-padded [r, cols] copy (the fp32 GEMMs take leading dimensions on the 16-byte grid)"""
    out = torch.zeros((t.shape[0], cols), dtype=torch.float32, device=t.device)
    out[:, :t.shape[1]] = t
    return out


class _ClsLinearFn(torch.autograd.Function):
    """logits = x W^T + b in fp32 on the n [CLS] rows (x may be a row-strided view)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        return ops.gemm_nt(x, W.detach(), b.detach())

    @staticmethod
    def backward(ctx, dl):
        x, W = ctx.saved_tensors
        C, d = W.shape
        Cp = (C + 3) // 4 * 4
        dlp = _pad4(dl, Cp)
        nig = ctx.needs_input_grad
        dx = ops.gemm_nt(dlp, _pad4(W.detach().t(), Cp)) if nig[0] else None
        dW = db = None
        if nig[1] or nig[2]:
            db = torch.zeros((Cp,), dtype=torch.float32, device=dl.device)
            dW = ops.gemm_tn(dlp, x, colsum=db)[:C]
            db = db[:C]
        return dx, dW, db


class _XentFn(torch.autograd.Function):
    """(mean cross-entropy, top-1 hits) of fp32 logits: svol_softmax_xent; backward dlogits x upstream."""

    @staticmethod
    def forward(ctx, logits, targets):
        loss, dlogits, correct = ops.softmax_xent(logits, targets)
        ctx.save_for_backward(dlogits)
        correct = correct.view(())
        ctx.mark_non_differentiable(correct)
        return loss.view(()), correct

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss, None


class SketchViTClassifier(nn.Module):
    def __init__(self, cfg=None, num_labels=19, finetune_layers=1, compute_dtype='bf16'):
        """num_labels: 19 (sketchy), 21 (tu_berlin) or 24 (quickdraw) in the reference (sketch_vit_finetune.py:89-94);
        finetune_layers = K >= 1: the last K layers, the final LayerNorm and the classifier train (:53-69);
        compute_dtype: 'bf16' or 'fp16', the extractor's (ViTExtractor): both paths and extract_features run in it; the classifier GEMM
        and the cross-entropy are fp32 either way.  fp16 training wants a scaled loss, as the head's (FlatAdamW.loss_scale)."""
        super().__init__()
        cfg = cfg or vit_base_config()
        if not 1 <= int(finetune_layers) <= cfg.num_hidden_layers:
            raise ValueError(f'finetune_layers must be in [1, {cfg.num_hidden_layers}], got {finetune_layers}')
        self.cfg = cfg
        self.num_labels = int(num_labels)
        self.vit = ViTExtractor(cfg, compute_dtype=compute_dtype, trainable=True, train_layers=int(finetune_layers))
        self.classifier = nn.Linear(cfg.hidden_size, self.num_labels)

    @property
    def finetune_layers(self) -> int:
        return self.vit.train_layers

    def _set_finetune_layers(self, K: int):
        nl = self.cfg.num_hidden_layers
        if not 1 <= K <= nl:
            raise ValueError(f'finetune_layers must be in [1, {nl}], got {K}')
        self.vit.train_layers = K
        self.vit.requires_grad_(False)
        for lyr in self.vit.layers[nl - K:]:
            lyr.requires_grad_(True)
        self.vit.layernorm.requires_grad_(True)
        self.classifier.requires_grad_(True)

    # ---- state dicts -----------------------------------------------------------------------------------------------------------------
    def load_hf_state_dict(self, sd):
        """state dict of transformers.ViTForImageClassification, 5.x or 4.x names (the extractor's renames)."""
        cls = {k[len('classifier.'):]: v for k, v in sd.items() if k.startswith('classifier.')}
        self.vit.load_hf_state_dict({k: v for k, v in sd.items() if not k.startswith('classifier.')})
        return self.classifier.load_state_dict(cls, strict=True)

    def load_reference_state_dict(self, sd):
        """state dict of the script's SketchViT wrapper (sketch_vit_finetune.py:73-77): ViTEmbeddings.X, layers_freeze.i.X,
        layers_unfreeze.j.X (-> layer N - K + j, K from the keys present), layer_norm.X, Classifier.X.  Sets finetune_layers = K."""
        nl = self.cfg.num_hidden_layers
        js = {int(m.group(1)) for m in (re.match(r'layers_unfreeze\.(\d+)\.', k) for k in sd) if m}
        fs = {int(m.group(1)) for m in (re.match(r'layers_freeze\.(\d+)\.', k) for k in sd) if m}
        K = len(js)
        if js != set(range(K)) or fs != set(range(nl - K)) or K < 1:
            raise ValueError(f'wrapper keys hold {len(fs)} frozen and {K} trained layers; the model has {nl}')
        out = OrderedDict()
        for k, v in sd.items():
            head, _, rest = k.partition('.')
            if head == 'ViTEmbeddings':
                k2 = 'vit.embeddings.' + rest
            elif head in ('layers_freeze', 'layers_unfreeze'):
                i, _, rest = rest.partition('.')
                k2 = f'vit.layers.{int(i) + (nl - K if head == "layers_unfreeze" else 0)}.' + hf_rename(rest)
            elif head == 'layer_norm':
                k2 = 'vit.layernorm.' + rest
            elif head == 'Classifier':
                k2 = 'classifier.' + rest
            else:
                raise KeyError(f'not a SketchViT wrapper key: {k}')
            out[k2] = v
        self.vit._wcache.clear()
        res = self.load_state_dict(out, strict=True)
        self._set_finetune_layers(K)
        return res

    def reference_state_dict(self):
        """this model under the wrapper's keys (what its ``model.state_dict()`` holds, :151)."""
        nl, K = self.cfg.num_hidden_layers, self.finetune_layers
        out = OrderedDict()
        for k, v in self.state_dict().items():
            if k.startswith('vit.embeddings.'):
                k2 = 'ViTEmbeddings.' + k[len('vit.embeddings.'):]
            elif k.startswith('vit.layers.'):
                i, _, rest = k[len('vit.layers.'):].partition('.')
                i = int(i)
                k2 = (f'layers_freeze.{i}.' if i < nl - K else f'layers_unfreeze.{i - (nl - K)}.') + rest
            elif k.startswith('vit.layernorm.'):
                k2 = 'layer_norm.' + k[len('vit.layernorm.'):]
            else:
                k2 = 'Classifier.' + k[len('classifier.'):]
            out[k2] = v
        # the wrapper registers its frozen layers before the trained ones, the norm and the classifier: the same order
        return out

    # ---- forward paths -----------------------------------------------------------------------------------------------------------
    def forward(self, pixel_values):
        """-> (before_norm [n, L, d], after_norm [n, L, d], logits [n, C]), every block on all tokens.  The reference applies the
        classifier to all L tokens and keeps row 0 (sketch_vit_finetune.py:84,141); here it runs on the [CLS] rows only, so logits is
        what the reference's ``out[:, 0, :]`` is."""
        after, before = self.vit(pixel_values, return_pre_norm=True)
        logits = _ClsLinearFn.apply(after[:, 0], self.classifier.weight, self.classifier.bias)
        return before, after, logits

    def cls_logits(self, pixel_values):
        """the training path (module docstring) -> logits [n, C] fp32."""
        if not pixel_values.is_cuda:
            raise RuntimeError('svol_amd SketchViTClassifier runs on the MI355X HIP kernels only (no CPU path)')
        vit = self.vit
        dt = vit.dtype
        n = pixel_values.shape[0]
        x32, L = vit._stream_train(pixel_values)
        for lyr in vit.layers[vit._first_trained():-1]:
            x32 = vit._layer_train(lyr, x32, n, L)
        lyr = vit.layers[-1]
        a = lyr.attention
        y = layers.LNStreamFn.apply(x32, lyr.layernorm_before.weight, lyr.layernorm_before.bias, None, dt, False)
        xc = _ViTClsAttnFn.apply(x32, y, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.k_proj.bias, a.v_proj.weight, a.v_proj.bias,
                                 a.o_proj.weight, a.o_proj.bias, vit._attn_weights(a), (n, L, self.cfg.num_attention_heads))
        xc = vit._mlp_train(lyr, xc)
        last, _ = layers.LNStreamFn.apply(xc, vit.layernorm.weight, vit.layernorm.bias, None, dt, True)
        return _ClsLinearFn.apply(last, self.classifier.weight, self.classifier.bias)

    def loss(self, pixel_values, targets):
        """-> (nn.CrossEntropyLoss()(cls_logits, targets), number of top-1 hits) (sketch_vit_finetune.py:107,141)."""
        return _XentFn.apply(self.cls_logits(pixel_values), targets)

    def extract_features(self, pixel_values):
        """the four tensors extract_sketch_features saves per sketch (sketch_vit_finetune.py:198-206), each [n, d] fp32:
        {'before_norm': {'class_token', 'feature_avg'}, 'after_norm': {...}}.  Eval mode, no autograd."""
        was = self.training
        self.eval()
        try:
            with torch.no_grad():
                before, after, _ = self.forward(pixel_values)
                return {name: {'class_token': t[:, 0].contiguous(), 'feature_avg': t[:, 1:].mean(1)}
                        for name, t in (('before_norm', before), ('after_norm', after))}
        finally:
            self.train(was)
