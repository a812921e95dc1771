"""ViT-B/16 frame + sketch feature extractor on the HIP kernels (reference
lib/modeling/backbone.py:11-62,116-132).

The reference wraps Hugging Face ``ViTModel`` (``google/vit-base-patch16-224-in21k``) and runs it frame by frame in a
Python loop after PIL preprocessing, keeping only the [CLS] state; its path is broken (``device`` is undefined,
backbone.py:30).  Here ``ViTExtractor`` IS the model — same parameter names as ``transformers.ViTModel(config,
add_pooling_layer=False)`` (5.x naming: ``embeddings.patch_embeddings.projection``, ``layers.{i}.attention.q_proj``
..., ``layernorm``; ``load_hf_state_dict`` also accepts the 4.x ``encoder.layer.{i}.attention.attention.query`` style)
— and it takes already-normalised ``pixel_values``, all frames of the batch at once:

    patchify (im2col kernel) -> ONE MFMA GEMM (768 x 768) -> [CLS] + position embeddings ->
    12 x { LN -> q|k|v GEMMs -> short-sequence attention (197 tokens, 12 heads, d_h = 64) -> out-proj GEMM + fp32 residual
           -> LN -> fc1 GEMM + erf-GELU -> fc2 GEMM + fp32 residual } -> LN

16-bit MFMA operands — ``compute_dtype='bf16'`` (the default) or ``'fp16'``, the reference's own mixed precision (apex amp) —, fp32
residual stream, frozen by default (the extractor is frozen in the reference: its features are normally pre-extracted,
preprocess/sketch_vit_feature_extractor.py).  The 16-bit stores are the patch rows, the LayerNorm outputs, q / k / v, the attention
output and gelu(fc1); the weights are cast to the same type.  fp16 rounds 8 x finer than bf16 and holds 65504 at most: the synthetic
weights of the tests stay far inside it, the activation ranges under the pretrained in21k weights have not been measured.  ``'fp32'``
raises: the short-sequence attention kernels have no fp32 form.  ``ViTBackbone.forward`` returns what the head
consumes at BASELINE configs[3]: the sketch's [CLS] state [B,1,768] and ALL 196 patch tokens of every frame
[B, T*196, 768].
LayerNorm uses the kernels' eps = 1e-5 where HF uses 1e-12: a relative change of 5e-6 at unit variance, three orders
below the bf16 operand rounding.

``ViTExtractor(trainable=True)`` in ``.train()`` mode is the extractor the reference optimises (train.py:72 hands every parameter
of build_model(args) to AdamW) or fine-tunes (preprocess/sketch_vit_finetune.py:43-69,103-143: ``train_layers=K`` trains the last
K layers and the final LayerNorm, the embeddings and the first 12 - K layers stay frozen and run without autograd).  Same kernels
and the same forward bits as the frozen path, one autograd Function per piece:

    _ViTEmbedFn   patchify + patch GEMM + [CLS] / position embeddings; backward dW, db = gemm_tn over the saved 16-bit patch rows,
                  dpos = colsum of the stream gradient viewed [n, (P+1)*d], dcls = its first row
    per layer     LNStreamFn(layernorm_before) -> _ViTAttnFn (q|k|v GEMMs, svol_attn_small_fwd_lse, out-proj + fp32 residual;
                  backward svol_attn_small_bwd into one packed dQKV, dx = dQKV [W_q; W_k; W_v] in one NT GEMM)
                  -> LNStreamFn(layernorm_after) -> MLPLNFn(gamma=None, GELU)
    final norm    LNStreamFn
The trainable path casts its own 16-bit weights at the start of every training forward: params.weights is refreshed by the head's
forward, which runs AFTER the backbone, and fused AdamW on ROCm does not bump ``_version``.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
from torch import nn

from .. import _lib, layers, ops, params
from ..ingest import FrameIngest, is_raw_frames, sketch_frames
from ..ops import _DT, _ptr, _stream


def vit_base_config(**over) -> SimpleNamespace:
    a = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, image_size=224,
             patch_size=16, num_channels=3, layer_norm_eps=1e-12)
    a.update(over)
    return SimpleNamespace(**a)


# transformers 4.x parameter names -> the 5.x names the modules here carry
HF_RENAMES = (('encoder.layer.', 'layers.'), ('attention.attention.query', 'attention.q_proj'),
              ('attention.attention.key', 'attention.k_proj'), ('attention.attention.value', 'attention.v_proj'),
              ('attention.output.dense', 'attention.o_proj'), ('intermediate.dense', 'mlp.fc1'), ('output.dense', 'mlp.fc2'))


def hf_rename(k: str) -> str:
    for a, b in HF_RENAMES:
        k = k.replace(a, b)
    return k


class _Attention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = (nn.Linear(d, d) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, d, f):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(d, f), nn.Linear(f, d)


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d = cfg.hidden_size
        self.attention = _Attention(d)
        self.layernorm_before = nn.LayerNorm(d, eps=cfg.layer_norm_eps)
        self.layernorm_after = nn.LayerNorm(d, eps=cfg.layer_norm_eps)
        self.mlp = _MLP(d, cfg.intermediate_size)


class _PatchEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.projection = nn.Conv2d(cfg.num_channels, cfg.hidden_size, kernel_size=cfg.patch_size, stride=cfg.patch_size)


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        n_tok = (cfg.image_size // cfg.patch_size) ** 2 + 1
        self.cls_token = nn.Parameter(torch.randn(1, 1, cfg.hidden_size))
        self.position_embeddings = nn.Parameter(torch.randn(1, n_tok, cfg.hidden_size))
        self.patch_embeddings = _PatchEmbeddings(cfg)


_DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def _patch_rows(pixel_values, p, dt=torch.bfloat16):
    """[n, C, H, W] fp32 -> (patch rows [n*P, C*p*p] of dtype dt, P)."""
    n, C, Hh, Ww = pixel_values.shape
    P = (Hh // p) * (Ww // p)
    pix = pixel_values.float().contiguous()
    patches = torch.empty((n * P, C * p * p), dtype=dt, device=pix.device)
    _lib.check(_lib.lib().svol_patchify(_ptr(pix), _ptr(patches), n, C, Hh, Ww, p, _DT[dt], _stream()), 'svol_patchify')
    return patches, P


def _embed(proj, cls, pos, n, P, d):
    x32 = torch.empty((n * (P + 1), d), dtype=torch.float32, device=proj.device)
    _lib.check(_lib.lib().svol_vit_embed(_ptr(proj), _ptr(cls), _ptr(pos), _ptr(x32), 0, n, P, d, _DT[torch.bfloat16], _stream()),
               'svol_vit_embed')
    return x32


class _ViTEmbedFn(torch.autograd.Function):
    """patchify -> patch GEMM (+ bias, fp32 out) -> [CLS] + position embeddings: the fp32 stream [n*(P+1), d].  No pixel gradient."""

    @staticmethod
    def forward(ctx, pixel_values, W, b, cls, pos, p, dt=torch.bfloat16):
        n = pixel_values.shape[0]
        d = W.shape[0]
        patches, P = _patch_rows(pixel_values, p, dt)
        Wc = ops.cast(W.detach().reshape(d, -1).contiguous(), dt)
        proj = ops.gemm_nt(patches, Wc, b, out_f32=True)
        x32 = _embed(proj, cls, pos, n, P, d)
        ctx.save_for_backward(patches)
        ctx.dims, ctx.wshape = (n, P, d), W.shape
        nig = ctx.needs_input_grad
        ctx.sinks = tuple(params.claim(t, nig[i]) for i, t in ((1, W), (2, b), (3, cls), (4, pos)))
        return x32

    @staticmethod
    def backward(ctx, dx32):
        (patches,) = ctx.saved_tensors
        n, P, d = ctx.dims
        sW, sb, sc, sp = ctx.sinks
        nig = ctx.needs_input_grad
        dx32 = dx32 if dx32.is_contiguous() else dx32.contiguous()
        dW = db = dcls = dpos = None
        if nig[1] or nig[2]:
            dproj = ops.cast(dx32.view(n, P + 1, d)[:, 1:].reshape(n * P, d), patches.dtype)
            grads = params.GradGroup(((sW, (d, patches.shape[1])), (sb, (d,))), dproj.device)
            grads.tn(dproj, patches, 0, 1)
            dW, db = grads.finish()
            dW = dW.view(ctx.wshape) if dW is not None else None
        if nig[3] or nig[4]:
            # position embeddings: the stream gradient summed over the images; the [CLS] token: the same sum's first row
            g = ops.colsum(dx32.view(n, (P + 1) * d))
            if sc is not None:
                sc.view.view(-1).add_(g[:d])
            elif nig[3]:
                dcls = g[:d].clone().view(1, 1, d)
            if sp is not None:
                sp.view.view(-1).add_(g)
            elif nig[4]:
                dpos = g.view(1, P + 1, d)
        return None, dW, db, dcls, dpos, None, None


class _ViTAttnFn(torch.autograd.Function):
    """x32 + o_proj(attention(q_proj(y), k_proj(y), v_proj(y))): the attention half of a pre-norm ViT layer (y = LN_before(x32),
    bf16 or fp16: the dtype of everything 16-bit here).  wc = (W_qkv [3d, d], W_qkv^T [d, 3d], W_o, W_o^T) of y's dtype, cast by the caller
    this forward."""

    @staticmethod
    def forward(ctx, x32, y, Wq, bq, Wk, bk, Wv, bv, Wo, bo, wc, dims):
        n, L, H = dims
        d = Wq.shape[0]
        dh = d // H
        Wqkv, WqkvT, Woc, WoT = wc
        dev = y.device
        qkv = torch.empty((n * L, 3 * d), dtype=y.dtype, device=dev)
        for j, b in enumerate((bq, bk, bv)):
            ops.gemm_nt(y, Wqkv[j * d:(j + 1) * d], b, out=qkv[:, j * d:(j + 1) * d])
        o, lse2 = ops.attn_small_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], n, H, L, dh, want_lse=True)
        out = ops.gemm_nt(o, Woc, bo, residual=x32, out_f32=True)
        ctx.save_for_backward(y, qkv, o, lse2)
        ctx.dims, ctx.WqkvT, ctx.WoT = dims, WqkvT, WoT
        nig = ctx.needs_input_grad
        ctx.sinks = tuple(params.claim(t, nig[i]) for i, t in enumerate((Wq, bq, Wk, bk, Wv, bv, Wo, bo), start=2))
        return out

    @staticmethod
    def backward(ctx, dout32):
        y, qkv, o, lse2 = ctx.saved_tensors
        n, L, H = ctx.dims
        d = o.shape[1]
        dout32 = dout32 if dout32.is_contiguous() else dout32.contiguous()
        ds = ops.cast(dout32, y.dtype)
        sk = ctx.sinks
        grads = params.GradGroup(((sk[6], (d, d)), (sk[7], (d,))), ds.device)
        grads.tn(ds, o, 0, 1)
        dWo, dbo = grads.finish()
        do = ops.gemm_nt(ds, ctx.WoT)
        dqkv = torch.empty((n * L, 3 * d), dtype=y.dtype, device=y.device)
        ops.attn_small_bwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, do, lse2, n, H, L, d // H,
                           dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:])
        grads = params.GradGroup([(sk[2 * j], (d, d)) for j in range(3)] + [(sk[2 * j + 1], (d,)) for j in range(3)], y.device)
        if grads.direct:
            for j in range(3):
                grads.tn(dqkv[:, j * d:(j + 1) * d], y, j, 3 + j)
        else:   # one launch for the three projections: dW_q | dW_k | dW_v and db_q | db_k | db_v are contiguous in the buffer
            ops.gemm_tn(dqkv, y, out=grads.buf[:3 * d * d].view(3 * d, d), colsum=grads.buf[3 * d * d:])
        g = grads.finish()
        g = tuple(t for j in range(3) for t in (g[j], g[3 + j]))
        dy = ops.gemm_nt(dqkv, ctx.WqkvT) if ctx.needs_input_grad[1] else None
        return (dout32, dy) + g + (dWo, dbo, None, None)


class ViTExtractor(nn.Module):
    def __init__(self, cfg=None, compute_dtype='bf16', trainable=False, train_layers=None):
        """trainable=False: the frozen extractor (no parameter requires grad).  trainable=True: every parameter trains
        (train.py:72), or with train_layers=K only the last K layers and the final LayerNorm (sketch_vit_finetune.py:43-69).
        compute_dtype: 'bf16' or 'fp16', the type of the MFMA operands and of every 16-bit activation (module docstring)."""
        super().__init__()
        cfg = cfg or vit_base_config()
        if compute_dtype not in _DTYPES:
            raise NotImplementedError(f"the short-sequence attention kernels take bf16 or fp16 operands (fp32 residual stream), not '{compute_dtype}'")
        self.cfg = cfg
        self.compute_dtype = compute_dtype
        self.dtype = _DTYPES[compute_dtype]
        self.embeddings = _Embeddings(cfg)
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.num_hidden_layers)])
        self.layernorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.requires_grad_(False)
        self._wcache = {}
        self.trainable = bool(trainable)
        nl = cfg.num_hidden_layers
        if train_layers is not None and not 0 <= int(train_layers) <= nl:
            raise ValueError(f'train_layers must be in [0, {nl}], got {train_layers}')
        self.train_layers = None if train_layers is None else int(train_layers)
        if self.trainable:
            first = 0 if self.train_layers is None else nl - self.train_layers
            if self.train_layers is None:
                self.embeddings.requires_grad_(True)
            for lyr in self.layers[first:]:
                lyr.requires_grad_(True)
            self.layernorm.requires_grad_(True)

    def load_hf_state_dict(self, sd):
        """state dict of transformers.ViTModel, 5.x names or the 4.x ``encoder.layer.N.attention.attention.query`` style."""
        out = {}
        for k, v in sd.items():
            if k.startswith('vit.'):
                k = k[4:]
            if k.startswith('pooler.'):
                continue
            out[hf_rename(k)] = v
        self._wcache.clear()
        return self.load_state_dict(out, strict=True)

    def _w(self, src):
        """[out, in] copy of a frozen fp32 weight in the extractor's dtype (refreshed if the parameter storage, its version or the dtype
        changed)."""
        ent = self._wcache.get(id(src))
        tag = (src.data_ptr(), src._version, self.dtype)
        if ent is None or ent[0] != tag:
            ent = (tag, ops.cast(src.detach().reshape(src.shape[0], -1).contiguous(), self.dtype))
            self._wcache[id(src)] = ent
        return ent[1]

    def uses_autograd(self) -> bool:
        return self.training and self.trainable and torch.is_grad_enabled()

    def forward(self, pixel_values: torch.Tensor, return_pre_norm: bool = False):
        """[n, C, H, W] fp32 (normalised) -> last_hidden_state [n, 1 + P, d] fp32."""
        if not pixel_values.is_cuda:
            raise RuntimeError('svol_amd ViTExtractor runs on the MI355X HIP kernels only (no CPU path)')
        if self.uses_autograd():
            return self._forward_train(pixel_values, return_pre_norm)
        with torch.no_grad():
            return self._forward_frozen(pixel_values, return_pre_norm)

    def _first_trained(self):
        nl = self.cfg.num_hidden_layers
        return 0 if self.train_layers is None else nl - self.train_layers

    def _forward_train(self, pixel_values, return_pre_norm):
        """autograd through the trained part (module docstring); the frozen prefix runs as in _forward_frozen, without autograd.
        The 16-bit copies of the trained weights are cast here, every call; the frozen path's copies of them are dropped."""
        n, d = pixel_values.shape[0], self.cfg.hidden_size
        x32, L = self._stream_train(pixel_values)
        for lyr in self.layers[self._first_trained():]:
            x32 = self._layer_train(lyr, x32, n, L)
        last, _ = layers.LNStreamFn.apply(x32, self.layernorm.weight, self.layernorm.bias, None, self.dtype, True)
        if return_pre_norm:
            return last.view(n, L, d), x32.view(n, L, d)
        return last.view(n, L, d)

    def _stream_train(self, pixel_values):
        """the fp32 stream in front of the first trained layer -> (x32 [n*L, d], L): the embedding Function when everything trains,
        else the frozen embeddings and layers without autograd.  Drops the frozen path's 16-bit copies of the trained weights."""
        n = pixel_values.shape[0]
        for t in self.parameters():
            if t.requires_grad:
                self._wcache.pop(id(t), None)
        if self.train_layers is None:
            emb = self.embeddings
            x32 = _ViTEmbedFn.apply(pixel_values, emb.patch_embeddings.projection.weight, emb.patch_embeddings.projection.bias,
                                    emb.cls_token, emb.position_embeddings, self.cfg.patch_size, self.dtype)
            return x32, x32.shape[0] // n
        with torch.no_grad():
            x32, L = self._embed_frozen(pixel_values)
            for lyr in self.layers[:self._first_trained()]:
                x32 = self._layer_frozen(lyr, x32, n, L)
        return x32, L

    def _attn_weights(self, a):
        """(W_qkv [3d, d], W_qkv^T, W_o, W_o^T) of a trained layer's attention in the extractor's dtype, cast now"""
        dt = self.dtype
        wqkv, wqkvT = ops.cast_transpose(torch.cat([a.q_proj.weight.detach(), a.k_proj.weight.detach(), a.v_proj.weight.detach()]), dt)
        woc, woT = ops.cast_transpose(a.o_proj.weight.detach(), dt)
        return wqkv, wqkvT, woc, woT

    def _mlp_train(self, lyr, x32):
        """x32 + fc2(gelu(fc1(LN_after(x32)))) with autograd, on however many rows x32 has"""
        dt = self.dtype
        y = layers.LNStreamFn.apply(x32, lyr.layernorm_after.weight, lyr.layernorm_after.bias, None, dt, False)
        m = lyr.mlp
        w1c, w1T = ops.cast_transpose(m.fc1.weight.detach(), dt)
        w2c, w2T = ops.cast_transpose(m.fc2.weight.detach(), dt)
        return layers.MLPLNFn.apply(x32, y, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, None, None, None, ops.ACT_GELU, None,
                                    (w1c, w1T, w2c, w2T))   # (gamma = None: no norm, the fp32 sum is the output)

    def _layer_train(self, lyr, x32, n, L):
        """one trained layer on all tokens (module docstring)"""
        a = lyr.attention
        y = layers.LNStreamFn.apply(x32, lyr.layernorm_before.weight, lyr.layernorm_before.bias, None, self.dtype, False)
        x32 = _ViTAttnFn.apply(x32, y, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.k_proj.bias, a.v_proj.weight,
                               a.v_proj.bias, a.o_proj.weight, a.o_proj.bias, self._attn_weights(a), (n, L, self.cfg.num_attention_heads))
        return self._mlp_train(lyr, x32)

    def _embed_frozen(self, pixel_values):
        """-> (fp32 stream [n*L, d], L)"""
        cfg = self.cfg
        emb = self.embeddings
        n, d = pixel_values.shape[0], cfg.hidden_size
        patches, P = _patch_rows(pixel_values, cfg.patch_size, self.dtype)
        proj = ops.gemm_nt(patches, self._w(emb.patch_embeddings.projection.weight), emb.patch_embeddings.projection.bias,
                           out_f32=True)
        del patches
        return _embed(proj, emb.cls_token, emb.position_embeddings, n, P, d), P + 1

    def _layer_frozen(self, lyr, x32, n, L):
        cfg = self.cfg
        dt = self.dtype
        d, H = cfg.hidden_size, cfg.num_attention_heads
        dev = x32.device
        a = lyr.attention
        _, y, _, _, _ = ops.layernorm_fwd(x32, lyr.layernorm_before.weight, lyr.layernorm_before.bias, dt)
        qkv = torch.empty((n * L, 3 * d), dtype=dt, device=dev)
        for j, lin in enumerate((a.q_proj, a.k_proj, a.v_proj)):
            ops.gemm_nt(y, self._w(lin.weight), lin.bias, out=qkv[:, j * d:(j + 1) * d])
        o, _ = ops.attn_small_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], n, H, L, d // H)
        x32 = ops.gemm_nt(o, self._w(a.o_proj.weight), a.o_proj.bias, residual=x32, out_f32=True)
        _, y, _, _, _ = ops.layernorm_fwd(x32, lyr.layernorm_after.weight, lyr.layernorm_after.bias, dt)
        hmid = ops.gemm_nt(y, self._w(lyr.mlp.fc1.weight), lyr.mlp.fc1.bias, ops.ACT_GELU)
        return ops.gemm_nt(hmid, self._w(lyr.mlp.fc2.weight), lyr.mlp.fc2.bias, residual=x32, out_f32=True)

    def _forward_frozen(self, pixel_values, return_pre_norm):
        n, d = pixel_values.shape[0], self.cfg.hidden_size
        x32, L = self._embed_frozen(pixel_values)
        for lyr in self.layers:
            x32 = self._layer_frozen(lyr, x32, n, L)
        last, _, _, _, _ = ops.layernorm_fwd(x32, self.layernorm.weight, self.layernorm.bias, self.dtype, want32=True, want_t=False)
        if return_pre_norm:
            return last.view(n, L, d), x32.view(n, L, d)
        return last.view(n, L, d)


class ViTBackbone(nn.Module):
    """backbone.py:11-62 on device: (src_sketch [B,1,C,H,W], src_video [B,T,C,H,W]) -> ([B,1,d], [B,T*P,d]).

    Raw frames — uint8 [B,T,H,W,3] (sketch [B,1,H,W,3]), or a list of B tensors [T,H_b,W_b,3] of any sizes — first go through the
    FrameIngest this backbone owns: what ViTFeatureExtractor(images=[frame]) does inside the reference's forward (backbone.py:31,49:
    PIL bilinear resize to 224 x 224, x 1/255, mean / std 0.5), bit for bit, into the fp32 NCHW pixel_values the extractor takes.
    ``pixel_preset`` overrides 'vit'.  ``sketch_filter`` / ``sketch_invert`` give the sketch an ingest of its own, with another of
    Pillow's filters and / or inverted source bytes (preprocess/quickdraw_array_to_pil.py:36 is sketch_filter='bicubic',
    sketch_invert=True on the 28 x 28 bitmaps); a raw sketch may be grey, uint8 [B,1,H,W] or [B,1,H,W,1] (what .convert('RGB')
    replicates, svol_dataset.py:212-229).  With both unset the sketch goes through the frames' ingest.  Float inputs take exactly
    the path they always took."""

    def __init__(self, video_backbone: ViTExtractor, sketch_backbone: ViTExtractor, use_sketch_cls_token: bool = True,
                 frames_per_launch: int = 512, pixel_preset=None, sketch_filter=None, sketch_invert=False, sketch_tokens='pooled'):
        super().__init__()
        self.sketch_tokens = sketch_tokens   # 'grid': all 197 tokens of every sketch go to the head (--sketch_attn tokens)
        s = video_backbone.cfg.image_size
        self.ingest = FrameIngest((s, s), pixel_preset or 'vit', out='nchw_f32')
        self.sketch_ingest = self.ingest
        if sketch_filter is not None or sketch_invert:
            self.sketch_ingest = FrameIngest((s, s), pixel_preset or 'vit', out='nchw_f32', filter=sketch_filter or 'bilinear', invert=sketch_invert)
        self.video_backbone = video_backbone
        self.sketch_backbone = sketch_backbone
        self.use_sketch_cls_token = use_sketch_cls_token
        self.frames_per_launch = frames_per_launch

    def forward(self, src_sketch, src_video):
        # gradients flow only where an extractor takes its autograd path (trainable, .train(), grad mode on)
        with torch.set_grad_enabled(self.sketch_backbone.uses_autograd() or self.video_backbone.uses_autograd()):
            B = len(src_video)
            if is_raw_frames(src_sketch):
                src_sketch = self.sketch_ingest(sketch_frames(src_sketch))
                src_sketch = src_sketch.view(B, -1, *src_sketch.shape[-3:])
            if is_raw_frames(src_video):
                src_video = self.ingest(src_video)
                src_video = src_video.view(B, -1, *src_video.shape[-3:])
            sk = self.sketch_backbone(src_sketch.reshape(-1, *src_sketch.shape[2:]))
            if self.sketch_tokens != 'grid':
                sk = sk[:, :1] if self.use_sketch_cls_token else sk[:, 1:].mean(1, keepdim=True)  # backbone.py:35-38
            frames = src_video.reshape(-1, *src_video.shape[2:])
            outs = [self.video_backbone(frames[i:i + self.frames_per_launch])[:, 1:]
                    for i in range(0, frames.shape[0], self.frames_per_launch)]
            vd = outs[0] if len(outs) == 1 else torch.cat(outs)
            return sk.reshape(B, -1, sk.shape[-1]).contiguous(), vd.reshape(B, -1, vd.shape[-1])
