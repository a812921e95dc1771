"""The per-op ``torch.autograd.Function`` s over the raw wrappers of ``ops``: the only path of the enc/dec Transformer, the ViT and
ResNet extractors, the input projections and the heads of every model, and the A/B reference of the block programs
(``SVOL_NO_BLOCKS=1``).  Where a parameter's gradient is written and what a Function returns for it is ``params.GradGroup``'s
business; the weight copies come from ``params.weights``.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib, ops
from .ops import (ACT_GELU, ACT_NONE, ACT_RELU, _DT, _ptr, _stream, act_bwd, attn_bwd, attn_fwd, attn_weights_mean, cast, colsum,
                  dropout, dropout_add, gemm_nt, gemm_nt_dact, gemm_nt_split, layernorm_bwd, layernorm_fwd)
from .params import SPLIT_V, GradGroup, claim, sink_view, unless_sunk, weights


def _pos_grad(dypos, pos_shape, D):
    """gradient of a broadcast positional operand (the learnable query embedding): sum over the batch."""
    rows = 1
    for n in pos_shape[:-1]:
        rows *= n
    g = colsum(dypos.reshape(-1, rows * D).contiguous())
    return cast(g.view(pos_shape), dypos.dtype)


class LayerNormFn(torch.autograd.Function):
    """y = dropout(LN(x)), compute dtype in / out (input projections, svanet.py:168-178)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, p, seed, seed_dev):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        _, y, _, mean, rstd = layernorm_fwd(x2, gamma, beta, x.dtype, None, p, seed, seed_dev=seed_dev)
        ctx.save_for_backward(x2, gamma, mean, rstd, seed_dev)
        ctx.p, ctx.seed, ctx.shp = p, seed, shp
        ctx.sinks = (claim(gamma, ctx.needs_input_grad[1]), claim(beta, ctx.needs_input_grad[2]))
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, gamma, mean, rstd, seed_dev = ctx.saved_tensors
        sg, sb = ctx.sinks
        _, dx, dg, db = layernorm_bwd(None, dy, None, x2, gamma, mean, rstd, x2.dtype, ctx.p, ctx.seed, seed_dev=seed_dev,
                                      dg_out=sink_view(sg), db_out=sink_view(sb))
        return dx.view(ctx.shp), unless_sunk(sg, dg), unless_sunk(sb, db), None, None, None


def layer_norm(x, gamma, beta, p=0.0, seed=0, seed_dev=None):
    return LayerNormFn.apply(x, gamma, beta, p, seed, seed_dev)


class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) (nn.Linear + F.relu / sigmoid).  out_f32: y is emitted in fp32 (it starts the
    fp32 residual stream); its gradient then arrives in fp32 and is cast once."""

    @staticmethod
    def forward(ctx, x, W, b, act, out_f32):
        if act == ACT_GELU:
            raise _lib.SvolHipError('LinearFn: GELU is only available fused in MLPLNFn')
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        Wc, WcT = weights.get(W, x.dtype)
        y = gemm_nt(x2, Wc, b, act, out_f32=out_f32)
        ctx.save_for_backward(x2, y if act != ACT_NONE else None)
        ctx.WcT, ctx.act, ctx.shp, ctx.has_b = WcT, act, shp, b is not None
        ctx.need_dx = ctx.needs_input_grad[0]
        epc = 4 if x.dtype == torch.float32 else 8
        ok = W.shape[0] % epc == 0
        ctx.sinks = (claim(W, ok and ctx.needs_input_grad[1]), claim(b, ok and ctx.needs_input_grad[2]))
        return y.view(*shp[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, y = ctx.saved_tensors
        N = dy.shape[-1]
        d = dy.reshape(-1, N)
        if not d.is_contiguous():
            d = d.contiguous()
        if d.dtype != x2.dtype:
            d = cast(d, x2.dtype)
        if ctx.act != ACT_NONE:
            d = act_bwd(d, y, ctx.act)
        # out-features that are not a multiple of the 16-byte chunk (2-class / 4-coordinate heads):
        # zero-pad the contraction / column dimension
        epc = 4 if d.dtype == torch.float32 else 8
        WcT = ctx.WcT
        Np = (N + epc - 1) // epc * epc
        if N % epc:
            dp = torch.zeros((d.shape[0], Np), dtype=d.dtype, device=d.device)
            dp[:, :N] = d
            wp = torch.zeros((WcT.shape[0], Np), dtype=WcT.dtype, device=WcT.device)
            wp[:, :N] = WcT
            d, WcT = dp, wp
        # db = column sums of d, fused into the dW GEMM; without gradient sinks dW and db share one zeroed buffer
        K_ = x2.shape[1]
        sW, sb = ctx.sinks
        grads = GradGroup(((sW, (Np, K_)), (sb, (Np,), ctx.has_b)), d.device)
        grads.tn(d, x2, 0, 1 if ctx.has_b else None)
        dW, db = grads.finish()
        if N != Np:   # (never with sinks)
            dW, db = dW[:N], db[:N] if ctx.has_b else None
        dx = gemm_nt(d, WcT).view(ctx.shp) if ctx.need_dx else None
        return dx, dW, db, None, None


def linear(x, W, b=None, act=ACT_NONE, out_f32=False):
    return LinearFn.apply(x, W, b, act, out_f32)


# ---- residual-stream blocks ------------------------------------------------------------------
# Every block maps the stream triple (x32 fp32 residual value, x compute-dtype copy, xpos = x + pos)
# to the next triple; the pre-norm sum s = x32 + f(x) stays fp32 and never leaves the block.
def _ln_out(s32, gamma, beta, pos_out, dt):
    y32, y, ypos, mean, rstd = layernorm_fwd(s32, gamma, beta, dt, pos_out, want32=True)
    return y32, y, ypos, mean, rstd


def _sd(drop):
    """the device-side step counter of drop = (p, seed_a, seed_b[, seed_dev]), or None"""
    return drop[3] if len(drop) > 3 else None


def _block_grad(dy32, dy, dypos, ln, dt, D, drop, sg, sbt, sb):
    """The opening of a residual block's backward: (dy32, dy, dypos) -> (ds32 the stream's gradient, g the gradient of the pre-norm sum
    in the compute dtype, dgamma, dbeta, column sums of g = the bias gradient of the Linear that fed the sum).  ln = (s32, gamma,
    mean, rstd) or None (pre-norm layers: the incoming fp32 stream gradient IS the gradient of the sum); sg / sbt / sb: the sinks
    of gamma, beta and that bias.  drop = (p, ., seed_residual[, seed_dev]): g passes the residual dropout's mask before it meets any GEMM —
    LayerNorm backward without column sums, then the mask in place, then colsum."""
    if ln is None:
        ds32 = dy32.reshape(-1, D)
        ds32 = ds32 if ds32.is_contiguous() else ds32.contiguous()
        dg = dbt = None
        if drop is None:
            g = cast(ds32, dt)
        else:
            g = torch.empty((ds32.shape[0], D), dtype=dt, device=ds32.device)   # (never ds32 itself: that is the stream's gradient)
            dropout(cast(ds32, dt), drop[0], drop[2], out=g, seed_dev=_sd(drop))
    elif drop is None:
        return layernorm_bwd(dy32, dy, dypos, *ln, dt, want32=True, want_colsum=True, dg_out=sink_view(sg), db_out=sink_view(sbt),
                             cs_out=sink_view(sb))
    else:
        ds32, g, dg, dbt = layernorm_bwd(dy32, dy, dypos, *ln, dt, want32=True, dg_out=sink_view(sg), db_out=sink_view(sbt))
        dropout(g, drop[0], drop[2], out=g, seed_dev=_sd(drop))
    return ds32, g, dg, dbt, colsum(g, out=sink_view(sb))


class MLPLNFn(torch.autograd.Function):
    """LN(x32 + fc2(act(fc1(x))))  — cross_modal_transformer.py:142-143,157-158 + MLP :163-179 (GELU); the FFN of the
    enc/dec Transformer (ReLU, transformer.py:191-193,245-247).  gamma None: no norm, the fp32 sum is the output
    (pre-norm layers, transformer.py:205-207: x is then LN(x32), not a copy of x32)."""

    @staticmethod
    def forward(ctx, x32, x, W1, b1, W2, b2, gamma, beta, pos_out, act=ACT_GELU, drop=None, wc=None):
        """drop = (p, seed_hidden, seed_residual[, seed_dev]): training-mode dropout of the enc/dec FFN — linear2(dropout(act(linear1 x)))
        and x + dropout2(.) (transformer.py:168,171,238-240).  seed_dev: a device int64 step counter (ops.dropout), kept alive on ctx and
        not a differentiable input; backward regenerates the masks through the same pointer, so the counter must not move between a
        step's forward and its backward.  wc = (W1, W1^T, W2, W2^T) in the compute dtype, cast by the caller
        (a module that runs before the forward that advances ``weights``' epoch); None: from ``weights``."""
        ctx.set_materialize_grads(False)
        if drop is not None and drop[0] <= 0.0:
            drop = None
        ctx.drop = drop
        shp = x.shape
        D = shp[-1]
        dt = x.dtype
        x2, x32_2 = x.reshape(-1, D), x32.reshape(-1, D)
        if wc is not None:
            W1c, W1T, W2c, W2T = wc
        else:
            W1c, W1T = weights.get(W1, dt)
            W2c, W2T = weights.get(W2, dt)
        if act == ACT_GELU:
            hid, aux = gemm_nt(x2, W1c, b1, ACT_GELU, want_pre=True)   # aux = pre-activation
        elif act == ACT_RELU:
            hid = aux = gemm_nt(x2, W1c, b1, ACT_RELU)                 # relu' = [hid > 0]
        else:
            raise _lib.SvolHipError('MLPLNFn: activation must be GELU or ReLU')
        if drop is not None:
            dropout(hid, drop[0], drop[1], out=hid, seed_dev=_sd(drop))   # (ReLU: aux IS hid — kept entries stay positive, dropped ones get relu' = 0, as the mask wants)
            s32 = dropout_add(gemm_nt(hid, W2c, b2, ACT_NONE, out_f32=True), x32_2 if x32_2.is_contiguous() else x32_2.contiguous(),
                              drop[0], drop[2], _sd(drop))
        else:
            s32 = gemm_nt(hid, W2c, b2, ACT_NONE, residual=x32_2, out_f32=True)
        ctx.W1T, ctx.W2T, ctx.shp, ctx.act, ctx.has_ln = W1T, W2T, shp, act, gamma is not None
        ctx.pos_shape = pos_out.shape if pos_out is not None else None
        nig = ctx.needs_input_grad
        ctx.sinks = tuple(claim(p_, nig[i]) for i, p_ in ((2, W1), (3, b1), (4, W2), (5, b2), (6, gamma), (7, beta)))
        if gamma is None:
            ctx.save_for_backward(x2, aux, hid, None, None, None, None)
            return s32.view(shp)
        y32, y, ypos, mean, rstd = _ln_out(s32, gamma, beta, pos_out, dt)
        ctx.save_for_backward(x2, aux, hid, s32, gamma, mean, rstd)
        if pos_out is not None:
            return y32.view(shp), y.view(shp), ypos.view(shp)
        return y32.view(shp), y.view(shp)

    @staticmethod
    def backward(ctx, dy32, dy=None, dypos=None):
        x2, aux, hid, s32, gamma, mean, rstd = ctx.saved_tensors
        dt = x2.dtype
        D = x2.shape[1]
        dpos = None
        if ctx.pos_shape is not None and ctx.needs_input_grad[8] and dypos is not None:
            dpos = _pos_grad(dypos, ctx.pos_shape, D)
        sW1, sb1, sW2, sb2, sg, sbt = ctx.sinks
        drop = ctx.drop
        ds32, ds, dg, dbt, db2 = _block_grad(dy32, dy, dypos, (s32, gamma, mean, rstd) if ctx.has_ln else None, dt, D, drop, sg, sbt,
                                             sb2)
        F_ = hid.shape[1]
        grads = GradGroup(((sW1, (F_, D)), (sW2, (D, F_))), ds.device)   # dW1 | dW2
        grads.tn(ds, hid, 1)
        # (ds W2) * act'(aux) and its column sums, one kernel
        if drop is not None:   # ... then the hidden dropout's mask, then the column sums
            dpre, _ = gemm_nt_dact(ds, ctx.W2T, aux, ctx.act, want_colsum=False)
            dropout(dpre, drop[0], drop[1], out=dpre, seed_dev=_sd(drop))
            db1 = colsum(dpre, out=sink_view(sb1))
        else:
            dpre, db1 = gemm_nt_dact(ds, ctx.W2T, aux, ctx.act, colsum_out=sink_view(sb1))
        grads.tn(dpre, x2, 0)
        dx = gemm_nt(dpre, ctx.W1T)
        dW1, dW2 = grads.finish()
        n_ = unless_sunk
        return (ds32.view(ctx.shp), dx.view(ctx.shp), dW1, n_(sb1, db1), dW2, n_(sb2, db2), n_(sg, dg), n_(sbt, dbt), dpos, None, None,
                None)


class AttnLNFn(torch.autograd.Function):
    """LN(xq32 + out_proj(MHA(q = Wq xq_pos, k = Wk xk_pos, v = Wv xv))) with packed in_proj
    (nn.MultiheadAttention + post-norm, cross_modal_transformer.py:137-141,145-149,151-156; transformer.py:183-189,
    237-250).  ``self_attn``: xk_pos is xq_pos and xv is xq (one packed projection buffer).  gamma None: no norm, the
    fp32 sum is the output (pre-norm layers, transformer.py:198-203: xq is then LN(xq32)).  ``need_weights``: also
    return the head-averaged attention weights [B,Lq,Lk] fp32 (no gradient flows into them)."""

    @staticmethod
    def forward(ctx, xq32, xq, xq_pos, xk_pos, xv, W_in, b_in, W_o, b_o, gamma, beta, pos_out, H, kbias, self_attn,
                need_weights=False, drop=None, core=None):
        """core = 'fewkeys' (cross configuration): the attention core runs on the many-queries / few-keys kernels
        (ops.attn_fewkeys_fwd / _bwd) where ops.attn_fewkeys_ok takes the shape, ops.attn_fewkeys_faster says they were measured
        faster and there is no dropout; otherwise, and always with core None, on attn_fwd / attn_bwd.  'fewkeys!' skips the speed rule.
        drop = (p, seed_attention, seed_residual[, seed_dev]): training-mode dropout of the enc/dec attention blocks — on the attention
        probabilities (nn.MultiheadAttention(dropout=p)) and on the block output before the residual add (dropout1 / dropout2,
        transformer.py:158-177,216-247).  The returned attention weights stay those of the undropped softmax.  seed_dev: a device int64
        step counter (ops.attn_fwd), kept alive on ctx, not a differentiable input; backward regenerates the masks through the same
        pointer, so the counter must not move between a step's forward and its backward."""
        ctx.set_materialize_grads(False)
        if drop is not None and drop[0] <= 0.0:
            drop = None
        ctx.drop = drop
        B, Lq, d = xq.shape
        dt = xq.dtype
        Lk = Lq if self_attn else xv.shape[1]
        dh = d // H
        # MIXED cross-attention (the bf16 model's query -> video attention): the few object queries travel in fp32
        # (xq / xq_pos fp32: q-projection, out-projection, residual and norm in exact fp32 GEMMs — a few hundred rows),
        # the L video tokens in bf16 (K / V projections and the attention core on the MFMA bf16 path).  q and O cross
        # the boundary through one rounding each.
        mixed = (not self_attn) and dt == torch.float32 and xv.dtype != torch.float32
        dkv = xv.dtype if mixed else dt
        Wc, WcT = weights.get(W_in, dkv)
        Woc, WoT = weights.get(W_o, dt)
        # bf16: the projection GEMM emits q already multiplied by d_h^-1/2 * log2(e) (rounded once, in the fp32
        # epilogue), which lets the attention kernels exponentiate raw MFMA results
        premul = (LOG2E / math.sqrt(dh)) if dkv != torch.float32 else 0.0
        qscale = _qscale(d, premul, xq.device) if premul else None
        a_qp = xq_pos.reshape(B * Lq, d)
        a_q = xq.reshape(B * Lq, d)
        a_kp = a_qp if self_attn else xk_pos.reshape(B * Lk, d)
        a_v = a_q if self_attn else xv.reshape(B * Lk, d)
        Wq32T = None
        # bf16: the V projection uses SPLIT weights (hi + lo, 16 mantissa bits; svol_gemm_nt_split) — see SPLIT_V
        Wv_hilo = weights.get_split(W_in, 2 * d, d) if (SPLIT_V and dkv == torch.bfloat16 and d % 32 == 0) else None
        if self_attn:
            qkv = torch.empty((B * Lq, 3 * d), dtype=dt, device=xq.device)
            gemm_nt(a_qp, Wc[:2 * d], b_in[:2 * d], out=qkv[:, :2 * d], colscale=qscale)
            q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        else:
            if mixed:
                W32, W32T = weights.get(W_in, torch.float32)
                Wq32T = W32T[:, :d]
                q = cast(gemm_nt(a_qp, W32[:d], b_in[:d], colscale=qscale[:d]), dkv)
            else:
                q = gemm_nt(a_qp, Wc[:d], b_in[:d], colscale=qscale[:d] if qscale is not None else None)
            kv = torch.empty((B * Lk, 2 * d), dtype=dkv, device=xq.device)
            k, v = kv[:, :d], kv[:, d:]
            gemm_nt(a_kp, Wc[d:2 * d], b_in[d:2 * d], out=k)
        if Wv_hilo is not None:   # the V projection, into its columns of the packed buffer
            gemm_nt_split(a_v, Wv_hilo, b_in[2 * d:], out=v)
        else:
            gemm_nt(a_v, Wc[2 * d:], b_in[2 * d:], out=v)
        if core not in (None, 'fewkeys', 'fewkeys!'):
            raise _lib.SvolHipError(f'AttnLNFn: unknown attention core {core!r}')
        # 'fewkeys': where the kernels take the shape AND were measured faster than attn_fwd / attn_bwd (ops.attn_fewkeys_faster);
        # 'fewkeys!': wherever they take the shape (benchmarks, tests)
        fewkeys = (core in ('fewkeys', 'fewkeys!') and not self_attn and drop is None and ops.attn_fewkeys_ok(dkv, Lk, dh)
                   and (core == 'fewkeys!' or ops.attn_fewkeys_faster(Lk, dh)))
        if fewkeys:
            o, lse2 = ops.attn_fewkeys_fwd(q, k, v, B, H, Lq, Lk, dh, kbias, premul)
        else:
            o, lse2 = attn_fwd(q, k, v, B, H, Lq, Lk, dh, kbias, premul, drop=(drop[0], drop[1], _sd(drop)) if drop is not None else None)
        att = attn_weights_mean(q, k, lse2, B, H, Lq, Lk, dh, kbias, premul) if need_weights else None
        if drop is not None:
            r32 = xq32.reshape(B * Lq, d)
            s32 = dropout_add(gemm_nt(cast(o, dt) if mixed else o, Woc, b_o, out_f32=True), r32 if r32.is_contiguous() else r32.contiguous(),
                              drop[0], drop[2], _sd(drop))
        else:
            s32 = gemm_nt(cast(o, dt) if mixed else o, Woc, b_o, residual=xq32.reshape(B * Lq, d), out_f32=True)
        ctx.WcT, ctx.WoT, ctx.dims, ctx.self_attn, ctx.premul = WcT, WoT, (B, H, Lq, Lk, dh, d), self_attn, premul
        ctx.mixed, ctx.Wq32T, ctx.fewkeys = mixed, Wq32T, fewkeys
        ctx.pos_shape = pos_out.shape if pos_out is not None else None
        ctx.has_ln = gamma is not None
        nig = ctx.needs_input_grad
        ctx.sinks = tuple(claim(p_, nig[i]) for i, p_ in ((5, W_in), (6, b_in), (7, W_o), (8, b_o), (9, gamma),
                                                           (10, beta)))
        if any(s_ is None for s_ in ctx.sinks[:6 if ctx.has_ln else 4]):  # all or nothing
            ctx.sinks = (None,) * 6
        shp = (B, Lq, d)
        if att is not None:
            ctx.mark_non_differentiable(att)
        tail = (att,) if att is not None else ()
        if gamma is None:
            ctx.save_for_backward(a_qp, a_q, a_kp, a_v, q, k, v, o, lse2, kbias, None, None, None, None)
            return (s32.view(shp),) + tail if tail else s32.view(shp)
        y32, y, ypos, mean, rstd = _ln_out(s32, gamma, beta, pos_out, dt)
        ctx.save_for_backward(a_qp, a_q, a_kp, a_v, q, k, v, o, lse2, kbias, s32, gamma, mean, rstd)
        if pos_out is not None:
            return (y32.view(shp), y.view(shp), ypos.view(shp)) + tail
        return (y32.view(shp), y.view(shp)) + tail

    @staticmethod
    def backward(ctx, dy32, *rest):
        a_qp, a_q, a_kp, a_v, q, k, v, o, lse2, kbias, s32, gamma, mean, rstd = ctx.saved_tensors
        B, H, Lq, Lk, dh, d = ctx.dims
        dt = a_q.dtype
        WcT, WoT = ctx.WcT, ctx.WoT  # WcT: [d, 3d] ; WoT: [d, d]
        dy = rest[0] if ctx.has_ln and len(rest) > 0 else None
        dypos = rest[1] if ctx.has_ln and ctx.pos_shape is not None and len(rest) > 1 else None
        dpos = None
        if ctx.pos_shape is not None and ctx.needs_input_grad[11] and dypos is not None:
            dpos = _pos_grad(dypos, ctx.pos_shape, d)
        sW_in, sb_in, sWo, sbo, sg, sbt = ctx.sinks   # (all or none)
        drop = ctx.drop
        # the block output's gradient passes the residual dropout's mask before out_proj's backward
        ds32, g, dg, dbt, dbo = _block_grad(dy32, dy, dypos, (s32, gamma, mean, rstd) if ctx.has_ln else None, dt, d, drop, sg, sbt,
                                            sbo)
        grads = GradGroup(((sW_in, (3 * d, d)), (sb_in, (3 * d,)), (sWo, (d, d))), g.device)   # dW_in | db_in | dW_o
        W_IN, B_IN, W_O = 0, 1, 2
        mixed = ctx.mixed
        adrop = (drop[0], drop[1], _sd(drop)) if drop is not None else None
        grads.tn(g, cast(o, dt) if mixed else o, W_O)
        do = gemm_nt(g, WoT)
        if mixed:
            do = cast(do, o.dtype)
        shq = (B, Lq, d)
        if ctx.self_attn:
            dqkv = torch.empty((B * Lq, 3 * d), dtype=dt, device=g.device)
            dq, dk, dv = dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:]
            attn_bwd(q, k, v, o, do, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbias, ctx.premul, drop=adrop)
            grads.tn(dqkv[:, :2 * d], a_qp, W_IN, B_IN, slice(0, 2 * d))
            grads.tn(dv, a_q, W_IN, B_IN, slice(2 * d, 3 * d))
            dxq_pos = gemm_nt(dqkv[:, :2 * d], WcT[:, :2 * d])  # d(x + pos) = [dq dk] W_qk
            dxq = gemm_nt(dv, WcT[:, 2 * d:])                    # d(x) through V
            dx = (dxq.view(shq), dxq_pos.view(shq), None, None)
        else:
            dq = torch.empty((B * Lq, d), dtype=q.dtype, device=g.device)
            dkv = torch.empty((B * Lk, 2 * d), dtype=k.dtype, device=g.device)
            dk, dv = dkv[:, :d], dkv[:, d:]
            if ctx.fewkeys:
                ops.attn_fewkeys_bwd(q, k, v, o, do, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbias, ctx.premul)
            else:
                attn_bwd(q, k, v, o, do, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbias, ctx.premul, drop=adrop)
            if mixed:
                dq = cast(dq, dt)
            grads.tn(dq, a_qp, W_IN, B_IN, slice(0, d))
            grads.tn(dk, a_kp, W_IN, B_IN, slice(d, 2 * d))
            grads.tn(dv, a_v, W_IN, B_IN, slice(2 * d, 3 * d))
            dxq_pos = gemm_nt(dq, ctx.Wq32T if mixed else WcT[:, :d])
            dxk_pos = gemm_nt(dk, WcT[:, d:2 * d])
            dxv = gemm_nt(dv, WcT[:, 2 * d:])
            shk = (B, Lk, d)
            dx = (None, dxq_pos.view(shq), dxk_pos.view(shk), dxv.view(shk))
        n_ = unless_sunk
        return (ds32.view(shq),) + dx + grads.finish() + (n_(sbo, dbo), n_(sg, dg), n_(sbt, dbt), dpos, None, None, None, None, None, None)


class LNStreamFn(torch.autograd.Function):
    """(y, y + pos) = LN(x32) in the compute dtype from the fp32 residual stream — the norm that OPENS a pre-norm
    block (transformer.py:198-199, 205, 267-268, 274, 280) and the decoder's shared output norm."""

    @staticmethod
    def forward(ctx, x32, gamma, beta, pos, dtype, want32):
        ctx.set_materialize_grads(False)
        shp = x32.shape
        D = shp[-1]
        x2 = x32.reshape(-1, D)
        y32, y, ypos, mean, rstd = layernorm_fwd(x2, gamma, beta, dtype, pos, want32=want32)
        ctx.save_for_backward(x2, gamma, mean, rstd)
        ctx.shp, ctx.dtype, ctx.has_pos, ctx.want32 = shp, dtype, pos is not None, want32
        ctx.pos_shape = pos.shape if pos is not None else None
        ctx.sinks = (claim(gamma, ctx.needs_input_grad[1]), claim(beta, ctx.needs_input_grad[2]))
        out = ((y32.view(shp),) if want32 else ()) + (y.view(shp),) + ((ypos.view(shp),) if pos is not None else ())
        return out if len(out) > 1 else out[0]

    @staticmethod
    def backward(ctx, *grads):
        x2, gamma, mean, rstd = ctx.saved_tensors
        g = list(grads)
        dy32 = g.pop(0) if ctx.want32 else None
        dy = g.pop(0)
        dypos = g.pop(0) if ctx.has_pos else None
        if dy32 is None and dy is None and dypos is None:
            return None, None, None, None, None, None
        sg, sb = ctx.sinks
        dpos = None
        if dypos is not None and ctx.needs_input_grad[3]:
            dpos = _pos_grad(dypos, ctx.pos_shape, x2.shape[1])
        dx32, _, dg, db = layernorm_bwd(dy32, dy, dypos, x2, gamma, mean, rstd, ctx.dtype, want32=True, want_t=False,
                                        dg_out=sink_view(sg), db_out=sink_view(sb))
        return dx32.view(ctx.shp), unless_sunk(sg, dg), unless_sunk(sb, db), dpos, None, None


LOG2E = 1.4426950408889634
_QSCALE = {}


def _qscale(d, premul, device):
    """per-column epilogue factor of the packed q|k projection: premul on the q columns, 1 on the k columns."""
    key = (d, premul, str(device))
    t = _QSCALE.get(key)
    if t is None:
        t = torch.ones((2 * d,), dtype=torch.float32, device=device)
        t[:d] = premul
        _QSCALE[key] = t
    return t


def mlp_ln(x32, x, W1, b1, W2, b2, gamma, beta, pos_out=None, act=ACT_GELU, drop=None):
    return MLPLNFn.apply(x32, x, W1, b1, W2, b2, gamma, beta, pos_out, act, drop)


def self_attn_ln(x32, x, x_pos, W_in, b_in, W_o, b_o, gamma, beta, pos_out, H, kbias=None, drop=None):
    return AttnLNFn.apply(x32, x, x_pos, None, None, W_in, b_in, W_o, b_o, gamma, beta, pos_out, H, kbias, True, False, drop)


def cross_attn_ln(xq32, xq, xq_pos, xk_pos, xv, W_in, b_in, W_o, b_o, gamma, beta, pos_out, H, kbias,
                  need_weights=False, drop=None, core=None):
    if core is None:   # (exactly the call it always was)
        return AttnLNFn.apply(xq32, xq, xq_pos, xk_pos, xv, W_in, b_in, W_o, b_o, gamma, beta, pos_out, H, kbias, False,
                              need_weights, drop)
    return AttnLNFn.apply(xq32, xq, xq_pos, xk_pos, xv, W_in, b_in, W_o, b_o, gamma, beta, pos_out, H, kbias, False,
                          need_weights, drop, core)


def ln_stream(x32, gamma, beta, pos, dtype, want32=False):
    return LNStreamFn.apply(x32, gamma, beta, pos, dtype, want32)


class GateFn(torch.autograd.Function):
    """(mem32, mem, mem + pos) with mem = LN1(x * (1 + a)), a = head-mean softmax of the 1-query
    sketch->video attention (cross_modal_transformer.py:122-127); u = per-(batch, head) folded
    key projection [B,H,d] fp32.  x32 is the fp32 residual stream."""

    @staticmethod
    def forward(ctx, x32, pos, u, gamma, beta, H):
        ctx.set_materialize_grads(False)
        B, L, D = x32.shape
        dt = pos.dtype
        x2 = x32.reshape(B * L, D).contiguous()
        assert x2.dtype == torch.float32
        pos2 = pos.reshape(B * L, D).contiguous()
        u = u.contiguous().float()
        y32 = torch.empty((B * L, D), dtype=torch.float32, device=x2.device)
        y = torch.empty((B * L, D), dtype=dt, device=x2.device)
        ypos = torch.empty((B * L, D), dtype=dt, device=x2.device)
        a = torch.empty((B * L,), dtype=torch.float32, device=x2.device)
        mean = torch.empty_like(a)
        rstd = torch.empty_like(a)
        ws = torch.empty((B * H * (L + 2),), dtype=torch.float32, device=x2.device)
        rc = _lib.lib().svol_gate_fwd(_ptr(x2), _ptr(pos2), _ptr(u), _ptr(gamma), _ptr(beta), _ptr(y32), _ptr(y),
                                      _ptr(ypos), _ptr(a), _ptr(mean), _ptr(rstd), _ptr(ws), B, L, D, H, _DT[dt],
                                      _stream())
        _lib.check(rc, 'svol_gate_fwd')
        ctx.save_for_backward(x2, pos2, u, gamma, a, mean, rstd, ws)
        ctx.dims = (B, L, D, H)
        ctx.sinks = (claim(gamma, ctx.needs_input_grad[3]), claim(beta, ctx.needs_input_grad[4]))
        return y32.view(B, L, D), y.view(B, L, D), ypos.view(B, L, D)

    @staticmethod
    def backward(ctx, dy32, dy, dypos):
        x2, pos2, u, gamma, a, mean, rstd, ws = ctx.saved_tensors
        B, L, D, H = ctx.dims
        cont = lambda t: None if t is None else t.reshape(B * L, D).contiguous()
        dy32, dy, dypos = cont(dy32), cont(dy), cont(dypos)
        dx32 = torch.empty_like(x2)
        sg, sb = ctx.sinks
        grads = GradGroup(((None, (B, H, D)), (sg, (D,)), (sb, (D,))), x2.device, each=True)   # one memset: du | dgamma | dbeta
        du, dg, db = grads.out
        ws2 = torch.empty((B * L + B * H,), dtype=torch.float32, device=x2.device)
        rc = _lib.lib().svol_gate_bwd(_ptr(dy32), _ptr(dy), _ptr(dypos), _ptr(x2), _ptr(pos2), _ptr(u), _ptr(gamma),
                                      _ptr(a), _ptr(mean), _ptr(rstd), _ptr(ws), _ptr(ws2), _ptr(dx32), _ptr(du),
                                      _ptr(dg), _ptr(db), B, L, D, H, _DT[pos2.dtype], _stream())
        _lib.check(rc, 'svol_gate_bwd')
        return (dx32.view(B, L, D), None) + grads.finish() + (None,)


def gate(x32, pos, u, gamma, beta, H):
    return GateFn.apply(x32, pos, u, gamma, beta, H)


class CastFn(torch.autograd.Function):
    """dtype change on the autograd tape (fp32 master parameter / feature -> compute dtype and back)."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return cast(x, dtype)

    @staticmethod
    def backward(ctx, dy):
        return cast(dy.contiguous(), ctx.src), None


def cast_ag(x, dtype):
    return x if x.dtype == dtype else CastFn.apply(x, dtype)


# ---- the forward -> backward turn: heads, criterion glue (csrc/heads.hip) ------------------------------------------------------------
FUSED_HEADS = os.environ.get('SVOL_NO_FUSED_HEADS') is None and os.environ.get('SVOL_DETERMINISTIC') is None


def heads_fusable(hs, class_embed, bbox_embed):
    """the one-launch heads take: fp32 decoder states of width D (multiple of 32, <= 512), Linear(D, 2) and a 3-layer MLP(D, D, 4)."""
    if not FUSED_HEADS or hs.dtype != torch.float32 or not hs.is_cuda:
        return False
    D = hs.shape[-1]
    ls = list(bbox_embed.layers)
    return (D % 32 == 0 and D <= 512 and len(ls) == 3 and tuple(class_embed.weight.shape) == (2, D) and class_embed.bias is not None
            and tuple(ls[0].weight.shape) == (D, D) and tuple(ls[1].weight.shape) == (D, D) and tuple(ls[2].weight.shape) == (4, D)
            and all(l.bias is not None for l in ls) and all(t.dtype == torch.float32 for t in (class_embed.weight, ls[0].weight)))


class HeadsFn(torch.autograd.Function):
    """(pred_logits, pred_boxes) of ALL decoder layers from the stacked states hs [..., D]: class_embed = Linear(D, 2) and
    bbox_embed = MLP(D, D, 4, 3) -> sigmoid (svanet.py:125-127) in ONE launch, exact fp32; the backward is one launch for dhs and the
    2- / 4-row weight gradients, the two D x D weight gradients go to the weight-gradient stream."""

    @staticmethod
    def forward(ctx, hs, Wc, bc, W0, b0, W1, b1, W2, b2):
        shp = hs.shape
        D = shp[-1]
        hs2 = hs.reshape(-1, D)
        if not hs2.is_contiguous():
            hs2 = hs2.contiguous()
        R = hs2.shape[0]
        dev = hs.device
        logits = torch.empty((R, 2), dtype=torch.float32, device=dev)
        boxes = torch.empty((R, 4), dtype=torch.float32, device=dev)
        hid = torch.empty((2, R, D), dtype=torch.float32, device=dev)
        rc = _lib.lib().svol_heads_fwd(_ptr(hs2), _ptr(Wc), _ptr(bc), _ptr(W0), _ptr(b0), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(logits),
                                       _ptr(hid[0]), _ptr(hid[1]), _ptr(boxes), R, D, _stream())
        _lib.check(rc, 'svol_heads_fwd')
        ctx.save_for_backward(hs2, hid, boxes, Wc, W0, W1, W2)
        ctx.shp = shp
        ni = ctx.needs_input_grad
        ctx.sinks = tuple(claim(p_, ni[i + 1]) for i, p_ in enumerate((Wc, bc, W0, b0, W1, b1, W2, b2)))
        return logits.view(*shp[:-1], 2), boxes.view(*shp[:-1], 4)

    @staticmethod
    def backward(ctx, dlogits, dboxes):
        hs2, hid, boxes, Wc, W0, W1, W2 = ctx.saved_tensors
        R, D = hs2.shape
        dev = hs2.device
        dlogits = torch.zeros((R, 2), dtype=torch.float32, device=dev) if dlogits is None else dlogits.reshape(R, 2).float().contiguous()
        dboxes = torch.zeros((R, 4), dtype=torch.float32, device=dev) if dboxes is None else dboxes.reshape(R, 4).float().contiguous()
        sWc, sbc, sW0, sb0, sW1, sb1, sW2, sb2 = ctx.sinks
        g = torch.empty((3, R, D), dtype=torch.float32, device=dev)   # dhs, g_pre0, g_pre1
        small = GradGroup(((sWc, (2, D)), (sW2, (4, D)), (sbc, (2,)), (sb2, (4,))), dev, each=True)
        dWc, dW2, dbc, db2 = small.out
        rc = _lib.lib().svol_heads_bwd(_ptr(dlogits), _ptr(dboxes), _ptr(hs2), _ptr(hid[0]), _ptr(hid[1]), _ptr(boxes), _ptr(Wc), _ptr(W0),
                                       _ptr(W1), _ptr(W2), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(dWc), _ptr(dbc), _ptr(dW2), _ptr(db2),
                                       R, D, _stream())
        _lib.check(rc, 'svol_heads_bwd')
        ni = ctx.needs_input_grad
        dWc, dW2, dbc, db2 = small.finish()
        out = [g[0].view(ctx.shp) if ni[0] else None, dWc, dbc]
        for gp, x, sW, sb, iw in ((g[1], hs2, sW0, sb0, 3), (g[2], hid[0], sW1, sb1, 5)):
            pair = GradGroup(((sW, (D, D)), (sb, (D,))), dev)
            pair.tn(gp, x, 0, 1)      # with sinks: off the critical path (weight-gradient stream)
            dW_, db_ = pair.finish()
            out += [dW_ if ni[iw] else None, db_ if ni[iw + 1] else None]
        out += [dW2, db2]
        return tuple(out)


def heads(hs, class_embed, bbox_embed):
    ls = bbox_embed.layers
    return HeadsFn.apply(hs, class_embed.weight, class_embed.bias, ls[0].weight, ls[0].bias, ls[1].weight, ls[1].bias, ls[2].weight, ls[2].bias)


class WeightedTotalFn(torch.autograd.Function):
    """sum(losses * w) over the [layers, 4] loss table (train.py:227-228) as one tiny launch each way."""

    @staticmethod
    def forward(ctx, losses, w):
        x = losses.contiguous()
        out = torch.empty((), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().svol_weighted_total(_ptr(x), _ptr(w), x.numel(), _ptr(out), _stream()), 'svol_weighted_total')
        ctx.save_for_backward(w)
        ctx.shape = losses.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        (w,) = ctx.saved_tensors
        d = dout.float().contiguous()
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=w.device)
        _lib.check(_lib.lib().svol_weighted_total_bwd(_ptr(w), _ptr(d), w.numel(), _ptr(dx), _stream()), 'svol_weighted_total_bwd')
        return dx, None


class SetCriterionFn(torch.autograd.Function):
    """All decoder layers' matching + losses in three launches (cost, LSAP, loss); no host sync.
    logits [NL,B,N,2], boxes [NL,B,N,4] fp32 -> losses [NL,4] = (label, bbox, giou, class_error)."""

    @staticmethod
    def forward(ctx, logits, boxes, packed, w_bbox, w_giou, w_class, eos_coef):
        NL = logits.shape[0]
        rows = logits.shape[1] * logits.shape[2]
        lg = logits.contiguous().float()
        bx = boxes.contiguous().float()
        match = match_all(lg, bx, packed, w_bbox, w_giou, w_class)
        losses = torch.empty((NL, 4), dtype=torch.float32, device=lg.device)
        g_label = torch.empty_like(lg)
        g_bbox = torch.empty_like(bx)
        g_giou = torch.empty_like(bx)
        rc = _lib.lib().svol_set_loss(_ptr(lg), _ptr(bx), _ptr(packed.tgt_boxes), _ptr(match), _ptr(losses),
                                      _ptr(g_label), _ptr(g_bbox), _ptr(g_giou), NL, rows, float(eos_coef),
                                      _ptr(packed.rebase_vid_off), logits.shape[2], _ptr(packed.status),
                                      _ptr(packed.box_status), packed.problems_per_layer, _stream())
        _lib.check(rc, 'svol_set_loss')
        ctx.save_for_backward(g_label, g_bbox, g_giou)
        ctx.mark_non_differentiable(match)
        return losses, match

    @staticmethod
    def backward(ctx, dl, _dmatch):
        g_label, g_bbox, g_giou = ctx.saved_tensors
        dl = dl.float()
        if FUSED_HEADS and dl.is_contiguous():   # one launch instead of five elementwise ones (csrc/heads.hip)
            dlog, dbox = torch.empty_like(g_label), torch.empty_like(g_bbox)
            NL = g_label.shape[0]
            rc = _lib.lib().svol_set_loss_bwd(_ptr(g_label), _ptr(g_bbox), _ptr(g_giou), _ptr(dl), _ptr(dlog), _ptr(dbox), NL,
                                              g_label.numel() // (2 * NL), _stream())
            _lib.check(rc, 'svol_set_loss_bwd')
            return dlog, dbox, None, None, None, None, None
        dlog = g_label * dl[:, 0].view(-1, 1, 1, 1)
        dbox = g_bbox * dl[:, 1].view(-1, 1, 1, 1) + g_giou * dl[:, 2].view(-1, 1, 1, 1)
        return dlog, dbox, None, None, None, None, None


def match_all(lg, bx, packed, w_bbox, w_giou, w_class):
    """cost blocks + batched LSAP for every problem in `packed`; returns match[R] int32
    (global target row per prediction row, -1 = unmatched)."""
    R = lg.shape[0] * lg.shape[1] * lg.shape[2]
    cost = torch.empty((max(1, packed.cost_numel),), dtype=torch.float32, device=lg.device)
    match = torch.empty((R,), dtype=torch.int32, device=lg.device)
    L = _lib.lib()
    rc = L.svol_match_cost(_ptr(lg), _ptr(bx), _ptr(packed.tgt_boxes), _ptr(packed.pred_off), _ptr(packed.pred_cnt),
                           _ptr(packed.tgt_off), _ptr(packed.tgt_cnt), _ptr(packed.cost_off), _ptr(cost),
                           packed.n_problems, float(w_bbox), float(w_giou), float(w_class), _ptr(packed.box_status),
                           _stream())
    _lib.check(rc, 'svol_match_cost')
    rc = L.svol_lsap_batched(_ptr(cost), _ptr(packed.cost_off), _ptr(packed.pred_off), _ptr(packed.pred_cnt),
                             _ptr(packed.tgt_off), _ptr(packed.tgt_cnt), _ptr(match), _ptr(packed.status),
                             packed.n_problems, packed.max_dim, _stream())
    _lib.check(rc, 'svol_lsap_batched')
    packed.last_cost = cost
    return match
