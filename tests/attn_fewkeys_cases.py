"""Many queries, few keys (csrc/attn_fewkeys.hip: svol_attn_fewkeys_fwd / _bwd): the cases, the inputs, the fp64 reference, the emulation
of the kernels' rounding sites and the figures (plain torch on the CPU, importable without the device library).
tests/test_attn_fewkeys_cases.py holds this file's emulation to the constants the device test quotes, tests/test_gpu_attn_fewkeys.py
runs the cases on the device.

1. Points (B, H, Lq, Lk, dh, family, mask, premul).  Lk in LKS: 1 (P = 1, dS = 0); 31 / 32 / 33 and 64 / 65: the edges of the 32-key
   blocks the kernels work in (one, two, three blocks: the backward splits its eight waves 8 / 4 / 2 ways over them); 49 (the 7 x 7
   grid), 197 (the ViT's tokens), 256 (the limit, eight blocks: one wave each).  Lq in LQS: 1; 33 and 160 (a ragged 32-query block, more
   than the forward's four waves); chunk_rows(1) = 256 (one chunk, one backward tile exactly) and 257 (two chunks, the second a one-row
   tail); 2049: chunk_rows = 512, so a workgroup walks TWO backward tiles and the fifth chunk is a one-row tail.  chunk_rows restates
   the library's rule (ops.attn_fewkeys_chunk; tests/test_attn_fewkeys_cases.py holds the two together).  Not the full product: every
   Lk at both head widths twice, the other coordinates cycling.
2. Families.  'normal': randn * 1.2.  'first' / 'last' / 'deep': the planted scores of tests/attn_cls_cases.py on every query row:
   channel 0 of every head is reserved, q0 = +-256 (+ in even batch rows) with the row's other channels scaled by 0.25, k0 = 0 except
   at key 0 / key Lk - 1, where it is +-KD: that key outscores every other by about 145 log2 units (P is one-hot); 'deep': every key
   at -+KD, every score about -145 units.  Every planted value is exact in bf16 and fp16.
3. Masks (kbias 0 / -inf, different per batch row, B = 2).  'edges': row 0 has its first key masked, row 1 its last.  'one_live': row 0
   has every key but Lk // 2 masked, row 1 its first and last.  The K and V rows of a masked key hold NaN: the contract is that they
   are not used.
4. premul: q is handed over already multiplied by d_h^-1/2 log2 e and rounded (what AttnLNFn's projection epilogue does); the
   reference takes that rounded q back through 1 / premul, dq stays the gradient with respect to the unscaled q.
5. Canary rows: k / v carry CANARY_ROWS rows behind B Lk, q / do behind B Lq; the kernels get views of the leading rows.  Canary keys
   are 64 sign(q of the last row) (they would win), canary v / q / do rows are NaN.
6. `figures`: slice errors (tests/slice_metrics.py) of o / dq per (batch, head) and of dk / dv per (batch, head, 64-key block); element
   errors on the same slices against the slice's largest reference entry; lse2; finiteness; dk / dv rows of masked keys exactly 0.  A
   reference that is identically zero (dq, dk under a one-hot P) is measured on dv's scale.
"""
from __future__ import annotations

import functools
import math

import torch

from tests import slice_metrics as S

LOG2E = 1.4426950408889634
BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = (BF16, FP16)
LKS = (1, 31, 32, 33, 49, 64, 65, 197, 256)
LQS = (1, 33, 160, 256, 257)
DHS = (32, 64)
FAMILIES = ('normal', 'first', 'last', 'deep')
MASKS = ('none', 'edges', 'one_live')
KEY_BLOCK = 64
CANARY_ROWS = 32
CANARY_MAG = 64.0
A = 256.0
KD = {32: 2.25, 64: 3.125}
TOL = {BF16: 1.2e-2, FP16: 1.5e-3}     # tests/gpu_checks.py TOL: o; the gradients take twice that
LSE_BAR = 2e-5                         # of max(1, max |lse2|)
TINY = 2.0 ** -126


def chunk_rows(Lq):
    """queries one workgroup walks (svol_attn_fewkeys_chunk_rows): at most 8 chunks of whole 256-query tiles"""
    return 256 * (-(-Lq // 2048))


def points():
    """[(B, H, Lq, Lk, dh, family, mask, premul)]"""
    assert chunk_rows(1) == 256 and chunk_rows(257) == 256 and chunk_rows(2049) == 512
    pts = []
    for sweep in range(2):
        for i, Lk in enumerate(LKS):
            for j, dh in enumerate(DHS):
                n = 2 * i + j + 3 * sweep
                mask = MASKS[(n + sweep) % 3] if Lk >= 3 else 'none'
                B = 2 if mask != 'none' else (1, 2)[n % 2]
                pts.append((B, (1, 3)[(n // 2 + sweep) % 2], LQS[n % len(LQS)], Lk, dh, FAMILIES[(n + i) % 4], mask, False))
    pts += [(1, 1, 2049, 49, 32, 'normal', 'none', False), (2, 1, 2049, 33, 64, 'normal', 'edges', True),
            (2, 3, 257, 49, 32, 'normal', 'edges', True), (1, 3, 160, 197, 64, 'normal', 'none', True)]
    return pts


def point_id(B, H, Lq, Lk, dh, fam, mask, premul):
    return f'B{B}-H{H}-Lq{Lq}-Lk{Lk}-dh{dh}-{fam}-{mask}' + ('-premul' if premul else '')


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def key_bias(B, Lk, mask):
    """[B, Lk] fp32 0 / -inf, or None"""
    if mask == 'none':
        return None
    assert B == 2 and Lk >= 3
    kb = torch.zeros((B, Lk), dtype=torch.float32)
    if mask == 'edges':
        kb[0, 0] = kb[1, Lk - 1] = -math.inf
    else:
        kb[0] = -math.inf
        kb[0, Lk // 2] = 0.0
        kb[1, 0] = kb[1, Lk - 1] = -math.inf
    return kb


@functools.lru_cache(maxsize=None)
def make_case(B, H, Lq, Lk, dh, family, mask, premul, dtype):
    """-> dict: q / do [B Lq + 32, d], k / v [B Lk + 32, d] (dtype, canary rows included), kbias, dims.  Shared: never modified."""
    d, Mq, Mk = H * dh, B * Lq, B * Lk
    seed = 1000 * Lk + Lq + dh
    q, do = _rnd((Mq + CANARY_ROWS, d), seed, 1.2), _rnd((Mq + CANARY_ROWS, d), seed + 1)
    k, v = _rnd((Mk + CANARY_ROWS, d), seed + 2, 1.2), _rnd((Mk + CANARY_ROWS, d), seed + 3, 1.2)
    if family != 'normal':
        q4, k4 = q[:Mq].view(B, Lq, H, dh), k[:Mk].view(B, Lk, H, dh)
        q4[..., 1:] *= 0.25
        k4[..., 0] = 0
        for b in range(B):
            s = 1.0 if b % 2 == 0 else -1.0
            q4[b, :, :, 0] = s * A
            if family == 'first':
                k4[b, 0, :, 0] = s * KD[dh]
            elif family == 'last':
                k4[b, Lk - 1, :, 0] = s * KD[dh]
            else:
                k4[b, :, :, 0] = -s * KD[dh]
    scale = 1.0 / math.sqrt(dh)
    pm = scale * LOG2E if premul else 0.0
    if premul:
        q = q * pm                            # (rounded once, below: the factor is applied in the projection's fp32 epilogue)
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    kb = key_bias(B, Lk, mask)
    if kb is not None:                        # the rows of masked keys are not to be used
        dead = (kb == -math.inf).reshape(-1)
        k[:Mk][dead] = math.nan
        v[:Mk][dead] = math.nan
    k[Mk:] = torch.where(q[Mq - 1].double() < 0, -CANARY_MAG, CANARY_MAG).to(dtype).expand(CANARY_ROWS, d)
    v[Mk:] = math.nan
    q[Mq:] = math.nan
    do[Mq:] = math.nan
    return dict(dims=(B, H, Lq, Lk, dh), family=family, mask=mask, premul=pm, dtype=dtype, q=q, k=k, v=v, do=do, kbias=kb)


def real(c):
    """the rows the kernels are handed: (q [B Lq, d], k, v [B Lk, d], do [B Lq, d])"""
    B, H, Lq, Lk, dh = c['dims']
    return c['q'][:B * Lq], c['k'][:B * Lk], c['v'][:B * Lk], c['do'][:B * Lq]


def _math(c, rounded):
    """fp64 attention of every query against the few keys and its gradients -> (o [B Lq, d], lse2 [B, H, Lq], dq, dk, dv).
    rounded: the kernels' rounding sites: the forward's unnormalised P = exp2(t - max) and the backward's P and dS are rounded to the
    operand type before their products, delta = dO . o takes the STORED o, and o / dq / dk / dv are stored in the operand type."""
    B, H, Lq, Lk, dh = c['dims']
    dt = c['dtype']
    r = (lambda t: t.to(dt).double()) if rounded else (lambda t: t)
    q, k, v, do = real(c)
    scale = 1.0 / math.sqrt(dh)
    q4 = q.double().view(B, Lq, H, dh).transpose(1, 2)                                  # [B, H, Lq, dh]
    if c['premul']:
        q4 = q4 / c['premul']
    do4 = do.double().view(B, Lq, H, dh).transpose(1, 2)
    k4, v4 = (torch.nan_to_num(t.double(), nan=0.0).view(B, Lk, H, dh).transpose(1, 2) for t in (k, v))   # masked keys: P = 0, rows unused
    t = torch.einsum('bhqc,bhjc->bhqj', q4, k4) * (scale * LOG2E)
    if c['kbias'] is not None:
        t = t + c['kbias'].double()[:, None, None, :]
    m = t.amax(-1, keepdim=True)
    e = torch.exp2(t - m)
    l = e.sum(-1, keepdim=True)
    lse2 = (m + torch.log2(l)).squeeze(-1)
    o = r(torch.einsum('bhqj,bhjc->bhqc', r(e), v4) / l)
    P = torch.exp2(t - lse2[..., None])
    delta = (do4 * o).sum(-1, keepdim=True)
    dS = r(P * (torch.einsum('bhqc,bhjc->bhqj', do4, v4) - delta))
    dq = r(scale * torch.einsum('bhqj,bhjc->bhqc', dS, k4))
    dk = r(scale * torch.einsum('bhqj,bhqc->bhjc', dS, q4))
    dv = r(torch.einsum('bhqj,bhqc->bhjc', r(P), do4))
    fq = lambda x: x.transpose(1, 2).reshape(B * Lq, H * dh)                            # noqa: E731
    fk = lambda x: x.transpose(1, 2).reshape(B * Lk, H * dh)                            # noqa: E731
    return fq(o), lse2, fq(dq), fk(dk), fk(dv)


@functools.lru_cache(maxsize=None)
def reference(*p):
    """fp64 -> (o, lse2, dq, dk, dv) (shared, never modified)"""
    return _math(make_case(*p), False)


def emulation(*p):
    return _math(make_case(*p), True)


def _slice_max(t, B, rows, H, dh, rb):
    """[B rows, H dh] -> max |t| per (batch, row block, head) [B, ceil(rows / rb), H]"""
    nb = -(-rows // rb)
    x = t.abs().view(B, rows, H, dh).amax(-1)
    x = torch.nn.functional.pad(x, (0, 0, 0, nb * rb - rows))
    return x.view(B, nb, rb, H).amax(2)


def figures(c, got, ref, slice_bar):
    """every figure of one point as {label: (value, bar)}; a figure holds when value <= bar.  got / ref: (o, lse2, dq, dk, dv)."""
    B, H, Lq, Lk, dh = c['dims']
    tol = TOL[c['dtype']]
    o, lse2, dq, dk, dv = (t.detach().double().cpu() for t in got)
    o_r, lse_r, dq_r, dk_r, dv_r = ref
    fig = {}
    finite = all(bool(torch.isfinite(t).all()) for t in (o, lse2, dq, dk, dv))
    fig['not finite'] = (0.0 if finite else math.inf, 0.0)
    dvn = float(dv_r.norm())
    dv_head = _slice_max(dv_r, B, Lk, H, dh, Lk)                                        # [B, 1, H]
    for tag, g, r, rows, rb in (('o', o, o_r, Lq, Lq), ('dq', dq, dq_r, Lq, Lq), ('dk', dk, dk_r, Lk, KEY_BLOCK), ('dv', dv, dv_r, Lk, KEY_BLOCK)):
        zero = float(r.abs().max()) < TINY
        if zero:
            r = torch.zeros_like(r)
        res = S.compare(tag, g.reshape(B, rows, H * dh), r.reshape(B, rows, H * dh), 'act', heads=H, ref_norm=dvn if zero else None, row_block=rb)
        fig[f'slice/{res.where}'] = (res.err if res.finite else math.inf, slice_bar)
        num = _slice_max(torch.nan_to_num(g - r, nan=math.inf), B, rows, H, dh, rb)
        den = _slice_max(r, B, rows, H, dh, rb)
        den = torch.where(den < TINY, dv_head.expand_as(den), den).clamp_min(1e-300)
        e = num / den
        i = int(e.argmax())
        b_, rem = divmod(i, e.shape[1] * H)
        fig[f'elem/{tag} [b={b_}, block={rem // H}, head={rem % H}]'] = (float(e.view(-1)[i]), tol if tag == 'o' else 2 * tol)
    err = torch.nan_to_num((lse2 - lse_r).abs(), nan=math.inf)
    fig['lse2'] = (float(err.max()), LSE_BAR * max(1.0, float(lse_r.abs().max())))
    if c['kbias'] is not None:
        dead = (c['kbias'] == -math.inf).reshape(-1)
        for tag, t in (('dk', dk), ('dv', dv)):
            fig[f'masked rows/{tag} = 0'] = (float(torch.nan_to_num(t[dead], nan=math.inf).abs().max()), 0.0)
    return fig


def failing(fig):
    return [label for label, (val, bar) in fig.items() if not val <= bar]


def worst_slice(fig):
    return max(v for label, (v, _) in fig.items() if label.startswith('slice/'))
