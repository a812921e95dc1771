"""Attention at head widths 40-64 (csrc/attention.hip's generic template at two d-tiles) at peaked scores and irregular key masks: the case table, the fault
runners and the attention-weights reference (plain torch on the CPU, importable without the device library).  The machinery -- the
planted inputs, the mask layouts, the figures -- is tests/attn_range_cases.py's, given this table instead of its own.
tests/test_attn_wide_range_cases.py holds this file to fp64 on the CPU, tests/test_gpu_attn_wide_range.py runs the cases on the device.

The wide forward works in 64-key tiles of two 32-key blocks, 128 queries per workgroup, and keeps ONE running maximum per row that it
updates after every 32-key block (m, m_use, alpha), rescaling both d-tile accumulators (O0: channels 0:32, O1: 32:64).  The layouts
of attn_range_cases at 128 keys are two whole tiles here; 'sub_dead' and 'pair' work at 32 keys.  The planted 'late' rows lift the
maximum by T_OVER (144 log2 units in bf16 / 32 in fp32 / 48 in fp16) in the last live 128 keys, the 'step' rows by about 4 units per
128 keys: LAZY_THR means nothing to these kernels today, a tuned one will have such a threshold.
"""
from __future__ import annotations

import math

import torch

from tests import attn_dropout_ref as R
from tests import attn_range_cases as A

BF16, FP16, FP32 = A.BF16, A.FP16, A.FP32
NINF, LOG2E = A.NINF, A.LOG2E
WIDE = ('wide', 'wide')


def _pts(*layouts):
    return tuple(('peaked', m) for m in ('none', 'finite') + layouts)


# name: dims (B, H, Lq, Lk, dh), pre-multiplied q, plan, points, fp32 twin as well -- the fields of attn_range_cases.CASES.  Each is the
# smallest shape that reaches what its comment says; no slice (128 query or key rows of a head) has fewer than 32 rows.  Every case
# runs 'none' and 'finite'; each other layout runs at two head widths or more and with both forms of q.
CASES = {
    # two query tiles, the second partial (72 rows); 8 key tiles, the last ragged (2 of 64); all four head layouts twice
    'wide64': dict(dims=(2, 4, 200, 450, 64), premul=True, plan=WIDE, points=_pts('sub_dead', 'pair', 'per_batch', 'first_dead'),
                   fp32=False),
    # scale * log2 e applied in the kernel: the only form the fp32 model uses
    'wide64_raw': dict(dims=(2, 4, 200, 450, 64), premul=False, plan=WIDE, points=_pts('zero', 'mid_dead', 'one_live', 'sub_dead'),
                       fp32=True),
    # one partial query tile; zero-padded second d-tile (16 columns); ragged last key tile (44 of 64)
    'wide48': dict(dims=(2, 2, 70, 300, 48), premul=False, plan=WIDE, points=_pts('first_dead', 'edge', 'pair', 'per_batch'), fp32=True),
    # the width no other test runs: 24 live columns in the second d-tile
    'wide56': dict(dims=(1, 4, 160, 450, 56), premul=True, plan=WIDE, points=_pts('zero', 'edge', 'one_live', 'pair'), fp32=True),
    # 8 live columns in the second d-tile
    'wide40': dict(dims=(1, 4, 160, 450, 40), premul=True, plan=WIDE, points=_pts('sub_dead', 'mid_dead'), fp32=True),
    # 18 key tiles (35 blocks): a long rescale chain, few queries
    'wide64_long': dict(dims=(1, 4, 100, 1100, 64), premul=True, plan=WIDE, points=_pts('edge', 'mid_dead'), fp32=False),
}
LAYOUTS = ('none', 'finite', 'zero', 'first_dead', 'mid_dead', 'one_live', 'edge', 'per_batch', 'sub_dead', 'pair')


def make_case(name, variant, layout, dtype):
    return A.make_case(name, variant, layout, dtype, CASES)


def points(dtype):
    """[(case, variant, layout)] of one dtype"""
    return A.points(dtype, CASES)


def bar_kind(layout):
    """the row of the slice-bar table a point belongs to: with two live keys dS is a difference of near-equal terms, and 'pair' has a
    bar of its own so that it loosens no other point's"""
    return 'pair' if layout == 'pair' else 'other'


# ----------------------------------------------------------------------------------------------------------------------
# fault runners: the fp64 reference with one deliberate defect of the kind a rewrite of the wide kernels can introduce
# -> (o, lse2, dq, dk, dv).  (The wide cases cover every (batch, head): c['sel'] is None.)
# ----------------------------------------------------------------------------------------------------------------------
def _scores2(c):
    """fp64 scores in log2 units [B, H, Lq, Lk], bias included"""
    B, H, Lq, Lk, dh = c['dims']
    s = R._heads(c['qref'], B, Lq, H, dh) @ R._heads(c['k'].double(), B, Lk, H, dh).transpose(-1, -2) * (LOG2E / math.sqrt(dh))
    if c['kb'] is not None:
        s = s + c['kb'].double()[:, None, None, :] * LOG2E
    return s


def fault_unguarded_anchor(c):
    """(a) no guard for "nothing live yet": a row whose leading 32-key block is all dead takes -inf as its maximum, exp2(-inf - (-inf))
    is NaN and stays; o and lse2 of such videos come out NaN"""
    B, H, Lq, Lk, dh = c['dims']
    o, lse2, dq, dk, dv = A.reference_of(c)
    bad = (c['kb'][:, :32] == NINF).all(-1)                       # [B]
    assert bool(bad.any())
    o3 = o.reshape(B, Lq, H * dh).clone()
    o3[bad] = math.nan
    lse2 = lse2.clone()
    lse2[bad] = math.nan
    return o3.reshape(B * Lq, H * dh), lse2, dq, dk, dv


def fault_second_dtile_not_rescaled(c):
    """(b) O1 (channels 32:) misses the `*= alpha`: the contribution of 32-key block t keeps the weight 2^(m_final - m_t) too large,
    m_t the running maximum after block t.  Blocks before any live key carry nothing."""
    B, H, Lq, Lk, dh = c['dims']
    o, lse2, dq, dk, dv = A.reference_of(c)
    s = _scores2(c)
    nb = A.cdiv(Lk, 32)
    sp = torch.nn.functional.pad(s, (0, nb * 32 - Lk), value=NINF)
    m_t = sp.view(B, H, Lq, nb, 32).amax(-1).cummax(-1).values       # [B, H, Lq, nb]
    w = torch.exp2(m_t[..., -1:] - m_t)
    w = torch.where(torch.isfinite(m_t), w, torch.zeros(()))
    w = w.repeat_interleave(32, -1)[..., :Lk]                        # per key
    P = torch.softmax(s * math.log(2.0), -1)
    v4 = R._heads(c['v'].double(), B, Lk, H, dh)
    o4 = R._heads(o, B, Lq, H, dh).clone()                           # [B, H, Lq, dh]
    o4[..., 32:] = (P * w) @ v4[..., 32:]
    return R._flat(o4, B, Lq, H, dh), lse2, dq, dk, dv


def fault_bias_from_the_wrong_half(c):
    """(c) the second 32 keys of every 64-key tile read the first half's bias (sbias + sub * 32 without the sub)"""
    Lk = c['dims'][3]
    kb = c['kb'].clone()
    for lo in range(32, Lk, 64):
        hi = min(lo + 32, Lk)
        kb[:, lo:hi] = c['kb'][:, lo - 32:hi - 32]
    return A.reference_of(c, kb)


def fault_ragged_tail_live(c):
    """(d) the keys past Lk of the last 64-key tile enter with score 0 and value 0 (the staged zero rows without their -inf)"""
    B, H, Lq, Lk, dh = c['dims']
    Lx = A.cdiv(Lk, 64) * 64
    assert Lx > Lk
    ext = lambda t: torch.nn.functional.pad(t.double().view(B, Lk, H * dh), (0, 0, 0, Lx - Lk)).reshape(B * Lx, H * dh)
    kb = None if c['kb'] is None else torch.nn.functional.pad(c['kb'], (0, Lx - Lk))
    o, lse2, dq, dk, dv = R.reference(c['qref'], ext(c['k']), ext(c['v']), c['do'], kb, None, 0.0, (B, H, Lq, Lx, dh))
    cut = lambda t: t.view(B, Lx, H * dh)[:, :Lk].reshape(B * Lk, H * dh)
    return o, lse2, dq, cut(dk), cut(dv)


# ----------------------------------------------------------------------------------------------------------------------
# attention weights (csrc/attn_weights.hip): att[b, n, l] = 1/H sum_h exp2(q.k c + kbias log2 e - lse2)
# ----------------------------------------------------------------------------------------------------------------------
# absolute bars on rows that are not planted: tests/gpu_checks.py check_attn_weights (fp16 takes bf16's: its operand roundings are 8
# times finer and the rest of the formula is fp32)
ATT_BAR = {FP32: 1e-5, BF16: 5e-3, FP16: 5e-3}
ATT_LAYOUTS = ('none', 'finite', 'sub_dead', 'pair')
ATT_CASES = {False: ('wide64_raw', 'wide48', 'wide56', 'wide40'), True: ('wide64_raw', 'wide48', 'wide56', 'wide40', 'wide64')}


def att_points(dtype):
    """[(case, layout)]: the first four cases in every dtype, wide64 in the 16-bit ones.  The layouts are ATT_LAYOUTS whether or not the
    case's parity points hold them."""
    return [(n, m) for n in ATT_CASES[dtype != FP32] for m in ATT_LAYOUTS]


def att_reference(c):
    """fp64 head-mean softmax of the rounded inputs (pre-multiplied q: the q the kernel effectively sees) -> [B, Lq, Lk]"""
    return torch.softmax(_scores2(c) * math.log(2.0), -1).mean(1)


def _fma32(s, a, b):
    """fp32 fmaf(a, b, s): the product of two fp32 values is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return (s.double() + a.double() * b.double()).float()


def att_emulation(c):
    """the kernel's chain in fp32 on the CPU: q c rounded to fp32, s = kb log2 e - lse2, fmaf over the channels in order, exp2, the sum
    over the heads in order, times 1/H.  lse2 is the forward's in fp32 as well: the scores as the MFMA steps accumulate them, times the
    scale, plus the bias, then m + log2 sum exp2(s - m).  On a planted row the weights kernel adds channel 0, the planted one, first and
    works near 0 from there on; the forward's accumulator holds T_OVER from its first step, and its roundings at that magnitude are
    what lse2 carries into att.  -> att [B, Lq, Lk] fp32"""
    B, H, Lq, Lk, dh = c['dims']
    f32 = torch.float32
    cq = torch.tensor(1.0) if c['pm'] else torch.tensor(1.0 / math.sqrt(dh), dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    q4, k4 = R._heads(c['q'].float(), B, Lq, H, dh), R._heads(c['k'].float(), B, Lk, H, dh)
    kbl = torch.zeros(B, Lk, dtype=f32) if c['kb'] is None else c['kb'] * torch.tensor(LOG2E, dtype=f32)
    kbl = kbl[:, None, None, :]
    # the forward's lse2: the MFMA steps of mma_first in their order (first_chunk), each step's products summed exactly and added to
    # the fp32 accumulator with one rounding -- 16-bit: channels [16 i, 16 i + 16) in step i; fp32: channels j and 32 + j in step j
    steps = [list(range(16 * i, min(16 * i + 16, dh))) for i in range(4)] if c['dtype'] != FP32 else \
        [[j] + ([32 + j] if 32 + j < dh else []) for j in range(32)]
    dot = torch.zeros(B, H, Lq, Lk, dtype=f32)
    for ch in steps:
        if ch:
            dot = (dot.double() + q4[..., ch].double() @ k4[..., ch].double().transpose(-1, -2)).float()
    s = dot * cq + kbl
    m = s.amax(-1, keepdim=True)
    lse2 = (m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True)))  # [B, H, Lq, 1]
    # the weights kernel
    qs = q4 * cq
    acc = (kbl - lse2).expand(B, H, Lq, Lk).contiguous()
    for e in range(dh):
        acc = _fma32(acc, k4[..., None, :, e], qs[..., :, None, e])
    p = torch.exp2(acc)
    att = torch.zeros(B, Lq, Lk, dtype=f32)
    for h in range(H):
        att = att + p[:, h]
    return att * torch.tensor(1.0 / H, dtype=f32)


def att_figures(c, att, bar_planted):
    """{label: (value, bar, 'max')} of one attention-weights point.  A row of att is planted when any head's row is."""
    B, H, Lq, Lk, dh = c['dims']
    ref = att_reference(c)
    att = att.detach().double().cpu()
    fig = {'not finite': (0.0 if bool(torch.isfinite(att).all()) else math.inf, 0.0, 'max')}
    prow = c['prow'].any(1)                                           # [B, Lq]
    d = torch.nan_to_num((att - ref).abs(), nan=math.inf).amax(-1)
    rs = torch.nan_to_num((att.sum(-1) - 1.0).abs(), nan=math.inf)
    for st, sel, bar in (('planted', prow, bar_planted), ('other', ~prow, ATT_BAR[c['dtype']])):
        fig[f'att {st}'] = (float(d[sel].max()), bar, 'max')
        fig[f'rowsum {st}'] = (float(rs[sel].max()), bar, 'max')
    if c['kb'] is not None and bool((c['kb'] == NINF).any()):
        gone = (c['kb'] == NINF)[:, None, :].expand(B, Lq, Lk)
        fig['masked_keys/att'] = (float(torch.nan_to_num(att[gone], nan=math.inf).abs().max()), 0.0, 'max')
    return fig
