"""Attention at peaked scores and irregular key masks: the launch plans, the planted inputs, the mask layouts, the figures and the
fault runners (plain torch on the CPU, importable without the device library).  tests/test_attn_range_cases.py holds this file to
fp64 on the CPU, tests/test_gpu_attn_range.py runs the cases on the device.

1. A dispatch twin: `plan()` restates attn_plan (csrc/attention_bf16.hip), the one function svol_attn_fwd_bf16_launch,
   svol_attn_bwd_bf16_launch and the scratch queries take their decisions from, under the names of its Fwd / Bwd enumerators
   ('fast2+redo' = fast2_redo, '2pass_m+ksplit' = two_pass_m with bwd_ksplit > 1), and so names the kernels a launch takes.
   tests/test_abi.py holds ws_floats and sp_shape_ok to the library over a grid of shapes.  CASES holds one smallest shape per plan.
2. Planted inputs (`make_case`).  check_attention's randn inputs with channel 0 of every head reserved: k[:, 0] = 0 except at planted
   keys (beta), q[:, 0] = 0 except at planted rows (a); a planted row's other channels are scaled by 0.25, so its score (log2 domain)
   is a * beta * f at a planted key (f = 1 for pre-multiplied q, else scale * log2 e) and within a few units of 0 everywhere else.
   Keys belong to a (batch, head), so each head carries ONE key layout and the row kinds that go with it:

     head layout   planted keys                                      row kinds (a)
     'late'        beta in the last live tile, beta - 1/(a f) in     'over' (a_hi: T = 144 log2 units in bf16 / fp32, 48 in fp16),
                   the live tile before it                           'near' (a smaller a: 90 / 12)
     'front'       beta in the first live tile                       'front' (a_hi)
     'step'        one key per live tile (the first 8), beta         'step_u' (steps just under LAZY_THR = 4: 3.75 / 3.61),
                   rising by a fixed amount                          'step_o' (a larger a: steps of 4.22 / 4.06)
     'none'        --                                                --

   Heads take the layouts in the cycle late, none, step, front.  Planted rows sit in the first and the last query tile of a planted
   head, at most four per tile, in different waves (32-row groups).  Variant 'calm' turns every 'over' row into a 'near' row.
3. Mask layouts (`key_bias`): first_dead, mid_dead, one_live, edge, per_batch, finite, zero, first_split_dead, cls65; sub_dead and
   pair at the granularity of the head-width 40-64 kernels.
4. `figures`: slice errors, element errors per (batch, head, 128-row tile) separately over planted and other rows / keys, lse2 per
   row set, gradient rows of -inf keys, finiteness.
5. Fault runners: the fp64 reference with one deliberate defect each.

make_case, key_bias, case_plan and points take the case table (CASES unless given); everything behind make_case works on the case
dict.  tests/attn_wide_range_cases.py holds the table, the faults and the attention-weights reference of head widths 40-64.
"""
from __future__ import annotations

import math

import torch

from tests import attn_dropout_ref as R

LOG2E = R.LOG2E
KT, SP_KEYS, LAZY_THR, KSPLIT_WGS = 128, 512, 4.0, 256
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
PSUM_MAX = {BF16: 1e30, FP16: 6.5e4}     # SVOL_H16_PSUM_MAX: the fast forward flags a workgroup whose row sum reaches it
# whole-tensor and per-tile element bars: tests/gpu_checks.py check_attention (TOL for o, 2 TOL for the gradients, its lse2 bars)
TOL = {FP32: 2e-5, BF16: 1.2e-2, FP16: 1.5e-3}
LSE_BAR = {FP32: 1e-5, BF16: 3e-3, FP16: 3e-3}


# ----------------------------------------------------------------------------------------------------------------------
# 1. the dispatch twin
# ----------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def plan_ksplit(B, H, Lq, Lk, dh, ws_floats=None):
    """-> (ksplit, tiles per split); ws_floats None: unbounded scratch"""
    nt, wgs = cdiv(Lk, KT), cdiv(Lq, 128) * H * B
    if wgs >= 192 or nt < 8:
        return 1, nt
    want = min(cdiv(KSPLIT_WGS, wgs), 16)
    tps = max(cdiv(nt, want), 2)
    ks = cdiv(nt, tps)
    need = ks * B * Lq * H * dh + ks * B * H * Lq * 2 + B * Lq * H * dh
    if ks < 2 or (ws_floats is not None and need > ws_floats):
        return 1, nt
    return ks, tps


def sp_shape_ok(B, H, Lq, Lk, dh, deterministic=False):
    return not deterministic and dh == 32 and H == 8 and (B * H) % 8 == 0 and Lq % KT == 0 and Lk % KT == 0 and Lk >= 2 * SP_KEYS


def sp_ws_floats(B, H, Lq, Lk):
    return B * Lq * H * 32 + B * H * 4 * 2 * (Lk % SP_KEYS) * 32


def ws_floats(B, H, Lq, Lk, dh):
    """svol_attn_ws_bytes / 4"""
    if dh > 32:                              # csrc/attention.hip, two d-tiles: no workspace
        return 0
    ks, _ = plan_ksplit(B, H, Lq, Lk, dh)
    if ks < 2:
        cls, redo = B * cdiv(Lk, KT), B * H * cdiv(Lq, 128)
        sp = sp_ws_floats(B, H, Lq, Lk) if sp_shape_ok(B, H, Lq, Lk, dh) else 0
        return max(cls, redo, sp)
    return ks * B * Lq * H * dh + ks * B * H * Lq * 2 + B * Lq * H * dh


def pre_masked_ok(B, H, Lq, Lk, dh):
    return plan_ksplit(B, H, Lq, Lk, dh)[0] == 1


def head_xcd(B, H, dh):
    if (B * H) % 8:
        return 0
    return 2 if (B * H) % 16 == 0 and H % 2 == 0 and dh == 32 else 1


def plan(B, H, Lq, Lk, dh, premul, has_kbias, ws_bytes=None, deterministic=False):
    """the kernels one forward and one backward of this launch take (drop_p = 0, the scratch ops.attn_fwd hands over unless given)
    -> dict(fwd, bwd, ksplit, tps, head_xcd)"""
    if dh > 32:                              # csrc/attention.hip, two d-tiles: one forward, one backward, no key split, no head-to-XCD deal
        return dict(fwd='wide', bwd='wide', ksplit=1, tps=cdiv(Lk, KT), head_xcd=0)
    ws_bytes = 4 * ws_floats(B, H, Lq, Lk, dh) if ws_bytes is None else ws_bytes
    ws = ws_bytes > 0
    masked = has_kbias or Lk % KT != 0
    ntk = cdiv(Lk, KT)
    pre = premul and (not masked or (pre_masked_ok(B, H, Lq, Lk, dh) and ws and ws_bytes >= B * ntk * 4))
    hx = head_xcd(B, H, dh) if pre else 0
    m = 'm' if masked else 'u'
    # forward
    ks, tps = plan_ksplit(B, H, Lq, Lk, dh, ws_bytes // 4) if (ws and not pre) else (1, ntk)
    if pre and masked:
        fwd = 'pre_masked'
    elif pre:
        nwg = cdiv(Lq, 128) * H * B
        fwd = 'fast2+redo' if hx and dh == 32 and ws and ws_bytes >= nwg * 4 else 'pre_all'
    else:
        fwd = ('ksplit_' if ks > 1 else 'general_') + m
    # backward
    ksb, tpsb = plan_ksplit(B, H, Lq, Lk, dh, ws_bytes // 4) if (ws and not pre and not deterministic) else (1, ntk)
    if pre and masked:
        bwd = 'bwd_pre_masked'
    elif pre:
        if hx and sp_shape_ok(B, H, Lq, Lk, dh, deterministic) and ws and ws_bytes >= 4 * sp_ws_floats(B, H, Lq, Lk):
            bwd = 'bwd_sp'
        else:
            dma = dh == 32 and Lq % KT == 0
            bwd = 'bwd_rot_dma' if dma else ('bwd_rot' if dh == 32 else 'bwd_pre')
    elif not deterministic and ksb > 1 and Lq <= KT and dh == 32:
        bwd = 'fq_' + ('m' if has_kbias else 'u')
    else:
        bwd = '2pass_' + m + ('+ksplit' if ksb > 1 else '')
    return dict(fwd=fwd, bwd=bwd, ksplit=ks, tps=tps, head_xcd=hx)


# name: dims (B, H, Lq, Lk, dh), pre-multiplied q, the (fwd, bwd) plan the twin must give, input points (variant, mask layout),
# fp32 twin as well.  'none': no bias pointer.
CASES = {
    # five key tiles: the three-buffer ring of the fast forward wraps; 80 workgroups
    'fast2+redo': dict(dims=(2, 8, 640, 640, 32), premul=True, plan=('fast2+redo', 'bwd_rot_dma'),
                       points=(('peaked', 'none'), ('calm', 'none')), fp32=True),
    'pre_all': dict(dims=(1, 4, 384, 384, 32), premul=True, plan=('pre_all', 'bwd_rot_dma'), points=(('peaked', 'none'),), fp32=False),
    'bwd_pre': dict(dims=(2, 8, 200, 384, 16), premul=True, plan=('pre_all', 'bwd_pre'), points=(('peaked', 'none'),), fp32=False),
    # two full 512-key groups and a 128-key tail group in query quarters (9 query tiles)
    'bwd_sp': dict(dims=(1, 8, 1152, 1152, 32), premul=True, plan=('fast2+redo', 'bwd_sp'), points=(('peaked', 'none'),), fp32=False),
    'pre_masked': dict(dims=(2, 8, 256, 700, 32), premul=True, plan=('pre_masked', 'bwd_pre_masked'),
                       points=tuple(('peaked', m) for m in ('first_dead', 'mid_dead', 'one_live', 'edge', 'per_batch', 'finite')),
                       fp32=False),
    # 66 key tiles (the issue's 8320 keys are 65 tiles, 0 .. 64: only ONE tile behind the refresh of the class masks; 8400 keys give
    # tile 65 as well, ragged).  192 workgroups: no key split.
    'pre_masked_65': dict(dims=(3, 8, 1024, 8400, 32), premul=True, plan=('pre_masked', 'bwd_pre_masked'),
                          points=(('peaked', 'cls65'),), fp32=False, heads=((0, 0), (1, 2), (2, 7))),
    'general': dict(dims=(2, 4, 70, 300, 16), premul=False, plan=('general_m', '2pass_m'),
                    points=tuple(('peaked', m) for m in ('none', 'first_dead', 'one_live', 'finite')), fp32=True),
    'general_u': dict(dims=(2, 4, 70, 384, 16), premul=False, plan=('general_u', '2pass_u'), points=(('peaked', 'none'),), fp32=True),
    # nt = 9, five splits of two tiles
    'ksplit_fq': dict(dims=(2, 8, 100, 1100, 32), premul=True, plan=('ksplit_m', 'fq_m'),
                      points=tuple(('peaked', m) for m in ('none', 'first_split_dead', 'mid_dead', 'finite')), fp32=True,
                      plan_none=('ksplit_m', 'fq_u')),
    'ksplit_2pass': dict(dims=(1, 8, 200, 1100, 32), premul=True, plan=('ksplit_m', '2pass_m+ksplit'),
                         points=tuple(('peaked', m) for m in ('first_split_dead', 'zero', 'edge')), fp32=True),
}
# every plan name the cases must reach ('plan_none': what the case takes without a bias pointer, where that differs)
PLANS_FWD = ('fast2+redo', 'pre_all', 'pre_masked', 'general_m', 'general_u', 'ksplit_m')
PLANS_BWD = ('bwd_rot_dma', 'bwd_pre', 'bwd_sp', 'bwd_pre_masked', '2pass_m', '2pass_u', 'fq_m', 'fq_u', '2pass_m+ksplit')
DT_NAME = R.DT_NAME


def case_plan(name, layout, cases=None):
    c = (CASES if cases is None else cases)[name]
    return plan(*c['dims'], c['premul'], layout != 'none')


def points(dtype, cases=None):
    """[(case, variant, layout)] of one dtype.  cases: a table like CASES (tests/attn_wide_range_cases.py holds the wide one)"""
    return [(n, v, m) for n, c in (CASES if cases is None else cases).items() if dtype != FP32 or c['fp32'] for v, m in c['points']]


# ----------------------------------------------------------------------------------------------------------------------
# 3. mask layouts
# ----------------------------------------------------------------------------------------------------------------------
NINF = float('-inf')
# two large finite biases on neighbouring keys of video 0: 87 and 87.78125 log2 units.  Dropping the low half of the 16-bit hi + lo
# pair moves the second by 0.22 (bf16) / 0.03 (fp16) units against the first: the two keys' shares of every row change
KB_BIG = (87.0 / LOG2E, 87.78125 / LOG2E)


def key_bias(name, layout, cases=None):
    """[B, Lk] fp32 additive key bias, or None.  Every video keeps at least one live key."""
    B, H, Lq, Lk, dh = (CASES if cases is None else cases)[name]['dims']
    if layout == 'none':
        return None
    kb = torch.zeros(B, Lk)
    if layout == 'zero':                     # all zero behind a non-null pointer
        return kb
    if layout == 'first_dead':
        kb[:, :128] = NINF
    elif layout == 'mid_dead':
        kb[:, 256:384] = NINF
    elif layout == 'one_live':               # one tile at -inf but for a single key
        t = 1 if Lk <= 384 else 2
        kb[:, t * 128:(t + 1) * 128] = NINF
        kb[:, t * 128 + 44] = 0
    elif layout == 'edge':                   # the live prefix ends exactly on a tile boundary, ragged Lk behind it
        kb[:, (Lk // 128 - 1) * 128:] = NINF
    elif layout == 'per_batch':              # video 0: zero bias; the others first_dead / mid_dead in turn
        for b in range(1, B):
            if b % 2:
                kb[b, :128] = NINF
            else:
                kb[b, 256:384] = NINF
    elif layout == 'finite':
        kb[:, 5::37] = -2.5
        kb[:, 11::53] = 1.75
        kb[:, 130:140] = NINF
        kb[:, Lk - 30:] = NINF
        kb[0, 200], kb[0, 201] = KB_BIG
    elif layout == 'first_split_dead':       # the whole first key split
        kb[:, :plan_ksplit(B, H, Lq, Lk, dh)[1] * KT] = NINF
    elif layout == 'cls65':                  # tile t and tile t + 64 in different classes; tile 65 is ragged (mixed) in every video
        T = lambda t: slice(t * 128, (t + 1) * 128)
        kb[0, T(1)] = NINF                   # video 0: 0 plain / 64 dead, 1 dead / 65 mixed, 2 mixed / 66 none
        kb[0, T(64)] = NINF
        kb[0, 2 * 128 + 7] = -2.5
        kb[1, T(0)] = NINF                   # video 1: 0 dead / 64 plain, 1 plain / 65 mixed, a dead tile between live ones
        kb[1, T(30)] = NINF
        kb[2, T(63)] = NINF                  # video 2: 63 dead, 64 with a single live key / 0 plain
        kb[2, T(64)] = NINF
        kb[2, 64 * 128 + 3] = 0
    elif layout == 'sub_dead':               # at the wide kernels' granularity (64-key tiles, 32-key blocks): a dead LEADING block
        kb[:, 0:32] = NINF                   # with the rest of its tile live, a dead block inside a live tile (96:128; 64:96 in
        kb[:, 96:128] = NINF                 # every video but the first), one whole dead tile (192:256)
        kb[:, 192:256] = NINF
        kb[1:, 64:96] = NINF
    elif layout == 'pair':                   # two live keys per video
        kb[:] = NINF
        kb[:, 70] = 0
        kb[:, Lk - 5] = 0
    else:
        raise ValueError(layout)
    return kb


def tile_classes(kb, Lk):
    """attn_tile_flags_bf16: [B, nt] of 0 (all zero), 2 (all -inf or past Lk), 1 (anything else)"""
    B, nt = kb.shape[0], cdiv(Lk, KT)
    pad = torch.full((B, nt * KT), NINF)
    pad[:, :Lk] = kb
    t = pad.view(B, nt, KT)
    dead, plain = (t == NINF).all(-1), (t == 0).all(-1)
    return torch.where(plain, 0, torch.where(dead, 2, 1))


# ----------------------------------------------------------------------------------------------------------------------
# 2. planted inputs
# ----------------------------------------------------------------------------------------------------------------------
HEAD_LAYOUTS = ('late', 'none', 'step', 'front')
ROW_OFFSETS = (5, 49, 95, 96)          # one row in each wave (32-row group) of a 128-query tile
T_OVER = {BF16: 144.0, FP16: 48.0, FP32: 32.0}
STEP_TILES = 3          # keys of a step head: the rise (two steps) stays 3 units under the fp16 flag threshold of the fast forward
DO_SCALE = 0.0625       # a planted row's dO: its gradient stays of the size of the benign rows' (a and beta multiply it)
QK_SCALE = 1.5          # check_attention's q and k


def _quant(x, bits=8):
    """x cut to ``bits`` significant bits (representable in bf16 and fp16)"""
    e = math.floor(math.log2(abs(x)))
    q = 2.0 ** (e - bits + 1)
    return math.floor(x / q) * q


def planted_spec(dtype, premul, dh):
    """a and beta of each kind.  f: log2 units per unit of a * beta"""
    f = 1.0 if premul else LOG2E / math.sqrt(dh)
    a_hi = 16.0 if premul else 32.0
    a_near = a_hi / 4 if dtype == FP16 else a_hi * 10 / 16
    beta = _quant(T_OVER[dtype] / (a_hi * f))
    kstep = 15 if premul else 20                      # beta rises by kstep / 16 from tile to tile, from 2
    a_step = a_hi / 4
    return dict(f=f, a=dict(over=a_hi, near=a_near, front=a_hi, step_u=a_step, step_o=a_step * 18 / 16), beta=beta,
                beta2=_quant(beta - 1.0 / (a_hi * f)), step=[(32 + kstep * i) / 16 for i in range(STEP_TILES)])


def head_layout(b, h, H):
    return HEAD_LAYOUTS[(b * H + h) % len(HEAD_LAYOUTS)]


def _planted_rows(layout, nth, tile, ntiles, rows, variant):
    """[(offset, kind)] of one query tile of a planted head; nth: index of the head among those of its layout"""
    if tile not in (0, ntiles - 1):
        return []
    first = tile == 0
    if layout == 'late':
        kinds = ('over', 'near') if first else (('over',) if nth % 2 == 0 else ('near',))
        if variant == 'calm':
            kinds = tuple('near' for _ in kinds)
    elif layout == 'front':
        kinds = ('front',)
    elif layout == 'step':
        kinds = ('step_u', 'step_o') if first else ('step_u',)
    else:
        return []
    return [(o, k) for o, k in zip(ROW_OFFSETS, kinds) if o < rows]


def _key_in_tile(live_b, t, Lk, off=37):
    """a live key of tile t of one video: at offset ``off`` if that key is live, else the tile's first live one"""
    lo, hi = t * KT, min((t + 1) * KT, Lk)
    if lo + off < hi and bool(live_b[lo + off]):
        return lo + off
    return lo + int(torch.nonzero(live_b[lo:hi])[0])


_MADE = {}


def make_case(name, variant, layout, dtype, cases=None):
    """one point of the table ``cases`` (CASES unless given), made once per table and shared"""
    cases = CASES if cases is None else cases
    key = (id(cases), name, variant, layout, dtype)
    if key not in _MADE:
        _MADE[key] = _make_case(cases, name, variant, layout, dtype)
    return _MADE[key]


def _make_case(cases, name, variant, layout, dtype):
    """-> dict: q (what the kernel is given), qref (fp64, the unscaled q it effectively sees), k, v, do (2-D [B L, H dh]), kb, pm,
    dims, prow [B, H, Lq] / pkey [B, H, Lk] (planted rows / keys), kinds {(b, h, row): kind}, sel (the (batch, head) pairs the
    reference covers, or None for all).  Shared between tests: never modified."""
    cs = cases[name]
    B, H, Lq, Lk, dh = dims = cs['dims']
    d = H * dh
    pm = LOG2E / math.sqrt(dh) if cs['premul'] else 0.0
    q, k, v, do = R._rnd((B * Lq, d), dtype, 30, QK_SCALE), R._rnd((B * Lk, d), dtype, 31, QK_SCALE), R._rnd((B * Lk, d), dtype, 32), \
        R._rnd((B * Lq, d), dtype, 33)
    if pm:
        q = (q.double() * pm).to(dtype)
    kb = key_bias(name, layout, cases)
    live = torch.ones(B, Lk, dtype=torch.bool) if kb is None else kb > NINF
    if layout == 'finite':                   # the two keys that KB_BIG lifts above all others carry opposite values
        v.view(B, Lk, H, dh)[0, 201] = -v.view(B, Lk, H, dh)[0, 200]
    sp = planted_spec(dtype, cs['premul'], dh)
    q4, k4, v4, do4 = q.view(B, Lq, H, dh), k.view(B, Lk, H, dh), v.view(B, Lk, H, dh), do.view(B, Lq, H, dh)
    q4[..., 0] = 0
    k4[..., 0] = 0
    prow, pkey = torch.zeros(B, H, Lq, dtype=torch.bool), torch.zeros(B, H, Lk, dtype=torch.bool)
    kinds, nth = {}, {}
    nqt = cdiv(Lq, 128)
    for b in range(B):
        live_tiles = [t for t in range(cdiv(Lk, KT)) if bool(live[b, t * KT:(t + 1) * KT].any())]
        for h in range(H):
            lay = head_layout(b, h, H)
            n = nth.get(lay, 0)
            nth[lay] = n + 1
            if lay == 'none':
                continue
            if lay == 'late':
                keys = [(_key_in_tile(live[b], live_tiles[-1], Lk), sp['beta'])]
                if len(live_tiles) > 1:
                    keys.append((_key_in_tile(live[b], live_tiles[-2], Lk, 90), sp['beta2']))
            elif lay == 'front':
                keys = [(_key_in_tile(live[b], live_tiles[0], Lk, 21), sp['beta'])]
            else:
                keys = [(_key_in_tile(live[b], t, Lk, 70), bt) for t, bt in zip(live_tiles, sp['step'])]
            for j, bt in keys:
                k4[b, j, h, 0] = bt
                pkey[b, h, j] = True
            # the two highest planted keys carry opposite values and a planted row's dO points along the top one's: the row's two
            # dP differ by twice a sum of 32 positive terms, so its dS is large against the rounding of delta whatever the draw
            top = sorted(keys, key=lambda jb: -jb[1])
            if len(top) > 1:
                v4[b, top[1][0], h, :] = -v4[b, top[0][0], h, :]
            vsign = torch.where(v4[b, top[0][0], h, :] < 0, -1.0, 1.0).double()
            for t in range(nqt):
                for off, kind in _planted_rows(lay, n, t, nqt, min(128, Lq - t * 128), variant):
                    r = t * 128 + off
                    q4[b, r, h, 1:] = (q4[b, r, h, 1:].double() * 0.25).to(dtype)
                    q4[b, r, h, 0] = sp['a'][kind]
                    do4[b, r, h, :] = (do4[b, r, h, :].double().abs() * vsign * DO_SCALE).to(dtype)
                    prow[b, h, r] = True
                    kinds[(b, h, r)] = kind
    qref = q.double() / pm if pm else q.double()
    return dict(name=name, variant=variant, layout=layout, dtype=dtype, dims=dims, pm=pm, q=q, qref=qref, k=k, v=v, do=do, kb=kb,
                prow=prow, pkey=pkey, kinds=kinds, sel=cs.get('heads'), spec=sp)


def over_workgroups(c):
    """the (batch, head, 128-query tile) triples that hold an 'over' row"""
    return sorted({(b, h, r // 128) for (b, h, r), kind in c['kinds'].items() if kind == 'over'})


def row_stats(c):
    """fp64, log2 domain, per row [B, H, Lq]: m0 (largest score of key tile 0), later (largest score behind tile 0) - m0, and
    L = log2 of the row sum the fast forward accumulates (sum of 2^(s - m0))"""
    B, H, Lq, Lk, dh = c['dims']
    s = R._heads(c['qref'], B, Lq, H, dh) @ R._heads(c['k'].double(), B, Lk, H, dh).transpose(-1, -2) * (LOG2E / math.sqrt(dh))
    if c['kb'] is not None:
        s = s + c['kb'].double()[:, None, None, :] * LOG2E
    m0 = s[..., :KT].max(-1).values
    later = s[..., KT:].max(-1).values - m0
    L = torch.logsumexp((s - m0[..., None]) * math.log(2.0), -1) / math.log(2.0)
    return m0, later, L


def expected_flags(c):
    """number of workgroups the fast forward must flag: those with a row whose sum reaches SVOL_H16_PSUM_MAX"""
    B, H, Lq, Lk, dh = c['dims']
    _, _, L = row_stats(c)
    hot = L >= math.log2(PSUM_MAX[c['dtype']])
    pad = cdiv(Lq, 128) * 128 - Lq
    hot = torch.nn.functional.pad(hot, (0, pad)).view(B, H, -1, 128).any(-1)
    return int(hot.sum())


# ----------------------------------------------------------------------------------------------------------------------
# references (the whole problem, or the (batch, head) pairs c['sel'] as a problem of one head per "video")
# ----------------------------------------------------------------------------------------------------------------------
def _sub2d(t, c, L):
    """[B L, H dh] -> the selected heads as [n L, dh]"""
    B, H, _, _, dh = c['dims']
    if c['sel'] is None:
        return t
    t4 = t.reshape(B, L, H, dh)
    return torch.cat([t4[b, :, h, :] for b, h in c['sel']], 0)


def _sub_bh(t, c):
    """[B, H, L] -> [n, 1, L]"""
    return t if c['sel'] is None else torch.stack([t[b, h] for b, h in c['sel']])[:, None]


def sub_dims(c):
    B, H, Lq, Lk, dh = c['dims']
    return c['dims'] if c['sel'] is None else (len(c['sel']), 1, Lq, Lk, dh)


def sub_kb(c, kb=None):
    kb = c['kb'] if kb is None else kb
    if kb is None or c['sel'] is None:
        return kb
    return torch.stack([kb[b] for b, _ in c['sel']])


def sub_inputs(c):
    Lq, Lk = c['dims'][2], c['dims'][3]
    return _sub2d(c['qref'], c, Lq), _sub2d(c['k'], c, Lk), _sub2d(c['v'], c, Lk), _sub2d(c['do'], c, Lq)


def sub_outputs(c, got):
    """a full-size (o, lse2, dq, dk, dv) cut to the selected heads"""
    Lq, Lk = c['dims'][2], c['dims'][3]
    o, lse2, dq, dk, dv = (t.detach().double().cpu() for t in got)
    return _sub2d(o, c, Lq), _sub_bh(lse2, c), _sub2d(dq, c, Lq), _sub2d(dk, c, Lk), _sub2d(dv, c, Lk)


def reference_of(c, kb='own'):
    """fp64 reference (attn_dropout_ref.reference without dropout) on the case's (sub-)problem -> o, lse2, dq, dk, dv"""
    q, k, v, do = sub_inputs(c)
    return R.reference(q, k, v, do, sub_kb(c) if isinstance(kb, str) else kb, None, 0.0, sub_dims(c))


def emulation_of(c):
    """attn_dropout_ref.emulate with the dtype's rounder (fp32: the formula in fp32 torch) -> o, lse2 (the reference's: the emulation
    keeps no lse), dq, dk, dv"""
    q, k, v, do = sub_inputs(c)
    if c['dtype'] == FP32:
        o, dq, dk, dv = R.emulate(q.float(), k, v, do, sub_kb(c), None, 0.0, sub_dims(c), None, torch.float32)
    else:
        o, dq, dk, dv = R.emulate(q, k, v, do, sub_kb(c), None, 0.0, sub_dims(c), R.rounder(c['dtype']), torch.float64)
    return o, dq, dk, dv


# ----------------------------------------------------------------------------------------------------------------------
# 4. figures
# ----------------------------------------------------------------------------------------------------------------------
def _tile_elem(got, ref, sets, dims_bhl):
    """got / ref [n, L, H, dh] fp64; sets {tag: [n, H, L] bool} -> {tag: (worst over (b, h, 128-row tile) of max |got - ref| over the
    set's rows of the tile / max |ref| over the whole (b, h), where)}"""
    n, H, L = dims_bhl
    diff = (got - ref).abs().amax(-1).permute(0, 2, 1)                 # [n, H, L]
    scale = ref.abs().amax(-1).permute(0, 2, 1).amax(-1).clamp_min(1e-300)   # [n, H]
    out = {}
    pad = cdiv(L, 128) * 128 - L
    for tag, s in sets.items():
        e = torch.where(s, diff, torch.zeros(())) / scale[..., None]
        e = torch.nn.functional.pad(e, (0, pad)).view(n, H, -1, 128).amax(-1)
        i = int(e.argmax())
        b, rem = divmod(i, e.shape[1] * e.shape[2])
        h, t = divmod(rem, e.shape[2])
        out[tag] = (float(e.view(-1)[i]), f'b={b}, head={h}, tile {t}')
    return out


def figures(c, got, ref, slice_bar, lse=True):
    """every figure of one point as {label: (value, bar, 'max')}.  got / ref: (o, lse2, dq, dk, dv) on the case's (sub-)problem."""
    n, H, Lq, Lk, dh = sub_dims(c)
    dt = c['dtype']
    o, lse2, dq, dk, dv = (t.detach().double().cpu() for t in got)
    o_r, lse_r, dq_r, dk_r, dv_r = ref
    fig = {}
    finite = all(bool(torch.isfinite(t).all()) for t in (o, lse2, dq, dk, dv))
    fig['not finite'] = (0.0 if finite else math.inf, 0.0, 'max')
    sl = R.slice_errors_dims((n, H, Lq, Lk, dh), (o, dq, dk, dv), (o_r, dq_r, dk_r, dv_r))
    for tag, r in sl.items():
        fig[f'slice/{tag} {r.where}'] = (r.err if r.finite else math.inf, slice_bar, 'max')
    prow, pkey = _sub_bh(c['prow'], c), _sub_bh(c['pkey'], c)
    for tag, g, r, L, pl, bar in (('o', o, o_r, Lq, prow, TOL[dt]), ('dq', dq, dq_r, Lq, prow, 2 * TOL[dt]),
                                  ('dk', dk, dk_r, Lk, pkey, 2 * TOL[dt]), ('dv', dv, dv_r, Lk, pkey, 2 * TOL[dt])):
        g4, r4 = g.reshape(n, L, H, dh), r.reshape(n, L, H, dh)
        g4 = torch.nan_to_num(g4, nan=math.inf)
        for st, (val, where) in _tile_elem(g4, r4, {'planted': pl, 'other': ~pl}, (n, H, L)).items():
            fig[f'elem/{tag} {st} [{where}]'] = (val, bar, 'max')
        whole = float((g4 - r4).abs().max() / (r4.abs().max() + 1e-12)) if finite else math.inf
        fig[f'whole/{tag}'] = (whole, bar, 'max')
    if lse:
        d = torch.nan_to_num((lse2 - lse_r).abs(), nan=math.inf)
        for st, s in (('planted', prow), ('other', ~prow)):
            if bool(s.any()):
                # per (batch, head): the set's worst row against the set's largest |lse2|
                num = torch.where(s, d, torch.zeros(())).amax(-1)
                den = torch.where(s, lse_r.abs(), torch.zeros(())).amax(-1) + 1e-12
                fig[f'lse2 {st}'] = (float((num / den).max()), LSE_BAR[dt], 'max')
    kb = sub_kb(c)
    if kb is not None and bool((kb == NINF).any()):
        gone = (kb == NINF).reshape(n * Lk)
        fig['masked_keys/dk'] = (float(torch.nan_to_num(dk[gone], nan=math.inf).abs().max()), 0.0, 'max')
        fig['masked_keys/dv'] = (float(torch.nan_to_num(dv[gone], nan=math.inf).abs().max()), 0.0, 'max')
    return fig


def failing(fig):
    return [label for label, (val, bar, _) in fig.items() if not val <= bar]


def worst_slice(fig):
    return max(v for label, (v, _, _) in fig.items() if label.startswith('slice/'))


# ----------------------------------------------------------------------------------------------------------------------
# 5. fault runners: the fp64 reference with one deliberate defect -> (o, lse2, dq, dk, dv) on the case's (sub-)problem
# ----------------------------------------------------------------------------------------------------------------------
def _rows_of(c, wgs):
    n, H, Lq, Lk, dh = sub_dims(c)
    m = torch.zeros(n, H, Lq, dtype=torch.bool)
    for b, h, t in wgs:
        m[b, h, t * 128:(t + 1) * 128] = True
    return m


def fault_redo_left_overflowed(c):
    """(a) a flagged workgroup keeps the fast forward's overflowed result: o = 0 and lse2 = inf on its rows, which then contribute
    nothing to the backward (exp2(s - inf) = 0)"""
    n, H, Lq, Lk, dh = sub_dims(c)
    rows = _rows_of(c, over_workgroups(c))                         # [n, H, Lq]
    q, k, v, do = sub_inputs(c)
    rows2d = rows.permute(0, 2, 1)[..., None].expand(n, Lq, H, dh).reshape(n * Lq, H * dh)
    o, lse2, dq, dk, dv = R.reference(q, k, v, torch.where(rows2d, torch.zeros((), dtype=do.dtype), do), sub_kb(c), None, 0.0, sub_dims(c))
    return torch.where(rows2d, torch.zeros((), dtype=o.dtype), o), torch.where(rows, math.inf, lse2), dq, dk, dv


def fault_redo_neighbour_stale(c):
    """(b) the flagged workgroup is recomputed, and so is the next workgroup of its head -- from the flagged one's rows"""
    n, H, Lq, Lk, dh = sub_dims(c)
    o, lse2, dq, dk, dv = reference_of(c)
    o4, nqt = o.reshape(n, Lq, H, dh).clone(), cdiv(Lq, 128)
    lse2 = lse2.clone()
    for b, h, t in over_workgroups(c):
        t2 = (t + 1) % nqt
        w = min(128, Lq - t2 * 128, Lq - t * 128)
        o4[b, t2 * 128:t2 * 128 + w, h] = o4[b, t * 128:t * 128 + w, h]
        lse2[b, h, t2 * 128:t2 * 128 + w] = lse2[b, h, t * 128:t * 128 + w]
    return o4.reshape(n * Lq, H * dh), lse2, dq, dk, dv


def fault_dead_first_tile_anchors(c):
    """(c) a dead first tile is treated as plain: its maximum, -inf, anchors the softmax and every later exp2(s - (-inf)) overflows;
    the rows of such a video come out NaN"""
    n, H, Lq, Lk, dh = sub_dims(c)
    o, lse2, dq, dk, dv = reference_of(c)
    bad = tile_classes(sub_kb(c), Lk)[:, 0] == 2                   # [n]
    assert bool(bad.any())
    o4 = o.reshape(n, Lq, H * dh).clone()
    o4[bad] = math.nan
    lse2 = lse2.clone()
    lse2[bad] = math.nan
    return o4.reshape(n * Lq, H * dh), lse2, dq, dk, dv


def fault_classes_not_refreshed(c):
    """(d) the classes of tiles 64 and above are read from tiles 0 .. 63: a tile read as plain runs without its bias (keys past Lk
    stay out), one read as dead is skipped, one read as mixed is right"""
    n, H, Lq, Lk, dh = sub_dims(c)
    kb = sub_kb(c).clone()
    cls = tile_classes(kb, Lk)
    assert cls.shape[1] > 64
    for b in range(n):
        for t in range(64, cls.shape[1]):
            seen = int(cls[b, t - 64])
            if seen == 0:
                kb[b, t * 128:(t + 1) * 128] = 0
            elif seen == 2:
                kb[b, t * 128:(t + 1) * 128] = NINF
    return reference_of(c, kb)


def fault_first_split(c):
    """(e) the first key split is dropped when it is live, or kept (bias ignored) when it is dead"""
    B, H, Lq, Lk, dh = c['dims']
    first = plan_ksplit(B, H, Lq, Lk, dh)[1] * KT
    kb = sub_kb(c)
    kb = torch.zeros(sub_dims(c)[0], Lk) if kb is None else kb.clone()
    dead = (kb[:, :first] == NINF).all(-1)
    kb[dead, :first] = 0
    kb[~dead, :first] = NINF
    return reference_of(c, kb)


def fault_bias_high_half_only(c, dtype=None):
    """(f) a finite bias enters the scores (log2 domain) with only the high 16-bit half of its hi + lo pair"""
    dtype = c['dtype'] if dtype is None else dtype
    kb = sub_kb(c).clone()
    fin = torch.isfinite(kb) & (kb != 0)
    assert bool(fin.any())
    kb[fin] = ((kb[fin].double() * LOG2E).to(dtype).double() / LOG2E).float()
    return reference_of(c, kb)
