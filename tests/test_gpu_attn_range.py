"""The dropout-free attention plans on the device at peaked scores and irregular key masks (tests/attn_range_cases.py: the dispatch
twin, the planted inputs, the mask layouts, the figures), against fp64.

  a. parity: every (plan case x input variant / mask layout x dtype) point of attn_range_cases.CASES through ops.attn_fwd and
     ops.attn_bwd.  Figures: slice errors on the (batch, head, 128-row tile) slices; element errors per (batch, head, 128-row tile)
     separately over planted and other rows (o, dq) / keys (dk, dv), against the largest reference entry of the (batch, head); lse2
     over planted and other rows; gradient rows of -inf keys exactly 0; every value finite.
  b. redo flags: svol_attn_fwd on the fast2+redo shape with a caller-owned scratch pre-filled with NaN patterns.  The number of
     flagged workgroups is the number of (batch, head, query tile) triples that hold an 'over' row (non-zero in bf16 and in fp16), 0
     with the 'calm' variant; the same launch's o and lse2 then feed the backward (attn_bwd_dq_bf16_rot + attn_bwd_dkdv_bf16_pre_dma).
  c. every forward plan twice on the planted inputs: bit-identical.

pre_masked_65 (3 x 8 heads x 1024 queries x 8400 keys) runs whole on the device; its fp64 reference covers three (batch, head)
pairs: the first (0, 0: 'late' keys, tile 1 and tile 64 dead), a middle one (1, 2: 'step' keys, tile 0 dead) and the last (2, 7:
'front' key, tile 64 with a single live key).

Slice bars (BARS): 3 x the worst slice error, over every point of the dtype, of attn_dropout_ref.emulate without dropout (fp32: the
formula in fp32 torch); tests/test_attn_range_cases.py re-derives the worst point and holds EMULATED to it.  The factor covers
accumulation order, the exp2 approximation and the fp32 atomics of the key split and of the single-pass backward.

    dtype   emulation (worst point)                          bar       device's worst slice
    bf16    5.85e-3   pre_masked_65, peaked, cls65           1.76e-2   6.52e-3 (pre_masked, one_live, dk)
    fp16    8.79e-4   general, peaked, finite                2.64e-3   8.79e-4 (general, finite, dk)
    fp32    1.28e-6   general, peaked, finite                3.84e-6   3.25e-6 (ksplit_fq, mid_dead, dk)

Whole-tensor and per-tile element bars are check_attention's: TOL[dtype] for o, 2 TOL[dtype] for the gradients, its lse2 bars.
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from tests import attn_range_cases as A
from tests.test_gpu_attn_dropout import check

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, FP16, FP32 = A.BF16, A.FP16, A.FP32
# worst slice error of the emulation per dtype, and where (case, variant, mask layout)
EMULATED = {BF16: (5.85e-3, ('pre_masked_65', 'peaked', 'cls65')), FP16: (8.79e-4, ('general', 'peaked', 'finite')),
            FP32: (1.28e-6, ('general', 'peaked', 'finite'))}
BARS = {dt: 3.0 * e for dt, (e, _) in EMULATED.items()}

POINTS = [(n, v, m, dt) for dt in (BF16, FP16, FP32) for n, v, m in A.points(dt)]
_id = lambda n, v, m, dt: f'{n}-{v}-{m}-{A.DT_NAME[dt]}'


def forward(c, ws=None, o=None, lse2=None):
    """ops.attn_fwd, or svol_attn_fwd with the caller's scratch and outputs -> o, lse2 (device)"""
    from svol_amd import _lib, ops
    B, H, Lq, Lk, dh = c['dims']
    q, k, v = (c[t].to(DEV) for t in 'qkv')
    kb = None if c['kb'] is None else c['kb'].to(DEV)
    if ws is None:
        return ops.attn_fwd(q, k, v, B, H, Lq, Lk, dh, kb, c['pm'])
    P = ops._ptr
    rc = _lib.lib().svol_attn_fwd(P(q), q.stride(0), P(k), k.stride(0), P(v), v.stride(0), P(o), o.stride(0), P(lse2),
                                  P(kb) if kb is not None else None, B, H, Lq, Lk, dh, 1.0 / math.sqrt(dh), c['pm'], P(ws),
                                  ws.numel() * 4, ops._dt(q), ops._stream())
    _lib.check(rc, 'svol_attn_fwd')
    return o, lse2


def backward(c, o, lse2):
    from svol_amd import ops
    B, H, Lq, Lk, dh = c['dims']
    q, k, v, do = (c[t].to(DEV) for t in ('q', 'k', 'v', 'do'))
    kb = None if c['kb'] is None else c['kb'].to(DEV)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ops.attn_bwd(q, k, v, o, do, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kb, c['pm'])
    torch.cuda.synchronize()
    return dq, dk, dv


@functools.lru_cache(maxsize=None)
def reference_of(name, variant, layout, dtype):
    """the fp64 reference of one point, computed once and shared (never modified)"""
    return A.reference_of(A.make_case(name, variant, layout, dtype))


def figures_of(c, got):
    ref = reference_of(c['name'], c['variant'], c['layout'], c['dtype'])
    return A.figures(c, A.sub_outputs(c, got), ref, BARS[c['dtype']])


def test_bars_are_check_attentions():
    from tests import gpu_checks as G
    assert A.TOL == G.TOL


@pytest.mark.parametrize('name,variant,layout,dtype', POINTS, ids=[_id(*p) for p in POINTS])
def test_parity_with_fp64_by_slice(name, variant, layout, dtype):
    c = A.make_case(name, variant, layout, dtype)
    o, lse2 = forward(c)
    dq, dk, dv = backward(c, o, lse2)
    check(figures_of(c, (o, lse2, dq, dk, dv)), _id(name, variant, layout, dtype))


@pytest.mark.parametrize('dtype', [BF16, FP16], ids=lambda d: A.DT_NAME[d])
def test_fast_forward_flags_exactly_the_overflowed_workgroups(dtype):
    """attn_fwd_bf16_fast2 flags a workgroup whose row sum left its range, attn_fwd_bf16_pre recomputes exactly those.  The scratch
    and the outputs start as NaN patterns: a flag that was never written is neither 0 nor 1, a row no kernel wrote is not finite."""
    from svol_amd import _lib
    name = 'fast2+redo'
    B, H, Lq, Lk, dh = A.CASES[name]['dims']
    nwg = B * H * A.cdiv(Lq, 128)
    need = int(_lib.lib().svol_attn_ws_bytes(B, H, Lq, Lk, dh))
    assert need >= nwg * 4
    counts = {}
    for variant in ('peaked', 'calm'):
        c = A.make_case(name, variant, 'none', dtype)
        ws = torch.full((need // 4,), math.nan, dtype=torch.float32, device=DEV)
        o = torch.full((B * Lq, H * dh), math.nan, dtype=dtype, device=DEV)
        lse2 = torch.full((B, H, Lq), math.nan, dtype=torch.float32, device=DEV)
        forward(c, ws, o, lse2)
        torch.cuda.synchronize()
        flags = ws.view(torch.int32)[:nwg].cpu()
        assert bool(((flags == 0) | (flags == 1)).all()), f'{variant}: a redo flag was not written: {flags.tolist()}'
        counts[variant] = int(flags.sum())
        want = len(A.over_workgroups(c))
        print(f'{A.DT_NAME[dtype]} {variant}: {counts[variant]} of {nwg} workgroups flagged, {want} hold an over row')
        assert counts[variant] == want == A.expected_flags(c)
        # the backward after a redo reads this launch's o and lse2
        dq, dk, dv = backward(c, o, lse2)
        check(figures_of(c, (o, lse2, dq, dk, dv)), f'redo {variant} {A.DT_NAME[dtype]}')
    assert counts['peaked'] > 0 and counts['calm'] == 0


FWD_POINTS = [(n, c['points'][-1][1], dt) for dt in (BF16, FP16, FP32) for n, c in A.CASES.items() if dt != FP32 or c['fp32']]


@pytest.mark.parametrize('name,layout,dtype', FWD_POINTS, ids=[f'{n}-{m}-{A.DT_NAME[dt]}' for n, m, dt in FWD_POINTS])
def test_forward_is_bit_reproducible_on_planted_inputs(name, layout, dtype):
    """every forward plan (the key split's combine included: it takes no atomics) twice on the peaked inputs"""
    c = A.make_case(name, 'peaked', layout, dtype)
    o1, l1 = forward(c)
    o2, l2 = forward(c)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1.float()).all()) and bool(torch.isfinite(l1).all())
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
