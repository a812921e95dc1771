"""The head-width 40-64 attention kernels (csrc/attention.hip at two d-tiles) and the attention weights recomputed from their lse2
(csrc/attn_weights.hip) on the device at peaked scores and irregular key masks, against fp64.  Cases, layouts and faults:
tests/attn_wide_range_cases.py; planted inputs and figures: tests/attn_range_cases.py.

  a. parity: every (wide case x mask layout x dtype) point through ops.attn_fwd and ops.attn_bwd.  Figures: slice errors on the
     (batch, head, 128-row tile) slices; element errors per (batch, head, 128-row tile) separately over planted and other rows (o, dq)
     / keys (dk, dv), against the largest reference entry of the (batch, head); lse2 over planted and other rows; gradient rows of
     -inf keys exactly 0; every value finite.
  b. forward and backward twice on the planted inputs: all five outputs bit-identical (no atomics, no scratch).
  c. no wide case asks for scratch.
  d. attention weights of the wide cases from the device forward's lse2, against the fp64 head-mean softmax of the same rounded
     inputs; return codes of svol_attn_weights_mean at head widths 40 ... 72 in every dtype.

Slice bars (BARS_WIDE): 3 x the worst slice error, over every wide point of the dtype, of attn_dropout_ref.emulate without dropout
(fp32: the formula in fp32 torch), the 'pair' layout (two live keys: dS is a difference of near-equal terms) in a row of its own;
tests/test_attn_wide_range_cases.py re-derives the worst points and holds EMULATED_WIDE to them.

    dtype        emulation (worst point)               bar       device's worst slice
    bf16         4.87e-3   wide40, finite              1.46e-2   4.90e-3 (wide40, finite, dq)
    bf16 pair    1.07e-2   wide48, pair                3.22e-2   1.01e-2 (wide48, pair, dk)
    fp16         8.65e-4   wide56, finite              2.60e-3   8.74e-4 (wide56, finite, dq)
    fp16 pair    1.13e-3   wide48, pair                3.38e-3   9.85e-4 (wide48, pair, dk)
    fp32         2.79e-6   wide40, mid_dead            8.37e-6   4.43e-6 (wide56, none, o)
    fp32 pair    1.75e-6   wide56, pair                5.26e-6   8.38e-7 (wide56, pair, dk)

Whole-tensor and per-tile element bars are check_attention's: TOL[dtype] for o, 2 TOL[dtype] for the gradients, its lse2 bars.

Attention weights (absolute, att and |row sum - 1|).  Rows that are not planted: check_attn_weights' bars, fp16 at bf16's.  Planted
rows: 3 x the worst error of attn_wide_range_cases.att_emulation (the kernel's fp32 chain behind an fp32 forward), re-derived on the
CPU like the slice bars.

    dtype   planted rows: emulation (worst point)   bar       device      other rows: bar   emulation   device
    bf16    5.07e-6   wide48, pair                  1.52e-5   9.25e-6     5e-3              3.4e-6      3.4e-6
    fp16    2.18e-6   wide64_raw, finite            6.54e-6   2.68e-6     5e-3              3.8e-6      3.8e-6
    fp32    2.09e-6   wide64_raw, pair              6.27e-6   3.30e-6     1e-5              3.5e-6      3.5e-6

The device's worst planted rows are row sums (bf16: wide64, sub_dead; fp16: wide64_raw, pair; fp32: wide56, none).
profiles/attn_wide.md keeps the same figures.
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from tests import attn_range_cases as A
from tests import attn_wide_range_cases as W
from tests.test_gpu_attn_dropout import check
from tests.test_gpu_attn_range import backward, forward

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, FP16, FP32 = A.BF16, A.FP16, A.FP32
# worst slice error of the emulation per dtype and bar row, and where (case, variant, mask layout)
EMULATED_WIDE = {
    BF16: {'other': (4.870e-3, ('wide40', 'peaked', 'finite')), 'pair': (1.0737e-2, ('wide48', 'peaked', 'pair'))},
    FP16: {'other': (8.651e-4, ('wide56', 'peaked', 'finite')), 'pair': (1.1254e-3, ('wide48', 'peaked', 'pair'))},
    FP32: {'other': (2.79e-6, ('wide40', 'peaked', 'mid_dead')), 'pair': (1.75e-6, ('wide56', 'peaked', 'pair'))},
}
BARS_WIDE = {dt: {kind: 3.0 * e for kind, (e, _) in rows.items()} for dt, rows in EMULATED_WIDE.items()}
# worst error of the attention-weights emulation on planted rows per dtype, and where (case, mask layout)
ATT_EMULATED = {BF16: (5.07e-6, ('wide48', 'pair')), FP16: (2.18e-6, ('wide64_raw', 'finite')), FP32: (2.09e-6, ('wide64_raw', 'pair'))}
ATT_BARS_PLANTED = {dt: 3.0 * e for dt, (e, _) in ATT_EMULATED.items()}
SVOL_E_UNSUPPORTED = -2   # include/svol_hip.h

POINTS = [(n, v, m, dt) for dt in (BF16, FP16, FP32) for n, v, m in W.points(dt)]
ATT_POINTS = [(n, m, dt) for dt in (BF16, FP16, FP32) for n, m in W.att_points(dt)]
TWICE = [(n, dt) for dt in (BF16, FP16, FP32) for n, c in W.CASES.items() if dt != FP32 or c['fp32']]
_id = lambda *p: '-'.join(A.DT_NAME.get(x, x) for x in p)


def slice_bar(layout, dtype):
    return BARS_WIDE[dtype][W.bar_kind(layout)]


@functools.lru_cache(maxsize=None)
def reference_of(name, variant, layout, dtype):
    """the fp64 reference of one point, computed once and shared (never modified)"""
    return A.reference_of(W.make_case(name, variant, layout, dtype))


def test_bars_are_check_attentions():
    from tests import gpu_checks as G
    assert A.TOL == G.TOL


@pytest.mark.parametrize('name,variant,layout,dtype', POINTS, ids=[_id(*p) for p in POINTS])
def test_parity_with_fp64_by_slice(name, variant, layout, dtype):
    c = W.make_case(name, variant, layout, dtype)
    o, lse2 = forward(c)
    dq, dk, dv = backward(c, o, lse2)
    fig = A.figures(c, A.sub_outputs(c, (o, lse2, dq, dk, dv)), reference_of(name, variant, layout, dtype), slice_bar(layout, dtype))
    check(fig, _id(name, variant, layout, dtype))


@pytest.mark.parametrize('name,dtype', TWICE, ids=[_id(*p) for p in TWICE])
def test_two_runs_give_the_same_bits_on_planted_inputs(name, dtype):
    """forward and backward twice under the 'finite' layout (-inf keys, finite biases, the two large ones): o, lse2, dq, dk, dv"""
    c = W.make_case(name, 'peaked', 'finite', dtype)
    runs = []
    for _ in range(2):
        o, lse2 = forward(c)
        runs.append((o, lse2) + backward(c, o, lse2))
    for tag, x, y in zip(('o', 'lse2', 'dq', 'dk', 'dv'), *runs):
        assert bool(torch.isfinite(x.float()).all()), f'{tag} is not finite'
        assert torch.equal(x, y), f'{tag}: two runs differ'


def test_no_wide_case_takes_scratch():
    from svol_amd import _lib
    for name, cs in W.CASES.items():
        assert int(_lib.lib().svol_attn_ws_bytes(*cs['dims'])) == 0 == A.ws_floats(*cs['dims']), name


@pytest.mark.parametrize('name,layout,dtype', ATT_POINTS, ids=[_id(*p) for p in ATT_POINTS])
def test_attention_weights_against_the_fp64_head_mean(name, layout, dtype):
    from svol_amd import ops
    c = W.make_case(name, 'peaked', layout, dtype)
    B, H, Lq, Lk, dh = c['dims']
    _, lse2 = forward(c)
    kb = None if c['kb'] is None else c['kb'].to(DEV)
    att = ops.attn_weights_mean(c['q'].to(DEV), c['k'].to(DEV), lse2, B, H, Lq, Lk, dh, kb, c['pm'])
    torch.cuda.synchronize()
    assert att.shape == (B, Lq, Lk) and att.dtype == torch.float32
    check(W.att_figures(c, att, ATT_BARS_PLANTED[dtype]), 'att ' + _id(name, layout, dtype))


def test_attention_weights_return_codes():
    """head widths 40, 48, 56 and 64 are served in every dtype; 72 is refused and nothing is written"""
    from svol_amd import _lib, ops
    lib, P = _lib.lib(), ops._ptr
    B, H, Lq, Lk = 1, 2, 5, 16
    for dtype in (FP32, BF16, FP16):
        for dh, want in ((40, 0), (48, 0), (56, 0), (64, 0), (72, SVOL_E_UNSUPPORTED)):
            q = torch.zeros((B * Lq, H * dh), dtype=dtype, device=DEV)
            k = torch.zeros((B * Lk, H * dh), dtype=dtype, device=DEV)
            lse2 = torch.full((B, H, Lq), 4.0, dtype=torch.float32, device=DEV)   # log2 of 16 keys at score 0
            att = torch.full((B, Lq, Lk), 7.0, dtype=torch.float32, device=DEV)
            rc = lib.svol_attn_weights_mean(P(q), q.stride(0), P(k), k.stride(0), P(lse2), None, P(att), B, H, Lq, Lk, dh,
                                            1.0 / math.sqrt(dh), 0.0, ops._DT[dtype], ops._stream())
            torch.cuda.synchronize()
            assert rc == want, (dh, dtype, rc)
            assert bool((att == (7.0 if want else 1.0 / Lk)).all()), (dh, dtype)
