"""The cases of tests/attn_small_cases.py (short-sequence attention, csrc/vit.hip) and tests/attn_cls_cases.py (one-query attention,
csrc/sketch_cls.hip) with fp16 operands: the ``_h16`` entry points' cases.  Both modules are used as they are; this one

  1. converts a case's tensors to fp16.  Every planted value (256, 0.75, beta2, 2.25 / 3.125, 3 / 4, 64) is exact in fp16, and a bf16
     draw of randn * 1.2 is too unless it lies under fp16's smallest normal (6.1e-5), where the conversion rounds to a multiple of
     2^-24: an error of 3.0e-8 at most (tests/test_attn_h16_cases.py);
  2. computes the fp64 reference and the emulation from the CONVERTED tensors: attn_dropout_ref.emulate with rounder(torch.float16)
     for the short-sequence kernels (P, dS and the outputs rounded to fp16), fp16 stores of o / dq / dk / dv for the one-query kernels
     (their arithmetic is fp32 throughout);
  3. re-bars the element figures ('elem/', 'deep/') at gpu_checks.TOL[torch.float16] = 1.5e-3 for o and twice that for the gradients.
     The slice bar is the caller's; lse2 (2e-5), finiteness and the L = 1 identities keep their bars.

Plain torch on the CPU, importable without the device library.
"""
from __future__ import annotations

import functools

import torch

from tests import attn_cls_cases as C
from tests import attn_dropout_ref as R
from tests import attn_small_cases as S

F16 = torch.float16
TOL = 1.5e-3              # tests/gpu_checks.py TOL[fp16]: o; the gradients take twice that


def _rebar(fig):
    """the figures with the element bars of the bf16 modules replaced by fp16's"""
    out = {}
    for label, (val, bar) in fig.items():
        if label.startswith(('elem/', 'deep/')):
            bar = TOL if label.startswith('elem/o ') else 2 * TOL
        out[label] = (val, bar)
    return out


def conversion_error(c, names):
    """max |fp16(t) - t| over the named tensors of a bf16 case"""
    return max(float((c[t].to(F16).double() - c[t].double()).abs().max()) for t in names)


# ----------------------------------------------------------------------------------------------------------------------
# short-sequence attention
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case(L, dh, family):
    """attn_small_cases.make_case with q, k, v, do in fp16 (canary rows included).  Shared between tests: never modified."""
    c = dict(S.make_case(L, dh, family))
    for t in ('q', 'k', 'v', 'do'):
        c[t] = c[t].to(F16)
    return c


def _small_operands(c):
    return tuple(S.real(c, c[t]) for t in ('q', 'k', 'v', 'do'))


@functools.lru_cache(maxsize=None)
def small_reference(L, dh, family):
    """fp64 from the fp16 tensors -> o, lse2 [n, H, L], dq, dk, dv (shared, never modified)"""
    c = small_case(L, dh, family)
    return R.reference(*_small_operands(c), None, None, 0.0, S._dims5(c))


def small_emulation(L, dh, family):
    """attn_dropout_ref.emulate with fp16 roundings at the kernels' rounding sites -> o, dq, dk, dv"""
    c = small_case(L, dh, family)
    return R.emulate(*_small_operands(c), None, None, 0.0, S._dims5(c), R.rounder(F16), torch.float64)


def small_figures(c, got, ref, slice_bar, lse=True):
    return _rebar(S.figures(c, got, ref, slice_bar, lse=lse))


# ----------------------------------------------------------------------------------------------------------------------
# one-query attention
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cls_case(n, H, L, dh, family):
    """attn_cls_cases.make_case with q, k, v, do in fp16 (canary rows included).  Shared between tests: never modified."""
    c = dict(C.make_case(n, H, L, dh, family))
    for t in ('q', 'k', 'v', 'do'):
        c[t] = c[t].to(F16)
    return c


@functools.lru_cache(maxsize=None)
def cls_reference(n, H, L, dh, family):
    """fp64 from the fp16 tensors -> (o, lse2, dq, dk, dv) (shared, never modified)"""
    c = cls_case(n, H, L, dh, family)
    return C._math(*C.real(c), c['dims'])


def cls_emulation(n, H, L, dh, family):
    """fp64 arithmetic, o / dq / dk / dv stored as fp16 -> (o, lse2, dq, dk, dv)"""
    o, lse2, dq, dk, dv = cls_reference(n, H, L, dh, family)
    r = lambda t: t.to(F16).double()   # noqa: E731
    return r(o), lse2, r(dq), r(dk), r(dv)


def cls_figures(c, got, ref, slice_bar):
    return _rebar(C.figures(c, got, ref, slice_bar))
