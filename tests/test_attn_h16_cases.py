"""tests/attn_h16_cases.py held to fp64 on the CPU: the fp16 conversion of the bf16 cases is exact at every planted value and within
an fp16 subnormal elsewhere, no figure of the fp16 emulation is non-finite, the slice bars of tests/test_gpu_attn_small_fp16.py and
tests/test_gpu_attn_cls_fp16.py are three times the emulation's worst points (re-derived here), every element figure of the emulation is
within half its fp16 bar, and each fault runner of tests/attn_small_cases.py still fails at least one figure at the fp16 bars.  Nothing
here loads the device library.

    kernels          worst slice error of the emulation                              slice bar   worst element figure
    short-sequence   8.71e-4  L = 225, dh = 64, planted, dk rows 224:225             2.61e-3     0.34 of its bar (dk, L = 32, dh = 64)
    one-query        4.49e-4  n2-H3-L65-dh64-deep, dk rows 64:65                     1.35e-3     0.30 of its bar (o, L = 65, dh = 32)
"""
import functools
import math

import pytest
import torch

from tests import attn_cls_cases as C
from tests import attn_h16_cases as H
from tests import attn_small_cases as S
from tests.test_gpu_attn_cls_fp16 import BARS as CLS_BARS
from tests.test_gpu_attn_cls_fp16 import EMULATED as CLS_EMULATED
from tests.test_gpu_attn_small_fp16 import BARS as SMALL_BARS
from tests.test_gpu_attn_small_fp16 import EMULATED as SMALL_EMULATED

SMALL_POINTS = S.points()
CLS_POINTS = C.points()
_pid = lambda p: S.point_id(*p)        # noqa: E731
OPERANDS = ('q', 'k', 'v', 'do')


def test_bars_are_fp16s():
    assert H.TOL == 1.5e-3 and SMALL_BARS == 3.0 * SMALL_EMULATED[0] and CLS_BARS == 3.0 * CLS_EMULATED[0]


def test_planted_values_are_exact_in_fp16_and_the_rest_within_a_subnormal():
    for dh in S.DHS:
        for x in (S.A, S.BETA, S.beta2(dh), S.KD[dh], S.KC[dh], S.CANARY_MAG, C.A, C.KD[dh], C.CANARY_MAG):
            assert float(torch.tensor(x, dtype=torch.float64).to(H.F16).double()) == x, (dh, x)
    # a bf16 value has 8 significant bits: exact in fp16 unless it lies under fp16's smallest normal, where fp16 steps by 2^-24
    worst = max([H.conversion_error(S.make_case(*p), OPERANDS) for p in SMALL_POINTS] +
                [H.conversion_error(C.make_case(*p), OPERANDS) for p in CLS_POINTS])
    print(f'largest conversion error of any input: {worst:.2e}')
    assert worst <= 2.0 ** -25
    for p in SMALL_POINTS:
        c, b = H.small_case(*p), S.make_case(*p)
        assert all(c[t].dtype == H.F16 and bool(torch.isfinite(c[t].float()).all()) for t in OPERANDS)
        # where bf16 holds a planted value, fp16 holds the same one
        for t in ('q', 'k'):
            ch0 = lambda x: x.double().view(x.shape[0], -1, p[1])[..., 0]      # noqa: E731
            assert torch.equal(ch0(c[t]), ch0(b[t])), (p, t)


@functools.lru_cache(maxsize=None)
def small_emulated_figures(point):
    c, ref = H.small_case(*point), H.small_reference(*point)
    o, dq, dk, dv = H.small_emulation(*point)
    return H.small_figures(c, (o, ref[1], dq, dk, dv), ref, SMALL_BARS, lse=False)


@functools.lru_cache(maxsize=None)
def cls_emulated_figures(point):
    return H.cls_figures(H.cls_case(*point), H.cls_emulation(*point), H.cls_reference(*point), CLS_BARS)


def _worst(figures, points, prefix):
    """(value, point, label) of the largest figure whose label starts with prefix, as a share of its bar for element figures"""
    best = (0.0, None, None)
    for p in points:
        for label, (val, bar) in figures(p).items():
            if label.startswith(prefix):
                x = val if prefix == 'slice/' else val / bar
                if x > best[0]:
                    best = (x, p, label)
    return best


def test_short_sequence_slice_bar_is_three_times_the_emulation():
    emu, where, rows = SMALL_EMULATED
    e, p, label = _worst(small_emulated_figures, SMALL_POINTS, 'slice/')
    print(f'short-sequence fp16 emulation: worst slice {e:.3e} at {S.point_id(*p)} {label}')
    assert p == where and label.startswith('slice/dk') and label.endswith(rows + ']'), (p, label)
    assert abs(e - emu) <= 0.01 * emu, (e, emu)
    assert abs(S.worst_slice(small_emulated_figures(where)) - emu) <= 0.01 * emu


def test_one_query_slice_bar_is_three_times_the_emulation():
    emu, where, rows = CLS_EMULATED
    e, p, label = _worst(cls_emulated_figures, CLS_POINTS, 'slice/')
    print(f'one-query fp16 emulation: worst slice {e:.3e} at {C.point_id(*p)} {label}')
    assert p == where and label.startswith('slice/dk') and label.endswith(rows + ']'), (p, label)
    assert abs(e - emu) <= 0.01 * emu, (e, emu)


def test_worst_element_figures_are_the_quoted_ones():
    x, p, label = _worst(small_emulated_figures, SMALL_POINTS, ('elem/', 'deep/'))
    print(f'short-sequence: {x:.2f} of its bar at {S.point_id(*p)} {label}')
    assert f'{x:.2f}' == '0.34' and p[:2] == (32, 64) and label.startswith('elem/dk')
    x, p, label = _worst(cls_emulated_figures, CLS_POINTS, 'elem/')
    print(f'one-query: {x:.2f} of its bar at {C.point_id(*p)} {label}')
    assert f'{x:.2f}' == '0.30' and p[2:4] == (65, 32) and label.startswith('elem/o')


@pytest.mark.parametrize('point', SMALL_POINTS, ids=_pid)
def test_short_sequence_emulation_is_finite_and_within_half_of_every_element_bar(point):
    bad = []
    for label, (val, bar) in small_emulated_figures(point).items():
        if not math.isfinite(val):
            bad.append(f'{label}: not finite')
        elif label.startswith(('elem/', 'deep/')):
            if not val <= 0.5 * bar:
                bad.append(f'{label}: {val:.3e} = {val / bar:.2f} of {bar:.1e}')
        elif not val <= bar:
            bad.append(f'{label}: {val:.3e} > {bar:.3e}')
    assert not bad, '; '.join(bad)


@pytest.mark.parametrize('point', CLS_POINTS, ids=lambda p: C.point_id(*p))
def test_one_query_emulation_is_finite_and_within_half_of_every_element_bar(point):
    bad = []
    for label, (val, bar) in cls_emulated_figures(point).items():
        if not math.isfinite(val):
            bad.append(f'{label}: not finite')
        elif label.startswith('elem/'):
            if not val <= 0.5 * bar:
                bad.append(f'{label}: {val:.3e} = {val / bar:.2f} of {bar:.1e}')
        elif not val <= bar:
            bad.append(f'{label}: {val:.3e} > {bar:.3e}')
    assert not bad, '; '.join(bad)


# ----------------------------------------------------------------------------------------------------------------------
# the fault runners of attn_small_cases on the fp16 tensors, against the fp16 reference at the fp16 bars.  (A runner that starts from
# the module's own reference starts from the bf16 tensors' one: 3e-8 of conversion error away, five orders under any bar.)
# ----------------------------------------------------------------------------------------------------------------------
FAULTS = [(S.fault_key_mask_off_by_one, [(33, 32, 'planted'), (97, 64, 'benign'), (225, 64, 'planted'), (255, 32, 'benign')], None),
          (S.fault_max_of_one_half_wave, [(33, 32, 'planted'), (256, 32, 'planted')], 'not finite'),
          (S.fault_padded_lanes_summed, [(33, 64, 'planted'), (225, 32, 'planted')], 'not finite'),
          (S.fault_second_trip_lse, [(129, 32, 'benign'), (225, 64, 'planted')], 'lse2'),
          (S.fault_dk_heads_exchanged, [(31, 64, 'planted'), (33, 32, 'benign')], 'slice/dk'),
          (S.fault_dq_last_block_left_out, [(225, 32, 'benign'), (256, 64, 'benign')], 'slice/dq')]


@pytest.mark.parametrize('fault,points,must', FAULTS, ids=[f[0].__name__ for f in FAULTS])
def test_fault_runners_still_fail_at_the_fp16_bars(fault, points, must):
    for point in points:
        c, ref = H.small_case(*point), H.small_reference(*point)
        clean = S.failing(H.small_figures(c, ref, ref, SMALL_BARS))
        assert not clean, clean
        bad = S.failing(H.small_figures(c, fault(c), ref, SMALL_BARS))
        print(f'{S.point_id(*point)} {fault.__name__}: caught by {len(bad)} figures: ' + '; '.join(bad[:6]))
        assert bad
        if must is not None:
            assert any(b.startswith(must) for b in bad), (must, bad)
