"""tests/row_kernel_cases.py on the CPU: every case's launch plan has the property its comment claims, the fp64 references are the
oracle's, the fp32 emulation of a correct kernel stays under half of every bar on every case (the inputs leave room), and five
planted defects, each applied to the emulation's output, push the per-row / per-column metric past twice its bar — the first of them
at a size the whole-tensor metric of the older tests does not see."""
import os
import re

import pytest
import torch

from tests import row_kernel_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---- launch plans -----------------------------------------------------------------------------------------------------------------------
def test_the_restated_constants_are_the_launchers():
    norm = open(os.path.join(ROOT, 'svol_amd', 'csrc', 'norm.hip')).read()
    gate = open(os.path.join(ROOT, 'svol_amd', 'csrc', 'gate.hip')).read()
    assert 'lnw_wgs = D <= 2048 ? 1024 : 512' in norm and '(M + 2047) / 2048' in norm
    for rung in ('D <= 256', 'D <= 512', 'D <= LN_MAX_PASSES * 256', 'D <= 2048', 'D <= 3072'):
        assert rung in norm
    assert re.search(r'atoll\(getenv\(names\[which\]\)\) : 4096', gate) and 'w[which] < 64 ? 64 : w[which]' in gate
    assert 'rows_per_wave(L, gate_waves(0) / B + 1)' in gate and 'rows_per_wave(M, gate_waves(1))' in gate
    assert 'rows_per_wave(L, gate_waves(2) / B + 1)' in gate


@pytest.mark.parametrize('case', R.LN_CASES, ids=lambda c: c.id)
def test_layernorm_plan_has_what_the_case_claims(case):
    pl = R.ln_plan(case.M, case.D)
    rung = R.ln_rung(case.D)
    assert pl['wide'] == rung.startswith('wide') and pl['NP'] == int(rung[-1])
    if case.claim == 'idle':
        assert pl['rpw'] == 1 and pl['owners'] == 3
        assert (pl['grid'], pl['live_owners_last_wg']) == ((3, 1) if pl['wide'] else (1, 3))     # narrow: one idle wave of four
    elif case.claim == 'one':
        assert pl['owners'] == 1 and pl['grid'] == 1
    elif case.claim == 'rpw2':
        assert not pl['wide'] and pl['rpw'] == 2 and pl['owners'] == 1025 and pl['rows_last_owner'] == 1
        assert pl['grid'] == 257 and pl['live_owners_last_wg'] == 1
    elif case.claim == 'rpw3':
        assert not pl['wide'] and pl['rpw'] == 3 and pl['owners'] == 1367 and pl['rows_last_owner'] == 1
        assert pl['grid'] == 342 and pl['live_owners_last_wg'] == 3
    elif case.claim == 'wide2':
        assert pl['wide'] and pl['rpw'] == 2 and pl['rows_last_owner'] == 1 and pl['grid'] == (case.M + 1) // 2
    else:
        raise AssertionError(case.claim)


def test_the_table_reaches_every_path_the_issue_names():
    walked = {R.ln_plan(c.M, c.D)['NP'] for c in R.LN_CASES if c.D <= 1024 and R.ln_plan(c.M, c.D)['rpw'] >= 2}
    assert walked == {1, 2, 4}
    assert {R.ln_plan(c.M, c.D)['NP'] for c in R.LN_CASES if c.D > 1024 and R.ln_plan(c.M, c.D)['rpw'] >= 2} == {2, 3, 4}
    assert any(0 < R.ln_plan(c.M, c.D)['live_owners_last_wg'] < 4 and R.ln_plan(c.M, c.D)['grid'] > 1 for c in R.LN_CASES if c.D <= 1024)
    many = {c.D for c in R.LN_CASES if c.M > 3}
    for name, widths in R.RUNGS.items():    # first and last width of every rung: one vector past the rung below, and the rung's limit
        first, last = widths[0], widths[-1]
        assert R.ln_rung(first) == name and R.ln_rung(last) == name
        assert first == 4 or R.ln_rung(first - 4) != name
        assert last == 4096 or R.ln_rung(last + 4) != name
        assert {first, last} <= {c.D for c in R.LN_CASES if c.M == 3} and first in many
        # the first width puts ONE vector into a new pass (252 and 1020 stop one vector short of a rung's limit)
        assert first % (1024 if first > 1024 else 256) == 4
    assert {252, 1020} <= many
    for c in R.LN_CASES:
        assert R.live_rows(c.M, R.ln_plan(c.M, c.D)['rpw'])[0] == 0


@pytest.mark.parametrize('case', R.GATE_CASES, ids=lambda c: c.id)
def test_gate_plan_has_what_the_case_claims(case):
    B, L, D, H = case.shape
    pl = R.gate_plan(B, L, D, H, case.waves)
    if case.claim == 'pair straddles':
        assert pl['rpw'] == 2 and pl['rpw1'] == 2 and L % 2 == 1
        assert pl['crossings'].count(1) == 1 and pl['max_crossings'] == 1           # exactly one wave's pair lies across the boundary
        w = pl['crossings'].index(1)
        assert (2 * w) // L == 0 and (2 * w + 1) // L == 1
    elif case.claim == 'rpw2 one video':
        assert B == 1 and pl['rpw'] == 2 and pl['rpw1'] == 2 and pl['max_crossings'] == 0 and pl['NP'] == 4
    elif case.claim == 'every wave crosses one':
        assert pl['rpw1'] == 4 and L == 3 and set(pl['crossings'][:-1]) == {1}
        assert pl['rpw'] == L and pl['grid_sc'] == (1, B) and pl['idle_waves_sc'] == 3   # a whole video per wave, three idle waves
    elif case.claim == 'crosses two':
        assert pl['rpw1'] == 5 and L == 2 and pl['max_crossings'] == 2 and min(pl['crossings']) == 2
        assert pl['rpw'] == L and pl['grid_sc'] == (1, B) and pl['idle_waves_sc'] == 3
    elif case.claim == 'ragged crossing':
        assert pl['rpw1'] >= 3 and L % pl['rpw1'] != 0 and pl['max_crossings'] == 1 and pl['waves_crossing'] == B - 1
    else:
        raise AssertionError(case.claim)
    assert pl['NP'] == (1 if D <= 256 else 2 if D <= 512 else 4) and pl['head_groups'] == -(-H // 8)


def test_the_gate_table_hands_over_across_one_and_across_several_boundaries():
    plans = [R.gate_plan(*c.shape, c.waves) for c in R.GATE_CASES]
    assert any(p['max_crossings'] == 1 for p in plans) and any(p['max_crossings'] >= 2 for p in plans)
    assert {p['NP'] for p in plans} == {1, 2, 4} and {p['head_groups'] for p in plans} == {1, 2, 4}
    # what tests/test_gpu_gate_heads.py's (3, 5, 64, 16) does NOT do: at M = 15 a wave has one row
    assert R.gate_plan(3, 5, 64, 16)['rpw1'] == 1 and R.gate_plan(3, 5, 64, 16)['max_crossings'] == 0


# ---- references ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [R.LnCase(3, 260, 'bf16', 'fp32', 'idle'), R.LnCase(3, 4, 'fp32', 'fp32', 'idle')], ids=lambda c: c.id)
def test_layernorm_reference_is_the_oracles_and_autograds(case):
    from oracle import svol_oracle as O
    inp, ref = R.ln_inputs(case), R.ln_reference(case)
    x, g, b = (inp[k].double().requires_grad_(True) for k in ('x', 'gamma', 'beta'))
    for p in (0.0, R.P_DROP):
        ks = R.keep_scale(case.M, case.D, p, F64)
        y = O.layer_norm(x, g, b) * (1.0 if ks is None else ks)
        assert R.whole_tensor_err(ref[p]['fwd']['y32'], y) < 1e-13
        assert R.whole_tensor_err(ref[p]['fwd']['ypos'], y + inp['pos'].double()[torch.arange(case.M) % R.POS_ROWS]) < 1e-13
        d = inp['dy32'].double() + inp['dy'].double() + inp['dy2'].double()
        dx, dg, db = torch.autograd.grad((y * d).sum(), (x, g, b))
        bw = ref[p]['bwd']
        assert R.whole_tensor_err(bw['dx32'], dx) < 1e-12
        assert R.whole_tensor_err(bw['dgamma'] - R.FILL, dg) < 1e-12 and R.whole_tensor_err(bw['dbeta'] - R.FILL, db) < 1e-12
        assert R.whole_tensor_err(bw['colsum'] - R.FILL, dx.sum(0)) < 1e-9 * float(bw['S']['colsum'].max() / dx.sum(0).abs().max())
    dx, = torch.autograd.grad((O.layer_norm(x, g, b) * inp['dy2'].double()).sum(), (x,))
    assert R.whole_tensor_err(ref['lean']['dx32'], dx) < 1e-12


@pytest.mark.parametrize('regime', R.GATE_REGIMES)
def test_gate_reference_is_gpu_checks_and_autograds(regime):
    from tests.gpu_checks import _gate_ref
    shape, t = (3, 50, 260, 9), 'bf16'
    inp, ref = R.gate_inputs(shape, t, regime), R.gate_reference(shape, t, regime)
    x, u, g, b = (inp[k].double().requires_grad_(True) for k in ('x', 'u', 'gamma', 'beta'))
    y, ypos = _gate_ref(x, inp['pos'].double(), u, g, b, shape[3])
    assert R.whole_tensor_err(ref['y32'], y) < 1e-13 and R.whole_tensor_err(ref['ypos'], ypos) < 1e-13
    loss = (y * inp['dy32'].double()).sum()
    if regime == 'unit':
        loss = loss + (y * inp['dy'].double()).sum() + (ypos * inp['dyp'].double()).sum()
    dx, du, dg, db = torch.autograd.grad(loss, (x, u, g, b))
    assert R.whole_tensor_err(ref['dx'], dx) < 1e-11 and R.whole_tensor_err(ref['dgamma'], dg) < 1e-11
    assert R.whole_tensor_err(ref['dbeta'], db) < 1e-11
    # du cancels to ~1e-6 of its terms at unit variance (LN1 forgets the per-token scale): held on the scale of its terms there
    assert float((ref['du'] - du).abs().max()) < 1e-11 * float((ref['du_scale'] / R.DU_RESIDUE).max())
    if regime == 'small_variance':
        assert R.whole_tensor_err(ref['du'], du) < 1e-9


def test_the_metrics_name_the_row_and_the_column():
    ref = torch.ones((2, 3, 4), dtype=F64)
    got = ref.clone()
    got[1, 2, 0] = 1.5
    assert R.row_err(got, ref) == (0.5, (1, 2))
    assert R.col_err(torch.tensor([1.0, 2.0, 3.5]), torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1.0, 1.0, 5.0])) == (0.1, 2)
    got[0, 0, 0] = float('nan')
    assert R.row_err(got, ref)[0] == float('inf')


def test_the_column_bars_come_from_the_emulation_table_alone():
    for (kernel, q, t), v in R.EMU_COL.items():
        assert 1e-9 < v < 1e-6      # (the issue's CPU probe: 1e-8 to 1.3e-7; dgamma's single-term sums come to 2.5e-7)
        assert R.col_bar(kernel, q, t) == max(32 * 2.0 ** -24, 16 * v) <= R.COL_CAP[t] / 20


# ---- the emulation stays under half of every bar ---------------------------------------------------------------------------------------
def _under_half(fig, what, t, rounded=('y', 'ypos', 'dx')):
    """half of every bar; of a 16-bit row output's bar, half of the fp32 part: the other part IS the rounding of a correct result"""
    def room(k, bar):
        ulp = R.HALF_ULP[t] if k.split('/')[-1] in rounded else 0.0
        return ulp + 0.5 * (bar - ulp)
    bad = [f'{k}: {v:.3e} at {w} against {room(k, bar):.3e} of {bar:.3e}' for k, (v, bar, w) in fig.items() if not v <= room(k, bar)]
    assert not bad, f'{what}: ' + '; '.join(bad)


@pytest.mark.parametrize('case', R.LN_CASES, ids=lambda c: c.id)
def test_layernorm_emulation_is_under_half_of_every_bar(case):
    fig = R.ln_emulation_figures(case)
    assert len(fig) == 2 * 10 + 3
    _under_half(fig, case.id, case.t)
    for p in (0.0, R.P_DROP):   # the kept set is readable off the emulation's y, as it has to be off the kernel's
        keep = R.ln_reference(case)[p]['keep']
        if keep is not None:
            assert bool(((R.ln_emulation(case)[p]['fwd']['y32'] != 0) == keep).all())


@pytest.mark.parametrize('regime', R.GATE_REGIMES)
@pytest.mark.parametrize('t', R.GATE_DTYPES)
@pytest.mark.parametrize('case', R.GATE_CASES, ids=lambda c: c.id)
def test_gate_emulation_is_under_half_of_every_bar(case, t, regime):
    fig = R.gate_emulation_figures(case, t, regime)
    assert len(fig) == len(R.GATE_KEYS)
    _under_half(fig, f'{case.id} {t} {regime}', t, rounded=('y', 'ypos'))
    if regime == 'small_variance':   # check_gate's two conditions on the regime: the gate is visible, du is not noise
        ref = R.gate_reference(case.shape, t, regime)
        assert float(ref['du'].abs().max() / ref['dx'].abs().max()) >= 1e-5


# ---- planted defects ------------------------------------------------------------------------------------------------------------------
WALKED = [R.LnCase(2049, 256, 'bf16', 'fp32', 'rpw2'), R.LnCase(2049, 512, 'bf16', 'fp32', 'rpw2'), R.LnCase(2049, 1024, 'bf16', 'fp32', 'rpw2')]


@pytest.mark.parametrize('case', WALKED, ids=lambda c: c.id)
def test_defect_a_a_row_normalised_with_the_next_rows_rstd(case):
    """the prefetch off by one (cur.rs read from nxt): row 1000 of owner 500 takes row 1001's rstd.  Seen by dgamma's col_err and by
    dx's row_err; NOT by the whole-tensor metric at the 16-bit column bar of the older tests, which is why this file exists"""
    r = 1000
    assert r % R.ln_plan(case.M, case.D)['rpw'] == 0 and case in R.LN_CASES
    ref, good, bad = R.ln_reference(case), R.ln_emulation(case), R.ln_emulation(case, rstd_defect_row=r)
    shift = abs(float(good[0.0]['fwd']['rstd'][r + 1] / good[0.0]['fwd']['rstd'][r]) - 1.0)
    fig = R.ln_figures(case, {k: bad[0.0]['bwd'][k] for k in ('dx32', 'dx', 'dgamma', 'colsum')}, ref, 0.0)
    old = R.whole_tensor_err(bad[0.0]['bwd']['dgamma'] - R.FILL, ref[0.0]['bwd']['dgamma'] - R.FILL)
    print(f'{case.id}: rstd off by {shift:.1%}; dgamma col_err {fig["p0.0/dgamma"][0]:.2e} (bar {fig["p0.0/dgamma"][1]:.2e}), dx row_err '
          f'{fig["p0.0/dx"][0]:.2e} at row {fig["p0.0/dx"][2]} (bar {fig["p0.0/dx"][1]:.2e}); whole-tensor dgamma {old:.2e} (bar 1e-2)')
    assert shift > 0.005
    assert fig['p0.0/dgamma'][0] >= 2 * fig['p0.0/dgamma'][1]
    assert fig['p0.0/dx32'][0] >= 2 * fig['p0.0/dx32'][1] and fig['p0.0/dx32'][2] == (r,)
    assert fig['p0.0/dx'][0] >= 2 * fig['p0.0/dx'][1] and fig['p0.0/dx'][2] == (r,)
    assert old < 1e-2                                                              # today's metric at today's bar lets it through
    clean = R.ln_figures(case, {k: good[0.0]['bwd'][k] for k in ('dx32', 'dx', 'dgamma', 'colsum')}, ref, 0.0)
    _under_half(clean, case.id, case.t)


@pytest.mark.parametrize('case', WALKED + [R.LnCase(4099, 1020, 'fp32', 'fp32', 'rpw3'), R.LnCase(1027, 2048, 'fp16', 'fp16', 'wide2')],
                         ids=lambda c: c.id)
def test_defect_b_the_last_row_of_an_owners_range_missing_from_dgamma(case):
    assert case in R.LN_CASES
    rpw = R.ln_plan(case.M, case.D)['rpw']
    r = 300 * rpw + rpw - 1
    ref, good = R.ln_reference(case), R.ln_emulation(case)
    for launch, bw in ((0.0, good[0.0]['bwd']), (R.P_DROP, good[R.P_DROP]['bwd']), ('lean', good['lean'])):
        got = {'dgamma': bw['dgamma'] - (bw['d'] * bw['xhat'])[r], 'dbeta': bw['dbeta'] - bw['d'][r]}
        fig = R.ln_figures(case, got, ref, launch)
        for k, (v, bar, where) in fig.items():
            print(f'{case.id} {k}: {v:.2e} at column {where} (bar {bar:.2e})')
            assert v >= 2 * bar


@pytest.mark.parametrize('D', [4, 252, 260, 516, 1020, 1028, 2052, 3076])
def test_defect_c_the_last_partial_vector_zero_in_dx(D):
    """columns >= D - 4 (the only vector of the last pass at 260, 516, 1028, 2052, 3076) not stored, in the last row"""
    case = R.LnCase(3, D, 'bf16', 'fp32', 'idle')
    assert case in R.LN_CASES
    ref, good = R.ln_reference(case), R.ln_emulation(case)
    for launch, bw in ((0.0, good[0.0]['bwd']), ('lean', good['lean'])):
        got = {k: bw[k].clone() for k in (('dx32', 'dx') if launch != 'lean' else ('dx32',))}
        for v in got.values():
            v[case.M - 1, D - 4:] = 0
        for k, (v, bar, where) in R.ln_figures(case, got, ref, launch).items():
            print(f'{case.id} {k}: {v:.2e} at row {where} (bar {bar:.2e})')
            assert v >= 2 * bar and where == (case.M - 1,)


@pytest.mark.parametrize('defect', ['cacc', 'mx'])
@pytest.mark.parametrize('case', R.GATE_W64, ids=lambda c: c.id)
def test_defects_d_and_e_at_the_batch_hand_over_are_seen_in_du(case, defect):
    """d: cacc not cleared at a batch boundary; e: the previous batch element's mx and 1 / sm kept after it — ONE wave of the backward
    LN pass, small-variance regime (where du is not noise), seen by du's (b, h) rows (dx's score term is printed beside it)"""
    t, regime = 'fp32', 'small_variance'
    ref = R.gate_reference(case.shape, t, regime)
    bad = R.gate_emulation(case.shape, t, regime, W=case.waves, defect=defect)
    fig = R.gate_figures(case.shape, t, regime, {k: bad[k] for k in ('dx', 'du')}, ref)
    plan = R.gate_plan(*case.shape, case.waves)
    w = plan['crossings'].index(next(c for c in plan['crossings'] if c > 0))
    b_hit = (w * plan['rpw1']) // case.L + 1
    for k, (v, bar, where) in fig.items():
        print(f'{case.id} {defect} {k}: {v:.2e} at {where} (bar {bar:.2e}); the wave hands over into batch element {b_hit}')
    assert fig['du'][0] >= 2 * fig['du'][1] and fig['du'][2][0] == b_hit


@pytest.mark.parametrize('defect', ['cacc', 'mx'])
def test_what_the_default_wave_target_shows_of_the_hand_over(defect):
    """At 4096 waves the one straddling pair leaks ONE row of 2051 into the next batch element's c: the figures are printed for
    profiles/row_kernel_tests.md; whether a (b, h) row moves past its bar depends on that one row's softmax weight, which is why the
    hand-over cases run at 64 waves in a child process"""
    for case in R.GATE_DEFAULT[:2]:
        ref = R.gate_reference(case.shape, 'fp32', 'small_variance')
        bad = R.gate_emulation(case.shape, 'fp32', 'small_variance', W=case.waves, defect=defect)
        fig = R.gate_figures(case.shape, 'fp32', 'small_variance', {k: bad[k] for k in ('dx', 'du')}, ref)
        for k, (v, bar, where) in fig.items():
            print(f'{case.id} {defect} {k}: {v:.2e} at {where} (bar {bar:.2e})')
            assert v == v
