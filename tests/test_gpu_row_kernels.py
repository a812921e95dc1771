"""The row kernels against fp64, row by row and column by column (tests/row_kernel_cases.py: the cases, their launch plans, the
references, the metrics and the bars; tests/test_row_kernel_cases.py proves on the CPU that the plans reach what they claim, that a
correct fp32 kernel has room under every bar, and that the metrics see five planted defects).

LayerNorm, through ops.layernorm_fwd / ops.layernorm_bwd (csrc/norm.hip, csrc/ln_row.h), per case:
    1. the full contract at p = 0 and p = 0.1 under the twin's mask: pos with 5 rows; y32, y, ypos; dy32 + dy + dy2 to dx32 + dx;
       dx_colsum; the three sinks pre-filled with 7
    2. the lean launch: dy2 alone to dx32 alone, no colsum
    3. (many-row cases) one live row: dy zero but for row r in {0, rpw - 1, rpw, M - 2, M - 1} — every other row of dx is exactly 0.0
       and the three column sums are their single term
The gate, through layers.gate and autograd (csrc/gate.hip), in check_gate's two regimes: in-process at the default wave targets, and
in a child process at SVOL_GATE_WAVES_SC = _LN = _AP = 64 (read once per process), where a wave's row range of the backward LN pass
crosses one or two batch boundaries; a second child adds SVOL_DETERMINISTIC=1 and asks two backward runs for the same bits.

Every figure is printed beside its bar with the row or column it comes from."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import row_kernel_cases as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def check(fig, what):
    bad = []
    for label, (val, bar, where) in fig.items():
        ok = val <= bar
        print(f'{what} {label}: {val:.3e} (<= {bar:.3e}) at {where}{"" if ok else "   <-- FAILS"}')
        if not ok:
            bad.append(f'{label}: {val:.3e} vs {bar:.3e} at {where}')
    assert not bad, f'{what}: ' + '; '.join(bad)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
def _ln_forward(case, d, p):
    from svol_amd import ops
    return ops.layernorm_fwd(d['x'], d['gamma'], d['beta'], R.DT[case.t], d['pos'], p, R.SEED0, want32=True)


@pytest.mark.parametrize('case', R.LN_CASES, ids=lambda c: c.id)
def test_layernorm_rows_and_columns_against_fp64(case):
    from svol_amd import ops
    t, D = R.DT[case.t], case.D
    inp, ref = R.ln_inputs(case), R.ln_reference(case)
    d = {k: v.to(DEV) for k, v in inp.items()}
    fig, stats0 = {}, None
    for p in (0.0, R.P_DROP):
        y32, y, ypos, mean, rstd = _ln_forward(case, d, p)
        sinks = [torch.full((D,), R.FILL, device=DEV) for _ in range(3)]
        dx32, dx, dg, db, cs = ops.layernorm_bwd(d['dy32'], d['dy'], d['dy2'], d['x'], d['gamma'], mean, rstd, t, p, R.SEED0, want32=True,
                                                 want_colsum=True, dg_out=sinks[0], db_out=sinks[1], cs_out=sinks[2])
        torch.cuda.synchronize()
        assert dg is sinks[0] and db is sinks[1] and cs is sinks[2]
        if p > 0:
            fig[f'p{p}/wrong keep bits'] = (float(((y32.cpu() != 0) != ref[p]['keep']).sum()), 0.0, None)
        else:
            stats0 = (mean, rstd)
        fig.update(R.ln_figures(case, dict(y32=y32, y=y, ypos=ypos, mean=mean, rstd=rstd, dx32=dx32, dx=dx, dgamma=dg, dbeta=db, colsum=cs),
                                ref, p))
    dx32, dx, dg, db = ops.layernorm_bwd(None, None, d['dy2'], d['x'], d['gamma'], stats0[0], stats0[1], t, want32=True, want_t=False)
    torch.cuda.synchronize()
    assert dx is None
    fig.update(R.ln_figures(case, dict(dx32=dx32, dgamma=dg, dbeta=db), ref, 'lean'))
    assert len(fig) == 2 * 10 + 1 + 3
    check(fig, f'layernorm {case.id}')


@pytest.mark.parametrize('case', [c for c in R.LN_CASES if c.M > 3], ids=lambda c: c.id)
def test_layernorm_one_live_row(case):
    """dy is zero except in row r: every other row of dx32 and dx is exactly 0.0, and dgamma, dbeta and the column sums of dx are the
    single terms d_r xhat_r, d_r and dx_r — with one term there is no order of summation to allow for"""
    from svol_amd import ops
    t, M, D = R.DT[case.t], case.M, case.D
    inp, ref = R.ln_inputs(case), R.ln_reference(case)
    d = {k: v.to(DEV) for k, v in inp.items()}
    _, _, _, mean, rstd = _ln_forward(case, d, 0.0)
    f64 = ref[0.0]['fwd']
    fig = {}
    for r in R.live_rows(M, R.ln_plan(M, D)['rpw']):
        dy = torch.zeros((M, D), dtype=t, device=DEV)
        dy[r] = d['dy'][r]
        dx32, dx, dg, db, cs = ops.layernorm_bwd(None, dy, None, d['x'], d['gamma'], mean, rstd, t, want32=True, want_colsum=True)
        torch.cuda.synchronize()
        others = torch.arange(M, device=DEV) != r
        fig[f'r{r}/non-zero dx32 outside the row'] = (float((dx32[others] != 0).sum()), 0.0, None)
        fig[f'r{r}/non-zero dx outside the row'] = (float((dx[others] != 0).sum()), 0.0, None)
        one = R.ln_bwd({'x': inp['x'][r:r + 1], 'gamma': inp['gamma']}, R.F64, None, f64['mean'][r:r + 1], f64['rstd'][r:r + 1],
                       d_override=inp['dy'][r:r + 1])
        for k, got, want in (('dgamma', dg, one['d'][0] * one['xhat'][0]), ('dbeta', db, one['d'][0]), ('colsum', cs, one['dx32'][0]),
                             ('dx32 row', dx32[r], one['dx32'][0])):
            err = (got.double().cpu() - want).abs()
            fig[f'r{r}/{k}'] = (float(err.max() / want.abs().max()) if bool(torch.isfinite(got).all()) else float('inf'), R.LIVE_ROW_BAR,
                                int(err.argmax()))
    check(fig, f'one live row {case.id}')


# ---- the gate -----------------------------------------------------------------------------------------------------------------------------
def gate_device(shape, t, regime):
    """forward and backward of layers.gate on check_gate's draws: the outputs, what GateFn saved (scores, a, mean, rstd) and the four
    gradients, on the host"""
    from svol_amd import layers
    B, L, D, H = shape
    inp = R.gate_inputs(shape, t, regime)
    leaf = {k: inp[k].to(DEV).requires_grad_(True) for k in ('x', 'u', 'gamma', 'beta')}
    y32, y, ypos = layers.gate(leaf['x'], inp['pos'].to(DEV), leaf['u'], leaf['gamma'], leaf['beta'], H)
    sv = y32.grad_fn.saved_tensors   # GateFn: (x2, pos2, u, gamma, a, mean, rstd, ws); the scores come first in ws
    got = dict(y32=y32, y=y, ypos=ypos, scores=sv[7][:B * H * L].view(B, H, L).clone(), a=sv[4].view(B, L).clone(),
               mean=sv[5].view(B, L).clone(), rstd=sv[6].view(B, L).clone())
    pairs = [(o, inp[k].to(DEV)) for o, k in ((y32, 'dy32'), (y, 'dy'), (ypos, 'dyp')) if k in inp]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    torch.cuda.synchronize()
    got.update(dx=leaf['x'].grad, du=leaf['u'].grad, dgamma=leaf['gamma'].grad, dbeta=leaf['beta'].grad)
    return {k: v.detach().cpu() for k, v in got.items()}


@pytest.mark.parametrize('regime', R.GATE_REGIMES)
@pytest.mark.parametrize('t', R.GATE_DTYPES)
@pytest.mark.parametrize('case', R.GATE_DEFAULT, ids=lambda c: c.id)
def test_gate_rows_and_columns_against_fp64(case, t, regime):
    """two rows per wave in the score pass, the backward LN pass and the backward apply pass (the default 4096 waves)"""
    assert 'SVOL_GATE_WAVES_LN' not in os.environ and 'SVOL_GATE_WAVES_SC' not in os.environ and 'SVOL_GATE_WAVES_AP' not in os.environ
    got = gate_device(case.shape, t, regime)
    fig = R.gate_figures(case.shape, t, regime, got, R.gate_reference(case.shape, t, regime))
    assert len(fig) == len(R.GATE_KEYS)
    check(fig, f'gate {case.id} {t} {regime}')


def _gate_child():
    det = os.environ.get('SVOL_DETERMINISTIC') == '1'
    for case in R.GATE_W64:
        for t in R.GATE_DTYPES:
            for regime in R.GATE_REGIMES:
                got = gate_device(case.shape, t, regime)
                fig = R.gate_figures(case.shape, t, regime, got, R.gate_reference(case.shape, t, regime))
                same = None
                if det:
                    again = gate_device(case.shape, t, regime)
                    same = all(torch.equal(got[k], again[k]) for k in ('dx', 'du', 'dgamma', 'dbeta'))
                print('CASE ' + json.dumps(dict(id=case.id, t=t, regime=regime, identical=same, fig=fig)), flush=True)


def _run_gate_child(extra_env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SVOL_GATE_WAVES_SC='64', SVOL_GATE_WAVES_LN='64', SVOL_GATE_WAVES_AP='64', PYTHONPATH=root, **extra_env)
    r = subprocess.run([sys.executable, '-c', 'from tests.test_gpu_row_kernels import _gate_child as f; f()'], env=env,
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    pts = [json.loads(ln[5:]) for ln in r.stdout.splitlines() if ln.startswith('CASE ')]
    assert len(pts) == len(R.GATE_W64) * len(R.GATE_DTYPES) * len(R.GATE_REGIMES), r.stdout[-3000:]
    return pts


def _check_points(pts, what):
    bad = []
    for pt in pts:
        assert len(pt['fig']) == len(R.GATE_KEYS), pt
        try:
            check({k: tuple(v) for k, v in pt['fig'].items()}, f'{what} {pt["id"]} {pt["t"]} {pt["regime"]}')
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, '\n'.join(bad)


def test_gate_hand_over_across_batch_boundaries_at_64_waves():
    """64 waves: (70, 3, 64, 8) every wave of the backward LN pass hands over once, (150, 2, 64, 8) twice (three batch elements per
    wave), (3, 50, 260, 9) and (2, 333, 36, 32) at a ragged place; the score pass takes a whole short video per wave"""
    _check_points(_run_gate_child({}), 'gate/64 waves')


def test_gate_hand_over_in_deterministic_mode():
    """... and with SVOL_DETERMINISTIC=1: the det_cc rows are indexed by batch element; same bars, two runs bit-identical"""
    pts = _run_gate_child({'SVOL_DETERMINISTIC': '1'})
    assert all(pt['identical'] is True for pt in pts), [(pt['id'], pt['t'], pt['regime']) for pt in pts if pt['identical'] is not True]
    _check_points(pts, 'gate/64 waves/deterministic')
