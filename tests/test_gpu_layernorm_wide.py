"""svol_layernorm_fwd / _bwd on rows of 1024 < D <= 4096 columns (csrc/norm.hip: lnw_fwd_kernel and the WPR = 4 instances of ln_bwd_kernel, one
workgroup of four waves per row) against fp64.

The method is test_gpu_attn_dropout.py::test_layernorm_dropout_against_the_twin's: beta = 4 keeps a kept output away from 0, so the
kept set is read off y and compared with the numpy twin of the keep function (tests/dropout_twin.py); y / dx / dgamma / dbeta are
compared with fp64 under the TWIN's mask.  Bars: that test's — TOL[dtype] for y and dx, 1e-4 (fp32) / 1e-2 (16-bit) for the column
reductions, 0 wrong keep bits.

    (1, 2048)      the pooled sketch row of a 2048-d extractor
    (5, 1028)      first width above the one-wave-per-row limit, ragged last vector (NV = 2)
    (9, 1536)      concat_to_seq on ViT features
    (7, 2048)      NV = 2, full
    (3, 4096)      NV = 4, the widest row
    (2051, 1280)   three rows per workgroup in the backward (684 of them), two rows in the last one
(5, 2560) in the variants reaches NV = 3.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest
import torch

from tests.dropout_twin import dropout_keep_numpy
from tests.guard_arena import FILLS, GuardArena

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
DT_NAME = {BF16: 'bf16', FP16: 'fp16', FP32: 'fp32'}
TOL = {FP32: 2e-5, BF16: 1.2e-2, FP16: 1.5e-3}          # tests/gpu_checks.py TOL, as test_layernorm_dropout_against_the_twin uses it
RED = {FP32: 1e-4, BF16: 1e-2, FP16: 1e-2}              # dgamma / dbeta / colsum
SHAPES = [(1, 2048), (5, 1028), (9, 1536), (7, 2048), (3, 4096), (2051, 1280)]
SEED0, COUNTER = (9 << 44) + (2 << 12) + 3, 5


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float('inf')
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def check(fig, what):
    bad = []
    for label, (val, bar) in fig.items():
        ok = val <= bar
        print(f'{what} {label}: {val:.3e} (<= {bar:.3e}){"" if ok else "   <-- FAILS"}')
        if not ok:
            bad.append(f'{label}: {val:.3e} vs {bar:.3e}')
    assert not bad, f'{what}: ' + '; '.join(bad)


def test_bars_are_the_narrow_tests():
    from tests import gpu_checks as G
    assert TOL == G.TOL


def make(M, D, dtype, x_dtype=None, beta4=True, seed=0):
    g = torch.Generator().manual_seed(40 + D + seed)
    x = torch.randn((M, D), generator=g).to(x_dtype or dtype)
    gamma = 0.5 + 0.05 * torch.randn((D,), generator=g)
    beta = torch.full((D,), 4.0) if beta4 else 0.1 * torch.randn((D,), generator=g)
    dy = torch.randn((M, D), generator=g).to(dtype)
    return x, gamma, beta, dy


def ln64(x64, g64, b64):
    mu = x64.mean(-1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
    return (x64 - mu) / torch.sqrt(var + 1e-5) * g64 + b64


def test_the_fp64_formula_is_the_oracles():
    from oracle import svol_oracle as O
    x, gamma, beta, _ = make(4, 1536, FP32, beta4=False)
    assert rel_err(ln64(x.double(), gamma.double(), beta.double()), O.layer_norm(x.double(), gamma.double(), beta.double())) < 1e-13


@pytest.mark.parametrize('via', ['host_seed', 'seed_dev'])
@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=lambda d: DT_NAME[d])
@pytest.mark.parametrize('M,D', SHAPES)
def test_wide_layernorm_against_fp64_under_the_twins_mask(M, D, dtype, via):
    from svol_amd import ops
    x, gamma, beta, dy = make(M, D, dtype)
    sdev = torch.tensor([COUNTER], dtype=torch.int64, device=DEV) if via == 'seed_dev' else None
    seed_eff = SEED0 + (COUNTER << 8) if via == 'seed_dev' else SEED0
    xd, gd, bd, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
    fig = {}
    for p in (0.0, 0.1, 0.5):
        want = torch.from_numpy(dropout_keep_numpy((M, D), p, seed_eff)) if p > 0 else torch.ones((M, D), dtype=torch.bool)
        _, y, _, mean, rstd = ops.layernorm_fwd(xd, gd, bd, dtype, None, p, SEED0, seed_dev=sdev)
        _, dx, dg, db = ops.layernorm_bwd(None, dyd, None, xd, gd, mean, rstd, dtype, p, SEED0, seed_dev=sdev)
        torch.cuda.synchronize()
        fig[f'p{p}/wrong keep bits'] = (float(((y.cpu() != 0) != want).sum()), 0.0)
        x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
        yr = ln64(x64, g64, b64) * (want.double() / (1.0 - p))
        (yr * dy.double()).sum().backward()
        fig[f'p{p}/y'] = (rel_err(y, yr), TOL[dtype])
        fig[f'p{p}/dx'] = (rel_err(dx, x64.grad), TOL[dtype])
        fig[f'p{p}/dgamma'] = (rel_err(dg, g64.grad), RED[dtype])
        fig[f'p{p}/dbeta'] = (rel_err(db, b64.grad), RED[dtype])
    check(fig, f'wide layernorm {M}x{D} {DT_NAME[dtype]} {via}')


VM, VD = 9, 1536


@pytest.mark.parametrize('D', [VD, 2560])
@pytest.mark.parametrize('dtype', [BF16, FP16], ids=lambda d: DT_NAME[d])
def test_fp32_input_with_16bit_outputs_every_output_and_gradient_operand(dtype, D):
    """x_f32 = 1; y32 + y + ypos with pos_rows = 3 < M; dy32 + dy + dy2 together to dx32 + dx; dx_colsum; every reduction destination
    pre-filled with 7: the kernels ACCUMULATE into them.  p = 0.1 through the device-side counter."""
    from svol_amd import ops
    M, p = VM, 0.1
    x, gamma, beta, dy = make(M, D, dtype, x_dtype=FP32, beta4=False)
    g = torch.Generator().manual_seed(5)
    pos = torch.randn((3, D), generator=g).to(dtype)
    dy32 = torch.randn((M, D), generator=g)
    dy2 = torch.randn((M, D), generator=g).to(dtype)
    sdev = torch.tensor([COUNTER], dtype=torch.int64, device=DEV)
    want = torch.from_numpy(dropout_keep_numpy((M, D), p, SEED0 + (COUNTER << 8))).double() / (1.0 - p)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y32, y, ypos, mean, rstd = ops.layernorm_fwd(xd, gd, bd, dtype, pos.to(DEV), p, SEED0, want32=True, seed_dev=sdev)
    sinks = [torch.full((D,), 7.0, device=DEV) for _ in range(3)]
    dx32, dx, dg, db, cs = ops.layernorm_bwd(dy32.to(DEV), dy.to(DEV), dy2.to(DEV), xd, gd, mean, rstd, dtype, p, SEED0, want32=True,
                                             want_colsum=True, seed_dev=sdev, dg_out=sinks[0], db_out=sinks[1], cs_out=sinks[2])
    torch.cuda.synchronize()
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    yr = ln64(x64, g64, b64) * want
    dsum = dy32.double() + dy.double() + dy2.double()
    (yr * dsum).sum().backward()
    posr = pos.double()[torch.arange(M) % 3]
    fig = {'y32': (rel_err(y32, yr), TOL[FP32]), 'y': (rel_err(y, yr), TOL[dtype]), 'ypos': (rel_err(ypos, yr.detach() + posr), TOL[dtype]),
           'dx32': (rel_err(dx32, x64.grad), TOL[FP32]), 'dx': (rel_err(dx, x64.grad), TOL[dtype]),
           'dgamma - 7': (rel_err(dg - 7.0, g64.grad), RED[dtype]), 'dbeta - 7': (rel_err(db - 7.0, b64.grad), RED[dtype]),
           # check_layernorm's dx_colsum figure: the column sums of dx cancel, so the error is set against max|dx| sqrt(M)
           'colsum - 7': (float((cs.double().cpu() - 7.0 - x64.grad.sum(0)).abs().max()) / (float(x64.grad.abs().max()) * M ** 0.5), RED[dtype])}
    check(fig, f'variants {M}x{D} {DT_NAME[dtype]}')


def test_limits_4100_and_4098_refused_1024_runs():
    from svol_amd import _lib, ops
    for D in (4100, 4098, 8192):
        x = torch.zeros((2, D), device=DEV)
        w = torch.ones((D,), device=DEV)
        with pytest.raises(_lib.SvolHipError, match='not supported'):
            ops.layernorm_fwd(x, w, w, FP32)
        with pytest.raises(_lib.SvolHipError, match='not supported'):
            ops.layernorm_bwd(None, x, None, x, w, torch.zeros(2, device=DEV), torch.ones(2, device=DEV), FP32)
    x, gamma, beta, dy = make(6, 1024, FP32, beta4=False)
    _, y, _, mean, rstd = ops.layernorm_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), FP32)
    assert rel_err(y, ln64(x.double(), gamma.double(), beta.double())) <= TOL[FP32]


@pytest.mark.parametrize('dtype', [BF16, FP32], ids=lambda d: DT_NAME[d])
@pytest.mark.parametrize('M,D', [(5, 1028), (7, 2048)])
def test_wide_layernorm_stays_inside_its_operands(M, D, dtype):
    """red zones around every output, hostile fills (-0.0, NaN, huge) around every input: the guards come back bit-identical, the
    results are finite, meet fp64 and do not change with the fill"""
    from svol_amd import _lib, ops
    lib, P = _lib.lib(), ops._ptr
    x, gamma, beta, dy = make(M, D, dtype, beta4=False)
    g = torch.Generator().manual_seed(11)
    pos = torch.randn((2, D), generator=g).to(dtype)
    dy32 = torch.randn((M, D), generator=g)
    ins = GuardArena()
    for nm, t in (('x', x), ('gamma', gamma), ('beta', beta), ('pos', pos), ('dy32', dy32), ('dy', dy)):
        ins.plan(nm, t.shape, t.dtype)
    i = ins.build()
    for nm, t in (('x', x), ('gamma', gamma), ('beta', beta), ('pos', pos), ('dy32', dy32), ('dy', dy)):
        i[nm].copy_(t)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    yr = ln64(x64, g64, b64)
    (yr * (dy32.double() + dy.double())).sum().backward()
    first = None
    for fill_name, word in FILLS:
        ins.refill(word)
        out = GuardArena()
        for nm in ('y32', 'dx32'):
            out.plan(nm, (M, D), FP32)
        for nm in ('y', 'ypos', 'dx'):
            out.plan(nm, (M, D), dtype)
        for nm in ('mean', 'rstd'):
            out.plan(nm, (M,), FP32)
        for nm in ('dgamma', 'dbeta', 'colsum'):
            out.plan(nm, (D,), FP32)
        o = out.build()
        for nm in ('dgamma', 'dbeta', 'colsum'):
            o[nm].zero_()
        dt, s = ops._DT[dtype], ops._stream()
        _lib.check(lib.svol_layernorm_fwd(P(i['x']), 0, P(i['gamma']), P(i['beta']), P(o['y32']), P(o['y']), P(o['ypos']), P(i['pos']), 2,
                                          P(o['mean']), P(o['rstd']), M, D, 0.0, 0, None, dt, s), 'svol_layernorm_fwd')
        _lib.check(lib.svol_layernorm_bwd(P(i['dy32']), P(i['dy']), None, P(i['x']), 0, P(i['gamma']), P(o['mean']), P(o['rstd']), P(o['dx32']),
                                          P(o['dx']), P(o['dgamma']), P(o['dbeta']), P(o['colsum']), M, D, 0.0, 0, None, dt, s), 'svol_layernorm_bwd')
        torch.cuda.synchronize()
        out.check(f'outputs, {fill_name} fill')
        ins.check(f'inputs, {fill_name} fill')
        got = {k: v.clone() for k, v in o.items()}
        for k, v in got.items():
            assert bool(torch.isfinite(v.float()).all()), f'{k} not finite under the {fill_name} fill'
        check({'y32': (rel_err(got['y32'], yr), TOL[dtype]), 'dx32': (rel_err(got['dx32'], x64.grad), TOL[dtype]),
               'dgamma': (rel_err(got['dgamma'], g64.grad), RED[dtype]), 'dbeta': (rel_err(got['dbeta'], b64.grad), RED[dtype])},
              f'guarded {M}x{D} {DT_NAME[dtype]} {fill_name}')
        if first is None:
            first = got
        else:   # (the row outputs have one writer each; the column sinks take atomics from several workgroups and may differ in the last bit)
            for k in ('y32', 'y', 'ypos', 'mean', 'rstd', 'dx32', 'dx'):
                assert torch.equal(first[k], got[k]), f'{k} changes with the fill around the inputs'


def _deterministic_child():
    from svol_amd import ops
    M, D, p = 2051, 1280, 0.1
    for dtype in (BF16, FP32):
        x, gamma, beta, dy = make(M, D, dtype, beta4=False)
        xd, gd, bd, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
        _, y, _, mean, rstd = ops.layernorm_fwd(xd, gd, bd, dtype, None, p, SEED0)
        runs = [ops.layernorm_bwd(None, dyd, None, xd, gd, mean, rstd, dtype, p, SEED0, want_colsum=True) for _ in range(2)]
        torch.cuda.synchronize()
        want = torch.from_numpy(dropout_keep_numpy((M, D), p, SEED0)).double() / (1.0 - p)
        x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
        (ln64(x64, g64, b64) * want * dy.double()).sum().backward()
        _, dx, dg, db, cs = runs[0]
        print('POINT ' + json.dumps(dict(dtype=DT_NAME[dtype], identical=all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:])),
                                         dx=rel_err(dx, x64.grad), dgamma=rel_err(dg, g64.grad), dbeta=rel_err(db, b64.grad))), flush=True)


def test_deterministic_mode_folds_the_wide_column_reductions_in_index_order():
    """SVOL_DETERMINISTIC=1 (read once per process: a child): 684 workgroups' partial rows through DetScratch / det_fold — the same bars,
    two launches bit-identical"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SVOL_DETERMINISTIC='1', PYTHONPATH=root)
    code = 'from tests.test_gpu_layernorm_wide import _deterministic_child as f; f()'
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    pts = [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith('POINT ')]
    assert len(pts) == 2, r.stdout
    for pt in pts:
        dt = {v: k for k, v in DT_NAME.items()}[pt['dtype']]
        assert pt['identical'], pt
        check({'dx': (pt['dx'], TOL[dt]), 'dgamma': (pt['dgamma'], RED[dt]), 'dbeta': (pt['dbeta'], RED[dt])}, f'deterministic {pt["dtype"]}')
