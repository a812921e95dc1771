"""Attention-probability dropout on the device (svol_attn_fwd_dropout / svol_attn_bwd_dropout: attn_fwd_bf16<masked> +
attn_combine_bf16, attn_delta_bf16, attn_bwd_dq_bf16<masked> + attn_dq_finish_bf16, attn_bwd_dkdv_bf16<masked>, their fp16 build and
the fp32 twins of csrc/attention.hip) and LayerNorm's fused dropout, against fp64 under the numpy twin's keep mask
(tests/dropout_twin.py) -- never under a mask the device drew.

  a. parity with the fp64 reference (tests/attn_dropout_ref.py: reference) slice by slice, at the launch plans of
     attn_dropout_ref.CASES; masked keys' gradient rows exactly 0; the dropped result is far from the undropped reference; column
     slices of a packed buffer; the atomic-free plan under SVOL_DETERMINISTIC=1 in a child process.
  b. mask probes: inputs that make o / dV / dQ / dK read the keep mask bit by bit as the forward, the dK/dV kernel's first product,
     the dQ kernel and the dK/dV kernel's second product applied it.  Zero wrong bits, no element left out.
  c. LayerNorm's fused dropout: the kept set against the twin, dx / dgamma / dbeta against fp64 under that mask.

Slice bars (BARS): 3 x the worst slice error, over every case and parameter point of the dtype, of a CPU emulation of the reference
with the operand dtype's roundings at the kernels' rounding sites (attn_dropout_ref.emulate; fp32: the formula in fp32 torch).  The
factor covers accumulation order, the exp2 approximation and the fp32 atomics of the key split.  `python -m tests.attn_dropout_ref`
prints the table; tests/test_attn_dropout_probe.py re-derives the worst point and holds BARS to it.

    dtype   emulation (worst case and point)                      bar       device's worst slice
    bf16    9.66e-3   U1, plain q, p = 0.5, seed 5                2.90e-2   [not measured yet]
    fp16    1.72e-3   S3, plain q, p = 0.5, the model-form seed   5.16e-3   [not measured yet]
    fp32    1.15e-6   S2, premultiplied q, p = 0.5, seed 5        3.45e-6   [not measured yet]

Whole-tensor bars are check_attention's: TOL[dtype] for o, 2 TOL[dtype] for the gradients, its lse2 bars.
"""
from __future__ import annotations

import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attn_dropout_ref as R
from tests.dropout_twin import dropout_keep_numpy

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
# worst slice error of the emulation per dtype, and where (case, premultiplied q, p, seed index)
EMULATED = {BF16: (9.66e-3, ('U1', False, 0.5, 0)), FP16: (1.72e-3, ('S3', False, 0.5, 1)), FP32: (1.15e-6, ('S2', True, 0.5, 0))}
BARS = {dt: 3.0 * e for dt, (e, _) in EMULATED.items()}
# whole-tensor bars of tests/gpu_checks.py: check_attention (TOL and the lse2 bars), kept as literals so that the CPU test of the
# probes can import this module without the device library
TOL = {FP32: 2e-5, BF16: 1.2e-2, FP16: 1.5e-3}
LSE_BAR = {FP32: 1e-5, BF16: 3e-3, FP16: 3e-3}

PARITY = [(n, dt) for dt in (BF16, FP16, FP32) for n in R.cases_of(dt)]
_id = lambda n, dt: f'{n}-{R.DT_NAME[dt]}'


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float('inf')
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def launch(name, q, k, v, do, kb, premul, p, seed, outs=None):
    """one forward + backward through svol_attn_fwd_dropout / svol_attn_bwd_dropout -> o, lse2, dq, dk, dv (device tensors)"""
    from svol_amd import ops
    B, H, Lq, Lk, dh, _ = R.CASES[name]
    qd, kd, vd, dod = (t if t.is_cuda else t.to(DEV) for t in (q, k, v, do))
    kbd = None if kb is None else kb.to(DEV)
    o, lse2 = ops.attn_fwd(qd, kd, vd, B, H, Lq, Lk, dh, kbd, premul, drop=(p, seed))
    dq, dk, dv = outs if outs is not None else (torch.empty((B * Lq, H * dh), dtype=qd.dtype, device=DEV),
                                                torch.empty((B * Lk, H * dh), dtype=qd.dtype, device=DEV),
                                                torch.empty((B * Lk, H * dh), dtype=qd.dtype, device=DEV))
    ops.attn_bwd(qd, kd, vd, o, dod, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbd, premul, drop=(p, seed))
    torch.cuda.synchronize()
    return o, lse2, dq, dk, dv


@functools.lru_cache(maxsize=None)
def reference_of(name, dtype, premul_on, p, seed):
    """inputs and the fp64 reference of one parity point, computed once and shared (never modified)"""
    B, H, Lq, Lk, dh, _ = R.CASES[name]
    pm = R.premuls(dh)[1] if premul_on else 0.0
    q, qref, k, v, do = R.make_inputs(name, dtype, pm)
    kb = R.key_bias(name)
    ref = R.reference(qref, k, v, do, kb, R.keep_mask(name, p, seed), p, (B, H, Lq, Lk, dh))
    return dict(pm=pm, q=q, qref=qref, k=k, v=v, do=do, kb=kb, ref=ref)


@functools.lru_cache(maxsize=None)
def undropped_o(name, dtype, premul_on):
    B, H, Lq, Lk, dh, _ = R.CASES[name]
    c = reference_of(name, dtype, premul_on, R.PS[0], R.SEEDS[0])
    return R.reference(c['qref'], c['k'], c['v'], c['do'], c['kb'], None, 0.0, (B, H, Lq, Lk, dh))[0]


def parity_figures(name, dtype, c, got):
    """every figure of one parity point as {label: (value, bar, 'max' | 'min')}"""
    o, lse2, dq, dk, dv = (t.detach().cpu() for t in got)
    o_r, lse_r, dq_r, dk_r, dv_r = c['ref']
    fig = {}
    sl = R.slice_errors(name, (o, dq, dk, dv), (o_r, dq_r, dk_r, dv_r))
    for tag, r in sl.items():
        fig[f'slice/{tag} {r.where}'] = (r.err if r.finite else math.inf, BARS[dtype], 'max')
    fig['whole/o'] = (rel_err(o, o_r), TOL[dtype], 'max')
    fig['whole/lse2'] = (rel_err(lse2, lse_r), LSE_BAR[dtype], 'max')
    for tag, g, r in (('dq', dq, dq_r), ('dk', dk, dk_r), ('dv', dv, dv_r)):
        fig[f'whole/{tag}'] = (rel_err(g, r), 2 * TOL[dtype], 'max')
    if c['kb'] is not None:   # gradient rows of masked keys: exactly zero
        B, H, Lq, Lk, dh, _ = R.CASES[name]
        gone = (c['kb'] != 0).reshape(B * Lk)
        fig['masked_keys/dk'] = (float(dk[gone].double().abs().max()), 0.0, 'max')
        fig['masked_keys/dv'] = (float(dv[gone].double().abs().max()), 0.0, 'max')
    return fig


def check(fig, what):
    bad = []
    for label, (val, bar, sense) in fig.items():
        ok = (val <= bar) if sense == 'max' else (val > bar)
        print(f'{what} {label}: {val:.3e} ({"<=" if sense == "max" else ">"} {bar:.3e}){"" if ok else "   <-- FAILS"}')
        if not ok:
            bad.append(f'{label}: {val:.3e} vs {bar:.3e}')
    assert not bad, f'{what}: ' + '; '.join(bad)


# ----------------------------------------------------------------------------------------------------------------------
# a. parity
# ----------------------------------------------------------------------------------------------------------------------
def test_whole_tensor_bars_are_check_attentions():
    from tests import gpu_checks as G
    assert TOL == G.TOL


@pytest.mark.parametrize('seed_i', [0, 1], ids=['seed_small', 'seed_model'])
@pytest.mark.parametrize('p', R.PS, ids=lambda p: f'p{p}')
@pytest.mark.parametrize('premul_on', [False, True], ids=['plain', 'premul'])
@pytest.mark.parametrize('name,dtype', PARITY, ids=[_id(*c) for c in PARITY])
def test_parity_with_fp64_by_slice(name, dtype, premul_on, p, seed_i):
    seed = R.SEEDS[seed_i]
    c = reference_of(name, dtype, premul_on, p, seed)
    got = launch(name, c['q'], c['k'], c['v'], c['do'], c['kb'], c['pm'], p, seed)
    assert all(bool(torch.isfinite(t).all()) for t in got), 'not finite'
    fig = parity_figures(name, dtype, c, got)
    # the mask really is applied: the same launch is far from the undropped reference
    o0 = undropped_o(name, dtype, premul_on)
    fig['element error of o against the UNDROPPED reference'] = (rel_err(got[0], o0), 0.1, 'min')
    check(fig, f'{name} {R.DT_NAME[dtype]} premul={premul_on} p={p} seed={seed}')


@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=lambda d: R.DT_NAME[d])
def test_column_slices_of_a_packed_buffer(dtype):
    """q, k, v read as column slices of one packed [M, 3 d] buffer, dq / dk / dv written into column slices of a wider buffer with
    sentinel columns between and after them and sentinel rows below: same bits as the contiguous launch (the plan takes no atomics),
    the reference's bars, nothing written outside the slices."""
    name, p, seed = 'P1', 0.1, R.SEEDS[1]
    B, H, L, _, dh, _ = R.CASES[name]
    d, M, pad = H * dh, B * L, 8
    c = reference_of(name, dtype, True, p, seed)
    qkv = torch.cat([c['q'], c['k'], c['v']], 1).to(DEV)
    buf = torch.full((M + 5, 3 * (d + pad)), 7.0, dtype=dtype, device=DEV)
    sl = [buf[:M, j * (d + pad):j * (d + pad) + d] for j in range(3)]
    got = launch(name, qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], c['do'], None, c['pm'], p, seed, outs=sl)
    plain = launch(name, c['q'], c['k'], c['v'], c['do'], None, c['pm'], p, seed)
    outside = torch.ones_like(buf, dtype=torch.bool)
    for j in range(3):
        outside[:M, j * (d + pad):j * (d + pad) + d] = False
    assert bool((buf[outside] == 7.0).all()), 'written outside the slices'
    for tag, a, b in zip(('o', 'lse2', 'dq', 'dk', 'dv'), got, plain):
        assert torch.equal(a, b), f'{tag}: column-slice launch differs from the contiguous one'
    check(parity_figures(name, dtype, c, got), f'packed {R.DT_NAME[dtype]}')


DET_POINTS = [(n, dt, pm) for n in ('S1', 'S2') for dt in (BF16, FP16) for pm in (False, True)]


def _deterministic_child():
    """runs in a child process under SVOL_DETERMINISTIC=1 (the library reads the variable once): one JSON line per point"""
    p, seed = 0.1, R.SEEDS[1]
    for name, dtype, premul_on in DET_POINTS:
        c = reference_of(name, dtype, premul_on, p, seed)
        a = launch(name, c['q'], c['k'], c['v'], c['do'], c['kb'], c['pm'], p, seed)
        b = launch(name, c['q'], c['k'], c['v'], c['do'], c['kb'], c['pm'], p, seed)
        fig = parity_figures(name, dtype, c, a)
        print('POINT ' + json.dumps(dict(name=name, dtype=R.DT_NAME[dtype], premul=premul_on,
                                         identical=all(torch.equal(x, y) for x, y in zip(a, b)),
                                         finite=all(bool(torch.isfinite(t).all()) for t in a),
                                         fig={k: [v[0], v[1]] for k, v in fig.items()})), flush=True)


def test_deterministic_mode_takes_no_key_split_and_is_bit_reproducible():
    """S1 and S2 once more under SVOL_DETERMINISTIC=1: the backward then takes no key split (dQ by the query-stationary pass over all
    keys, no atomics).  The same bars, and two launches bit-identical."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SVOL_DETERMINISTIC='1', PYTHONPATH=root)
    code = 'from tests.test_gpu_attn_dropout import _deterministic_child as f; f()'
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    pts = [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith('POINT ')]
    assert len(pts) == len(DET_POINTS), r.stdout
    for pt in pts:
        what = f'deterministic {pt["name"]} {pt["dtype"]} premul={pt["premul"]}'
        assert pt['finite'] and pt['identical'], f'{what}: finite={pt["finite"]} identical={pt["identical"]}'
        check({k: (v[0], v[1], 'max') for k, v in pt['fig'].items()}, what)


# ----------------------------------------------------------------------------------------------------------------------
# b. mask probes
# ----------------------------------------------------------------------------------------------------------------------
PROBES = [(n, dt) for n in R.PROBE_CASES for dt in (BF16, FP32)] + [('M1', FP16)]
PROBE_SEED = R.SEEDS[1]


@functools.lru_cache(maxsize=None)
def twin_mask(name):
    return R.keep_mask(name, R.PROBE_P, PROBE_SEED)


@pytest.mark.parametrize('kind', ['fwd', 'dv', 'dq', 'dk'])
@pytest.mark.parametrize('name,dtype', PROBES, ids=[_id(*c) for c in PROBES])
def test_mask_probe_reads_the_twins_bits(name, dtype, kind):
    """every window of every case: each valid (row, key) element of the mask is read once per probe family"""
    def run(q, k, v, do, kb):
        o, _, dq, dk, dv = launch(name, q, k, v, do, kb, 0.0, R.PROBE_P, PROBE_SEED)
        return o, dq, dk, dv
    rec = R.probe(kind, name, run, dtype)
    wrong, missed = rec.mismatches(twin_mask(name), R.expected_seen(name))
    print(f'{name} {R.DT_NAME[dtype]} {kind}: {int(rec.seen.sum())} bits read, {wrong} wrong, {missed} left out')
    assert wrong == 0 and missed == 0, f'{kind} probe on {name}: {wrong} wrong bits, {missed} elements left out'


# ----------------------------------------------------------------------------------------------------------------------
# c. LayerNorm's fused dropout
# ----------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(77, 256), (33, 512), (100, 32), (5, 1024)]


@pytest.mark.parametrize('via', ['host_seed', 'seed_dev'])
@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize('M,D', LN_SHAPES)
def test_layernorm_dropout_against_the_twin(M, D, dtype, via):
    """svol_layernorm_fwd / _bwd with p > 0: the kept set IS the twin's (recovered through beta = 4: |gamma xhat| stays below 4, so a
    kept output is never 0); y, dx, dgamma, dbeta against fp64 under the twin's mask at check_layernorm's bars.  seed_dev: the device-side
    step counter enters as seed + (counter << 8) (csrc/norm.hip)."""
    from oracle import svol_oracle as O
    from svol_amd import ops
    g = torch.Generator().manual_seed(40 + D)
    x = torch.randn((M, D), generator=g).to(dtype)
    gamma = 0.5 + 0.05 * torch.randn((D,), generator=g)
    beta = torch.full((D,), 4.0)
    dy = torch.randn((M, D), generator=g).to(dtype)
    seed0, counter = (9 << 44) + (2 << 12) + 3, 5
    sdev = torch.tensor([counter], dtype=torch.int64, device=DEV) if via == 'seed_dev' else None
    seed_eff = seed0 + (counter << 8) if via == 'seed_dev' else seed0
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    fig = {}
    for p in (0.1, 0.5):
        want = torch.from_numpy(dropout_keep_numpy((M, D), p, seed_eff))
        _, y, _, mean, rstd = ops.layernorm_fwd(xd, gd, bd, dtype, None, p, seed0, seed_dev=sdev)
        _, dx, dg, db = ops.layernorm_bwd(None, dy.to(DEV), None, xd, gd, mean, rstd, dtype, p, seed0, seed_dev=sdev)
        torch.cuda.synchronize()
        kept = y.cpu() != 0
        fig[f'p{p}/wrong keep bits'] = (float((kept != want).sum()), 0.0, 'max')
        x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
        yr = O.layer_norm(x64, g64, b64) * (want.double() / (1.0 - p))
        (yr * dy.double()).sum().backward()
        fig[f'p{p}/y'] = (rel_err(y, yr), TOL[dtype], 'max')
        fig[f'p{p}/dx'] = (rel_err(dx, x64.grad), TOL[dtype], 'max')
        fig[f'p{p}/dgamma'] = (rel_err(dg, g64.grad), 1e-4 if dtype == FP32 else 1e-2, 'max')
        fig[f'p{p}/dbeta'] = (rel_err(db, b64.grad), 1e-4 if dtype == FP32 else 1e-2, 'max')
    check(fig, f'layernorm dropout {M}x{D} {R.DT_NAME[dtype]} {via}')
