"""The row kernels of csrc/norm.hip, csrc/gate.hip and csrc/ln_row.h, case by case: the shapes, what each launch does with them (a
restatement of the launchers' arithmetic), dtype-generic references that run at fp64 (the reference) and at fp32 (an emulation of a
correct kernel: the proof that the inputs leave room under the bars), per-row and per-column metrics, and the bars.  No device code:
tests/test_row_kernel_cases.py runs all of this anywhere, tests/test_gpu_row_kernels.py puts the kernels beside it.

Metrics
    row_err(got, ref)      per row (the last axis): max_c |got - ref| / max_c |ref|; the worst row and its index.  A whole-tensor
                           maximum hides a row that is wrong by 10 % behind the largest row of the tensor.
    col_err(got, ref, S)   per column: |got_c - ref_c| / S_c, S_c the fp64 sum over rows of the ABSOLUTE terms of the column's sum
                           (dgamma: sum |d xhat|, dbeta: sum |d|, colsum: sum rstd (|g| + |s1| + |xhat s2|)).  Where the kernel adds
                           into a pre-filled sink, the fill is a term of that sum like any other and |fill| is part of S_c (a sum of
                           three terms that lands beside a 7.0 is rounded on 7's scale, whatever the kernel does).

Bars (none is taken from a kernel's own figure)
    fp32 row outputs       2e-5 (gate dx 4e-5): the project's fp32 bar (tests/gpu_checks.py), now per row
    16-bit row outputs     half an ulp of the row maximum (2^-8 bf16, 2^-11 fp16: an element is rounded relative to itself, and it is at
                           most its row's maximum) plus the fp32 bar
    mean                   32 * 2^-24 * sum_c |x| / D (about 22 fp32 additions per lane and tree)
    rstd                   1e-5 relative (test_resnet_training_kernels' bar for an rsqrt)
    column reductions      max(32 * 2^-24, 16 x the emulation's worst col_err over the table) per quantity and dtype, capped by 1e-4
                           (fp32) / 1e-2 (16-bit).  EMU_COL below holds the emulation's figures (measure_emulation() prints them); 16
                           because the device sums in another order (lane-serial, four waves through LDS, workgroups by atomics)
                           and consumes its own mean and rstd
    gate scores, a, du     check_gate's: 2e-5 of the (b, h) row's maximum, 1e-4 element by element, 3e-5 of max |dx| per (b, h) row;
                           small-variance regime: y32 5e-5, dx 2e-4 per (b, l) row, du 1e-3 per (b, h) row (a row that is a
                           cancellation residue of its terms is held on their scale: du_row_scale)
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from tests.dropout_twin import dropout_keep_numpy

F64, F32 = torch.float64, torch.float32
DT = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
HALF_ULP = {'fp32': 0.0, 'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}
EPS = 1e-5
SEED0 = (9 << 44) + (2 << 12) + 3
POS_ROWS = 5
FILL = 7.0
P_DROP = 0.1

FP32_ROW = 2e-5
GATE_DX = 4e-5
MEAN_BAR = 32 * 2.0 ** -24
RSTD_BAR = 1e-5
COL_FLOOR = 32 * 2.0 ** -24
COL_CAP = {'fp32': 1e-4, 'bf16': 1e-2, 'fp16': 1e-2}
LIVE_ROW_BAR = 2e-5
SCORES_BAR, A_BAR, DU_ON_DX_BAR = 2e-5, 1e-4, 3e-5
SMALL_VAR = {'y32': 5e-5, 'dx': 2e-4, 'du': 1e-3}

# The emulation's worst col_err over the case tables below (CPU, fp32 against fp64; measure_emulation()), per kernel, quantity and
# output dtype.  The column bars are derived from these and from nothing else.
EMU_COL = {
    ('ln', 'dgamma', 'fp32'): 2.382e-7, ('ln', 'dgamma', 'bf16'): 2.283e-7, ('ln', 'dgamma', 'fp16'): 2.520e-7,
    ('ln', 'dbeta', 'fp32'): 1.040e-7, ('ln', 'dbeta', 'bf16'): 9.329e-8, ('ln', 'dbeta', 'fp16'): 1.034e-7,
    ('ln', 'colsum', 'fp32'): 1.117e-7, ('ln', 'colsum', 'bf16'): 1.094e-7, ('ln', 'colsum', 'fp16'): 1.217e-7,
    ('gate', 'dgamma', 'fp32'): 3.181e-8, ('gate', 'dgamma', 'bf16'): 2.926e-8, ('gate', 'dgamma', 'fp16'): 3.812e-8,   # (both regimes)
    ('gate', 'dbeta', 'fp32'): 1.327e-8, ('gate', 'dbeta', 'bf16'): 1.198e-8, ('gate', 'dbeta', 'fp16'): 1.198e-8,
}


def row_bar(t, base=FP32_ROW):
    return HALF_ULP[t] + base


def col_bar(kernel, quantity, t):
    return min(COL_CAP[t], max(COL_FLOOR, 16.0 * EMU_COL[(kernel, quantity, t)]))


# ---- metrics ------------------------------------------------------------------------------------------------------------------------
def _f64(t):
    return t.detach().to('cpu', F64)


def row_err(got, ref):
    """(worst, index): max over the last axis of |got - ref| over max over the last axis of |ref|, the worst row and its index in
    the leading axes ((row,), (b, l) or (b, h)); inf when got is not finite"""
    got, ref = _f64(got).reshape(ref.shape), _f64(ref)
    if not bool(torch.isfinite(got).all()):
        return float('inf'), None
    num, den = (got - ref).abs().amax(-1), ref.abs().amax(-1)
    # (a row whose reference is all zero — four columns, all dropped — has to come back as exact zeros)
    e = torch.where(den > 0, num / den, torch.where(num > 0, torch.full_like(num, float('inf')), torch.zeros_like(num))).reshape(-1)
    i = int(e.argmax())
    return float(e[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape[:-1]))


def col_err(got, ref, S):
    """(worst, column): |got_c - ref_c| / S_c"""
    got, ref, S = _f64(got), _f64(ref), _f64(S)
    if not bool(torch.isfinite(got).all()):
        return float('inf'), None
    e = (got - ref).abs() / S
    i = int(e.argmax())
    return float(e[i]), i


def scaled_err(got, ref, scale):
    """(worst, index) of |got - ref| / scale element by element: mean against sum |x| / D, rstd and a against themselves, du against
    max |dx|"""
    got, ref = _f64(got).reshape(ref.shape), _f64(ref)
    if not bool(torch.isfinite(got).all()):
        return float('inf'), None
    e = ((got - ref).abs() / scale).reshape(-1)
    i = int(e.argmax())
    return float(e[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))


def whole_tensor_err(got, ref):
    """the metric the older tests use: one number per tensor"""
    got, ref = _f64(got), _f64(ref)
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


# ---- LayerNorm: cases and launch plans -------------------------------------------------------------------------------------------------
RUNGS = {'narrow NP1': (4, 36, 252, 256), 'narrow NP2': (260, 384, 512), 'narrow NP4': (516, 768, 1020, 1024),
         'wide NP2': (1028, 2048), 'wide NP3': (2052, 3072), 'wide NP4': (3076, 4096)}
NARROW = RUNGS['narrow NP1'] + RUNGS['narrow NP2'] + RUNGS['narrow NP4']
WIDTHS = NARROW + RUNGS['wide NP2'] + RUNGS['wide NP3'] + RUNGS['wide NP4']
ALL_PAIRS = (('bf16', 'bf16'), ('bf16', 'fp32'), ('fp16', 'fp16'), ('fp16', 'fp32'), ('fp32', 'fp32'))   # (T, TX)
MANY_ROW_PAIRS = (('bf16', 'fp32'), ('fp16', 'fp16'), ('fp32', 'fp32'))   # the model's stream, and the two uniform ones


@dataclass(frozen=True)
class LnCase:
    M: int
    D: int
    t: str      # dtype of the compute-dtype outputs and gradients
    tx: str     # dtype of x
    claim: str  # what the launch plan must show (tests/test_row_kernel_cases.py asserts it)

    @property
    def id(self):
        return f'{self.M}x{self.D}-{self.t}-x{self.tx}'


def _ln_cases():
    out = []
    for D in WIDTHS:    # one workgroup (narrow) with one idle wave; three one-row workgroups (wide)
        out += [LnCase(3, D, t, tx, 'idle') for t, tx in ALL_PAIRS]
    for D in (4, 1024, 4096):
        out += [LnCase(1, D, t, tx, 'one') for t, tx in MANY_ROW_PAIRS]
    for D in NARROW:    # rpw = 2, 1025 owners, the last owner has one row, the last workgroup one live owner
        out += [LnCase(2049, D, t, tx, 'rpw2') for t, tx in MANY_ROW_PAIRS]
    for D in (36, 260, 1020):   # rpw = 3, 1367 owners
        out += [LnCase(4099, D, t, tx, 'rpw3') for t, tx in MANY_ROW_PAIRS]
    for M, Ds in ((1027, (1028, 2048)), (515, (2052, 3076, 4096))):   # two rows per workgroup, the last workgroup has one
        for D in Ds:
            out += [LnCase(M, D, t, tx, 'wide2') for t, tx in MANY_ROW_PAIRS]
    return out


LN_CASES = _ln_cases()


def _cdiv(a, b):
    return -(-a // b)


def ln_plan(M, D):
    """svol_layernorm_bwd's launch (csrc/norm.hip), restated"""
    wide = D > 1024
    if wide:
        NP = 2 if D <= 2048 else 3 if D <= 3072 else 4
        wgs = 1024 if D <= 2048 else 512
        rpw = max(1, _cdiv(M, wgs))
        owners = _cdiv(M, rpw)
        grid = owners
        live_last = 1
    else:
        NP = 1 if D <= 256 else 2 if D <= 512 else 4
        rpw = max(1, _cdiv(M, 2048))
        owners = _cdiv(M, rpw)
        grid = _cdiv(owners, 4)
        live_last = owners - 4 * (grid - 1)
    return dict(wide=wide, NP=NP, rpw=rpw, owners=owners, grid=grid, rows_last_owner=M - (owners - 1) * rpw, live_owners_last_wg=live_last,
                last_vector_cols=D - 4 * ((D - 1) // 4), passes_used=_cdiv(D, 1024 if wide else 256))


def ln_rung(D):
    return next(k for k, v in RUNGS.items() if v[0] <= D <= v[-1])


def live_rows(M, rpw):
    return sorted({r for r in (0, rpw - 1, rpw, M - 2, M - 1) if 0 <= r < M})


# ---- LayerNorm: inputs and the dtype-generic reference -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def ln_inputs(case):
    M, D = case.M, case.D
    t, tx = DT[case.t], DT[case.tx]
    g = torch.Generator().manual_seed(7000 + 8192 * (M % 97) + D)
    x = torch.randn((M, D), generator=g)
    if M == 1:  # one row: a column "sum" is the single term d xhat, as ill-conditioned as xhat is where x meets the row's mean.  Keep
        x = torch.sign(x) * (0.25 + x.abs())   # |x - mean| >= 0.2, so that the term's own rounding is what the column metric sees
    x = x.to(tx)
    gamma = 0.5 + 0.05 * torch.randn((D,), generator=g)
    beta = torch.full((D,), 4.0)    # a kept output stays away from 0: the kept set is read off y
    pos = torch.randn((POS_ROWS, D), generator=g).to(t)
    dy32 = torch.randn((M, D), generator=g)
    dy = torch.randn((M, D), generator=g).to(t)
    dy2 = torch.randn((M, D), generator=g).to(t)
    return dict(x=x, gamma=gamma, beta=beta, pos=pos, dy32=dy32, dy=dy, dy2=dy2)


def keep_scale(M, D, p, dt):
    """the twin's mask over 1 - p, formed as the kernel forms it (inv_keep = 1.f / (1.f - p) in fp32) when dt is fp32"""
    if p == 0.0:
        return None
    keep = torch.from_numpy(dropout_keep_numpy((M, D), p, SEED0))
    if dt == F32:
        inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
        return keep.to(F32) * inv
    return keep.to(F64) / (1.0 - p)


def colsum(terms, fill=None):
    """row after row (cumsum: the least favourable order at fp32), onto the fill when there is one"""
    if fill is not None:
        terms = torch.cat([torch.full_like(terms[:1], fill), terms])
    return torch.cumsum(terms, 0)[-1]


def ln_stats(xs, dt):
    D = xs.shape[-1]
    mean = xs.sum(-1) / D
    xc = xs - mean[..., None]
    rstd = 1.0 / torch.sqrt((xc * xc).sum(-1) / D + EPS)
    return mean, rstd


def ln_fwd(inp, dt, ks, t_out=None):
    """LayerNorm forward at dtype dt.  t_out: round the compute-dtype outputs to it (the emulation)"""
    x, gamma, beta, pos = (inp[k].to(dt) for k in ('x', 'gamma', 'beta', 'pos'))
    M = x.shape[0]
    mean, rstd = ln_stats(x, dt)
    y32 = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    if ks is not None:
        y32 = y32 * ks
    ypos = y32 + pos[torch.arange(M) % pos.shape[0]]
    y = y32
    if t_out is not None:
        y, ypos = y32.to(t_out), ypos.to(t_out)
    return dict(y32=y32, y=y, ypos=ypos, mean=mean, rstd=rstd)


def ln_bwd(inp, dt, ks, mean, rstd, operands=('dy32', 'dy', 'dy2'), fill=None, t_out=None, with_S=False, d_override=None):
    """LayerNorm backward at dtype dt from the given mean and rstd (the kernel consumes them as operands)"""
    x, gamma = inp['x'].to(dt), inp['gamma'].to(dt)
    D = x.shape[-1]
    if d_override is not None:
        d = d_override.to(dt)
    else:
        d = None
        for k in operands:
            d = inp[k].to(dt) if d is None else d + inp[k].to(dt)
    if ks is not None:
        d = d * ks
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = d * gamma
    s1, s2 = g.sum(-1) / D, (g * xhat).sum(-1) / D
    dx32 = rstd[:, None] * (g - s1[:, None] - xhat * s2[:, None])
    out = dict(dx32=dx32, dx=dx32 if t_out is None else dx32.to(t_out), dgamma=colsum(d * xhat, fill), dbeta=colsum(d, fill),
               colsum=colsum(dx32, fill), d=d, xhat=xhat)
    if with_S:
        f = 0.0 if fill is None else abs(fill)
        out['S'] = dict(dgamma=(d * xhat).abs().sum(0) + f, dbeta=d.abs().sum(0) + f,
                        colsum=(rstd[:, None] * (g.abs() + s1.abs()[:, None] + (xhat * s2[:, None]).abs())).sum(0) + f)
    return out


@functools.lru_cache(maxsize=2)
def ln_reference(case):
    """fp64, from the rounded inputs the kernel sees: forward and the full backward at p = 0 and p = P_DROP (sinks filled with FILL),
    and the lean backward (dy2 only, p = 0, no fill)"""
    inp = ln_inputs(case)
    ref = {}
    for p in (0.0, P_DROP):
        ks = keep_scale(case.M, case.D, p, F64)
        f = ln_fwd(inp, F64, ks)
        ref[p] = dict(fwd=f, bwd=ln_bwd(inp, F64, ks, f['mean'], f['rstd'], fill=FILL, with_S=True), keep=None if ks is None else ks != 0)
    f = ref[0.0]['fwd']
    ref['lean'] = ln_bwd(inp, F64, None, f['mean'], f['rstd'], operands=('dy2',), with_S=True)
    ref['mean_scale'] = inp['x'].double().abs().sum(-1) / case.D
    return ref


def ln_emulation(case, rstd_defect_row=None):
    """fp32, outputs rounded to the output dtype.  rstd_defect_row = r: the backward takes row r's rstd from row r + 1 (planted
    defect a)"""
    inp = ln_inputs(case)
    t = DT[case.t]
    emu = {}
    for p in (0.0, P_DROP):
        ks = keep_scale(case.M, case.D, p, F32)
        f = ln_fwd(inp, F32, ks, t_out=t)
        rstd = f['rstd']
        if rstd_defect_row is not None:
            rstd = rstd.clone()
            rstd[rstd_defect_row] = f['rstd'][rstd_defect_row + 1]
        emu[p] = dict(fwd=f, bwd=ln_bwd(inp, F32, ks, f['mean'], rstd, fill=FILL, t_out=t))
    f = emu[0.0]['fwd']
    emu['lean'] = ln_bwd(inp, F32, None, f['mean'], f['rstd'], operands=('dy2',), t_out=t)
    return emu


def ln_figures(case, got, ref, launch):
    """{label: (value, bar, where)} of one launch's outputs against the fp64 reference.  got: dict with any of y32, y, ypos, mean,
    rstd, dx32, dx, dgamma, dbeta, colsum; launch: 0.0 / P_DROP (the full contract) or 'lean'"""
    fig = {}
    t = case.t
    fwd = ref[launch]['fwd'] if launch != 'lean' else None
    bwd = ref[launch]['bwd'] if launch != 'lean' else ref['lean']
    tag = f'p{launch}' if launch != 'lean' else 'lean'
    for k, bar in (('y32', FP32_ROW), ('y', row_bar(t)), ('ypos', row_bar(t))):
        if k in got:
            fig[f'{tag}/{k}'] = (*row_err(got[k], fwd[k]), bar)
    if 'mean' in got:
        fig[f'{tag}/mean'] = (*scaled_err(got['mean'], fwd['mean'], ref['mean_scale']), MEAN_BAR)
        fig[f'{tag}/rstd'] = (*scaled_err(got['rstd'], fwd['rstd'], fwd['rstd']), RSTD_BAR)
    for k, bar in (('dx32', FP32_ROW), ('dx', row_bar(t))):
        if k in got:
            fig[f'{tag}/{k}'] = (*row_err(got[k], bwd['dx32']), bar)
    for k in ('dgamma', 'dbeta', 'colsum'):
        if k in got:
            fig[f'{tag}/{k}'] = (*col_err(got[k], bwd[k], bwd['S'][k]), col_bar('ln', k, t))
    return {k: (v[0], v[2], v[1]) for k, v in fig.items()}


# ---- the gate: cases and launch plans ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GateCase:
    B: int
    L: int
    D: int
    H: int
    waves: int      # the wave target of the three row-walk kernels (4096 unless SVOL_GATE_WAVES_* say otherwise)
    claim: str

    @property
    def shape(self):
        return (self.B, self.L, self.D, self.H)

    @property
    def id(self):
        return 'B%dL%dD%dH%d' % self.shape


GATE_DEFAULT = [GateCase(2, 2051, 36, 5, 4096, 'pair straddles'),     # two rows per wave in all three row walks; L odd: one wave's pair straddles the boundary
                GateCase(2, 2051, 260, 9, 4096, 'pair straddles'),    # NP = 2, two head groups
                GateCase(1, 4101, 516, 8, 4096, 'rpw2 one video')]    # NP = 4
# SVOL_GATE_WAVES_SC = _LN = _AP = 64 (read once per process: these run in a child)
GATE_W64 = [GateCase(70, 3, 64, 8, 64, 'every wave crosses one'),     # rpw1 = 4 over L = 3: every wave of four rows meets exactly one boundary
            GateCase(150, 2, 64, 8, 64, 'crosses two'),               # rpw1 = 5 over L = 2: every wave meets two boundaries (three batch elements)
            GateCase(3, 50, 260, 9, 64, 'ragged crossing'),           # rpw1 = 3, and 50 is not a multiple of it
            GateCase(2, 333, 36, 32, 64, 'ragged crossing')]          # rpw1 = 11, four head groups
GATE_CASES = GATE_DEFAULT + GATE_W64
GATE_REGIMES = ('unit', 'small_variance')
GATE_DTYPES = ('fp32', 'bf16', 'fp16')


def gate_plan(B, L, D, H, W=4096):
    """svol_gate_fwd's and svol_gate_bwd's launches (csrc/gate.hip), restated.  W: the wave target, floor 64"""
    W = max(W, 64)
    M = B * L
    NP = 1 if D <= 256 else 2 if D <= 512 else 4
    rpw = max(1, _cdiv(L, W // B + 1))                  # score pass and backward apply pass: rows of ONE batch element per wave
    grid_x = _cdiv(L, 4 * rpw)
    rpw1 = max(1, _cdiv(M, W))                          # backward LN pass: rows of the flat [B L] range
    waves1 = _cdiv(M, rpw1)
    crossings = [((min((w + 1) * rpw1, M) - 1) // L) - (w * rpw1) // L for w in range(waves1)]
    return dict(NP=NP, head_groups=_cdiv(H, 8), rpw=rpw, grid_sc=(grid_x, B), live_waves_sc=_cdiv(L, rpw), idle_waves_sc=4 * grid_x - _cdiv(L, rpw),
                rpw1=rpw1, waves1=waves1, grid1=_cdiv(waves1, 4), rows_last_wave1=M - (waves1 - 1) * rpw1,
                max_crossings=max(crossings), waves_crossing=sum(1 for c in crossings if c > 0), crossings=crossings)


def _rnd(shape, dtype, seed, scale=1.0):    # tests/gpu_checks.py::_rnd
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


@functools.lru_cache(maxsize=3)
def gate_inputs(shape, t, regime):
    """check_gate's draws in its two regimes (tests/gpu_checks.py)"""
    B, L, D, H = shape
    dt = DT[t]
    if regime == 'unit':
        x, pos = _rnd((B, L, D), F32, 40), _rnd((B, L, D), dt, 41)
        u = _rnd((B, H, D), F32, 42, 0.2)
        g, b = 1 + 0.1 * _rnd((D,), F32, 43), 0.1 * _rnd((D,), F32, 44)
        grads = dict(dy32=_rnd((B, L, D), F32, 47), dy=_rnd((B, L, D), dt, 45), dyp=_rnd((B, L, D), dt, 46))
    else:   # rows whose variance is below LayerNorm's epsilon and a peaked softmax: the gate is visible, du is of everything's size
        x, pos = 1e-3 * _rnd((B, L, D), F32, 50), _rnd((B, L, D), dt, 51)
        u = _rnd((B, H, D), F32, 52, 8.0 / math.sqrt(D))
        g, b = 1 + 0.1 * _rnd((D,), F32, 53), 0.1 * _rnd((D,), F32, 54)
        grads = dict(dy32=_rnd((B, L, D), F32, 55))
    return dict(x=x, pos=pos, u=u, gamma=g, beta=b, **grads)


def gate_fwd(inp, dt, t_out=None):
    x, pos, u, gamma, beta = (inp[k].to(dt) for k in ('x', 'pos', 'u', 'gamma', 'beta'))
    H = u.shape[1]
    tp = x + pos
    s = torch.einsum('bld,bhd->bhl', tp, u)
    mx = s.amax(-1)
    e = torch.exp(s - mx[..., None])
    sm = e.sum(-1)
    p = e / sm[..., None]
    a = p.sum(1) / H
    xs = x * (1 + a[..., None])
    mean, rstd = ln_stats(xs, dt)
    y32 = (xs - mean[..., None]) * rstd[..., None] * gamma + beta
    ypos = y32 + pos
    y = y32
    if t_out is not None:
        y, ypos = y32.to(t_out), ypos.to(t_out)
    return dict(scores=s, mx=mx, sm=sm, p=p, a=a, xs=xs, mean=mean, rstd=rstd, y32=y32, y=y, ypos=ypos, tp=tp)


def gate_softmax_rows(s, mx, sm):
    return torch.exp(s - mx[..., None]) / sm[..., None]


def gate_bwd_ln(inp, dt, f, with_S=False):
    """pass 1: LN1 backward, dx's first term, da, dgamma, dbeta and c[b, h] = sum_l p da / H"""
    x, gamma = inp['x'].to(dt), inp['gamma'].to(dt)
    B, L, D = x.shape
    H = f['p'].shape[1]
    d = None
    for k in ('dy32', 'dy', 'dyp'):
        if k in inp:
            d = inp[k].to(dt) if d is None else d + inp[k].to(dt)
    a, rstd = f['a'], f['rstd']
    xhat = (f['xs'] - f['mean'][..., None]) * rstd[..., None]
    g = d * gamma
    s1, s2 = g.sum(-1) / D, (g * xhat).sum(-1) / D
    ds1 = rstd[..., None] * (g - s1[..., None] - xhat * s2[..., None])
    da = (ds1 * x).sum(-1)
    out = dict(dx_ln=ds1 * (1 + a[..., None]), da=da, dgamma=colsum((d * xhat).reshape(B * L, D)), dbeta=colsum(d.reshape(B * L, D)),
               cc=(f['p'] * da[:, None, :]).sum(-1) / H)
    if with_S:
        out['S'] = dict(dgamma=(d * xhat).abs().reshape(B * L, D).sum(0), dbeta=d.abs().reshape(B * L, D).sum(0))
    return out


def gate_bwd_apply(inp, dt, f, b1, cc=None):
    """pass 3: dscore = p (da / H - c), dx += dscore u, du = sum_l dscore (x + pos), row after row"""
    u = inp['u'].to(dt)
    H = u.shape[1]
    cc = b1['cc'] if cc is None else cc
    dscore = f['p'] * (b1['da'][:, None, :] / H - cc[..., None])
    dx = b1['dx_ln'] + torch.einsum('bhl,bhd->bld', dscore, u)
    du = torch.cumsum(dscore[..., None] * f['tp'][:, None, :, :], 2)[:, :, -1]
    return dict(dx=dx, du=du)


DU_RESIDUE = 2.0 ** -8


def du_row_scale(f, b1):
    """The denominator of du's per-(b, h) row figure: the row's maximum, as in row_err, but never less than DU_RESIDUE of T, the sum of
    the absolute terms of du[b, h, :] = sum_l p_l (da_l / H - c) (x + pos)_l with c = sum_l p_l da_l / H.  Where the softmax of a
    short video is one-hot, da_l / H - c cancels and the whole row is a residue (1e-13 of its terms at L = 3): no fp32 kernel holds
    that to 1e-3 of itself.  fp32 leaves about 32 * 2^-24 T (the allowance mean and the column floor get), which is 4.9e-4 of
    2^-8 T: half the 1e-3 bar.  A row above 0.4 % of its terms is measured exactly as row_err measures it."""
    H = f['p'].shape[1]
    absda = b1['da'].abs()[:, None, :] / H
    T = (f['p'] * (absda + (f['p'] * absda).sum(-1, keepdim=True)) * f['tp'].abs().amax(-1)[:, None, :]).sum(-1)
    return torch.maximum(b1['du_rowmax'] if 'du_rowmax' in b1 else torch.zeros_like(T), DU_RESIDUE * T)


@functools.lru_cache(maxsize=2)
def gate_reference(shape, t, regime):
    inp = gate_inputs(shape, t, regime)
    f = gate_fwd(inp, F64)
    b1 = gate_bwd_ln(inp, F64, f, with_S=True)
    ref = dict(f)
    ref.update(b1)
    ref.update(gate_bwd_apply(inp, F64, f, b1))
    b1['du_rowmax'] = ref['du'].abs().amax(-1)
    ref['mean_scale'] = f['xs'].abs().sum(-1) / shape[2]
    ref['du_scale'] = du_row_scale(f, b1)
    return ref


def gate_emulation(shape, t, regime, W=None, defect=None):
    """fp32, y and ypos rounded to the output dtype.  defect, with the backward LN pass's wave ranges at wave target W: 'cacc' — the
    first wave that crosses a batch boundary does not clear its c sum there (planted defect d); 'mx' — it keeps the previous batch
    element's max and 1 / sum after the boundary (planted defect e)"""
    inp = gate_inputs(shape, t, regime)
    B, L, D, H = shape
    f = gate_fwd(inp, F32, t_out=DT[t])
    b1 = gate_bwd_ln(inp, F32, f)
    cc = None
    if defect is not None:
        plan = gate_plan(B, L, D, H, W)
        w = next(i for i, c in enumerate(plan['crossings']) if c > 0)
        r0, r1 = w * plan['rpw1'], min((w + 1) * plan['rpw1'], B * L)
        b0 = r0 // L
        before = [r - b0 * L for r in range(r0, r1) if r // L == b0]           # the wave's rows of batch element b0 ...
        after = [r - (b0 + 1) * L for r in range(r0, r1) if r // L == b0 + 1]  # ... and of b0 + 1
        cc = b1['cc'].clone()
        if defect == 'cacc':
            cc[b0 + 1] += (f['p'][b0][:, before] * b1['da'][b0][before]).sum(-1) / H
        elif defect == 'mx':
            wrong = gate_softmax_rows(f['scores'][b0 + 1][:, after], f['mx'][b0], f['sm'][b0])
            cc[b0 + 1] += ((wrong - f['p'][b0 + 1][:, after]) * b1['da'][b0 + 1][after]).sum(-1) / H
        else:
            raise ValueError(defect)
    out = dict(f)
    out.update(b1)
    out.update(gate_bwd_apply(inp, F32, f, b1, cc))
    return out


def gate_figures(shape, t, regime, got, ref):
    """{label: (value, bar, where)}.  got: y32, y, ypos, scores, a, mean, rstd, dx, du, dgamma, dbeta (any subset)"""
    small = regime == 'small_variance'
    fig = {}

    def put(k, val_where, bar):
        fig[k] = (val_where[0], bar, val_where[1])
    for k, bar in (('y32', SMALL_VAR['y32'] if small else FP32_ROW), ('y', row_bar(t, SMALL_VAR['y32'] if small else FP32_ROW)),
                   ('ypos', row_bar(t, SMALL_VAR['y32'] if small else FP32_ROW))):
        if k in got:
            put(k, row_err(got[k], ref['y32'] if k != 'ypos' else ref['ypos']), bar)
    if 'scores' in got:
        put('scores', row_err(got['scores'], ref['scores']), SCORES_BAR)
    if 'a' in got:
        put('a', scaled_err(got['a'], ref['a'], ref['a']), A_BAR)
    if 'mean' in got:
        put('mean', scaled_err(got['mean'], ref['mean'], ref['mean_scale']), MEAN_BAR)
        put('rstd', scaled_err(got['rstd'], ref['rstd'], ref['rstd']), RSTD_BAR)
    if 'dx' in got:
        put('dx', row_err(got['dx'], ref['dx']), SMALL_VAR['dx'] if small else GATE_DX)
    if 'du' in got:
        if small:   # per (b, h) row, a row that is a cancellation residue held on the scale of its terms (du_row_scale)
            e = (_f64(got['du']).reshape(ref['du'].shape) - ref['du']).abs().amax(-1) / ref['du_scale']
            i = int(e.reshape(-1).argmax())
            bad = not bool(torch.isfinite(_f64(got['du'])).all())
            put('du', (float('inf') if bad else float(e.reshape(-1)[i]), (i // shape[3], i % shape[3])), SMALL_VAR['du'])
        else:   # LN1 forgets the per-token scale: du is ~1e-6 of the other gradients, and is held on dx's scale
            e = (_f64(got['du']).reshape(ref['du'].shape) - ref['du']).abs().amax(-1) / float(ref['dx'].abs().max())
            i = int(e.reshape(-1).argmax())
            bad = not bool(torch.isfinite(_f64(got['du'])).all())
            put('du_vs_dx_scale', (float('inf') if bad else float(e.reshape(-1)[i]), (i // shape[3], i % shape[3])), DU_ON_DX_BAR)
    for k in ('dgamma', 'dbeta'):
        if k in got:
            put(k, col_err(got[k], ref[k], ref['S'][k]), col_bar('gate', k, t))
    return fig


# ---- the emulation's figures: what EMU_COL and profiles/row_kernel_tests.md hold ----------------------------------------------------------
def ln_emulation_figures(case):
    ref, emu = ln_reference(case), ln_emulation(case)
    fig = {}
    for launch in (0.0, P_DROP):
        got = dict(emu[launch]['fwd'])
        got.update({k: emu[launch]['bwd'][k] for k in ('dx32', 'dx', 'dgamma', 'dbeta', 'colsum')})
        fig.update(ln_figures(case, got, ref, launch))
    fig.update(ln_figures(case, {k: emu['lean'][k] for k in ('dx32', 'dgamma', 'dbeta')}, ref, 'lean'))
    return fig


GATE_KEYS = ('y32', 'y', 'ypos', 'scores', 'a', 'mean', 'rstd', 'dx', 'du', 'dgamma', 'dbeta')


def gate_emulation_figures(case, t, regime):
    ref, emu = gate_reference(case.shape, t, regime), gate_emulation(case.shape, t, regime)
    return gate_figures(case.shape, t, regime, {k: emu[k] for k in GATE_KEYS}, ref)


def measure_emulation(verbose=True):
    """the worst emulation figure per kernel, quantity and output dtype over the tables: python -m tests.row_kernel_cases"""
    worst = {}

    def take(kernel, t, fig):
        for k, (v, _bar, _where) in fig.items():
            q = k.split('/')[-1]
            worst[(kernel, q, t)] = max(worst.get((kernel, q, t), 0.0), v)
    for case in LN_CASES:
        take('ln', case.t, ln_emulation_figures(case))
    for case in GATE_CASES:
        for t in GATE_DTYPES:
            for regime in GATE_REGIMES:
                take('gate/' + regime, t, gate_emulation_figures(case, t, regime))
    if verbose:
        for k in sorted(worst):
            print(k, f'{worst[k]:.3e}')
    return worst


if __name__ == '__main__':
    measure_emulation()
