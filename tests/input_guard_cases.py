"""The case tables of tests/test_gpu_input_guards.py: every C-ABI entry of the hot path at the smallest shapes that reach its edge
handling, with all of its INPUT operands described as slots of one hostile arena (tests/guard_arena.py) and its fp64 reference as
plain torch.  Importable without the device library; tests/test_input_guard_cases.py holds it to the dispatch twins on the CPU.

A case is a Spec:
    ins    name -> In(tensor, ld, col, slot): a dense buffer, a column slice of rows `ld` elements apart (everything else in those
           rows is a gap word of the arena), or -- with `slot` -- one column range of a PACKED buffer shared with other operands
           (q | k | v of one [M, 3d] buffer: the neighbours of a row's k columns are its own q and v)
    outs   name -> Out(shape, dtype, ld, col, init, slot, scratch): init None = poisoned with NaN before every run (an output the
           kernel must write), a tensor = the accumulation target's start values; scratch = no reference
    ref    spec -> {output name: fp64 tensor}, from the rounded inputs the kernel sees
    bars   output name -> (tolerance, metric): the bars of tests/gpu_checks.py for that op and dtype
    biteq  the outputs must not change by a bit when the arena's fill changes (entries the suite holds to run-to-run bit equality)
Inputs are drawn as tests/gpu_checks.py's _rnd draws them.
"""
from __future__ import annotations

import functools
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from tests import attn_cls_cases as CLS
from tests import attn_range_cases as A
from tests import attn_small_cases as SM
from tests import attn_wide_range_cases as W

FP32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
TOL = {FP32: 2e-5, BF16: 1.2e-2, FP16: 1.5e-3}          # tests/gpu_checks.py TOL
DT_NAME = {FP32: 'fp32', BF16: 'bf16', FP16: 'fp16'}
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID, ACT_RELU_RES, ACT_GELU_D = 0, 1, 2, 3, 4, 5
LOG2E = 1.4426950408889634
NOMINAL_CUS = 256          # the MI355X's compute units: what the CPU test sizes the balanced GEMM case with


def _rnd(shape, dtype, seed, scale=1.0):
    """tests/gpu_checks.py _rnd"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


class In:
    def __init__(self, t, ld=None, col=0, slot=None):
        self.t, self.ld, self.col, self.slot = t, ld, col, slot


class Out:
    def __init__(self, shape, dtype, ld=None, col=0, init=None, slot=None, scratch=False):
        self.shape, self.dtype, self.ld, self.col, self.init, self.slot, self.scratch = tuple(shape), dtype, ld, col, init, slot, scratch


class Spec:
    def __init__(self, family, name, entry, dtype, dims, ins, outs, ref, bars, biteq=False, plan=None):
        self.family, self.name, self.entry, self.dtype, self.dims = family, name, entry, dtype, dims
        self.ins, self.outs, self._ref, self.bars, self.biteq, self.plan = ins, outs, ref, bars, biteq, plan

    @property
    def id(self):
        return f'{self.entry}/{self.name}/{DT_NAME[self.dtype]}'

    def x(self, name):
        """an input as fp64"""
        return self.ins[name].t.double()

    def ref(self):
        return self._ref(self)


# ---- metrics (tests/gpu_checks.py) -------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """max |got - ref| / max |ref|: gpu_checks.rel_err"""
    if not torch.isfinite(got).all():
        return float('inf')
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def abs_err(got, ref):
    return float((got - ref).abs().max()) if torch.isfinite(got).all() else float('inf')


def l2_err(got, ref):
    """tests/test_gpu_resnet.py rel: ||got - ref|| / ||ref||"""
    return float((got - ref).norm() / max(float(ref.norm()), 1e-30)) if torch.isfinite(got).all() else float('inf')


def elem_rel_err(got, ref):
    """max |got - ref| / ref, element by element (check_gate's gate weights)"""
    return float(((got - ref).abs() / ref.abs()).max()) if torch.isfinite(got).all() else float('inf')


METRICS = {'rel': rel_err, 'abs': abs_err, 'l2': l2_err, 'elem': elem_rel_err}


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_d(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act(x, a):
    if a in (ACT_RELU, ACT_RELU_RES):
        return torch.relu(x)
    if a in (ACT_GELU, ACT_GELU_D):
        return gelu(x)
    if a == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


# ==============================================================================================================================
# GEMM: the cascade of svol_amd/csrc/gemm_call.h as one pure function
# ==============================================================================================================================
def nt_family(dtype, M, N, K, *, lda, ldb, ldc, epi=0, act=ACT_NONE, res=False, pre=False, colscale=False, aux=False, out_f32=False,
              kwrap=None, ldr=0, ldp=0, ldaux=0, cus=NOMINAL_CUS):
    """-> (family 1..6 of gemm_call.h's NT list, variant): which kernel family takes one svol_gemm_nt / _split / _dact call whose
    pointers are 16-byte aligned.  Restates gemm_call.h:4-18 with the conditions of the plan functions it summarises (fast_fits,
    ws_plan, n256_plan, skinny_plan, tile_plan, skinny_f32_ok, gemm_nt_dispatch).  variant: 'balanced' / 'tiles128' for family 2,
    'k32' / 'k64' for family 4, 'epi1-composed' for the generic composition of family 6, else ''.
    There is no library query to hold this function to (the library has no entry that names the family it took, and none is added for
    it): it is held to the header by reading, and the device test holds every case to the results only."""
    kwrap = K if kwrap is None else kwrap
    is16 = dtype in (BF16, FP16)
    if is16:
        fits = (kwrap == K or (2 * kwrap == K and kwrap % 32 == 0)) and K % 32 == 0 and lda % 8 == 0 and ldb % 8 == 0      # gemm_call.h:6-7
        fits = fits and ldc % 4 == 0 and (not res or ldr % 4 == 0) and (not pre or ldp % 4 == 0) and (not aux or ldaux % 4 == 0)
        if fits:
            # 1. weight-stationary (gemm_call.h:8-9)
            ws = kwrap == K and K == 256 and N % 64 == 0 and M >= 4096
            if epi:
                ws = ws and aux and not out_f32 and ldc % 8 == 0 and ldaux % 8 == 0
            elif out_f32:
                ws = ws and res and act == ACT_NONE and not pre and not colscale and ldr % 4 == 0
            else:
                ws = ws and not res and act in (ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_D) and ldc % 8 == 0 and (not pre or ldp % 8 == 0)
            if ws:
                return 1, ''
            # 2. full-width tiles (gemm_call.h:10-12)
            n256 = N % 256 == 0 and K % 32 == 0 and K >= 512 and M >= 4096 and epi == 0 and not pre and not colscale
            n256 = n256 and (act == ACT_NONE or (act in (ACT_GELU, ACT_RELU) and not out_f32)) and (not res or out_f32)
            n256 = n256 and (ldc % 4 == 0 if out_f32 else ldc % 8 == 0)
            if n256:
                return 2, 'balanced' if N == 256 and M > 128 * cus else 'tiles128'
            # 3. skinny split-K (gemm_call.h:13)
            if M <= 2048 and K % 256 == 0 and N % 64 == 0 and kwrap % (K // 4) == 0:
                return 3, ''
            # 4. 128 x 128 tiles (gemm_call.h:14)
            if (M + 127) // 128 <= 65535:
                return 4, 'k64' if K % 64 == 0 and K >= 1024 and kwrap % 64 == 0 else 'k32'
    # 5. fp32 skinny (gemm_call.h:16)
    if dtype == FP32 and kwrap == K and M <= 2048 and K % 128 == 0 and N % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 \
            and (not res or ldr % 4 == 0) and (not pre or ldp % 4 == 0) and (not aux or ldaux % 4 == 0):
        return 5, ''
    # 6. the generic kernel (gemm_call.h:17-18)
    epc = 8 if is16 else 4
    if K % epc or lda % epc or ldb % epc:
        return None, 'unsupported'
    if epi:
        return (6, 'epi1-composed') if ldc == N and ldaux == N else (None, 'unsupported')
    return 6, ''


def tn_family(dtype, N, K, *, lda, ldb):
    """-> family 1..2 of gemm_call.h's TN list (gemm_call.h:19-23; tn_plan, tn_generic_plan) for 16-byte aligned operands"""
    if dtype in (BF16, FP16) and N % 8 == 0 and K % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0:
        return 1
    epc = 8 if dtype in (BF16, FP16) else 4
    if N % epc == 0 and K % epc == 0 and lda % epc == 0 and ldb % epc == 0:
        return 2
    return None


H16 = (BF16, FP16)
ALL = (FP32, BF16, FP16)
# name: entry, (M, N, K) -- M 'bal' = 128 x CUs + 5 --, epilogue options, dtypes, the (family, variant) the 16-bit / the fp32 call takes.
# A and B are column slices (ld = width + 64) everywhere: every family's plan takes a stride; res, pre and aux are slices as well,
# except in the generic epi 1 composition, which takes dense C and aux only.
GEMM_NT = OrderedDict([
    ('ws_colscale', dict(entry='nt', mnk=(4099, 320, 256), bias=True, colscale=True, dtypes=H16, fam=(1, ''))),
    ('ws_gelu_d', dict(entry='nt', mnk=(4099, 320, 256), bias=True, act=ACT_GELU_D, pre=True, dtypes=H16, fam=(1, ''))),
    ('ws_f32_res', dict(entry='nt', mnk=(4099, 256, 256), bias=True, res=True, out_f32=True, dtypes=H16, fam=(1, ''))),
    ('ws_epi1', dict(entry='dact', mnk=(4133, 512, 256), act=ACT_GELU, colsum=True, dtypes=H16, fam=(1, ''))),
    ('n256', dict(entry='nt', mnk=(4099, 256, 512), bias=True, act=ACT_GELU, dtypes=H16, fam=(2, 'tiles128'))),
    ('n256_f32_res', dict(entry='nt', mnk=(4099, 512, 512), bias=True, res=True, out_f32=True, dtypes=H16, fam=(2, 'tiles128'))),
    ('n256_balanced', dict(entry='nt', mnk=('bal', 256, 512), bias=True, dtypes=H16, fam=(2, 'balanced'))),
    ('n256_split', dict(entry='split', mnk=(4099, 256, 256), bias=True, dtypes=(BF16,), fam=(2, 'tiles128'))),
    ('skinny', dict(entry='nt', mnk=(257, 64, 256), bias=True, act=ACT_RELU, res=True, dtypes=H16, fam=(3, ''))),
    ('skinny_f32_colscale', dict(entry='nt', mnk=(257, 64, 256), bias=True, colscale=True, res=True, out_f32=True, dtypes=H16, fam=(3, ''))),
    ('tiles_k32', dict(entry='nt', mnk=(300, 200, 96), bias=True, act=ACT_GELU, pre=True, res=True, dtypes=ALL, fam=(4, 'k32'), fam32=(6, ''))),
    ('tiles_k64', dict(entry='nt', mnk=(130, 72, 1024), bias=True, act=ACT_SIGMOID, res=True, dtypes=H16, fam=(4, 'k64'))),
    ('tiles_epi1', dict(entry='dact', mnk=(300, 256, 64), act=ACT_RELU, colsum=True, dtypes=H16, fam=(4, 'k32'))),
    ('f32_skinny', dict(entry='nt', mnk=(100, 32, 128), bias=True, act=ACT_RELU, res=True, dtypes=(FP32,), fam32=(5, ''))),
    ('f32_skinny_epi1', dict(entry='dact', mnk=(130, 64, 128), act=ACT_GELU, colsum=True, dtypes=(FP32,), fam32=(5, ''))),
    ('generic', dict(entry='nt', mnk=(257, 130, 8), bias=True, res=True, dtypes=ALL, fam=(6, ''), fam32=(6, ''))),
    ('generic_epi1', dict(entry='dact', mnk=(77, 96, 40), act=ACT_GELU, colsum=True, dense=True, dtypes=ALL, fam=(6, 'epi1-composed'),
                          fam32=(6, 'epi1-composed'))),
    ('generic_split', dict(entry='split', mnk=(257, 72, 40), bias=True, dtypes=(BF16,), fam=(6, ''))),
])


def gemm_nt_mnk(row, cus=NOMINAL_CUS):
    M, N, K = row['mnk']
    return (128 * cus + 5 if M == 'bal' else M), N, K


def gemm_nt_family_of(row, dtype, cus=NOMINAL_CUS):
    """the twin's answer for one table row, from the leading dimensions gemm_nt_spec gives its slots"""
    M, N, K = gemm_nt_mnk(row, cus)
    dense = row.get('dense', False)
    ldn = N if dense else N + 64
    split = row['entry'] == 'split'
    return nt_family(dtype, M, N, 2 * K if split else K, lda=K + 64, ldb=(2 * K if split else K) + 64, ldc=ldn,
                     epi=int(row['entry'] == 'dact'), act=row.get('act', ACT_NONE), res=row.get('res', False), pre=row.get('pre', False),
                     colscale=row.get('colscale', False), aux=row['entry'] == 'dact', out_f32=row.get('out_f32', False),
                     kwrap=K, ldr=ldn, ldp=ldn, ldaux=ldn, cus=cus)


def _gemm_nt_ref(s):
    d = s.dims
    A_, B_ = s.x('A'), s.x('B')
    if d['entry'] == 'split':
        K = d['K']
        return {'C': A_ @ (B_[:, :K] + B_[:, K:]).t() + s.x('bias')}
    z = A_ @ B_.t()
    if d['entry'] == 'dact':
        aux = s.x('aux')
        dd = {ACT_GELU: gelu_d(aux), ACT_GELU_D: aux, ACT_RELU: (aux > 0).double()}[d['act']]
        C = z * dd
        out = {'C': C}
        if 'colsum' in s.outs:
            out['colsum'] = s.outs['colsum'].init.double() + C.sum(0)
        return out
    if 'bias' in s.ins:
        z = z + s.x('bias')
    out = {}
    if 'pre' in s.outs:
        out['pre'] = gelu_d(z) if d['act'] == ACT_GELU_D else z
    if 'colscale' in s.ins:
        z = z * s.x('colscale')
    C = act(z, d['act'])
    if 'res' in s.ins:
        C = C + s.x('res')
    out['C'] = C
    return out


def gemm_nt_spec(name, dtype, cus=NOMINAL_CUS):
    row = GEMM_NT[name]
    M, N, K = gemm_nt_mnk(row, cus)
    entry, dense, f32o = row['entry'], row.get('dense', False), row.get('out_f32', False)
    ldn = None if dense else N + 64
    odt = FP32 if f32o else dtype
    ins = OrderedDict()
    ins['A'] = In(_rnd((M, K), dtype, 1), K + 64, 32)
    if entry == 'split':      # [hi | lo] of an fp32 weight, as svol_cast_split writes it
        w = _rnd((N, K), FP32, 2, 1.0 / math.sqrt(K))
        hi = w.to(BF16)
        ins['B'] = In(torch.cat([hi, (w - hi.float()).to(BF16)], 1), 2 * K + 64, 32)
    else:
        ins['B'] = In(_rnd((N, K), dtype, 2, 1.0 / math.sqrt(K)), K + 64, 32)
    if row.get('bias'):
        ins['bias'] = In(_rnd((N,), FP32, 3))
    if row.get('colscale'):
        ins['colscale'] = In((torch.arange(N) % 3 + 1).float() * 0.5)
    if row.get('res'):
        ins['res'] = In(_rnd((M, N), odt, 4), ldn, 0)
    outs = OrderedDict()
    outs['C'] = Out((M, N), odt, ldn, 0 if dense else 64)
    if row.get('pre'):
        outs['pre'] = Out((M, N), dtype, ldn, 32)
    bars = {'C': ((2e-5 if dtype == FP32 else 1e-5) if f32o else TOL[dtype], 'rel'), 'pre': (TOL[dtype], 'rel')}
    if entry == 'split':
        bars['C'] = (4.5e-3, 'rel')                         # check_gemm_split: one bf16 rounding of the result
    if entry == 'dact':
        ins['aux'] = In(torch.relu(_rnd((M, N), dtype, 52)) if row['act'] == ACT_RELU else _rnd((M, N), dtype, 52), ldn, 0)
        if row.get('colsum'):
            outs['colsum'] = Out((N,), FP32, init=torch.zeros(N))
            bars['colsum'] = (1e-4 if dtype == FP32 else 1e-2, 'rel')
    dims = dict(entry=entry, M=M, N=N, K=K, act=row.get('act', ACT_NONE), out_f32=int(f32o))
    fam = gemm_nt_family_of(row, dtype, cus)
    return Spec('gemm_nt', name, 'svol_gemm_nt' + {'nt': '', 'split': '_split', 'dact': '_dact'}[entry], dtype, dims, ins, outs, _gemm_nt_ref,
                bars, biteq=entry != 'dact', plan=fam)


def gemm_nt_points():
    return [(n, dt) for n, r in GEMM_NT.items() for dt in r['dtypes']]


# ---- TN -----------------------------------------------------------------------------------------------------------------------
# name: problems [(Mc, N, K)], entry.  A [Mc, N] and B [Mc, K] are column slices (ld = width + 64), C [N, K] fp32 is a slice as well.
# 'grouped': two problems whose operands are neighbours in the arena, accumulated into non-zero targets.
GEMM_TN = OrderedDict([
    ('333x200x136', dict(entry='tn', probs=[(333, 200, 136)], dtypes=ALL, zero=True)),
    ('797x64x256', dict(entry='tn', probs=[(797, 64, 256)], dtypes=ALL, zero=True)),
    ('64x8x8', dict(entry='tn', probs=[(64, 8, 8)], dtypes=ALL, zero=True)),
    ('300x24x40', dict(entry='tn', probs=[(300, 24, 40)], dtypes=ALL, zero=False)),
    ('group_of_two', dict(entry='grouped', probs=[(333, 200, 136), (797, 64, 256)], dtypes=ALL, zero=False)),
    ('group_odd', dict(entry='grouped', probs=[(300, 24, 40), (64, 8, 8)], dtypes=ALL, zero=False)),
])


def gemm_tn_family_of(row, dtype):
    return tuple(tn_family(dtype, N, K, lda=N + 64, ldb=K + 64) for (_, N, K) in row['probs'])


def _tn_colsum_err(i):
    def f(got, ref, s=None):
        a = s.x(f'A{i}')
        return float((got - ref).abs().max()) / float(a.abs().sum(0).max())       # check_gemm_tn's colsum figure
    return f


def _gemm_tn_ref(s):
    out = {}
    for i in range(s.dims['n']):
        a, b = s.x(f'A{i}'), s.x(f'B{i}')
        out[f'C{i}'] = s.outs[f'C{i}'].init.double() + a.t() @ b
        out[f'cs{i}'] = s.outs[f'cs{i}'].init.double() + a.sum(0)
    return out


def gemm_tn_spec(name, dtype):
    row = GEMM_TN[name]
    ins, outs, bars = OrderedDict(), OrderedDict(), {}
    for i, (Mc, N, K) in enumerate(row['probs']):
        ins[f'A{i}'] = In(_rnd((Mc, N), dtype, 7 + 10 * i), N + 64, 32)
        ins[f'B{i}'] = In(_rnd((Mc, K), dtype, 8 + 10 * i), K + 64, 32)
    for i, (Mc, N, K) in enumerate(row['probs']):
        z = row['zero']
        outs[f'C{i}'] = Out((N, K), FP32, K + 32, 32, init=torch.zeros(N, K) if z else _rnd((N, K), FP32, 70 + i))
        outs[f'cs{i}'] = Out((N,), FP32, init=torch.zeros(N) if z else _rnd((N,), FP32, 80 + i))
        if z:        # check_gemm_tn
            bars[f'C{i}'] = (5e-5 if dtype == FP32 else 2e-5, 'rel')
            bars[f'cs{i}'] = (2e-6, _tn_colsum_err(i))
        else:        # check_gemm_tn_grouped: accumulation into non-zero targets
            bars[f'C{i}'] = bars[f'cs{i}'] = (2e-5 if dtype == FP32 else 1e-4, 'rel')
    return Spec('gemm_tn', name, 'svol_gemm_tn' + ('_grouped' if row['entry'] == 'grouped' else ''), dtype,
                dict(n=len(row['probs']), probs=row['probs']), ins, outs, _gemm_tn_ref, bars, plan=gemm_tn_family_of(row, dtype))


def gemm_tn_points():
    return [(n, dt) for n, r in GEMM_TN.items() for dt in r['dtypes']]


# ==============================================================================================================================
# Attention
# ==============================================================================================================================
# (table, case, has key bias, batch override): every plan of tests/attn_range_cases.py CASES (but pre_masked_65: eight thousand
# keys, and the range tests run it) and of the head-width 40-64 table; each ragged-Lk plan also with B = 1, where the only
# batch element's key tail borders the guard.
def _attn_rows():
    rows = []
    for tab, cases in (('narrow', A.CASES), ('wide', W.CASES)):
        for name, c in cases.items():
            if name == 'pre_masked_65':
                continue
            B, H, Lq, Lk, dh = c['dims']
            for masked in sorted({m != 'none' for _, m in c['points']}):
                rows.append((tab, name, masked, None))
                if Lk % 128 and B > 1:
                    rows.append((tab, name, masked, 1))
    return rows


ATTN_ROWS = _attn_rows()


def attn_case(tab, name, B1=None):
    c = (A.CASES if tab == 'narrow' else W.CASES)[name]
    B, H, Lq, Lk, dh = c['dims']
    return (B1 or B, H, Lq, Lk, dh), c['premul'], c


def attn_layout(tab, name):
    """the mask layout a masked row runs: the case's first point with a key bias"""
    c = (A.CASES if tab == 'narrow' else W.CASES)[name]
    return next(m for _, m in c['points'] if m != 'none')


def attn_plan(tab, name, masked, B1=None):
    dims, premul, _ = attn_case(tab, name, B1)
    return A.plan(*dims, premul, masked)


def attn_row_id(row):
    tab, name, masked, B1 = row
    return f'{tab}-{name}{"-kbias" if masked else ""}{"-B1" if B1 else ""}'


def attn_dtypes(row):
    c = attn_case(row[0], row[1])[2]
    return ALL if c['fp32'] else H16


def _mha(q, k, v, B, H, Lq, Lk, dh, kb):
    """tests/gpu_checks.py _attn_ref"""
    q4, k4, v4 = (t.view(B, L, H, dh).transpose(1, 2) for t, L in ((q, Lq), (k, Lk), (v, Lk)))
    s = q4 @ k4.transpose(-1, -2) / math.sqrt(dh)
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    p = torch.softmax(s, -1)
    return (p @ v4).transpose(1, 2).reshape(B * Lq, H * dh), torch.logsumexp(s, -1) / math.log(2.0), p


@functools.lru_cache(maxsize=None)
def attn_problem(tab, name, masked, B1, dtype):
    """inputs (check_attention's draws, q pre-multiplied where the case says so) and the fp64 forward and backward of one row;
    shared between the forward and the backward spec, never modified"""
    (B, H, Lq, Lk, dh), premul, c = attn_case(tab, name, B1)
    d = H * dh
    q, k, v = _rnd((B * Lq, d), dtype, 30, 1.5), _rnd((B * Lk, d), dtype, 31, 1.5), _rnd((B * Lk, d), dtype, 32)
    do = _rnd((B * Lq, d), dtype, 33)
    kb = None
    if masked:
        cases = A.CASES if tab == 'narrow' else W.CASES
        kb = A.key_bias(name, attn_layout(tab, name), cases)[:B].contiguous()
    pm = LOG2E / math.sqrt(dh) if premul else 0.0
    if premul:
        q = (q.double() * pm).to(dtype)
    q64 = (q.double() / pm if premul else q.double()).requires_grad_(True)      # the unscaled q the kernel effectively sees
    k64, v64 = k.double().requires_grad_(True), v.double().requires_grad_(True)
    o, lse2, _ = _mha(q64, k64, v64, B, H, Lq, Lk, dh, kb)
    (o * do.double()).sum().backward()
    return dict(dims=(B, H, Lq, Lk, dh), pm=pm, q=q, k=k, v=v, do=do, kb=kb, o=o.detach(), lse2=lse2.detach(), dq=q64.grad, dk=k64.grad,
                dv=v64.grad)


def _attn_ins(p, dtype):
    B, H, Lq, Lk, dh = p['dims']
    d = H * dh
    ins = OrderedDict()
    if Lq == Lk:     # self-attention: q | k | v of one packed [M, 3d] buffer
        ins['q'], ins['k'], ins['v'] = In(p['q'], 3 * d, 0, 'qkv'), In(p['k'], 3 * d, d, 'qkv'), In(p['v'], 3 * d, 2 * d, 'qkv')
    else:            # cross-attention: q on its own, k | v of one [B Lk, 2d] buffer
        ins['q'] = In(p['q'], d + 64, 32)
        ins['k'], ins['v'] = In(p['k'], 2 * d, 0, 'kv'), In(p['v'], 2 * d, d, 'kv')
    if p['kb'] is not None:
        ins['kbias'] = In(p['kb'])
    return ins


def attn_spec(row, dtype, kind):
    tab, name, masked, B1 = row
    p = attn_problem(tab, name, masked, B1, dtype)
    B, H, Lq, Lk, dh = p['dims']
    d = H * dh
    ins = _attn_ins(p, dtype)
    outs = OrderedDict()
    lse_bar = (1e-5 if dtype == FP32 else 3e-3, 'rel')       # check_attention's lse2 bars
    if kind == 'fwd':
        outs['o'] = Out((B * Lq, d), dtype, d + 64, 64)
        outs['lse2'] = Out((B, H, Lq), FP32)
        ref = lambda s: {'o': p['o'], 'lse2': p['lse2']}     # noqa: E731
        bars = {'o': (TOL[dtype], 'rel'), 'lse2': lse_bar}
    else:
        ins['o'] = In(p['o'].to(dtype), d + 64, 32)
        ins['do'] = In(p['do'], d + 64, 0)
        ins['lse2'] = In(p['lse2'].float())
        if Lq == Lk:
            outs['dq'], outs['dk'], outs['dv'] = (Out((B * Lq, d), dtype, 3 * d, i * d, slot='dqkv') for i in range(3))
        else:
            outs['dq'] = Out((B * Lq, d), dtype, d + 64, 64)
            outs['dk'], outs['dv'] = (Out((B * Lk, d), dtype, 2 * d, i * d, slot='dkv') for i in range(2))
        outs['delta'] = Out((3 * B * H * Lq,), FP32, scratch=True)
        ref = lambda s: {'dq': p['dq'], 'dk': p['dk'], 'dv': p['dv']}     # noqa: E731
        bars = {n: (2 * TOL[dtype], 'rel') for n in ('dq', 'dk', 'dv')}
    pl = attn_plan(tab, name, masked, B1)
    return Spec('attention', attn_row_id(row), 'svol_attn_' + kind, dtype, dict(B=B, H=H, Lq=Lq, Lk=Lk, dh=dh, pm=p['pm'], ws=True), ins, outs,
                ref, bars, biteq=kind == 'fwd', plan=pl['fwd' if kind == 'fwd' else 'bwd'])


# svol_attn_weights_mean (check_attn_weights): a masked ragged cross-attention at head width 32 and one at 64, plain and pre-multiplied q
ATTN_WEIGHTS = OrderedDict([('d32_masked', ((2, 8, 100, 700, 32), True, True)), ('d8_tiny', ((2, 4, 8, 24, 8), True, False)),
                            ('d64_ragged', ((1, 4, 37, 300, 64), False, True)), ('one_key', ((3, 2, 5, 1, 32), False, False))])


def attn_weights_spec(name, dtype):
    (B, H, Lq, Lk, dh), masked, premul = ATTN_WEIGHTS[name]
    d = H * dh
    q, k = _rnd((B * Lq, d), dtype, 60, 1.5), _rnd((B * Lk, d), dtype, 61, 1.5)
    kb = None
    if masked:
        kb = torch.zeros(B, Lk)
        kb[:, Lk - Lk // 4:] = float('-inf')
    pm = LOG2E / math.sqrt(dh) if premul else 0.0
    if premul:
        q = (q.double() * pm).to(dtype)
    q64 = q.double() / pm if premul else q.double()
    _, lse2, prob = _mha(q64, k.double(), k.double(), B, H, Lq, Lk, dh, kb)
    ins = OrderedDict(q=In(q, d + 64, 32), k=In(k, 2 * d, 0, 'kv'), v_unused=In(_rnd((B * Lk, d), dtype, 62), 2 * d, d, 'kv'), lse2=In(lse2.float()))
    if masked:
        ins['kbias'] = In(kb)
    outs = OrderedDict(att=Out((B, Lq, Lk), FP32))
    att = prob.mean(1)
    return Spec('attention', name, 'svol_attn_weights_mean', dtype, dict(B=B, H=H, Lq=Lq, Lk=Lk, dh=dh, pm=pm), ins, outs, lambda s: {'att': att},
                {'att': (1e-5 if dtype == FP32 else 5e-3, 'abs')})


# short sequences (the ViT extractor, L <= 256) and the one-query [CLS] block: lengths on both sides of the kernels' 32- / 64-key
# blocks, both head widths, the packed layouts the model uses
ATTN_SMALL = [(L, dh) for L in (33, 97, 225) for dh in SM.DHS]
ATTN_CLS = [(L, dh) for L in (1, 2, 65, 197) for dh in CLS.DHS]


def attn_cls_kinds(L):
    """one key: the forward only.  The backward's dq and dk are exactly zero there when lse2 carries the forward's own bits; their fp64
    reference is zero, and a bar relative to it has no scale"""
    return ('fwd',) if L == 1 else ('fwd', 'bwd')


@functools.lru_cache(maxsize=None)
def _small_problem(L, dh, dtype):
    n, H = SM.N_IMAGES, SM.heads_of(L)
    d = H * dh
    q, k, v, do = (_rnd((n * L, d), dtype, 30 + i, s) for i, s in enumerate((1.5, 1.5, 1.0, 1.0)))
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    o, lse2, _ = _mha(q64, k64, v64, n, H, L, L, dh, None)
    (o * do.double()).sum().backward()
    return dict(q=q, k=k, v=v, do=do, o=o.detach(), lse2=lse2.detach(), dq=q64.grad, dk=k64.grad, dv=v64.grad, n=n, H=H)


def attn_small_spec(L, dh, dtype, kind):
    p = _small_problem(L, dh, dtype)
    n, H = p['n'], p['H']
    d = H * dh
    ins = OrderedDict(q=In(p['q'], 3 * d, 0, 'qkv'), k=In(p['k'], 3 * d, d, 'qkv'), v=In(p['v'], 3 * d, 2 * d, 'qkv'))
    outs = OrderedDict()
    if kind == 'fwd':
        outs['o'] = Out((n * L, d), dtype, d + 64, 64)
        outs['lse2'] = Out((n, H, L), FP32)
        ref = lambda s: {'o': p['o'], 'lse2': p['lse2']}     # noqa: E731
        bars = {'o': (TOL[dtype], 'rel'), 'lse2': (3e-3, 'rel')}
    else:
        ins['o'], ins['do'], ins['lse2'] = In(p['o'].to(dtype), d + 64, 32), In(p['do'], d + 64, 0), In(p['lse2'].float())
        outs['dq'], outs['dk'], outs['dv'] = (Out((n * L, d), dtype, 3 * d, i * d, slot='dqkv') for i in range(3))
        ref = lambda s: {'dq': p['dq'], 'dk': p['dk'], 'dv': p['dv']}     # noqa: E731
        bars = {x: (2 * TOL[dtype], 'rel') for x in ('dq', 'dk', 'dv')}
    return Spec('attention', f'L{L}-dh{dh}', f'svol_attn_small_{"fwd_lse" if kind == "fwd" else "bwd"}_h16', dtype, dict(n=n, H=H, L=L, dh=dh),
                ins, outs, ref, bars, biteq=kind == 'fwd')


@functools.lru_cache(maxsize=None)
def _cls_problem(L, dh, dtype):
    n, H = 2, 3
    d = H * dh
    q, do = _rnd((n, d), dtype, 30, 1.5), _rnd((n, d), dtype, 33)
    k, v = _rnd((n * L, d), dtype, 31, 1.5), _rnd((n * L, d), dtype, 32)
    o, lse2, dq, dk, dv = CLS._math(q, k, v, do, (n, H, L, dh))
    return dict(q=q, k=k, v=v, do=do, o=o, lse2=lse2, dq=dq, dk=dk, dv=dv, n=n, H=H)


def attn_cls_spec(L, dh, dtype, kind):
    p = _cls_problem(L, dh, dtype)
    n, H = p['n'], p['H']
    d = H * dh
    ins = OrderedDict(q=In(p['q'], d + 64, 32), k=In(p['k'], 2 * d, 0, 'kv'), v=In(p['v'], 2 * d, d, 'kv'))
    outs = OrderedDict()
    if kind == 'fwd':
        outs['o'] = Out((n, d), dtype, d + 64, 64)
        outs['lse2'] = Out((n, H), FP32)
        ref = lambda s: {'o': p['o'], 'lse2': p['lse2']}     # noqa: E731
        bars = {'o': (TOL[dtype], 'rel'), 'lse2': (3e-3, 'rel')}
    else:
        ins['o'], ins['do'], ins['lse2'] = In(p['o'].to(dtype), d + 64, 32), In(p['do'], d + 64, 0), In(p['lse2'].float())
        outs['dq'] = Out((n, d), dtype, d + 64, 64)
        outs['dk'], outs['dv'] = (Out((n * L, d), dtype, 2 * d, i * d, slot='dkv') for i in range(2))
        ref = lambda s: {'dq': p['dq'], 'dk': p['dk'], 'dv': p['dv']}     # noqa: E731
        bars = {x: (2 * TOL[dtype], 'rel') for x in ('dq', 'dk', 'dv')}
    return Spec('attention', f'L{L}-dh{dh}', f'svol_attn_cls_{kind}_h16', dtype, dict(n=n, H=H, L=L, dh=dh), ins, outs, ref, bars,
                biteq=kind == 'fwd')


# ==============================================================================================================================
# Row kernels
# ==============================================================================================================================
LN_DS = (32, 100, 252, 256, 512, 768, 1024)
LN_MS = (5, 2049, 4100)          # above 2048 rows the backward walks more than one row per wave, with a last wave of one row
LN_POS_ROWS = {5: 3, 2049: 100, 4100: 100}       # pos_rows < M, pos exactly pos_rows x D: the row behind it is the arena's


def ln_points():
    return [(M, D) for M in LN_MS for D in LN_DS]


def ln_x_f32(M, D):
    """fp32 residual-stream input but for two widths, which read compute-dtype rows (the input projections' LayerNorm)"""
    return D not in (100, 512)


def _colsum_err(M):
    def f(got, ref, s=None):
        return float((got - ref).abs().max()) / float(s.ref_dx_max * math.sqrt(M))     # check_layernorm's dx_colsum figure
    return f


@functools.lru_cache(maxsize=None)
def _ln_problem(M, D, dtype):
    xdt = FP32 if ln_x_f32(M, D) else dtype
    pr = LN_POS_ROWS[M]
    x = _rnd((M, D), xdt, 14)
    g, b = 1 + 0.1 * _rnd((D,), FP32, 15), 0.1 * _rnd((D,), FP32, 16)
    pos = _rnd((pr, D), dtype, 17)
    dy32, dy, dyp = _rnd((M, D), FP32, 22), _rnd((M, D), dtype, 18), _rnd((M, D), dtype, 19)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
    yr = layer_norm(x64, g64, b64)
    ypr = yr + pos.double()[torch.arange(M) % pr]
    (yr * (dy.double() + dy32.double()) + ypr * dyp.double()).sum().backward()
    mu = x.double().mean(-1)
    rstd = 1.0 / torch.sqrt(((x.double() - mu[:, None]) ** 2).mean(-1) + 1e-5)
    return dict(x=x, g=g, b=b, pos=pos, dy32=dy32, dy=dy, dyp=dyp, y=yr.detach(), ypos=ypr.detach(), mean=mu, rstd=rstd, dx=x64.grad,
                dg=g64.grad, db=b64.grad)


def ln_spec(M, D, dtype, kind):
    p = _ln_problem(M, D, dtype)
    xf = ln_x_f32(M, D)
    f32 = lambda: Out((M, D), FP32)          # noqa: E731
    tt = lambda: Out((M, D), dtype)          # noqa: E731
    if kind == 'fwd':
        ins = OrderedDict(x=In(p['x']), gamma=In(p['g']), beta=In(p['b']), pos=In(p['pos']))
        outs = OrderedDict(y32=f32(), y=tt(), ypos=tt(), mean=Out((M,), FP32), rstd=Out((M,), FP32))
        ref = lambda s: {'y32': p['y'], 'y': p['y'], 'ypos': p['ypos'], 'mean': p['mean'], 'rstd': p['rstd']}     # noqa: E731
        # mean / rstd: fp32 statistics, held to y32's bar (y32 is (x - mean) rstd gamma + beta)
        bars = {'y32': (2e-5, 'rel'), 'y': (TOL[dtype], 'rel'), 'ypos': (TOL[dtype], 'rel'), 'mean': (2e-5, 'rel'), 'rstd': (2e-5, 'rel')}
    else:
        ins = OrderedDict(dy32=In(p['dy32']), dy=In(p['dy']), dy2=In(p['dyp']), x=In(p['x']), gamma=In(p['g']), mean=In(p['mean'].float()),
                          rstd=In(p['rstd'].float()))
        z = lambda: Out((D,), FP32, init=torch.zeros(D))          # noqa: E731
        outs = OrderedDict(dx32=f32(), dx=tt(), dgamma=z(), dbeta=z(), colsum=z())
        ref = lambda s: {'dx32': p['dx'], 'dx': p['dx'], 'dgamma': p['dg'], 'dbeta': p['db'], 'colsum': p['dx'].sum(0)}     # noqa: E731
        par = 1e-4 if dtype == FP32 else 1e-2
        bars = {'dx32': ((2e-5 + (0 if dtype == FP32 else TOL[dtype])) if xf else TOL[dtype], 'rel'), 'dx': (TOL[dtype], 'rel'),
                'dgamma': (par, 'rel'), 'dbeta': (par, 'rel'), 'colsum': (2e-5 if dtype == FP32 else 1e-2, _colsum_err(M))}
    s = Spec('rows', f'M{M}-D{D}', 'svol_layernorm_' + kind, dtype, dict(M=M, D=D, x_f32=int(xf), pos_rows=LN_POS_ROWS[M]), ins, outs, ref, bars,
             biteq=kind == 'fwd')
    s.ref_dx_max = float(p['dx'].abs().max())
    return s


# ---- the sketch -> video gate ----------------------------------------------------------------------------------------------
GATE_SHAPES = ((2, 52, 64, 8), (1, 12, 252, 7), (2, 3001, 256, 8))      # (B, L, D, H); the last: L % 4 != 0, no fused entry


def gate_fusable(B, L, D, H):
    return L % 4 == 0 and D <= 256          # svol_layernorm_gate_scores_fwd (include/svol_hip.h)


@functools.lru_cache(maxsize=None)
def _gate_problem(B, L, D, H, dtype):
    """check_gate's draws and check_gate_scores_fused's LN3 in front: s3 -> LN3 -> x (= m32) -> gate with u"""
    M = B * L
    s3 = _rnd((M, D), FP32, 60)
    g3, b3 = 1 + 0.1 * _rnd((D,), FP32, 62), 0.1 * _rnd((D,), FP32, 63)
    x = _rnd((B, L, D), FP32, 40)
    pos = _rnd((B, L, D), dtype, 41)
    u = _rnd((B, H, D), FP32, 42, 0.2)
    g, b = 1 + 0.1 * _rnd((D,), FP32, 43), 0.1 * _rnd((D,), FP32, 44)
    dy32, dy, dyp = _rnd((B, L, D), FP32, 47), _rnd((B, L, D), dtype, 45), _rnd((B, L, D), dtype, 46)
    x64, u64, g64, b64 = (t.double().requires_grad_(True) for t in (x, u, g, b))
    sc = torch.einsum('bld,bhd->bhl', x64 + pos.double(), u64)
    a = torch.softmax(sc, -1).mean(1)
    xs = x64 * (1 + a[..., None])
    y = layer_norm(xs, g64, b64)
    ypos = y + pos.double()
    (y * (dy.double() + dy32.double()) + ypos * dyp.double()).sum().backward()
    xsd = xs.detach()
    mean = xsd.mean(-1)
    rstd = 1.0 / torch.sqrt(((xsd - mean[..., None]) ** 2).mean(-1) + 1e-5)
    scd = sc.detach()
    mx = scd.max(-1).values
    ws = torch.cat([scd.reshape(-1), mx.reshape(-1), torch.exp(scd - mx[..., None]).sum(-1).reshape(-1)])
    # the fused LN3 of the layer before, whose output is a DIFFERENT x: its own scores
    m3 = layer_norm(s3.double(), g3.double(), b3.double())
    mu3 = s3.double().mean(-1)
    rstd3 = 1.0 / torch.sqrt(((s3.double() - mu3[:, None]) ** 2).mean(-1) + 1e-5)
    sc3 = torch.einsum('bld,bhd->bhl', (m3 + pos.double().view(M, D)).view(B, L, D), u.double())
    return dict(s3=s3, g3=g3, b3=b3, m3=m3, mu3=mu3, rstd3=rstd3, sc3=sc3, x=x, pos=pos, u=u, g=g, b=b, dy32=dy32, dy=dy, dyp=dyp, sc=scd,
                a=a.detach(), y=y.detach(), ypos=ypos.detach(), mean=mean, rstd=rstd, ws=ws, dx=x64.grad, du=u64.grad, dg=g64.grad, db=b64.grad)


def _du_err(got, ref, s=None):
    return float((got - ref).abs().max()) / s.ref_dx_max         # check_gate: du on dx's scale


def gate_spec(shape, dtype, entry):
    """entry: svol_gate_fwd | svol_gate_fwd_scored | svol_layernorm_gate_scores_fwd | svol_gate_bwd"""
    B, L, D, H = shape
    M = B * L
    p = _gate_problem(B, L, D, H, dtype)
    nws = B * H * (L + 2)
    f2 = lambda t: t.reshape(M, D)          # noqa: E731
    gate_outs = lambda ws: OrderedDict(y32=Out((M, D), FP32), y=Out((M, D), dtype), ypos=Out((M, D), dtype), a=Out((M,), FP32),          # noqa: E731
                                       mean=Out((M,), FP32), rstd=Out((M,), FP32), ws=ws)
    gate_ref = lambda s: {'y32': f2(p['y']), 'y': f2(p['y']), 'ypos': f2(p['ypos']), 'a': p['a'].reshape(-1), 'mean': p['mean'].reshape(-1),          # noqa: E731
                          'rstd': p['rstd'].reshape(-1), 'ws': p['ws']}
    gate_bars = {'y32': (2e-5, 'rel'), 'y': (TOL[dtype], 'rel'), 'ypos': (TOL[dtype], 'rel'), 'a': (1e-4, 'elem'), 'mean': (2e-5, 'rel'),
                 'rstd': (2e-5, 'rel'), 'ws': (2e-5, 'rel')}
    base = OrderedDict(x32=In(f2(p['x'])), pos=In(f2(p['pos'])), u=In(p['u']), gamma=In(p['g']), beta=In(p['b']))
    if entry == 'svol_gate_fwd':
        ins, outs, ref, bars = base, gate_outs(Out((nws,), FP32)), gate_ref, gate_bars
    elif entry == 'svol_gate_fwd_scored':      # ws[0 .. BHL) already holds the scores: an operand that is also written behind
        start = torch.cat([p['sc'].reshape(-1).float(), torch.zeros(2 * B * H)])
        ins, outs, ref, bars = base, gate_outs(Out((nws,), FP32, init=start)), gate_ref, gate_bars
    elif entry == 'svol_layernorm_gate_scores_fwd':
        ins = OrderedDict(x32=In(p['s3']), gamma=In(p['g3']), beta=In(p['b3']), pos=In(f2(p['pos'])), u_next=In(p['u']))
        outs = OrderedDict(y32=Out((M, D), FP32), y=Out((M, D), dtype), ypos=Out((M, D), dtype), mean=Out((M,), FP32), rstd=Out((M,), FP32),
                           scores=Out((B * H * L,), FP32))
        ref = lambda s: {'y32': p['m3'], 'y': p['m3'], 'ypos': p['m3'] + p['pos'].double().view(M, D), 'mean': p['mu3'], 'rstd': p['rstd3'],          # noqa: E731
                         'scores': p['sc3'].reshape(-1)}
        bars = {'y32': (2e-5, 'rel'), 'y': (TOL[dtype], 'rel'), 'ypos': (TOL[dtype], 'rel'), 'mean': (2e-5, 'rel'), 'rstd': (2e-5, 'rel'),
                'scores': (2e-5, 'rel')}
    else:
        ins = OrderedDict(dy32=In(f2(p['dy32'])), dy=In(f2(p['dy'])), dy2=In(f2(p['dyp'])), x32=In(f2(p['x'])), pos=In(f2(p['pos'])), u=In(p['u']),
                          gamma=In(p['g']), a=In(p['a'].reshape(-1).float()), mean=In(p['mean'].reshape(-1).float()),
                          rstd=In(p['rstd'].reshape(-1).float()), ws=In(p['ws'].float()))
        outs = OrderedDict(dx32=Out((M, D), FP32), du=Out((B, H, D), FP32, init=torch.zeros(B, H, D)), dgamma=Out((D,), FP32, init=torch.zeros(D)),
                           dbeta=Out((D,), FP32, init=torch.zeros(D)), ws2=Out((B * L + B * H,), FP32, scratch=True))
        ref = lambda s: {'dx32': f2(p['dx']), 'du': p['du'], 'dgamma': p['dg'], 'dbeta': p['db']}          # noqa: E731
        par = 1e-4 if dtype == FP32 else 1e-2
        bars = {'dx32': (4e-5 if dtype == FP32 else 1e-2, 'rel'), 'du': (3e-5, _du_err), 'dgamma': (par, 'rel'), 'dbeta': (par, 'rel')}
    s = Spec('rows', f'B{B}L{L}D{D}H{H}', entry, dtype, dict(B=B, L=L, D=D, H=H), ins, outs, ref, bars, biteq=entry == 'svol_gate_fwd')
    s.ref_dx_max = float(p['dx'].abs().max())
    return s


def gate_points():
    pts = []
    for sh in GATE_SHAPES:
        pts += [(sh, 'svol_gate_fwd'), (sh, 'svol_gate_bwd')]
        if gate_fusable(*sh):
            pts += [(sh, 'svol_layernorm_gate_scores_fwd'), (sh, 'svol_gate_fwd_scored')]
    return pts


GATE_VEC_SHAPES = ((2, 64, 8), (3, 252, 7))        # (B, D, H)


def gate_vectors_spec(shape, kind):
    B, D, H = shape
    dh = D // H
    sk = _rnd((B, D), FP32, 71)
    Win, b_in = _rnd((3 * D, D), FP32, 72, 3.0 / math.sqrt(D)), 0.3 * _rnd((3 * D,), FP32, 70)
    du = _rnd((B, H, D), FP32, 73)
    sk64, W64, bi64 = (t.double().requires_grad_(True) for t in (sk, Win, b_in))
    q = sk64 @ W64[:D].t() + bi64[:D]
    u = torch.einsum('bhj,hjd->bhd', q.view(B, H, dh), W64[D:2 * D].view(H, dh, D)) / math.sqrt(dh)
    if kind == 'fwd':
        ins = OrderedDict(skch=In(sk), W_in=In(Win), b_in=In(b_in))
        outs = OrderedDict(q=Out((B, D), FP32), u=Out((B, H, D), FP32))
        ref = lambda s: {'q': q.detach(), 'u': u.detach()}          # noqa: E731
        bars = {'q': (1e-5, 'rel'), 'u': (1e-5, 'rel')}             # check_gate_against_mha's bar on u
    else:
        (u * du.double()).sum().backward()
        dW0, db0 = _rnd((3 * D, D), FP32, 74), _rnd((3 * D,), FP32, 75)
        ins = OrderedDict(du=In(du), skch=In(sk), W_in=In(Win), q=In(q.detach().float()))
        outs = OrderedDict(dq_ws=Out((B * D,), FP32, scratch=True), dskch=Out((B, D), FP32), dW_in=Out((3 * D, D), FP32, init=dW0),
                           db_in=Out((3 * D,), FP32, init=db0))
        ref = lambda s: {'dskch': sk64.grad, 'dW_in': dW0.double() + W64.grad, 'db_in': db0.double() + bi64.grad}          # noqa: E731
        bars = {n: (TOL[FP32], 'rel') for n in ('dskch', 'dW_in', 'db_in')}
    return Spec('rows', f'B{B}D{D}H{H}', 'svol_gate_vectors_' + kind, FP32, dict(B=B, D=D, H=H), ins, outs, ref, bars)


# ---- small element-wise and reduction kernels (check_small_ops, check_dropout_mask, check_posenc) ----------------------------
def dropout_spec(dtype, add):
    from tests.dropout_twin import dropout_keep_numpy
    shape, p, seed = (1, 4097), 0.25, 5
    keep = torch.from_numpy(dropout_keep_numpy(shape, p, seed)).double() / (1.0 - p)
    if add:
        t, r = _rnd(shape, FP32, 14), _rnd(shape, FP32, 15)
        return Spec('rows', 'n4097', 'svol_dropout_add', FP32, dict(n=4097, row_len=4097, p=p, seed=seed), OrderedDict(t32=In(t), res32=In(r)),
                    OrderedDict(out32=Out(shape, FP32)), lambda s: {'out32': r.double() + t.double() * keep}, {'out32': (TOL[FP32], 'rel')})
    x = _rnd(shape, dtype, 14)
    return Spec('rows', 'n4097', 'svol_dropout', dtype, dict(n=4097, row_len=4097, p=p, seed=seed), OrderedDict(x=In(x)),
                OrderedDict(y=Out(shape, dtype)), lambda s: {'y': x.double() * keep}, {'y': (TOL[dtype], 'rel')})


def act_bwd_spec(dtype, a):
    n = 1003
    dy, aux = _rnd((n,), dtype, 11), _rnd((n,), dtype, 12)
    if a == ACT_SIGMOID:           # aux is the OUTPUT y
        aux = torch.sigmoid(aux.double()).to(dtype)
        d = aux.double() * (1 - aux.double())
    else:
        d = gelu_d(aux.double()) if a == ACT_GELU else (aux.double() > 0).double()
    return Spec('rows', f'act{a}', 'svol_act_bwd', dtype, dict(n=n, act=a), OrderedDict(dy=In(dy), aux=In(aux)), OrderedDict(dpre=Out((n,), dtype)),
                lambda s: {'dpre': dy.double() * d}, {'dpre': (TOL[dtype], 'rel')})


def colsum_spec(dtype):
    X = _rnd((777, 130), dtype, 9)
    return Spec('rows', '777x130', 'svol_colsum', dtype, dict(M=777, N=130, ld=130 + 64), OrderedDict(X=In(X, 130 + 64, 32)),
                OrderedDict(out=Out((130,), FP32, init=torch.zeros(130))), lambda s: {'out': X.double().sum(0)}, {'out': (1e-5, 'rel')})


def cast_spec(dtype, transpose):
    if transpose:
        Wt = _rnd((70, 50), FP32, 10)
        return Spec('rows', '70x50', 'svol_cast_transpose', dtype, dict(R=70, C=50), OrderedDict(src=In(Wt)),
                    OrderedDict(dst=Out((70, 50), dtype), dstT=Out((50, 70), dtype)),
                    lambda s: {'dst': Wt.to(dtype).double(), 'dstT': Wt.to(dtype).t().double()}, {'dst': (0.0, 'rel'), 'dstT': (0.0, 'rel')})
    x = _rnd((1003,), FP32, 14)
    return Spec('rows', 'n1003', 'svol_cast', dtype, dict(n=1003), OrderedDict(src=In(x)), OrderedDict(dst=Out((1003,), dtype)),
                lambda s: {'dst': x.to(dtype).double()}, {'dst': (0.0, 'rel')})


def posenc_spec(dtype, D):
    from oracle import svol_oracle as O
    mask = torch.ones(3, 150)
    mask[1, 100:] = 0
    mask[2, 7:] = 0
    ref = O.position_embedding_sine(mask.bool(), D).double()
    return Spec('rows', f'B3L150D{D}', 'svol_posenc_sine', dtype, dict(B=3, L=150, D=D), OrderedDict(mask=In(mask)),
                OrderedDict(pos=Out((3, 150, D), dtype)), lambda s: {'pos': ref}, {'pos': (2e-5 if dtype == FP32 else 8e-3, 'rel')})


def small_op_specs(dtype):
    out = [dropout_spec(dtype, False), colsum_spec(dtype), cast_spec(dtype, False), cast_spec(dtype, True), posenc_spec(dtype, 32),
           posenc_spec(dtype, 256)]
    out += [act_bwd_spec(dtype, a) for a in (ACT_RELU, ACT_GELU, ACT_SIGMOID)]
    if dtype == FP32:
        out += [dropout_spec(FP32, True)] + [gate_vectors_spec(sh, k) for sh in GATE_VEC_SHAPES for k in ('fwd', 'bwd')]
    return out


# ==============================================================================================================================
# ResNet kernels (bf16 and fp16; bars and the L2 metric of tests/test_gpu_resnet.py)
# ==============================================================================================================================
# (N, H, W, C, Cout, k, stride, pad), act, residual: the first image's top border and the last image's bottom border meet the guards
CONVS = (((3, 13, 9, 64, 128, 3, 2, 1), ACT_RELU, False), ((2, 14, 14, 64, 64, 3, 1, 1), ACT_RELU_RES, True),
         ((2, 12, 12, 128, 256, 1, 2, 0), ACT_NONE, False))


def _nchw(t, n, H, W, C):
    return t.double().view(n, H, W, C).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _unfold(x4, k, s, p, pad_value=0.0):
    """[n, C, H, W] -> [n Ho Wo, k k C] in (ky, kx, c) order"""
    n, C = x4.shape[:2]
    cols = F.unfold(F.pad(x4, (p, p, p, p), value=pad_value), k, stride=s)          # [n, C k k, L]
    return cols.view(n, C, k, k, -1).permute(0, 4, 2, 3, 1).reshape(-1, k * k * C)


def conv_spec(i, dtype):
    (n, H, W, C, Cout, k, s, p), a, has_res = CONVS[i]
    Ho, Wo = _out_hw(H, W, k, s, p)
    M, K = n * Ho * Wo, k * k * C
    x = _rnd((n * H * W, C), dtype, 90)
    w = _rnd((Cout, K), dtype, 91, 1.0 / math.sqrt(K))
    bias = _rnd((Cout,), FP32, 92)
    res = _rnd((M, Cout), dtype, 93)
    ins = OrderedDict(x=In(x), w=In(w, K + 64, 32), bias=In(bias))
    if has_res:
        ins['residual'] = In(res)

    def ref(spec):
        w4 = w.double().view(Cout, k, k, C).permute(0, 3, 1, 2)
        z = _nhwc(F.conv2d(_nchw(x, n, H, W, C), w4, bias.double(), s, p))
        if has_res:
            z = z + res.double()
        return {'y': act(z, a)}
    return Spec('resnet', f'{n}x{H}x{W}x{C}-{Cout}k{k}s{s}p{p}', 'svol_conv_nhwc', dtype, dict(N=n, H=H, W=W, C=C, Cout=Cout, k=k, s=s, p=p, act=a,
                                                                                              ldw=K + 64), ins,
                OrderedDict(y=Out((M, Cout), dtype)), ref, {'y': (TOL[dtype], 'rel')}, biteq=True)


def im2col_spec(dtype, nchw):
    n, H, W, C, k, s, p = (2, 13, 9, 3, 3, 2, 1) if nchw else (3, 13, 9, 8, 3, 2, 1)
    Ho, Wo = _out_hw(H, W, k, s, p)
    K = k * k * C
    Kp = (K + 31) // 32 * 32
    if nchw:         # the stem: fp32 NCHW pixels, converted on the way
        x = _rnd((n, C, H, W), FP32, 94)
        x4, strides = x.double(), (C * H * W, W, 1, H * W)
    else:
        x = _rnd((n * H * W, C), dtype, 94)
        x4, strides = _nchw(x, n, H, W, C), (H * W * C, W * C, C, 1)
    cols = torch.zeros(n * Ho * Wo, Kp, dtype=torch.float64)
    cols[:, :K] = _unfold(x4, k, s, p).to(dtype).double()
    return Spec('resnet', 'nchw-fp32' if nchw else 'nhwc', 'svol_im2col', dtype, dict(N=n, H=H, W=W, C=C, k=k, s=s, p=p, Kp=Kp, strides=strides,
                                                                                      src_f32=int(nchw)), OrderedDict(x=In(x)),
                OrderedDict(cols=Out((n * Ho * Wo, Kp), dtype)), lambda sp: {'cols': cols}, {'cols': (0.0, 'abs')}, biteq=True)


@functools.lru_cache(maxsize=None)
def _pool_problem(dtype):
    n, H, W, C, k, s, p = 2, 9, 9, 16, 3, 2, 1
    Ho, Wo = _out_hw(H, W, k, s, p)
    x = torch.relu(_rnd((n * H * W, C), dtype, 95))          # post-ReLU zeros: ties
    dy = _rnd((n * Ho * Wo, C), dtype, 96)
    win = _unfold(_nchw(x, n, H, W, C), k, s, p, float('-inf')).view(-1, k * k, C)          # [M, k k, C]
    y = win.max(1).values
    idx = win.argmax(1)           # the first maximum of the (ky, kx) scan
    dx = torch.zeros(n, H, W, C, dtype=torch.float64)
    m = torch.arange(n * Ho * Wo)
    b_, oy, ox = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    for c in range(C):
        iy, ix = oy * s - p + idx[:, c] // k, ox * s - p + idx[:, c] % k
        dx[:, :, :, c].index_put_((b_, iy, ix), dy[:, c].double(), accumulate=True)
    return dict(dims=dict(N=n, H=H, W=W, C=C, k=k, s=s, p=p), x=x, dy=dy, y=y, idx=idx, dx=dx.view(-1, C), M=n * Ho * Wo)


def pool_specs(dtype):
    q = _pool_problem(dtype)
    d, M, C = q['dims'], q['M'], q['dims']['C']
    idx8 = q['idx'].to(torch.uint8)
    yield Spec('resnet', '2x9x9x16', 'svol_maxpool_nhwc', dtype, d, OrderedDict(x=In(q['x'])), OrderedDict(y=Out((M, C), dtype)),
               lambda s: {'y': q['y']}, {'y': (0.0, 'l2')}, biteq=True)
    yield Spec('resnet', '2x9x9x16', 'svol_maxpool_idx_nhwc', dtype, d, OrderedDict(x=In(q['x'])),
               OrderedDict(y=Out((M, C), dtype), idx=Out((M, C), torch.uint8)), lambda s: {'y': q['y'], 'idx': q['idx'].double()},
               {'y': (0.0, 'l2'), 'idx': (0.0, 'abs')}, biteq=True)
    yield Spec('resnet', '2x9x9x16', 'svol_maxpool_bwd_nhwc', dtype, d, OrderedDict(dy=In(q['dy']), idx=In(idx8)),
               OrderedDict(dx=Out((d['N'] * d['H'] * d['W'], C), dtype)), lambda s: {'dx': q['dx']}, {'dx': (3e-3, 'l2')})
    n, HW, Ca = 3, 49, 40
    xa = _rnd((n * HW, Ca), dtype, 97)
    yield Spec('resnet', '3x49x40', 'svol_avgpool_nhwc', dtype, dict(N=n, HW=HW, C=Ca), OrderedDict(x=In(xa)), OrderedDict(y=Out((n, Ca), FP32)),
               lambda s: {'y': xa.double().view(n, HW, Ca).mean(1)}, {'y': (1e-5, 'abs')}, biteq=True)


def bn_specs(dtype):
    """train-mode BatchNorm's four kernels at M = 1237 rows (no multiple of any row chunk), C = 32 (include/svol_hip.h: C / 8 a divisor
    of 256, which 40 columns are not)"""
    M, C = 1237, 32
    z = _rnd((M, C), dtype, 100)
    dy, idt = _rnd((M, C), dtype, 101), _rnd((M, C), dtype, 102)
    gamma, beta = 1 + 0.1 * _rnd((C,), FP32, 103), 0.1 * _rnd((C,), FP32, 104)
    zd = z.double()
    sums = zd.sum(0)
    mean = (sums.float().double() / M)
    var = ((zd - mean) ** 2).sum(0) / M
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = (gamma.double() * rstd).float()
    shift = (beta.double() - mean * scale.double()).float()
    y = torch.relu(zd * scale.double() + shift.double() + idt.double())
    y16 = y.to(dtype)
    g = dy.double() * (y16.double() > 0)
    mean32, rstd32 = mean.float(), rstd.float()
    xhat = (zd - mean32.double()) * rstd32.double()
    sum_g, sum_gx = g.sum(0), (g * xhat).sum(0)
    sg32, sgx32 = sum_g.float(), sum_gx.float()
    dz = gamma.double() * rstd32.double() * (g - sg32.double() / M - xhat * sgx32.double() / M)
    d = dict(M=M, C=C)
    zero = lambda: Out((C,), FP32, init=torch.zeros(C))          # noqa: E731
    tag = f'M{M}C{C}'
    yield Spec('resnet', tag + '-sums', 'svol_bn_colstats', dtype, dict(d, shift_scale=0.0), OrderedDict(z=In(z)), OrderedDict(sum=zero(), sumsq=zero()),
               lambda s: {'sum': sums, 'sumsq': (zd ** 2).sum(0)}, {'sum': (1e-5, 'rel'), 'sumsq': (1e-5, 'rel')})
    yield Spec('resnet', tag + '-centred', 'svol_bn_colstats', dtype, dict(d, shift_scale=1.0 / M), OrderedDict(z=In(z), shift=In(sums.float())),
               OrderedDict(sum=zero(), sumsq=zero()), lambda s: {'sumsq': ((zd - mean) ** 2).sum(0)}, {'sumsq': (1e-5, 'rel')})
    yield Spec('resnet', tag, 'svol_bn_apply', dtype, dict(d, relu=1), OrderedDict(z=In(z), scale=In(scale), shift=In(shift), residual=In(idt)),
               OrderedDict(y=Out((M, C), dtype)), lambda s: {'y': y}, {'y': (4e-3, 'l2')})
    yield Spec('resnet', tag, 'svol_bn_bwd_reduce', dtype, d, OrderedDict(dy=In(dy), y=In(y16), z=In(z), mean=In(mean32), rstd=In(rstd32)),
               OrderedDict(sum_g=zero(), sum_gx=zero()), lambda s: {'sum_g': sum_g, 'sum_gx': sum_gx}, {'sum_g': (1e-5, 'l2'), 'sum_gx': (1e-5, 'l2')})
    yield Spec('resnet', tag, 'svol_bn_bwd_apply', dtype, d,
               OrderedDict(dy=In(dy), y=In(y16), z=In(z), mean=In(mean32), rstd=In(rstd32), gamma=In(gamma), sum_g=In(sg32), sum_gx=In(sgx32)),
               OrderedDict(dz=Out((M, C), dtype), dres=Out((M, C), dtype)), lambda s: {'dz': dz, 'dres': g}, {'dz': (4e-3, 'l2'), 'dres': (1e-6, 'l2')})


def conv_train_specs(dtype):
    """the gathers of the backward pass at an odd image: col2im, the weight gradient gathered inside the GEMM, the weight pack"""
    n, H, W, C, Cout, k, s, p = 3, 9, 11, 16, 32, 3, 2, 1
    Ho, Wo = _out_hw(H, W, k, s, p)
    M, K = n * Ho * Wo, k * k * C
    Kp = (K + 31) // 32 * 32
    d = dict(N=n, H=H, W=W, C=C, Cout=Cout, k=k, s=s, p=p, Kp=Kp)
    tag = f'{n}x{H}x{W}x{C}-{Cout}k{k}s{s}p{p}'
    dcols = _rnd((M, K), dtype, 110)
    x = _rnd((n * H * W, C), dtype, 111)
    dz = _rnd((M, Cout), dtype, 112)
    w = _rnd((Cout, C, k, k), FP32, 113, 0.1)

    def col2im_ref(sp):
        c5 = dcols.double().view(n, Ho * Wo, k, k, C).permute(0, 4, 2, 3, 1).reshape(n, C * k * k, Ho * Wo)
        return {'dx': _nhwc(F.fold(c5, (H, W), k, padding=p, stride=s))}
    # dcols: K columns of rows Kp apart -- the header gives columns K .. ldcols - 1 of dcols no meaning
    yield Spec('resnet', tag, 'svol_col2im_nhwc', dtype, d, OrderedDict(dcols=In(dcols, Kp, 0)), OrderedDict(dx=Out((n * H * W, C), dtype)), col2im_ref,
               {'dx': (5e-3, 'l2')})

    def wgrad_ref(sp):
        out = torch.zeros(Cout, Kp, dtype=torch.float64)
        out[:, :K] = dz.double().t() @ _unfold(_nchw(x, n, H, W, C), k, s, p)
        return {'dwp': out}
    yield Spec('resnet', tag, 'svol_conv_wgrad_nhwc', dtype, d, OrderedDict(dz=In(dz), x=In(x)),
               OrderedDict(dwp=Out((Cout, Kp), FP32, init=torch.zeros(Cout, Kp))), wgrad_ref, {'dwp': (1e-5, 'l2')})
    for flip in (0, 1):
        rows = C if flip else Cout
        Kf = k * k * (Cout if flip else C)
        Kpf = (Kf + 31) // 32 * 32 + 32          # one spare 32-column group: zero beyond kh kw Cin

        def pack_ref(sp, flip=flip, rows=rows, Kf=Kf, Kpf=Kpf):
            out = torch.zeros(rows, Kpf, dtype=torch.float64)
            w16 = w.to(dtype).double()
            out[:, :Kf] = (w16.flip(2, 3).permute(1, 2, 3, 0) if flip else w16.permute(0, 2, 3, 1)).reshape(rows, Kf)
            return {'out': out}
        yield Spec('resnet', f'{tag}-flip{flip}', 'svol_conv_weight_pack', dtype, dict(d, Kp=Kpf, flip=flip), OrderedDict(w=In(w)),
                   OrderedDict(out=Out((rows, Kpf), dtype)), pack_ref, {'out': (0.0, 'l2')})


def resnet_specs(dtype):
    for i in range(len(CONVS)):
        yield conv_spec(i, dtype)
    yield im2col_spec(dtype, False)
    yield im2col_spec(dtype, True)
    yield from pool_specs(dtype)
    yield from bn_specs(dtype)
    yield from conv_train_specs(dtype)
