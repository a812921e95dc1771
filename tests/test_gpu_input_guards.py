"""No kernel result may depend on memory outside its operands.

tests/test_gpu_guards.py puts red zones around everything a kernel WRITES; this file does the same for what it READS.  Every input
operand of a call -- bias, key bias, statistics, index tensors included -- is a slot of one arena (tests/guard_arena.py), column
slices with the rest of their rows as gap words, packed q | k | v rows as the model lays them out; outputs and scratch are slots of
a second arena.  The call runs three times: the input arena's guards and gaps hold fp32 -0.0, then NaN, then 6.7e35 / 57344 (finite and
huge: what a max or a compare would let through where it swallows a NaN).  After each run the return code is SVOL_OK, both arenas'
guards and gaps are bit-identical to their fill, every output is finite and meets its fp64 reference at the bar tests/gpu_checks.py
holds that op to; entries the suite holds to run-to-run bit equality give the same bits under all three fills.  A kernel that
stages a ragged tile without predicating it, uses a tile it prefetched too far, reads a neighbour's columns of a packed row or
gathers padding pixels from the previous image row fails here, whatever the allocator happens to leave behind its operands
elsewhere.  The 256 KB guards keep every such read inside the one allocation.

The case tables, their fp64 references and the dispatch twins that say which kernel a case reaches are tests/input_guard_cases.py
(held to the twins on the CPU by tests/test_input_guard_cases.py).  All calls go through the C-ABI with raw pointers and explicit
leading dimensions.
"""
import ctypes
import math

import pytest
import torch

from tests import input_guard_cases as G
from tests.guard_arena import FILLS, NEG0, GuardArena

pytestmark = pytest.mark.gpu
DT_IDS = {G.FP32: 'fp32', G.BF16: 'bf16', G.FP16: 'fp16'}


def _api():
    from svol_amd import _lib, ops
    return _lib.lib(), _lib, ops


def _P(t):
    return 0 if t is None else t.data_ptr()


# ---- one adapter per entry point: (lib, spec, inputs, outputs, dtype code, stream) -> return code ---------------------------------
def _ld(t):
    return t.stride(0)


def _gemm_nt(L, s, i, o, dt, st):
    d = s.dims
    C = o['C']
    if d['entry'] == 'split':
        return L.svol_gemm_nt_split(_P(i['A']), _ld(i['A']), _P(i['B']), _ld(i['B']), _P(C), _ld(C), _P(i['bias']), d['M'], d['N'], d['K'], st)
    if d['entry'] == 'dact':
        return L.svol_gemm_nt_dact(_P(i['A']), _ld(i['A']), _P(i['B']), _ld(i['B']), _P(C), _ld(C), _P(i['aux']), _ld(i['aux']), d['act'],
                                   _P(o.get('colsum')), d['M'], d['N'], d['K'], dt, st)
    pre, res = o.get('pre'), i.get('res')
    return L.svol_gemm_nt(_P(i['A']), _ld(i['A']), None, 0, _P(i['B']), _ld(i['B']), _P(C), _ld(C), _P(i.get('bias')), _P(i.get('colscale')), d['act'],
                          _P(pre), _ld(pre) if pre is not None else 0, _P(res), _ld(res) if res is not None else 0, d['out_f32'], d['M'], d['N'],
                          d['K'], dt, st)


def _gemm_tn(L, s, i, o, dt, st):
    from svol_amd import _lib
    n = s.dims['n']
    arr = (_lib.TnProblem * n)()
    for j, (Mc, N, K) in enumerate(s.dims['probs']):
        a, b, c = i[f'A{j}'], i[f'B{j}'], o[f'C{j}']
        arr[j] = _lib.TnProblem(_P(a), _ld(a), _P(b), _ld(b), _P(c), _ld(c), _P(o[f'cs{j}']), Mc, N, K)
    if s.entry == 'svol_gemm_tn_grouped':
        return L.svol_gemm_tn_grouped(ctypes.cast(arr, ctypes.c_void_p), n, dt, st)
    q = arr[0]
    return L.svol_gemm_tn(q.A, q.lda, q.B, q.ldb, q.C, q.ldc, q.colsum, q.Mc, q.N, q.K, dt, st)


def _attn_dims(s):
    d = s.dims
    return d['B'], d['H'], d['Lq'], d['Lk'], d['dh'], 1.0 / math.sqrt(d['dh']), float(d['pm'])


def _attn_fwd(L, s, i, o, dt, st):
    B, H, Lq, Lk, dh, sc, pm = _attn_dims(s)
    ws = o.get('ws')
    return L.svol_attn_fwd(_P(i['q']), _ld(i['q']), _P(i['k']), _ld(i['k']), _P(i['v']), _ld(i['v']), _P(o['o']), _ld(o['o']), _P(o['lse2']),
                           _P(i.get('kbias')), B, H, Lq, Lk, dh, sc, pm, _P(ws), ws.numel() * 4 if ws is not None else 0, dt, st)


def _attn_bwd(L, s, i, o, dt, st):
    B, H, Lq, Lk, dh, sc, pm = _attn_dims(s)
    ws = o.get('ws')
    return L.svol_attn_bwd(_P(i['q']), _ld(i['q']), _P(i['k']), _ld(i['k']), _P(i['v']), _ld(i['v']), _P(i['o']), _ld(i['o']), _P(i['do']),
                           _ld(i['do']), _P(i['lse2']), _P(o['delta']), _P(i.get('kbias')), _P(o['dq']), _ld(o['dq']), _P(o['dk']), _ld(o['dk']),
                           _P(o['dv']), _ld(o['dv']), B, H, Lq, Lk, dh, sc, pm, _P(ws), ws.numel() * 4 if ws is not None else 0, dt, st)


def _attn_weights(L, s, i, o, dt, st):
    B, H, Lq, Lk, dh, sc, pm = _attn_dims(s)
    return L.svol_attn_weights_mean(_P(i['q']), _ld(i['q']), _P(i['k']), _ld(i['k']), _P(i['lse2']), _P(i.get('kbias')), _P(o['att']), B, H, Lq, Lk,
                                    dh, sc, pm, dt, st)


def _attn_short(fwd):
    def call(L, s, i, o, dt, st):
        d = s.dims
        fn = getattr(L, s.entry)
        sc = 1.0 / math.sqrt(d['dh'])
        head = (_P(i['q']), _ld(i['q']), _P(i['k']), _ld(i['k']), _P(i['v']), _ld(i['v']))
        if fwd:
            return fn(*head, _P(o['o']), _ld(o['o']), _P(o['lse2']), d['n'], d['H'], d['L'], d['dh'], sc, dt, st)
        return fn(*head, _P(i['o']), _ld(i['o']), _P(i['do']), _ld(i['do']), _P(i['lse2']), _P(o['dq']), _ld(o['dq']), _P(o['dk']), _ld(o['dk']),
                  _P(o['dv']), _ld(o['dv']), d['n'], d['H'], d['L'], d['dh'], sc, dt, st)
    return call


def _ln_fwd(L, s, i, o, dt, st):
    d = s.dims
    return L.svol_layernorm_fwd(_P(i['x']), d['x_f32'], _P(i['gamma']), _P(i['beta']), _P(o['y32']), _P(o['y']), _P(o['ypos']), _P(i['pos']),
                                d['pos_rows'], _P(o['mean']), _P(o['rstd']), d['M'], d['D'], 0.0, 0, None, dt, st)


def _ln_bwd(L, s, i, o, dt, st):
    d = s.dims
    return L.svol_layernorm_bwd(_P(i['dy32']), _P(i['dy']), _P(i['dy2']), _P(i['x']), d['x_f32'], _P(i['gamma']), _P(i['mean']), _P(i['rstd']),
                                _P(o['dx32']), _P(o['dx']), _P(o['dgamma']), _P(o['dbeta']), _P(o['colsum']), d['M'], d['D'], 0.0, 0, None, dt, st)


def _gate_fwd(L, s, i, o, dt, st):
    d = s.dims
    return getattr(L, s.entry)(_P(i['x32']), _P(i['pos']), _P(i['u']), _P(i['gamma']), _P(i['beta']), _P(o['y32']), _P(o['y']), _P(o['ypos']),
                               _P(o['a']), _P(o['mean']), _P(o['rstd']), _P(o['ws']), d['B'], d['L'], d['D'], d['H'], dt, st)


def _ln_gate_scores(L, s, i, o, dt, st):
    d = s.dims
    return L.svol_layernorm_gate_scores_fwd(_P(i['x32']), _P(i['gamma']), _P(i['beta']), _P(o['y32']), _P(o['y']), _P(o['ypos']), _P(i['pos']),
                                            _P(o['mean']), _P(o['rstd']), _P(i['u_next']), _P(o['scores']), d['B'], d['L'], d['D'], d['H'], dt, st)


def _gate_bwd(L, s, i, o, dt, st):
    d = s.dims
    return L.svol_gate_bwd(_P(i['dy32']), _P(i['dy']), _P(i['dy2']), _P(i['x32']), _P(i['pos']), _P(i['u']), _P(i['gamma']), _P(i['a']),
                           _P(i['mean']), _P(i['rstd']), _P(i['ws']), _P(o['ws2']), _P(o['dx32']), _P(o['du']), _P(o['dgamma']), _P(o['dbeta']),
                           d['B'], d['L'], d['D'], d['H'], dt, st)


def _conv(L, s, i, o, dt, st):
    d = s.dims
    return L.svol_conv_nhwc(_P(i['x']), _P(i['w']), _ld(i['w']), _P(o['y']), _P(i['bias']), d['act'], _P(i.get('residual')), d['N'], d['H'], d['W'],
                            d['C'], d['Cout'], d['k'], d['k'], d['s'], d['p'], dt, st)


def _im2col(L, s, i, o, dt, st):
    d = s.dims
    sn, sh, sw, sc = d['strides']
    return L.svol_im2col(_P(i['x']), sn, sh, sw, sc, 0 if d['src_f32'] else dt, _P(o['cols']), d['Kp'], d['N'], d['H'], d['W'], d['C'], d['k'],
                         d['k'], d['s'], d['p'], dt, st)


def _geom(d):
    return d['N'], d['H'], d['W'], d['C']


CALLS = {
    'svol_gemm_nt': _gemm_nt, 'svol_gemm_nt_split': _gemm_nt, 'svol_gemm_nt_dact': _gemm_nt, 'svol_gemm_tn': _gemm_tn,
    'svol_gemm_tn_grouped': _gemm_tn, 'svol_attn_fwd': _attn_fwd, 'svol_attn_bwd': _attn_bwd, 'svol_attn_weights_mean': _attn_weights,
    'svol_attn_small_fwd_lse_h16': _attn_short(True), 'svol_attn_small_bwd_h16': _attn_short(False),
    'svol_attn_cls_fwd_h16': _attn_short(True), 'svol_attn_cls_bwd_h16': _attn_short(False),
    'svol_layernorm_fwd': _ln_fwd, 'svol_layernorm_bwd': _ln_bwd, 'svol_gate_fwd': _gate_fwd, 'svol_gate_fwd_scored': _gate_fwd,
    'svol_layernorm_gate_scores_fwd': _ln_gate_scores, 'svol_gate_bwd': _gate_bwd,
    'svol_gate_vectors_fwd': lambda L, s, i, o, dt, st: L.svol_gate_vectors_fwd(_P(i['skch']), _P(i['W_in']), _P(i['b_in']), _P(o['q']), _P(o['u']),
                                                                                s.dims['B'], s.dims['D'], s.dims['H'], st),
    'svol_gate_vectors_bwd': lambda L, s, i, o, dt, st: L.svol_gate_vectors_bwd(_P(i['du']), _P(i['skch']), _P(i['W_in']), _P(i['q']), _P(o['dq_ws']),
                                                                                _P(o['dskch']), _P(o['dW_in']), _P(o['db_in']), s.dims['B'],
                                                                                s.dims['D'], s.dims['H'], st),
    'svol_dropout': lambda L, s, i, o, dt, st: L.svol_dropout(_P(i['x']), _P(o['y']), s.dims['n'], s.dims['row_len'], s.dims['p'], s.dims['seed'], dt, st),
    'svol_dropout_add': lambda L, s, i, o, dt, st: L.svol_dropout_add(_P(i['t32']), _P(i['res32']), _P(o['out32']), s.dims['n'], s.dims['row_len'],
                                                                      s.dims['p'], s.dims['seed'], st),
    'svol_act_bwd': lambda L, s, i, o, dt, st: L.svol_act_bwd(_P(i['dy']), _P(i['aux']), _P(o['dpre']), s.dims['act'], s.dims['n'], dt, st),
    'svol_colsum': lambda L, s, i, o, dt, st: L.svol_colsum(_P(i['X']), _ld(i['X']), _P(o['out']), s.dims['M'], s.dims['N'], dt, st),
    'svol_cast': lambda L, s, i, o, dt, st: L.svol_cast(_P(i['src']), 0, _P(o['dst']), dt, s.dims['n'], st),
    'svol_cast_transpose': lambda L, s, i, o, dt, st: L.svol_cast_transpose(_P(i['src']), _P(o['dst']), _P(o['dstT']), dt, s.dims['R'], s.dims['C'], st),
    'svol_posenc_sine': lambda L, s, i, o, dt, st: L.svol_posenc_sine(_P(i['mask']), _P(o['pos']), s.dims['B'], s.dims['L'], s.dims['D'], dt, st),
    'svol_conv_nhwc': _conv, 'svol_im2col': _im2col,
    'svol_maxpool_nhwc': lambda L, s, i, o, dt, st: L.svol_maxpool_nhwc(_P(i['x']), _P(o['y']), *_geom(s.dims), s.dims['k'], s.dims['s'], s.dims['p'], dt, st),
    'svol_maxpool_idx_nhwc': lambda L, s, i, o, dt, st: L.svol_maxpool_idx_nhwc(_P(i['x']), _P(o['y']), _P(o['idx']), *_geom(s.dims), s.dims['k'],
                                                                                s.dims['s'], s.dims['p'], dt, st),
    'svol_maxpool_bwd_nhwc': lambda L, s, i, o, dt, st: L.svol_maxpool_bwd_nhwc(_P(i['dy']), _P(i['idx']), _P(o['dx']), *_geom(s.dims), s.dims['k'],
                                                                                s.dims['s'], s.dims['p'], dt, st),
    'svol_avgpool_nhwc': lambda L, s, i, o, dt, st: L.svol_avgpool_nhwc(_P(i['x']), _P(o['y']), s.dims['N'], s.dims['HW'], s.dims['C'], dt, st),
    'svol_bn_colstats': lambda L, s, i, o, dt, st: L.svol_bn_colstats(_P(i['z']), _P(i.get('shift')), s.dims['shift_scale'], _P(o['sum']), _P(o['sumsq']),
                                                                      s.dims['M'], s.dims['C'], dt, st),
    'svol_bn_apply': lambda L, s, i, o, dt, st: L.svol_bn_apply(_P(i['z']), _P(i['scale']), _P(i['shift']), _P(i['residual']), s.dims['relu'], _P(o['y']),
                                                                s.dims['M'], s.dims['C'], dt, st),
    'svol_bn_bwd_reduce': lambda L, s, i, o, dt, st: L.svol_bn_bwd_reduce(_P(i['dy']), _P(i['y']), _P(i['z']), _P(i['mean']), _P(i['rstd']), _P(o['sum_g']),
                                                                          _P(o['sum_gx']), s.dims['M'], s.dims['C'], dt, st),
    'svol_bn_bwd_apply': lambda L, s, i, o, dt, st: L.svol_bn_bwd_apply(_P(i['dy']), _P(i['y']), _P(i['z']), _P(i['mean']), _P(i['rstd']), _P(i['gamma']),
                                                                        _P(i['sum_g']), _P(i['sum_gx']), _P(o['dz']), _P(o['dres']), s.dims['M'],
                                                                        s.dims['C'], dt, st),
    'svol_col2im_nhwc': lambda L, s, i, o, dt, st: L.svol_col2im_nhwc(_P(i['dcols']), _ld(i['dcols']), _P(o['dx']), *_geom(s.dims), s.dims['k'],
                                                                      s.dims['k'], s.dims['s'], s.dims['p'], dt, st),
    'svol_conv_wgrad_nhwc': lambda L, s, i, o, dt, st: L.svol_conv_wgrad_nhwc(_P(i['dz']), _P(i['x']), _P(o['dwp']), *_geom(s.dims), s.dims['Cout'],
                                                                              s.dims['k'], s.dims['k'], s.dims['s'], s.dims['p'], s.dims['Kp'], dt, st),
    'svol_conv_weight_pack': lambda L, s, i, o, dt, st: L.svol_conv_weight_pack(_P(i['w']), _P(o['out']), s.dims['Cout'], s.dims['C'], s.dims['k'],
                                                                                s.dims['k'], s.dims['Kp'], s.dims['flip'], dt, st),
}


# ---- the runner ---------------------------------------------------------------------------------------------------------------
def _plan(ar, items, shape_of, dtype_of):
    """dense slots, strided slots and packed slots (several operands in column ranges of one dense buffer)"""
    packed = {}
    for name, x in items.items():
        shape, dtype = shape_of(x), dtype_of(x)
        if x.slot is not None:
            if x.slot not in packed:
                packed[x.slot] = []
                ar.plan(x.slot, (shape[0], x.ld), dtype)
            packed[x.slot].append((name, x.col, shape[1]))
        elif x.ld is not None:
            ar.plan(name, shape, dtype, x.ld, x.col)
        else:
            ar.plan(name, shape, dtype)
    t = ar.build()
    for slot, members in packed.items():
        at = 0
        for _, col, w in sorted(members, key=lambda m: m[1]):
            assert col == at, f'{slot}: a packed buffer holds operands only, side by side'
            at += w
        assert at == t[slot].shape[1], slot
        for name, col, w in members:
            t[name] = t[slot][:, col:col + w]
    return t


def _raw(t):
    return t.contiguous().view(-1).view(torch.uint8).clone()


def run_spec(s):
    L, _lib, ops = _api()
    call = CALLS[s.entry]
    ain, aout = GuardArena(), GuardArena()
    tin = _plan(ain, s.ins, lambda x: tuple(x.t.shape), lambda x: x.t.dtype)
    for name, x in s.ins.items():
        tin[name].copy_(x.t)
    outs = dict(s.outs)
    if s.dims.get('ws'):          # the attention scratch: as large as the library asks for this shape
        d = s.dims
        need = int(L.svol_attn_ws_bytes(d['B'], d['H'], d['Lq'], d['Lk'], d['dh']))
        if need:
            outs['ws'] = G.Out((need // 4,), G.FP32, scratch=True)
    tout = _plan(aout, outs, lambda o: o.shape, lambda o: o.dtype)
    ref = s.ref()
    dt, st = ops._DT[s.dtype], ops._stream()
    first = {}
    for fill_name, word in FILLS:
        what = f'{s.id} [{fill_name} behind the inputs]'
        ain.refill(word)
        for name, o in outs.items():
            if o.init is not None:
                tout[name].copy_(o.init)
            elif o.scratch:
                tout[name].fill_(-0.0)
            elif o.dtype.is_floating_point:
                tout[name].fill_(float('nan'))          # an output the call must write: poisoned
            else:
                tout[name].fill_(255)
        rc = call(L, s, tin, tout, dt, st)
        torch.cuda.synchronize()
        assert rc == 0, f'{what}: return code {rc} ({_lib.lib().svol_strerror(rc).decode()}): a wrong table row, not a skip'
        ain.check(what + ', input arena')
        aout.check(what + ', output arena')
        for name, x in s.ins.items():
            assert torch.equal(_raw(tin[name]), _raw(x.t.to(tin[name].device))), f'{what}: input {name} was written'
        for name, o in outs.items():
            if o.scratch:
                continue
            got = tout[name].double().cpu()
            assert bool(torch.isfinite(got).all()), f'{what}: output {name} is not finite ({int((~torch.isfinite(got)).sum())} of {got.numel()} elements)'
            if name in ref:
                tol, metric = s.bars[name]
                err = METRIC(metric)(got, ref[name].reshape(got.shape), s)
                assert err <= tol, f'{what}: output {name}: {err:.3e} > {tol:.1e}'
            if s.biteq:
                if fill_name == 'neg0':
                    first[name] = _raw(tout[name])
                else:
                    assert torch.equal(first[name], _raw(tout[name])), f'{what}: output {name} differs in bits from the run over -0.0 guards'


def METRIC(m):
    if callable(m):
        return lambda got, ref, s: m(got, ref, s=s)
    return lambda got, ref, s: G.METRICS[m](got, ref)


def _run_all(specs):
    n = 0
    for s in specs:
        run_spec(s)
        n += 1
    assert n > 0


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the families ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', G.ALL, ids=DT_IDS.get)
def test_gemm_nt_reads_only_its_operands(dtype):
    """svol_gemm_nt / _split / _dact: one case per family of gemm_call.h's NT cascade, ragged M, A, B, res, pre and aux as column
    slices; the balanced deep-K variant at 128 x CUs + 5 rows of this device"""
    names = [n for n, r in G.GEMM_NT.items() if dtype in r['dtypes']]
    cus = _cus()
    if dtype != G.FP32:
        assert G.gemm_nt_family_of(G.GEMM_NT['n256_balanced'], dtype, cus) == (2, 'balanced')
    _run_all(G.gemm_nt_spec(n, dtype, cus) for n in names)


@pytest.mark.parametrize('dtype', G.ALL, ids=DT_IDS.get)
def test_gemm_tn_reads_only_its_operands(dtype):
    """svol_gemm_tn / _grouped: ragged row chunks, A and B as column slices, two problems whose operands are neighbours, non-zero targets"""
    _run_all(G.gemm_tn_spec(n, dtype) for n, r in G.GEMM_TN.items() if dtype in r['dtypes'])


ATTN_POINTS = [(row, dt) for row in G.ATTN_ROWS for dt in G.attn_dtypes(row)]          # (a case without an fp32 twin in its table has no fp32 point)


@pytest.mark.parametrize('row,dtype', ATTN_POINTS, ids=[f'{G.attn_row_id(r)}-{DT_IDS[d]}' for r, d in ATTN_POINTS])
def test_attention_reads_only_its_operands(row, dtype):
    """svol_attn_fwd / _bwd at every launch plan of the two tables: q | k | v from one packed [M, 3d] buffer (self-attention) or k | v
    from [B Lk, 2d] (cross-attention); ragged key counts also with B = 1, where the only key tail borders the guard"""
    _run_all(G.attn_spec(row, dtype, kind) for kind in ('fwd', 'bwd'))
    G.attn_problem.cache_clear()


@pytest.mark.parametrize('dtype', G.ALL, ids=DT_IDS.get)
def test_attention_weights_read_only_their_operands(dtype):
    _run_all(G.attn_weights_spec(n, dtype) for n in G.ATTN_WEIGHTS)


@pytest.mark.parametrize('dtype', G.H16, ids=DT_IDS.get)
def test_short_sequence_attention_reads_only_its_operands(dtype):
    """svol_attn_small_* (packed q | k | v) and svol_attn_cls_* (one query, packed k | v) in both 16-bit types"""
    _run_all(G.attn_small_spec(L, dh, dtype, kind) for L, dh in G.ATTN_SMALL for kind in ('fwd', 'bwd'))
    _run_all(G.attn_cls_spec(L, dh, dtype, kind) for L, dh in G.ATTN_CLS for kind in G.attn_cls_kinds(L))


@pytest.mark.parametrize('M', G.LN_MS)
@pytest.mark.parametrize('dtype', G.ALL, ids=DT_IDS.get)
def test_layernorm_reads_only_its_operands(dtype, M):
    """svol_layernorm_fwd / _bwd: every width path, pos of exactly pos_rows x D with pos_rows < M, and row counts at which the
    backward walks more than one row per wave"""
    _run_all(G.ln_spec(M, D, dtype, kind) for D in G.LN_DS for kind in ('fwd', 'bwd'))
    G._ln_problem.cache_clear()


@pytest.mark.parametrize('dtype', G.ALL, ids=DT_IDS.get)
def test_gate_reads_only_its_operands(dtype):
    """svol_gate_fwd / _bwd / _fwd_scored / svol_layernorm_gate_scores_fwd"""
    _run_all(G.gate_spec(sh, dtype, entry) for sh, entry in G.gate_points())
    G._gate_problem.cache_clear()


@pytest.mark.parametrize('dtype', G.ALL, ids=DT_IDS.get)
def test_small_row_kernels_read_only_their_operands(dtype):
    """dropout, dropout-add, act_bwd, colsum on a slice, cast, cast-transpose, the sine position encoding, the gate vectors"""
    _run_all(G.small_op_specs(dtype))


@pytest.mark.parametrize('dtype', G.H16, ids=DT_IDS.get)
def test_resnet_kernels_read_only_their_operands(dtype):
    """the gathered-A convolution (image borders at the guards), im2col from both layouts, the pools, train-mode BatchNorm, col2im, the
    weight gradient gathered inside the GEMM, the weight pack"""
    _run_all(G.resnet_specs(dtype))


def test_the_guards_are_the_existing_width():
    assert GuardArena().guard * 4 == 1 << 18 and GuardArena().fill == NEG0


def test_a_read_past_an_operand_is_seen_under_the_second_fill():
    """The harness against a call that does depend on memory outside an operand: the 128 x 128 tile GEMM is handed an A slot that ends
    32 columns short of the K it is told.  Those columns are gap words of A's own rows (the read stays inside the arena).  Over -0.0 the
    product is that of A padded with zeros and every check passes -- the forgiving neighbour the suite has lived with; over NaN the run
    fails."""
    s, padded = G.gemm_nt_spec('tiles_k32', G.BF16), G.gemm_nt_spec('tiles_k32', G.BF16)
    K, a = s.dims['K'], s.ins['A']
    assert a.ld - a.col - K >= 0 and a.col + K <= a.ld
    s.ins['A'] = G.In(a.t[:, :K - 32].contiguous(), a.ld, a.col)
    full = a.t.clone()
    full[:, K - 32:] = 0
    padded.ins['A'] = G.In(full, a.ld, a.col)
    ref = padded.ref()
    s._ref = lambda _s: ref
    with pytest.raises(AssertionError, match=r'\[nan behind the inputs\]: output \w+ is not finite'):
        run_spec(s)
