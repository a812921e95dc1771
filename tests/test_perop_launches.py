"""The per-op autograd path on CPU tensors against a recording stand-in for the library: which C entry points each Function
calls and in which order, where its weight-gradient GEMMs write, which parameter gradients it hands back to autograd and how many
zero fills it allocates — in the modes {no gradient sinks, every sink, one sink missing} x {LN, no LN} x {dropout, none}.

The expected sequences are written out below from the Functions' code; the stand-in computes nothing, so every assertion is about
call structure, never about values.
"""
import itertools

import pytest
import torch

from svol_amd import _lib, ops, wgrad
from svol_amd import layers as Lyr, params as P

D, F, B, L, H = 32, 64, 2, 8, 4
BF, F32 = torch.bfloat16, torch.float32
MODES = ('none', 'all', 'one')


class _Recorder:
    """every svol_* attribute records (name, args) and returns 0"""

    def __init__(self):
        self.calls, self.zeros, self.adds = [], 0, []

    def __getattr__(self, name):
        if not name.startswith('svol_'):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name[5:], args))
            return 0
        return call

    def names(self, start=0):
        return [n for n, _ in self.calls[start:]]


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(_lib, 'lib', lambda: r)
    monkeypatch.setattr(_lib, 'check', lambda rc, name: None)
    for mod in (ops, Lyr):
        monkeypatch.setattr(mod, '_ptr', lambda t: 0 if t is None else t.data_ptr())
        monkeypatch.setattr(mod, '_stream', lambda: 0)
    monkeypatch.setattr(ops, '_current_stream_obj', lambda: None)
    monkeypatch.setattr(wgrad, 'ASYNC', False)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    zeros, add_ = torch.zeros, torch.Tensor.add_

    def counted_zeros(*a, **k):
        r.zeros += 1
        return zeros(*a, **k)

    def logged_add_(self, *a, **k):
        r.adds.append(self.data_ptr())
        return add_(self, *a, **k)
    monkeypatch.setattr(torch, 'zeros', counted_zeros)
    monkeypatch.setattr(torch.Tensor, 'add_', logged_add_)
    return r


def _param(*shape):
    return torch.nn.Parameter(torch.randn(*shape))


def _act(*shape, dtype=BF):
    return torch.randn(*shape).to(dtype).requires_grad_(True)


def _give_sinks(params, mode, missing):
    """the way BucketedGradAllReduce makes them: p.grad is a view of a flat bucket, p._svol_sink = GradSink(p.grad).
    -> {name: (first byte, past-the-end byte)} of the sink views"""
    have = [n for n in params if mode == 'all' or (mode == 'one' and n != missing)]
    flat = torch.full((sum(params[n].numel() for n in have) + 1,), 7.0)
    spans, o = {}, 0
    for n in have:
        p = params[n]
        p.grad = flat[o:o + p.numel()].view_as(p)
        p._svol_sink = P.GradSink(p.grad)
        spans[n] = (p.grad.data_ptr(), p.grad.data_ptr() + 4 * p.numel())
        o += p.numel()
    return spans


def _check(rec, outs, params, spans, fwd, bwd, direct, nzeros, adds=()):
    """fwd / bwd: the expected symbol sequences; direct: per svol_gemm_tn of the backward, whether it writes into sinks; nzeros: zero
    fills of the backward; adds: the parameters whose sink gets an add_ from the Function."""
    assert rec.names() == fwd
    n0, rec.zeros, rec.adds = len(rec.calls), 0, []
    outs = [o for o in (outs if isinstance(outs, tuple) else (outs,)) if o.requires_grad]
    names = list(params)
    grads = torch.autograd.grad(outs, [params[n] for n in names], [torch.ones_like(o) for o in outs], allow_unused=True)
    assert rec.names(n0) == bwd
    inside = lambda ptr: any(a <= ptr < b for a, b in spans.values())
    tn = [a for n, a in rec.calls[n0:] if n == 'gemm_tn']
    assert len(tn) == len(direct)
    for a, dr in zip(tn, direct):
        assert inside(a[4]) == dr, 'out of a svol_gemm_tn'
        if a[6]:
            assert inside(a[6]) == dr, 'colsum of a svol_gemm_tn'
    # a gradient is handed to autograd exactly where no sink took it
    assert {n: g is None for n, g in zip(names, grads)} == {n: n in spans for n in names}
    assert rec.zeros == nzeros
    assert sorted(rec.adds) == sorted(spans[n][0] for n in adds)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_linear_out_features_multiple_of_8(rec, mode):
    prm = {'W': _param(16, D), 'b': _param(16)}
    spans = _give_sinks(prm, mode, 'b')
    y = Lyr.linear(_act(B, L, D), prm['W'], prm['b'], ops.ACT_RELU)
    direct = mode == 'all'
    _check(rec, y, prm, spans, ['cast_transpose', 'gemm_nt'], ['act_bwd', 'gemm_tn', 'gemm_nt'], [direct], 0 if direct else 1,
           ['W'] if mode == 'one' else [])


@pytest.mark.parametrize('mode', MODES)
def test_linear_two_out_features_never_uses_sinks(rec, mode):
    prm = {'W': _param(2, D), 'b': _param(2)}
    _give_sinks(prm, mode, 'b')
    y = Lyr.linear(_act(B, L, D), prm['W'], prm['b'])
    # zero-padded dy and W^T, and the dW | db buffer
    _check(rec, y, prm, {}, ['cast_transpose', 'gemm_nt'], ['gemm_tn', 'gemm_nt'], [False], 3)


def _open_bwd(ln, drop, cast_first=True):
    """the opening of a residual block's backward"""
    if drop:
        return (['layernorm_bwd'] if ln else (['cast'] if cast_first else [])) + ['dropout', 'colsum']
    return ['layernorm_bwd'] if ln else (['cast'] if cast_first else []) + ['colsum']


def _open_zeros(have, ln, drop, bias):
    """zero fills of that opening: layernorm_bwd's dgamma | dbeta | column-sum rows, colsum's own output"""
    if ln and drop:
        return int(not ('gamma' in have and 'beta' in have)) + int(bias not in have)
    if ln:
        return int(not all(n in have for n in ('gamma', 'beta', bias)))
    return int(bias not in have)


@pytest.mark.parametrize('mode,ln,drop,act', [m + (a,) for m in itertools.product(MODES, (True, False), (True, False))
                                              for a in (ops.ACT_GELU, ops.ACT_RELU)])
def test_mlp_ln(rec, mode, ln, drop, act):
    prm = {'W1': _param(F, D), 'b1': _param(F), 'W2': _param(D, F), 'b2': _param(D)}
    if ln:
        prm.update(gamma=_param(D), beta=_param(D))
    spans = _give_sinks(prm, mode, 'W1')
    outs = Lyr.mlp_ln(_act(B, L, D, dtype=F32), _act(B, L, D), prm['W1'], prm['b1'], prm['W2'], prm['b2'], prm.get('gamma'),
                      prm.get('beta'), None, act, (0.1, 11, 12) if drop else None)
    fwd = ['cast_transpose', 'cast_transpose', 'gemm_nt'] + (['dropout', 'gemm_nt', 'dropout_add'] if drop else ['gemm_nt'])
    fwd += ['layernorm_fwd'] if ln else []
    bwd = _open_bwd(ln, drop) + ['gemm_tn', 'gemm_nt_dact'] + (['dropout', 'colsum'] if drop else []) + ['gemm_tn', 'gemm_nt']
    direct = mode == 'all'
    nz = _open_zeros(spans, ln, drop, 'b2') + int(not direct) + int('b1' not in spans)
    _check(rec, outs, prm, spans, fwd, bwd, [direct, direct], nz, ['W2'] if mode == 'one' else [])


@pytest.mark.parametrize('mode,ln,drop,kind', [m + (k,) for m in itertools.product(MODES, (True, False), (True, False))
                                               for k in ('self', 'cross', 'mixed')])
def test_attn_ln(rec, mode, ln, drop, kind):
    prm = {'W_in': _param(3 * D, D), 'b_in': _param(3 * D), 'W_o': _param(D, D), 'b_o': _param(D)}
    if ln:
        prm.update(gamma=_param(D), beta=_param(D))
    spans = _give_sinks(prm, mode, 'b_o')
    dq = F32 if kind == 'mixed' else BF
    tail = (prm['W_in'], prm['b_in'], prm['W_o'], prm['b_o'], prm.get('gamma'), prm.get('beta'), None, H, None)
    dr = (0.1, 11, 12) if drop else None
    x32, x, xpos = _act(B, L, D, dtype=F32), _act(B, L, D, dtype=dq), _act(B, L, D, dtype=dq)
    if kind == 'self':
        outs = Lyr.self_attn_ln(x32, x, xpos, *tail, drop=dr)
    else:
        outs = Lyr.cross_attn_ln(x32, x, xpos, _act(B, L, D), _act(B, L, D), *tail, drop=dr)
    mixed = kind == 'mixed'
    fwd = ['cast_transpose', 'cast_transpose', 'cast_split']
    fwd += {'self': ['gemm_nt', 'gemm_nt_split'], 'cross': ['gemm_nt', 'gemm_nt', 'gemm_nt_split'],
            'mixed': ['cast_transpose', 'gemm_nt', 'cast', 'gemm_nt', 'gemm_nt_split']}[kind]
    fwd += ['attn_ws_bytes', 'attn_fwd_dropout'] + (['cast'] if mixed else []) + ['gemm_nt'] + (['dropout_add'] if drop else [])
    fwd += ['layernorm_fwd'] if ln else []
    bwd = _open_bwd(ln, drop, cast_first=not mixed)   # (the queries' fp32 stream gradient needs no cast)
    bwd += (['cast'] if mixed else []) + ['gemm_tn', 'gemm_nt'] + (['cast'] if mixed else []) + ['attn_ws_bytes', 'attn_bwd_dropout']
    if kind == 'self':
        bwd += ['gemm_tn'] * 2 + ['gemm_nt'] * 2
    else:
        bwd += (['cast'] if mixed else []) + ['gemm_tn'] * 3 + ['gemm_nt'] * 3
    direct = mode == 'all'   # all or nothing over the block's parameters
    if not direct:
        spans = {}
    nz = _open_zeros(spans, ln, drop, 'b_o') + int(not direct)
    _check(rec, outs, prm, spans, fwd, bwd, [direct] * (3 if kind == 'self' else 4), nz)


@pytest.mark.parametrize('mode', MODES)
def test_ln_stream(rec, mode):
    prm = {'gamma': _param(D), 'beta': _param(D)}
    spans = _give_sinks(prm, mode, 'beta')
    y = Lyr.ln_stream(_act(B, L, D, dtype=F32), prm['gamma'], prm['beta'], None, BF)
    _check(rec, y, prm, spans, ['layernorm_fwd'], ['layernorm_bwd'], [], int(mode != 'all'))


@pytest.mark.parametrize('mode', MODES)
def test_gate(rec, mode):
    prm = {'gamma': _param(D), 'beta': _param(D)}
    spans = _give_sinks(prm, mode, 'gamma')
    outs = Lyr.gate(_act(B, L, D, dtype=F32), torch.randn(B, L, D).to(BF), _act(B, H, D, dtype=F32), prm['gamma'], prm['beta'], H)
    _check(rec, outs, prm, spans, ['gate_fwd'], ['gate_bwd'], [], 1)   # du | dgamma | dbeta: always one fill
    a = rec.calls[-1][1]
    for n, ptr in (('gamma', a[14]), ('beta', a[15])):   # svol_gate_bwd: ..., du, dgamma, dbeta
        assert (ptr == prm[n].grad.data_ptr()) if n in spans else not any(lo <= ptr < hi for lo, hi in spans.values())


@pytest.mark.parametrize('mode', MODES)
def test_heads(rec, mode):
    prm = {'Wc': _param(2, D), 'bc': _param(2), 'W0': _param(D, D), 'b0': _param(D), 'W1': _param(D, D), 'b1': _param(D),
           'W2': _param(4, D), 'b2': _param(4)}
    spans = _give_sinks(prm, mode, 'W0')
    outs = Lyr.HeadsFn.apply(_act(3, B, 5, D, dtype=F32), *prm.values())
    nz = {'none': 3, 'all': 0, 'one': 1}[mode]   # the 2- / 4-row gradients' buffer, one buffer per D x D pair
    _check(rec, outs, prm, spans, ['heads_fwd'], ['heads_bwd', 'gemm_tn', 'gemm_tn'], [mode == 'all', mode != 'none'], nz,
           ['b0'] if mode == 'one' else [])
    a = rec.calls[-3][1]   # svol_heads_bwd: dWc, dbc, dW2, db2
    for n, ptr in zip(('Wc', 'bc', 'W2', 'b2'), a[13:17]):
        assert (ptr == prm[n].grad.data_ptr()) if n in spans else not any(lo <= ptr < hi for lo, hi in spans.values())
