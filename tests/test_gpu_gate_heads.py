"""The sketch -> video gate above eight heads (csrc/gate.hip: 8 < H <= 32 runs the score pass and the backward apply pass once per
group of eight heads, and the forward apply pass with one head per lane), kernel by kernel.

A model's outputs are nearly blind to the gate -- LN1(x (1 + a)) forgets the per-token scale up to its epsilon -- and the head
butterfly of the score pass once mixed heads for rounds without moving a loss.  So the quantities are check_gate's
(tests/gpu_checks.py), looked at directly, at its bars:

    y32 2e-5 | y, ypos TOL[dtype] | saved scores 2e-5 of their maximum | saved a 1e-4 element by element | dx 4e-5 (fp32) / 1e-2 |
    du on dx's scale 3e-5 | dgamma, dbeta 1e-4 (fp32) / 1e-2

and in its small-variance regime, where the gate is visible: y32 5e-5, dx 2e-4, du 1e-3 on its own scale.  On top: a head-mixing
test (u zero but for one head: every other head's saved scores are exactly 0.0), check_gate_against_mha's two comparisons, the return
codes at H = 33, write guards and hostile fills around the six entries at H = 16 (tests/guard_arena.py through the runner of
tests/test_gpu_input_guards.py) and run-to-run bit equality under SVOL_DETERMINISTIC=1.
"""
import ctypes
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
_DT = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
UNSUPPORTED = -2

SHAPES = [(2, 37, 36, 9),        # one head past a group
          (3, 50, 96, 12),
          (2, 130, 128, 16),
          (1, 77, 512, 16),      # two 16-byte column groups per lane
          (2, 24, 528, 24),      # past 512 columns, three groups of heads
          (1, 21, 1024, 32),     # four column groups, four groups of heads
          (3, 5, 64, 16)]        # short videos, M = 15: one row per wave, so NO wave crosses a batch element here (the cc hand-over of
                                 # gate_bwd_ln_kernel is reached by tests/test_gpu_row_kernels.py at 64 waves)
_ids = lambda shapes: ['B%dL%dD%dH%d' % s for s in shapes]   # noqa: E731


def _hold(res):
    for k, (e, t) in res.items():
        print(f'{k}: err={e:.3e} tol={t:.1e}{"" if e <= t else "   <-- FAILS"}')
    bad = {k: v for k, v in res.items() if not (v[0] <= v[1])}
    assert not bad, '\n'.join(f'{k}: err={e:.3e} tol={t:.1e}' for k, (e, t) in bad.items())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids(SHAPES))
def test_gate_against_fp64(shape, dtype):
    """check_gate's first regime (its draws, its quantities, its bars) at more than eight heads"""
    from svol_amd import layers
    from tests.gpu_checks import TOL, _gate_ref, _rnd, rel_err
    dt = _DT[dtype]
    B, L, D, H = shape
    x, pos = _rnd((B, L, D), torch.float32, 40), _rnd((B, L, D), dt, 41)
    u = _rnd((B, H, D), torch.float32, 42, 0.2)
    g = 1 + 0.1 * _rnd((D,), torch.float32, 43)
    b = 0.1 * _rnd((D,), torch.float32, 44)
    dy32, dy, dyp = _rnd((B, L, D), torch.float32, 47), _rnd((B, L, D), dt, 45), _rnd((B, L, D), dt, 46)
    xd = x.to(DEV).requires_grad_(True)
    ud = u.to(DEV).requires_grad_(True)
    gd, bd = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y32, y, ypos = layers.gate(xd, pos.to(DEV), ud, gd, bd, H)
    x64, u64 = x.double().requires_grad_(True), u.double().requires_grad_(True)
    g64, b64 = g.double().requires_grad_(True), b.double().requires_grad_(True)
    yr, ypr = _gate_ref(x64, pos.double(), u64, g64, b64, H)
    res = {}
    res['y32'] = (rel_err(y32, yr), 2e-5)
    res['y'] = (rel_err(y, yr), TOL[dt])
    res['ypos'] = (rel_err(ypos, ypr), TOL[dt])
    sv = y32.grad_fn.saved_tensors   # GateFn: (x2, pos2, u, gamma, a, mean, rstd, ws)
    s64 = torch.einsum('bld,bhd->bhl', x64.detach() + pos.double(), u64.detach())
    res['scores'] = (float((sv[7][:B * H * L].view(B, H, L).double().cpu() - s64).abs().max() / s64.abs().max()), 2e-5)
    a64 = torch.softmax(s64, -1).mean(1).reshape(-1)
    res['a'] = (float(((sv[4].double().cpu() - a64).abs() / a64).max()), 1e-4)
    (yr * (dy.double() + dy32.double()) + ypr * dyp.double()).sum().backward()
    torch.autograd.backward([y32, y, ypos], [dy32.to(DEV), dy.to(DEV), dyp.to(DEV)])
    res['dx'] = (rel_err(xd.grad, x64.grad), 4e-5 if dt == torch.float32 else 1e-2)
    scale = float(x64.grad.abs().max())
    res['du_abs_vs_dx_scale'] = (float((ud.grad.cpu().double() - u64.grad).abs().max()) / scale, 3e-5)
    res['dgamma'] = (rel_err(gd.grad, g64.grad), 1e-4 if dt == torch.float32 else 1e-2)
    res['dbeta'] = (rel_err(bd.grad, b64.grad), 1e-4 if dt == torch.float32 else 1e-2)
    _hold(res)


SMALL_VARIANCE = [(2, 52, 64, 16), (2, 200, 256, 32)]


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape', SMALL_VARIANCE, ids=_ids(SMALL_VARIANCE))
def test_gate_where_it_is_visible(shape, dtype):
    """check_gate's second regime: rows whose variance is below LayerNorm's epsilon and a peaked softmax -- the outputs depend on the
    gate weights to first order and du is of the size of everything else"""
    from oracle import svol_oracle as O
    from svol_amd import layers
    from tests.gpu_checks import _gate_ref, _rnd, rel_err
    dt = _DT[dtype]
    B, L, D, H = shape
    x, pos = 1e-3 * _rnd((B, L, D), torch.float32, 50), _rnd((B, L, D), dt, 51)
    u = _rnd((B, H, D), torch.float32, 52, 8.0 / math.sqrt(D))
    g = 1 + 0.1 * _rnd((D,), torch.float32, 53)
    b = 0.1 * _rnd((D,), torch.float32, 54)
    dy32 = _rnd((B, L, D), torch.float32, 55)
    xd, ud = x.to(DEV).requires_grad_(True), u.to(DEV).requires_grad_(True)
    y32, y, ypos = layers.gate(xd, pos.to(DEV), ud, g.to(DEV), b.to(DEV), H)
    x64, u64 = x.double().requires_grad_(True), u.double().requires_grad_(True)
    yr, _ = _gate_ref(x64, pos.double(), u64, g.double(), b.double(), H)
    y_off = O.layer_norm(x.double(), g.double(), b.double())
    res = {}
    res['gate_is_visible'] = (1e-2 / max(float((yr.detach() - y_off).abs().max() / yr.detach().abs().max()), 1e-30), 1.0)
    res['y32'] = (rel_err(y32, yr), 5e-5)
    (yr * dy32.double()).sum().backward()
    y32.backward(dy32.to(DEV))
    res['dx'] = (rel_err(xd.grad, x64.grad), 2e-4)
    res['du'] = (rel_err(ud.grad, u64.grad), 1e-3)
    res['du_is_not_noise'] = (1e-5 / max(float(u64.grad.abs().max() / x64.grad.abs().max()), 1e-30), 1.0)
    _hold(res)


@pytest.mark.parametrize('H,D,h0', [(H, D, h0) for H, D in ((16, 64), (9, 36)) for h0 in (0, 7, 8, H - 1)])
def test_scores_do_not_mix_heads(H, D, h0):
    """u is zero except for head h0: every other head's saved scores are exactly 0.0 (a butterfly or a group offset that put one
    head's sum into another's slot would show there), head h0's are non-zero and its fp64 dot products"""
    from svol_amd import layers
    from tests.gpu_checks import _rnd
    B, L = 2, 37
    x, pos = _rnd((B, L, D), torch.float32, 40), _rnd((B, L, D), torch.float32, 41)
    u = torch.zeros((B, H, D))
    u[:, h0] = _rnd((B, D), torch.float32, 42, 0.2)
    g, b = torch.ones(D), torch.zeros(D)
    y32, _, _ = layers.gate(x.to(DEV).requires_grad_(True), pos.to(DEV), u.to(DEV), g.to(DEV), b.to(DEV), H)
    sc = y32.grad_fn.saved_tensors[7][:B * H * L].view(B, H, L).cpu()   # GateFn's ws: the scores come first
    others = [h for h in range(H) if h != h0]
    assert int((sc[:, others] != 0.0).sum()) == 0, {h: float(sc[:, h].abs().max()) for h in others if float(sc[:, h].abs().max()) > 0}
    s64 = torch.einsum('bld,bd->bl', x.double() + pos.double(), u[:, h0].double())
    assert bool((sc[:, h0] != 0.0).all())
    err = float((sc[:, h0].double() - s64).abs().max() / s64.abs().max())
    print(f'H{H} h0={h0}: scores of the one head err={err:.3e} tol=2.0e-05')
    assert err <= 2e-5


MHA = [(2, 52, 64, 16), (3, 200, 256, 32), (1, 77, 96, 12), (2, 40, 72, 9)]


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape', MHA, ids=_ids(MHA))
def test_gate_against_the_attention_it_replaces(shape, dtype):
    """check_gate_against_mha's two comparisons: the gate vectors against their formula, the saved gate weights against the
    head-averaged weights of the oracle's one-query mha"""
    from oracle import svol_oracle as O
    from svol_amd import layers
    from svol_amd.modeling.cross_modal_transformer import CrossModalTransformerLayer
    from tests.gpu_checks import _rnd
    dt = _DT[dtype]
    B, L, D, H = shape
    torch.manual_seed(7)
    layer = CrossModalTransformerLayer(D, H, 2 * D)
    m = layer.sketch_video_cross_attn
    with torch.no_grad():   # (the default initialisation leaves the in_proj bias at zero)
        m.in_proj_bias.copy_(0.3 * _rnd((3 * D,), torch.float32, 70))
        m.in_proj_weight.mul_(3.0)
    layer = layer.to(DEV)
    sk = _rnd((B, D), torch.float32, 71)
    x, pos = _rnd((B, L, D), torch.float32, 72), _rnd((B, L, D), dt, 73)
    u = layer.gate_vectors(sk.to(DEV))
    y32, _, _ = layers.gate(x.to(DEV), pos.to(DEV), u, layer.norm1.weight, layer.norm1.bias, H)
    a_dev = y32.grad_fn.saved_tensors[4].double().cpu().view(B, L)
    W, bb = m.in_proj_weight.detach().double().cpu(), m.in_proj_bias.detach().double().cpu()
    dh = D // H
    q = sk.double() @ W[:D].T + bb[:D]
    u_ref = torch.einsum('bhj,hjd->bhd', q.view(B, H, dh), W[D:2 * D].view(H, dh, D)) / math.sqrt(dh)
    res = {}
    res['u'] = (float((u.double().cpu() - u_ref).abs().max() / u_ref.abs().max()), 1e-5)
    kv = x.double() + pos.double()
    _, att1 = O.mha(sk.double()[:, None, :], kv, kv, W, bb, m.out_proj.weight.detach().double().cpu(),
                    m.out_proj.bias.detach().double().cpu(), H, need_output=False)
    att1 = att1[:, 0, :]
    res['a_vs_att1'] = (float(((a_dev - att1).abs() / att1).max()), 2e-4)
    res['att1_is_not_uniform'] = (float(1.0 / (att1.max() * L)), 0.5)   # (a flat softmax would hide a wrong score)
    _hold(res)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def test_33_heads_are_refused_and_nothing_is_written():
    """H = 33 (D = 132: a multiple of 4 and of 33, so the head count is the only reason): SVOL_E_UNSUPPORTED from the six entries and
    every output still holds its sentinel"""
    from svol_amd import _lib, ops
    lib = _lib.lib()
    P, st = ops._ptr, ops._stream()
    B, L, D, H = 2, 8, 132, 33
    M = B * L
    SENT = -77.0
    f = lambda *sh: torch.randn(sh, device=DEV)               # noqa: E731
    o = lambda *sh: torch.full(sh, SENT, device=DEV)          # noqa: E731
    x, pos, u, gamma, beta = f(M, D), f(M, D), f(B, H, D), f(D), f(D)
    a, mean, rstd, ws = f(M), f(M), f(M).abs() + 1, f(B * H * (L + 2))
    skch, W, bias, q, du_in = f(B, D), f(3 * D, D), f(3 * D), f(B, D), f(B, H, D)
    dt = ops._DT[torch.float32]
    outs = dict(y32=o(M, D), y=o(M, D), ypos=o(M, D), a=o(M), mean=o(M), rstd=o(M), ws=o(B * H * (L + 2)), ws2=o(M + B * H), dx=o(M, D),
                du=o(B, H, D), dg=o(D), db=o(D), q=o(B, D), u=o(B, H, D), dq=o(B, D), dskch=o(B, D), dW=o(3 * D, D), dbin=o(3 * D))
    t = outs
    rcs = {}
    rcs['svol_gate_fwd'] = lib.svol_gate_fwd(P(x), P(pos), P(u), P(gamma), P(beta), P(t['y32']), P(t['y']), P(t['ypos']), P(t['a']),
                                             P(t['mean']), P(t['rstd']), P(t['ws']), B, L, D, H, dt, st)
    rcs['svol_gate_bwd'] = lib.svol_gate_bwd(P(x), None, None, P(x), P(pos), P(u), P(gamma), P(a), P(mean), P(rstd), P(ws), P(t['ws2']),
                                             P(t['dx']), P(t['du']), P(t['dg']), P(t['db']), B, L, D, H, dt, st)
    rcs['svol_gate_vectors_fwd'] = lib.svol_gate_vectors_fwd(P(skch), P(W), P(bias), P(t['q']), P(t['u']), B, D, H, st)
    rcs['svol_gate_vectors_bwd'] = lib.svol_gate_vectors_bwd(P(du_in), P(skch), P(W), P(q), P(t['dq']), P(t['dskch']), P(t['dW']), P(t['dbin']),
                                                             B, D, H, st)
    rcs['svol_gate_vectors_fwd_multi'] = lib.svol_gate_vectors_fwd_multi(P(skch), _ptr_array([W]), _ptr_array([bias]), _ptr_array([t['q']]),
                                                                         _ptr_array([t['u']]), 1, B, D, H, st)
    rcs['svol_gate_vectors_bwd_multi'] = lib.svol_gate_vectors_bwd_multi(_ptr_array([du_in]), P(skch), _ptr_array([W]), _ptr_array([q]),
                                                                         _ptr_array([t['dq']]), _ptr_array([t['dskch']]), _ptr_array([t['dW']]),
                                                                         _ptr_array([t['dbin']]), 1, B, D, H, st)
    torch.cuda.synchronize()
    assert all(rc == UNSUPPORTED for rc in rcs.values()), rcs
    touched = [k for k, v in outs.items() if not bool((v == SENT).all())]
    assert not touched, touched
    # ... and 32 heads at the same width per head are taken (so it was the head count)
    rc = lib.svol_gate_vectors_fwd(P(f(B, 128)), P(f(3 * 128, 128)), P(f(3 * 128)), P(o(B, 128)), P(o(B, 32, 128)), B, 128, 32, st)
    torch.cuda.synchronize()
    assert rc == 0, rc


# ---- write guards and hostile fills: every operand and every output a slot of a guard arena, three fills behind the inputs ----------
def _multi_fwd(L, s, i, o, dt, st):
    return L.svol_gate_vectors_fwd_multi(i['skch'].data_ptr(), _ptr_array([i['W_in']]), _ptr_array([i['b_in']]), _ptr_array([o['q']]),
                                         _ptr_array([o['u']]), 1, s.dims['B'], s.dims['D'], s.dims['H'], st)


def _multi_bwd(L, s, i, o, dt, st):
    return L.svol_gate_vectors_bwd_multi(_ptr_array([i['du']]), i['skch'].data_ptr(), _ptr_array([i['W_in']]), _ptr_array([i['q']]),
                                         _ptr_array([o['dq_ws']]), _ptr_array([o['dskch']]), _ptr_array([o['dW_in']]),
                                         _ptr_array([o['db_in']]), 1, s.dims['B'], s.dims['D'], s.dims['H'], st)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('entry', ['svol_gate_fwd', 'svol_gate_bwd'])
def test_gate_at_16_heads_stays_inside_its_buffers_and_reads_only_its_operands(entry, dtype):
    from tests import input_guard_cases as G
    from tests.test_gpu_input_guards import run_spec
    for sh in ((2, 52, 64, 16), (2, 301, 256, 16)):
        run_spec(G.gate_spec(sh, _DT[dtype], entry))
    G._gate_problem.cache_clear()


@pytest.mark.parametrize('kind', ['fwd', 'bwd'])
@pytest.mark.parametrize('multi', [False, True], ids=['single', 'multi'])
def test_gate_vectors_at_16_heads_stay_inside_their_buffers_and_read_only_their_operands(kind, multi, monkeypatch):
    from tests import input_guard_cases as G
    from tests import test_gpu_input_guards as IG
    for sh in ((2, 64, 16), (3, 256, 16)):
        s = G.gate_vectors_spec(sh, kind)
        if multi:
            s.entry += '_multi'
            monkeypatch.setitem(IG.CALLS, s.entry, _multi_fwd if kind == 'fwd' else _multi_bwd)
        IG.run_spec(s)


# ---- deterministic mode --------------------------------------------------------------------------------------------------------
def _child_main():
    import hashlib
    from svol_amd import layers
    from tests.gpu_checks import _rnd
    B, L, D, H = 2, 130, 128, 16
    dt = torch.bfloat16
    x, pos = _rnd((B, L, D), torch.float32, 40), _rnd((B, L, D), dt, 41)
    u = _rnd((B, H, D), torch.float32, 42, 0.2)
    g, b = 1 + 0.1 * _rnd((D,), torch.float32, 43), 0.1 * _rnd((D,), torch.float32, 44)
    dy32, dy, dyp = _rnd((B, L, D), torch.float32, 47), _rnd((B, L, D), dt, 45), _rnd((B, L, D), dt, 46)
    runs = []
    for _ in range(2):
        leaves = [t.to(DEV).requires_grad_(True) for t in (x, u, g, b)]
        y32, y, ypos = layers.gate(leaves[0], pos.to(DEV), leaves[1], leaves[2], leaves[3], H)
        torch.autograd.backward([y32, y, ypos], [dy32.to(DEV), dy.to(DEV), dyp.to(DEV)])
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0 for t in leaves)
        runs.append({n: hashlib.sha256(t.grad.cpu().numpy().tobytes()).hexdigest() for n, t in zip(('dx', 'du', 'dgamma', 'dbeta'), leaves)})
    print('CHILD ' + json.dumps(runs))


def test_two_deterministic_runs_at_16_heads_are_bit_identical():
    """SVOL_DETERMINISTIC=1 (read once by the library: a child process): gate forward + backward at (2, 130, 128, 16) twice; dx, du,
    dgamma and dbeta carry the same bits (the det_cc / det_du scratch is sized by H and filled group by group)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SVOL_DETERMINISTIC='1', PYTHONPATH=root)
    r = subprocess.run([sys.executable, '-c', 'from tests.test_gpu_gate_heads import _child_main; _child_main()'], env=env,
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('CHILD ')]
    assert line, r.stdout[-3000:]
    a, b = json.loads(line[-1][6:])
    assert a == b, (a, b)
