"""tests/input_guard_cases.py on the CPU: the tables reach every kernel family they claim (under the dispatch twins), every fp64
reference is finite, and every operand fits the arena's rules -- so a device run cannot meet a wrong table row first."""
import pytest
import torch

from tests import attn_range_cases as A
from tests import input_guard_cases as G
from tests.guard_arena import GuardArena


def _check_spec(s):
    """the reference is finite and has a bar for every checked output; the operands plan into a CPU arena"""
    ref = s.ref()
    for name, o in s.outs.items():
        if o.scratch:
            continue
        assert name in ref or o.init is not None, (s.id, name, 'an output without a reference')
        if name in ref:
            assert name in s.bars and s.bars[name][0] >= 0, (s.id, name)
            r = ref[name]
            assert tuple(r.shape) == o.shape and r.dtype == torch.float64, (s.id, name, tuple(r.shape), o.shape)
            assert bool(torch.isfinite(r).all()), (s.id, name)
    ar = GuardArena(device='cpu', guard_bytes=1 << 18)
    seen = set()
    for name, i in s.ins.items():
        t = i.t
        assert i.slot is not None or bool(torch.isfinite(t.double()).all()) or name == 'kbias', (s.id, name)
        if i.slot is None:
            ar.plan(name, t.shape, t.dtype, i.ld if t.dim() == 2 else None, i.col)
        elif i.slot not in seen:
            seen.add(i.slot)
            ar.plan(i.slot, (t.shape[0], i.ld), t.dtype)
    assert ar.guard * 4 >= 1 << 18


def test_gemm_nt_cases_reach_every_family_of_the_cascade():
    reached = set()
    for name, row in G.GEMM_NT.items():
        for dt in row['dtypes']:
            want = row['fam32'] if dt == G.FP32 else row['fam']
            got = G.gemm_nt_family_of(row, dt)
            assert got == want, (name, dt, got, want)
            reached.add(got)
            M = G.gemm_nt_mnk(row)[0]
            assert M % 128 and M % 16, (name, 'ragged M')
    assert {f for f, _ in reached} == {1, 2, 3, 4, 5, 6}
    assert {(2, 'balanced'), (2, 'tiles128'), (4, 'k32'), (4, 'k64'), (6, 'epi1-composed')} <= reached
    for entry in ('nt', 'split', 'dact'):
        assert any(r['entry'] == entry for r in G.GEMM_NT.values())
    # the balanced variant is claimed at the device's CU count, whatever it is
    for cus in (64, 256, 304):
        assert G.gemm_nt_family_of(G.GEMM_NT['n256_balanced'], G.BF16, cus) == (2, 'balanced')


def test_gemm_tn_cases_reach_both_families():
    reached = set()
    for name, row in G.GEMM_TN.items():
        for dt in row['dtypes']:
            fam = G.gemm_tn_family_of(row, dt)
            assert all(f == (2 if dt == G.FP32 else 1) for f in fam), (name, dt, fam)
            reached.update(fam)
    assert reached == {1, 2}
    assert any(r['entry'] == 'grouped' and len(r['probs']) == 2 for r in G.GEMM_TN.values())
    assert any(not r['zero'] for r in G.GEMM_TN.values())


def test_attention_cases_reach_every_plan():
    fwd, bwd, wide = set(), set(), set()
    for row in G.ATTN_ROWS:
        tab, name, masked, B1 = row
        pl = G.attn_plan(tab, name, masked, B1)
        own = G.attn_plan(tab, name, masked)
        assert (pl['fwd'], pl['bwd']) == (own['fwd'], own['bwd']), (row, 'the B = 1 variant leaves its plan')
        dims, premul, c = G.attn_case(tab, name)
        want = c.get('plan_none', c['plan']) if not masked else c['plan']
        assert (own['fwd'], own['bwd']) == tuple(want), (row, own, want)
        if tab == 'wide':
            wide.add(dims[4])
            assert pl['fwd'] == 'wide'
        else:
            fwd.add(pl['fwd'])
            bwd.add(pl['bwd'])
        if B1:
            assert dims[3] % 128 and dims[0] > 1
    assert fwd == set(A.PLANS_FWD), set(A.PLANS_FWD) ^ fwd
    assert bwd == set(A.PLANS_BWD), set(A.PLANS_BWD) ^ bwd
    assert {40, 48, 64} <= wide
    ragged = {(t, n, m) for t, n, m, b in G.ATTN_ROWS if G.attn_case(t, n)[0][3] % 128 and G.attn_case(t, n)[0][0] > 1}
    assert ragged == {(t, n, m) for t, n, m, b in G.ATTN_ROWS if b == 1}
    assert all(n != 'pre_masked_65' for _, n, _, _ in G.ATTN_ROWS)


@pytest.mark.parametrize('name,dt', G.gemm_nt_points(), ids=lambda v: v if isinstance(v, str) else G.DT_NAME[v])
def test_gemm_nt_references_are_finite(name, dt):
    s = G.gemm_nt_spec(name, dt, cus=8)          # (the balanced case at a small CU count: the reference's size is the device test's business)
    _check_spec(s)
    assert s.ins['A'].ld == s.dims['K'] + 64 and s.ins['B'].ld - s.ins['B'].t.shape[1] == 64


@pytest.mark.parametrize('name,dt', G.gemm_tn_points(), ids=lambda v: v if isinstance(v, str) else G.DT_NAME[v])
def test_gemm_tn_references_are_finite(name, dt):
    _check_spec(G.gemm_tn_spec(name, dt))


@pytest.mark.parametrize('row', G.ATTN_ROWS, ids=G.attn_row_id)
def test_attention_references_are_finite(row):
    for dt in G.attn_dtypes(row):
        for kind in ('fwd', 'bwd'):
            s = G.attn_spec(row, dt, kind)
            _check_spec(s)
            assert ('qkv' in {i.slot for i in s.ins.values()}) == (s.dims['Lq'] == s.dims['Lk'])
        G.attn_problem.cache_clear()


def test_other_attention_references_are_finite():
    for dt in G.ALL:
        for name in G.ATTN_WEIGHTS:
            _check_spec(G.attn_weights_spec(name, dt))
    for dt in G.H16:
        for kind in ('fwd', 'bwd'):
            for L, dh in G.ATTN_SMALL:
                _check_spec(G.attn_small_spec(L, dh, dt, kind))
            for L, dh in G.ATTN_CLS:
                if kind in G.attn_cls_kinds(L):
                    _check_spec(G.attn_cls_spec(L, dh, dt, kind))


@pytest.mark.parametrize('dt', G.ALL, ids=lambda v: G.DT_NAME[v])
def test_row_kernel_references_are_finite(dt):
    for M, D in G.ln_points():
        for kind in ('fwd', 'bwd'):
            s = G.ln_spec(M, D, dt, kind)
            _check_spec(s)
            if kind == 'fwd':
                assert s.ins['pos'].t.shape == (s.dims['pos_rows'], D) and s.dims['pos_rows'] < M
        G._ln_problem.cache_clear()
    for sh, entry in G.gate_points():
        _check_spec(G.gate_spec(sh, dt, entry))
    G._gate_problem.cache_clear()
    assert not G.gate_fusable(*G.GATE_SHAPES[2]) and G.gate_fusable(*G.GATE_SHAPES[0]) and G.gate_fusable(*G.GATE_SHAPES[1])
    for s in G.small_op_specs(dt):
        _check_spec(s)


@pytest.mark.parametrize('dt', G.H16, ids=lambda v: G.DT_NAME[v])
def test_resnet_references_are_finite(dt):
    seen = set()
    for s in G.resnet_specs(dt):
        _check_spec(s)
        seen.add(s.entry)
    assert seen == {'svol_conv_nhwc', 'svol_im2col', 'svol_maxpool_nhwc', 'svol_maxpool_idx_nhwc', 'svol_maxpool_bwd_nhwc', 'svol_avgpool_nhwc',
                    'svol_bn_colstats', 'svol_bn_apply', 'svol_bn_bwd_reduce', 'svol_bn_bwd_apply', 'svol_col2im_nhwc', 'svol_conv_wgrad_nhwc',
                    'svol_conv_weight_pack'}


def test_reference_helpers_against_torch():
    x = torch.randn(50, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    assert float((G.gelu_d(x.detach()) - x.grad).abs().max()) < 1e-12
    assert float((G.gelu(x.detach()) - torch.nn.functional.gelu(x.detach())).abs().max()) < 1e-12
    y = torch.randn(7, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    g, b = torch.randn(12, dtype=torch.float64), torch.randn(12, dtype=torch.float64)
    assert float((G.layer_norm(y, g, b) - torch.nn.functional.layer_norm(y, (12,), g, b, 1e-5)).abs().max()) < 1e-12
    # the unfold helper is torch's convolution
    x4 = torch.randn(2, 3, 7, 5, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, dtype=torch.float64)
    got = G._unfold(x4, 3, 2, 1) @ w.permute(0, 2, 3, 1).reshape(4, -1).t()
    assert float((got - G._nhwc(torch.nn.functional.conv2d(x4, w, None, 2, 1))).abs().max()) < 1e-12
