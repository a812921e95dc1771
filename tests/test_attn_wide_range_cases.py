"""tests/attn_wide_range_cases.py held to fp64 on the CPU: the dispatch twin covers head widths above 32, the planted inputs are exact
and sit where the cases say, every layout runs at two head widths and with both forms of q, the slice bars and the attention-weights
bars of tests/test_gpu_attn_wide_range.py are three times their emulations, the inputs leave the device its share of every project
bar, and each fault runner is caught by the stated kind of figure.  Nothing here loads the device library."""
import functools

import pytest
import torch

from tests import attn_range_cases as A
from tests import attn_wide_range_cases as W
from tests.test_gpu_attn_wide_range import ATT_BARS_PLANTED, ATT_EMULATED, BARS_WIDE, EMULATED_WIDE, slice_bar

BF16, FP16, FP32 = A.BF16, A.FP16, A.FP32
_dt = lambda d: A.DT_NAME[d]
ALL_POINTS = [(n, v, m, dt) for dt in (BF16, FP16, FP32) for n, v, m in W.points(dt)]
_pid = lambda p: f'{p[0]}-{p[1]}-{p[2]}-{_dt(p[3])}'


# ----------------------------------------------------------------------------------------------------------------------
# the dispatch twin and the table
# ----------------------------------------------------------------------------------------------------------------------
def test_twin_sends_head_widths_above_32_to_the_wide_kernels():
    for name, cs in W.CASES.items():
        B, H, Lq, Lk, dh = cs['dims']
        for _, layout in cs['points']:
            p = A.case_plan(name, layout, W.CASES)
            assert (p['fwd'], p['bwd']) == cs['plan'] == ('wide', 'wide') and p['ksplit'] == 1 and p['head_xcd'] == 0, (name, p)
        assert A.ws_floats(*cs['dims']) == 0
    # the boundary of the dispatch: 32 stays with the tuned kernels, whatever the scratch
    assert A.plan(2, 8, 100, 1100, 32, True, True)['fwd'] == 'ksplit_m' and A.ws_floats(2, 8, 100, 1100, 32) > 0
    assert A.plan(2, 8, 100, 1100, 40, True, True, ws_bytes=1 << 30)['fwd'] == 'wide' and A.ws_floats(2, 8, 100, 1100, 40) == 0


def test_the_table_is_what_its_comments_say():
    dims = {n: c['dims'] for n, c in W.CASES.items()}
    assert dims == {'wide64': (2, 4, 200, 450, 64), 'wide64_raw': (2, 4, 200, 450, 64), 'wide48': (2, 2, 70, 300, 48),
                    'wide56': (1, 4, 160, 450, 56), 'wide40': (1, 4, 160, 450, 40), 'wide64_long': (1, 4, 100, 1100, 64)}
    assert [n for n, c in W.CASES.items() if c['premul']] == ['wide64', 'wide56', 'wide40', 'wide64_long']
    assert [n for n, c in W.CASES.items() if not c['fp32']] == ['wide64', 'wide64_long']
    # no slice with fewer than 32 rows (rounding on a couple of rows is not signal); ragged last 64-key tiles
    for B, H, Lq, Lk, dh in dims.values():
        assert all(L % 128 == 0 or L % 128 >= 32 for L in (Lq, Lk)) and 32 < dh <= 64 and dh % 8 == 0
    assert 450 % 64 == 2 and 300 % 64 == 44 and A.cdiv(450, 64) == 8 and A.cdiv(1100, 64) == 18
    # every case runs none and finite; each other layout at two head widths or more and with both forms of q
    seen = {}
    for n, c in W.CASES.items():
        lay = [m for _, m in c['points']]
        assert lay[:2] == ['none', 'finite'] and len(set(lay)) == len(lay), n
        for m in lay:
            seen.setdefault(m, set()).add((c['dims'][4], c['premul']))
    assert set(seen) == set(W.LAYOUTS)
    for m, s in seen.items():
        assert len({dh for dh, _ in s}) >= 2 and {pm for _, pm in s} == {True, False}, (m, s)


def test_sub_dead_and_pair_are_at_the_wide_kernels_granularity():
    kb = A.key_bias('wide64', 'sub_dead', W.CASES)
    dead = (kb == A.NINF).view(2, -1)
    blocks = lambda b: [bool(dead[b, i:i + 32].all()) for i in range(0, 256, 32)]
    assert blocks(0) == [True, False, False, True, False, False, True, True]      # a dead leading block, a dead block in a live tile
    assert blocks(1) == [True, False, True, True, False, False, True, True]       # and one whole dead 64-key tile (192:256)
    assert not bool(dead[:, 256:].any()) and bool(((kb == 0) | dead).all())
    kb = A.key_bias('wide48', 'pair', W.CASES)
    assert [torch.nonzero(kb[b] == 0).view(-1).tolist() for b in range(2)] == [[70, 295]] * 2 and bool((kb[kb != 0] == A.NINF).all())


# ----------------------------------------------------------------------------------------------------------------------
# the planted inputs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=_dt)
def test_planted_values_round_trip_through_the_dtype(dtype):
    for premul, dh in ((True, 64), (False, 64), (False, 48), (True, 56), (True, 40)):
        sp = A.planted_spec(dtype, premul, dh)
        vals = list(sp['a'].values()) + [sp['beta'], sp['beta2']] + sp['step']
        for x in vals:
            assert float(torch.tensor(x, dtype=torch.float64).to(dtype).double()) == x, (premul, dh, x)
        # with pre-multiplied q the steps of the two step kinds straddle the threshold a lazy rescale would have; planted_spec's
        # plain-q steps were sized for head width 16 and are about half as high at scale * log2 e = 0.18 ... 0.23: both kinds rise
        d = (sp['step'][1] - sp['step'][0]) * sp['f']
        if premul:
            assert 3.5 < sp['a']['step_u'] * d < A.LAZY_THR < sp['a']['step_o'] * d < 4.5
        else:
            assert 1.5 < sp['a']['step_u'] * d < sp['a']['step_o'] * d < A.LAZY_THR
        # the two keys of a late head are about one unit apart (bf16's eight bits at plain q: 1.67 units at head width 48)
        assert 0.5 < sp['a']['over'] * (sp['beta'] - sp['beta2']) * sp['f'] < 2.0


@pytest.mark.parametrize('point', ALL_POINTS, ids=_pid)
def test_planted_rows_and_keys_are_where_the_case_says(point):
    c = W.make_case(*point)
    B, H, Lq, Lk, dh = c['dims']
    q0 = c['q'].view(B, Lq, H, dh)[..., 0].transpose(1, 2).double()
    k0 = c['k'].view(B, Lk, H, dh)[..., 0].transpose(1, 2).double()
    assert torch.equal(q0 != 0, c['prow']) and torch.equal(k0 != 0, c['pkey'])
    for (b, h, r), kind in c['kinds'].items():
        assert float(q0[b, h, r]) == c['spec']['a'][kind]
    live = torch.ones(B, Lk, dtype=torch.bool) if c['kb'] is None else c['kb'] > A.NINF
    assert bool(live.any(-1).all()), 'a video without a live key'
    assert not bool((c['pkey'] & ~live[:, None, :]).any()), 'a planted key is masked'
    for t in ('q', 'k', 'v', 'do'):
        assert bool(torch.isfinite(c[t].float()).all())
    # at most four rows per query tile, in different waves; the first and the last workgroup hold one; a whole head holds none
    rows = torch.nn.functional.pad(c['prow'], (0, A.cdiv(Lq, 128) * 128 - Lq)).view(B, H, -1, 4, 32).sum(-1)
    assert int(rows.max()) == 1
    assert bool(c['prow'][0, 0, :128].any()) and bool(c['prow'][B - 1, H - 1, (A.cdiv(Lq, 128) - 1) * 128:].any())
    assert bool((~c['prow'].any(-1)).any())
    kinds = set(c['kinds'].values())
    assert {'near', 'front', 'over'} <= kinds
    if B * H > 2:
        assert {'step_u', 'step_o'} <= kinds
    # the maximum of an 'over' row rises late: its largest score sits behind the first 64-key tile, T_OVER units up
    # (where every 128 keys hold a live one: elsewhere the last live tile may be the first)
    m0, later, _ = A.row_stats(c)
    for (b, h, r), kind in c['kinds'].items():
        if kind == 'over' and c['layout'] in ('none', 'zero', 'finite'):
            assert float(later[b, h, r]) > 0.5 * A.T_OVER[c['dtype']], (b, h, r, float(later[b, h, r]))


# ----------------------------------------------------------------------------------------------------------------------
# bars
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emulated_figures(point):
    c = W.make_case(*point)
    ref = A.reference_of(c)
    o, dq, dk, dv = A.emulation_of(c)
    return A.figures(c, (o, ref[1], dq, dk, dv), ref, slice_bar(point[2], point[3]), lse=False)


@pytest.mark.parametrize('kind', ['other', 'pair'])
@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=_dt)
def test_slice_bars_are_three_times_the_emulation(dtype, kind):
    """the recorded worst point of each row of the table, re-derived (16-bit: fp64 arithmetic with exact roundings; fp32: the summation
    order of the host's fp32 matrix product moves it, so to 30 %), and no other point of the row above it"""
    emu, where = EMULATED_WIDE[dtype][kind]
    assert W.bar_kind(where[2]) == kind
    e = A.worst_slice(emulated_figures(where + (dtype,)))
    assert abs(e - emu) <= (0.3 if dtype == FP32 else 0.01) * emu, (e, emu)
    assert BARS_WIDE[dtype][kind] == 3.0 * emu
    n_pts = 0
    for n, v, m in W.points(dtype):
        if W.bar_kind(m) == kind:
            w = A.worst_slice(emulated_figures((n, v, m, dtype)))
            assert w <= emu * (1.3 if dtype == FP32 else 1.01), (n, v, m, w, emu)
            n_pts += 1
    assert n_pts >= 2


# The share of a bar the emulation may use: one third on the planted sets and on the whole tensors, one half on the benign sets, as at
# head width 32.  Where the wide points do not meet that, the point is held to its own recorded share (two decimals, rounded up; the
# fp32 emulation moves with the host's summation order and gets 15 %); TOL is check_attention's and does not move.
#   fp32, o on planted rows and whole: the fp32 formula rounds a 64-term score at 32 log2 units; recorded 0.52 on planted rows
#       (wide64_raw, sub_dead; 0.46 without a mask) and 0.37 whole.
#   bf16 under 'pair': with two live keys dS = P (dP - delta) cancels to the rounding of delta on every row; recorded 0.58 (dk, benign
#       keys, wide48), 0.52 (dq, benign rows, wide56), 0.39 (whole dq, wide64), 0.36 (dk, planted keys, wide56).
#   bf16 wide64_raw / finite, dq on planted rows: 0.40.
def allowed_share(point, label):
    name, _, layout, dtype = point
    benign = ' other ' in label
    if dtype == FP32 and label.startswith(('elem/o planted', 'whole/o')):
        return 0.6
    if dtype == BF16 and layout == 'pair':
        return 0.58 if benign else 0.39
    if dtype == BF16 and (name, layout) == ('wide64_raw', 'finite') and label.startswith('elem/dq planted'):
        return 0.40
    return 0.5 if benign else 1.0 / 3.0


@pytest.mark.parametrize('point', ALL_POINTS, ids=_pid)
def test_emulation_leaves_the_device_its_share_of_every_project_bar(point):
    """a condition on the INPUTS (tests/test_attn_range_cases.py): the operand dtype's roundings alone use up no more of TOL / 2 TOL
    than allowed_share says, so that the device keeps a factor over the emulation on every element and whole-tensor figure"""
    bad = []
    for label, (val, bar, _) in emulated_figures(point).items():
        if label.startswith(('elem/', 'whole/')):
            share = allowed_share(point, label)
            if not val <= share * bar:
                bad.append(f'{label}: {val:.3e} = {val / bar:.2f} of {bar:.1e} (allowed {share:.2f})')
        elif not val <= bar:
            bad.append(f'{label}: {val:.3e} > {bar:.3e}')
    assert not bad, '; '.join(bad)


# ----------------------------------------------------------------------------------------------------------------------
# attention weights
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def att_emulated_figures(name, layout, dtype):
    c = W.make_case(name, 'peaked', layout, dtype)
    return W.att_figures(c, W.att_emulation(c), ATT_BARS_PLANTED[dtype])


def _att_planted(fig):
    return max(fig['att planted'][0], fig['rowsum planted'][0])


@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=_dt)
def test_attention_weight_bars_on_planted_rows_are_three_times_the_emulation(dtype):
    """the recorded worst point, re-derived (the chain is fp32 torch on the host: to 30 %), no other point above it; on the rows that
    are not planted the emulation stays under half of check_attn_weights' bar; -inf keys are exactly 0"""
    emu, where = ATT_EMULATED[dtype]
    e = _att_planted(att_emulated_figures(*where, dtype))
    assert abs(e - emu) <= 0.3 * emu, (e, emu)
    assert ATT_BARS_PLANTED[dtype] == 3.0 * emu
    pts = W.att_points(dtype)
    assert len(pts) == (20 if dtype != FP32 else 16)
    for n, m in pts:
        fig = att_emulated_figures(n, m, dtype)
        assert _att_planted(fig) <= 1.3 * emu, (n, m, fig)
        for label in ('att other', 'rowsum other'):
            assert fig[label][0] <= 0.5 * W.ATT_BAR[dtype], (n, m, label, fig[label])
        assert fig['not finite'][0] == 0.0 and fig.get('masked_keys/att', (0.0,))[0] == 0.0


def test_attention_weights_reference_is_the_softmax_head_mean():
    """att_reference against torch's softmax over natural-unit scores, and a wrong lse2 is seen: half a unit in one head's row moves
    that row of att past every bar"""
    c = W.make_case('wide48', 'peaked', 'finite', FP32)
    B, H, Lq, Lk, dh = c['dims']
    from tests import attn_dropout_ref as R
    s = R._heads(c['qref'], B, Lq, H, dh) @ R._heads(c['k'].double(), B, Lk, H, dh).transpose(-1, -2) / dh ** 0.5
    want = torch.softmax(s + c['kb'].double()[:, None, None, :], -1).mean(1)
    ref = W.att_reference(c)
    assert float((ref - want).abs().max()) < 1e-14 and float((ref.sum(-1) - 1).abs().max()) < 1e-13
    assert not A.failing(W.att_figures(c, ref, ATT_BARS_PLANTED[FP32]))
    off = ref.clone()
    off[0, 7] *= 1.0 + (2.0 ** 0.5 - 1.0) / H
    assert {'att other', 'rowsum other'} <= set(A.failing(W.att_figures(c, off, ATT_BARS_PLANTED[FP32])))


# ----------------------------------------------------------------------------------------------------------------------
# fault runners: each defect is caught by the stated kind of figure (at the loosest bars, bf16's, unless said otherwise)
# ----------------------------------------------------------------------------------------------------------------------
def _caught(c, got, must=None):
    bar = slice_bar(c['layout'], c['dtype'])
    ref = A.reference_of(c)
    clean = A.failing(A.figures(c, ref, ref, bar))
    assert not clean, clean                      # the reference itself passes every figure
    bad = A.failing(A.figures(c, got, ref, bar))
    whole = [b for b in bad if b.startswith('whole/')]
    print(f'{c["name"]} {c["layout"]}: caught by {len(bad)} figures ({len(whole)} whole-tensor): ' + '; '.join(bad[:6]))
    assert bad
    if must is not None:
        assert any(b.startswith(must) for b in bad), (must, bad)
    return bad


@pytest.mark.parametrize('name,layout', [('wide64', 'sub_dead'), ('wide64', 'first_dead'), ('wide48', 'first_dead'), ('wide40', 'sub_dead')])
def test_fault_a_unguarded_anchor(name, layout):
    c = W.make_case(name, 'peaked', layout, BF16)
    _caught(c, W.fault_unguarded_anchor(c), 'not finite')


@pytest.mark.parametrize('name,layout', [('wide64', 'none'), ('wide48', 'first_dead'), ('wide40', 'sub_dead'), ('wide64_long', 'finite')])
def test_fault_b_second_d_tile_not_rescaled(name, layout):
    c = W.make_case(name, 'peaked', layout, BF16)
    got = W.fault_second_dtile_not_rescaled(c)
    ref = A.reference_of(c)
    dh = c['dims'][4]
    o, o_r = got[0].view(-1, c['dims'][1], dh), ref[0].view(-1, c['dims'][1], dh)
    assert torch.equal(o[..., :32], o_r[..., :32]) and not torch.equal(o[..., 32:], o_r[..., 32:])   # the first d-tile is right
    _caught(c, got, ('slice/', 'elem/'))


@pytest.mark.parametrize('name,layout', [('wide64', 'sub_dead'), ('wide40', 'sub_dead'), ('wide64', 'finite'), ('wide48', 'finite')])
def test_fault_c_sub_block_bias_from_the_wrong_half(name, layout):
    c = W.make_case(name, 'peaked', layout, BF16)
    _caught(c, W.fault_bias_from_the_wrong_half(c), ('masked_keys/', 'slice/'))


def test_fault_d_ragged_tail_live():
    """wide48 / edge gives the slice and element figures: behind a live prefix of 128 keys the 20 keys past Lk = 300 of the last tile
    take a visible share of every row.  Among 450 live keys (wide64 without a mask) two more at score 0 are only just seen."""
    c = W.make_case('wide48', 'peaked', 'edge', BF16)
    bad = _caught(c, W.fault_ragged_tail_live(c), ('slice/', 'elem/'))
    assert any(b.startswith('slice/') for b in bad) and any(b.startswith('elem/') for b in bad)
    c = W.make_case('wide64', 'peaked', 'none', BF16)
    _caught(c, W.fault_ragged_tail_live(c))


@pytest.mark.parametrize('dtype', [BF16, FP16], ids=_dt)
def test_fault_e_finite_bias_with_its_high_half_only(dtype):
    """at the dtype's own bars (tests/test_attn_range_cases.py, fault f)"""
    c = W.make_case('wide64', 'peaked', 'finite', dtype)
    bad = _caught(c, A.fault_bias_high_half_only(c))
    assert any(b.startswith(('slice/', 'elem/')) for b in bad)
