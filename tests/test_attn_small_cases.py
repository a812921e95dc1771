"""tests/attn_small_cases.py held to fp64 on the CPU: the reference is autograd's, the planted inputs are exact and meet the conditions
their layouts promise, the canary keys hold their margin, the bf16 emulation leaves the device its share of every bar, the slice bar
of tests/test_gpu_attn_small.py is three times the emulation, each of the six fault runners is caught by at least one figure, and the
whole-tensor asserts of tests/test_gpu_vit.py / test_gpu_vit_train.py let fault 1 pass behind the last image at L = 197.  Nothing here loads the device
library."""
import functools
import math

import pytest
import torch

from tests import attn_dropout_ref as R
from tests import attn_small_cases as A
from tests.test_gpu_attn_small import BARS, EMULATED

POINTS = A.points()
PLANTED = [p for p in POINTS if p[2] == 'planted']
_pid = lambda p: A.point_id(*p)        # noqa: E731
F = lambda dh: A.LOG2E / math.sqrt(dh)  # noqa: E731


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('point', [(33, 32, 'planted'), (97, 64, 'benign'), (225, 32, 'planted')], ids=_pid)
def test_reference_is_autograd_and_the_emulation_without_rounding_is_the_reference(point):
    """attn_dropout_ref.reference takes its gradients from autograd; attn_dropout_ref.emulate, the same formula written out with the
    kernels' rounding sites, equals it when nothing is rounded"""
    c = A.make_case(*point)
    n, H, L, dh = c['dims']
    o, lse2, dq, dk, dv = A.reference(*point)
    ops = [A.real(c, c[t]) for t in ('q', 'k', 'v', 'do')]
    for tag, r, e in zip(('o', 'dq', 'dk', 'dv'), (o, dq, dk, dv), R.emulate(*ops, None, None, 0.0, (n, H, L, L, dh))):
        assert float((r - e).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max())), tag
    # and independently: softmax in fp64, torch.autograd.grad with dO
    q, k, v = (t.double().view(n, L, H, dh).transpose(1, 2).clone().requires_grad_(True) for t in ops[:3])
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    out = torch.softmax(s, -1) @ v
    g = torch.autograd.grad(out, (q, k, v), ops[3].double().view(n, L, H, dh).transpose(1, 2))
    for tag, r, e in zip(('dq', 'dk', 'dv'), (dq, dk, dv), g):
        assert float((r - R._flat(e, n, L, H, dh)).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max())), tag
    assert float((lse2 - torch.logsumexp(s.detach(), -1) / math.log(2.0)).abs().max()) <= 1e-12 * 256


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def test_cases_cover_every_length_and_both_widths():
    assert {p[0] for p in POINTS} == set(A.LENGTHS) >= {1, 31, 32, 33, 97, 128, 129, 224, 225, 255, 256}
    assert len(POINTS) == len(A.LENGTHS) * 2 * 2
    for L in A.LENGTHS:
        n, H, _, _ = A.dims_of(L, 32)
        assert n >= 2 and H % 2 == 1
    # every layout occurs at every length, 'first' in image 0 only (image 1's leading keys are image 0's canaries)
    for H in (3, 5):
        lays = [A.layout_of(b, h, H) for b in range(2) for h in range(H)]
        assert set(lays) == set(A.LAYOUTS)
        assert 'first' not in [A.layout_of(1, h, H) for h in range(H)]


def test_planted_values_are_exact_in_bf16():
    for dh in A.DHS:
        for x in (A.A, A.BETA, A.beta2(dh), A.KD[dh], A.KC[dh], A.CANARY_MAG):
            assert float(torch.tensor(x, dtype=torch.float64).to(A.BF16).double()) == x, (dh, x)
        # the two 'pair' keys are about one log2 unit apart, 'first' / 'deep' / 'high' keys past the fp32 exponent range of exp2, the
        # canary keys 20 units above those
        assert 0.5 < A.A * (A.BETA - A.beta2(dh)) * F(dh) < 1.5
        assert A.A * A.KD[dh] * F(dh) >= 128 + 8 + 4          # log2 256 keys, and 4 units for the other channels
        assert A.A * (A.KC[dh] - A.KD[dh]) * F(dh) >= 20 + 8 + 4


@pytest.mark.parametrize('point', PLANTED, ids=_pid)
def test_planted_rows_keys_and_canaries_are_where_the_case_says(point):
    c = A.make_case(*point)
    n, H, L, dh = c['dims']
    M = n * L
    for t in ('q', 'k', 'v', 'do'):
        assert c[t].shape == (M + A.CANARY_ROWS, H * dh) and bool(torch.isfinite(c[t].float()).all())
    q0 = A.real(c, c['q']).view(n, L, H, dh)[..., 0].transpose(1, 2).double()
    k0 = A.real(c, c['k']).view(n, L, H, dh)[..., 0].transpose(1, 2).double()
    assert torch.equal(q0 != 0, c['prow']) and torch.equal(k0 != 0, c['pkey'])
    last0 = (A.nblocks(L) - 1) * A.BLOCK
    for (b, h), lay in c['layouts'].items():
        rows = c['rows'][(b, h)]
        assert torch.equal(torch.nonzero(c['prow'][b, h])[:, 0], torch.tensor(rows, dtype=torch.long))
        assert all(float(q0[b, h, r]) == A.sign_of(b) * A.A for r in rows)
        if lay == 'none':
            assert not rows
            continue
        assert rows[0] == 0
        if lay != 'pair' or last0 == 0 or L - last0 >= 8:
            assert rows[-1] == L - 1
        # both half-waves of the key-stationary phase (bit 2 of the in-block row) in the first block and, where it has the rows,
        # in the last
        if L >= 6:
            assert {r & 4 for r in rows if r < A.BLOCK} == {0, 4}
        if L - last0 >= 6 and last0 > 0:
            assert {r & 4 for r in rows if r >= last0} == {0, 4}
    # canary rows: magnitude 64, keys at KC with the sign that outscores the last image's planted rows
    for t in ('q', 'v', 'do'):
        assert bool((c[t][M:].double().abs() == A.CANARY_MAG).all())
    assert bool((c['k'][M:].view(-1, H, dh)[..., 0].double() == A.sign_of(n - 1) * A.KC[dh]).all())


@pytest.mark.parametrize('point', PLANTED, ids=_pid)
def test_layouts_meet_their_conditions(point):
    """fp64, log2 units: 'deep' rows have lse2 <= -128 and 'high' rows lse2 >= +128; a 'first' / 'last' row's top key is where the
    layout says, 'first' by 128 units or more; the two 'pair' keys are the row's two largest, in different half-waves of the forward
    (bit 2 of the in-block key index) and, from L = 33 on, in different 32-key blocks; every canary key an image's planted rows could
    reach outscores each of their real keys by 20 units or more"""
    c = A.make_case(*point)
    n, H, L, dh = c['dims']
    s = A.scores2(c)
    lse2 = A.reference(*point)[1]
    seen = set()
    for (b, h), lay in c['layouts'].items():
        rows = c['rows'][(b, h)]
        if not rows:
            continue
        seen.add(lay)
        own = s[b, h, rows, :L]
        if lay == 'deep':
            assert float(lse2[b, h, rows].max()) <= -128
        elif lay == 'high':
            assert float(lse2[b, h, rows].min()) >= 128
        elif lay == 'first' and L > 1:
            assert bool((own.argmax(-1) == 0).all())
            assert float((own[:, 0] - own[:, 1:].max(-1).values).min()) >= 128
        elif lay == 'last' and L > 1:
            assert bool((own.argmax(-1) == L - 1).all())
            assert float((own[:, L - 1] - own[:, :L - 1].max(-1).values).min()) >= 20
        elif lay == 'pair' and L > 1:
            top, low = A.pair_keys(L, b)
            assert low >= (A.neighbour_canaries(L) if b else 0)
            assert (top & 4) != (low & 4) and (L <= A.BLOCK or top // A.BLOCK != low // A.BLOCK)
            assert bool((own.topk(2, -1).indices == torch.tensor([top, low])).all())
            gap = own[:, top] - own[:, low]
            assert 0.9 < float(gap.min()) and float(gap.max()) < 1.2, gap
        ncan = A.CANARY_ROWS if b == n - 1 else A.neighbour_canaries(L)
        if ncan:
            margin = float((s[b, h, rows, L:L + ncan].min(-1).values - own.max(-1).values).min())
            assert margin >= 20, (b, h, lay, margin)
    assert seen == set(A.LAYOUTS) - {'none'}
    if L % A.BLOCK and L > 4:
        assert A.neighbour_canaries(L) >= 1        # the row fault 1 reads behind image 0 is a canary


# ----------------------------------------------------------------------------------------------------------------------
# bars
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emulated_figures(point):
    c = A.make_case(*point)
    ref = A.reference(*point)
    o, dq, dk, dv = A.emulation(*point)
    return A.figures(c, (o, ref[1], dq, dk, dv), ref, BARS, lse=False)


def test_slice_bar_is_three_times_the_emulation():
    """the recorded worst point, re-derived (fp64 arithmetic with exact bf16 roundings), and no other point above it"""
    emu, where = EMULATED
    e = A.worst_slice(emulated_figures(where))
    assert abs(e - emu) <= 0.01 * emu, (e, emu)
    assert BARS == 3.0 * emu
    for p in POINTS:
        w = A.worst_slice(emulated_figures(p))
        assert w <= emu * 1.01, (p, w, emu)


@pytest.mark.parametrize('point', POINTS, ids=_pid)
def test_emulation_leaves_the_device_its_share_of_every_bar(point):
    """A condition on the INPUTS: bf16's roundings alone stay within one third of every element bar on the planted rows and keys
    (the 'deep' heads' dk / dv included) and within one half on the benign sets, the convention of tests/test_attn_range_cases.py.
    A, the k0 values, DO_SCALE, the rows a 'pair' head plants and the number of neighbour canaries were tuned to it; no bar was.  The
    L = 1 identities hold exactly under the emulation."""
    bad = []
    for label, (val, bar) in emulated_figures(point).items():
        if label.startswith(('elem/', 'deep/')):
            share = 0.5 if ' other ' in label else 1.0 / 3.0
            if not val <= share * bar:
                bad.append(f'{label}: {val:.3e} = {val / bar:.2f} of {bar:.1e}')
        elif not val <= bar:
            bad.append(f'{label}: {val:.3e} > {bar:.3e}')
    assert not bad, '; '.join(bad)


def test_fp32_evaluation_of_lse2_stays_far_inside_its_bar():
    """the kernel's formula m c + log2(sum exp2(s c - m c)) in fp32 arithmetic on the host against fp64, per row set as the lse2
    figure takes it: |lse2| reaches 155, where one fp32 ulp is 1.5e-5 absolute and 1e-7 of the bar's scale"""
    worst = 0.0
    for p in POINTS:
        c = A.make_case(*p)
        ref = A.reference(*p)
        fig = A.figures(c, (ref[0], A.lse2_fp32(c).double(), ref[2], ref[3], ref[4]), ref, BARS)
        worst = max([worst] + [v for label, (v, _) in fig.items() if label.startswith('lse2')])
    print(f'fp32 evaluation of lse2: worst {worst:.2e} of max(1, max |lse2|); bar {A.LSE_BAR:.0e}')
    assert worst <= A.LSE_BAR / 4


# ----------------------------------------------------------------------------------------------------------------------
# fault runners: each defect is caught by at least one figure
# ----------------------------------------------------------------------------------------------------------------------
def _caught(point, fault, must=None):
    c = A.make_case(*point)
    ref = A.reference(*point)
    clean = A.failing(A.figures(c, ref, ref, BARS))
    assert not clean, clean                      # the reference itself passes every figure
    bad = A.failing(A.figures(c, fault(c), ref, BARS))
    print(f'{A.point_id(*point)}: caught by {len(bad)} figures: ' + '; '.join(bad[:6]))
    assert bad
    if must is not None:
        assert any(b.startswith(must) for b in bad), (must, bad)
    return bad


RAGGED = [p for p in POINTS if p[0] % A.BLOCK and p[0] > 1]


@pytest.mark.parametrize('point', RAGGED, ids=_pid)
def test_fault_1_key_mask_off_by_one(point):
    """at every ragged length, in both families (benign: the canary row's v of magnitude 64 behind the last image)"""
    bad = _caught(point, A.fault_key_mask_off_by_one)
    if point[2] == 'planted':
        assert any(b.startswith('elem/o planted') for b in bad) and any(b.startswith('slice/') for b in bad)


@pytest.mark.parametrize('point', [(33, 32, 'planted'), (129, 64, 'planted'), (256, 32, 'planted')], ids=_pid)
def test_fault_2_row_maximum_of_one_half_wave(point):
    """the 'first' rows overflow: their top key is in the other half-wave, 128 units above.  (A maximum that is merely too small
    changes nothing a figure could see: the softmax does not depend on it.)"""
    _caught(point, A.fault_max_of_one_half_wave, 'not finite')


@pytest.mark.parametrize('point', [p for p in RAGGED if p[2] == 'planted'], ids=_pid)
def test_fault_3_padded_key_lanes_summed_into_real_keys(point):
    bad = _caught(point, A.fault_padded_lanes_summed, 'not finite')
    assert any(b.startswith('deep/') for b in bad)


@pytest.mark.parametrize('point', [(129, 32, 'benign'), (225, 64, 'planted'), (256, 32, 'benign')], ids=_pid)
def test_fault_4_second_trip_writes_the_first_trips_lse2(point):
    _caught(point, A.fault_second_trip_lse, 'lse2')


@pytest.mark.parametrize('point', [(31, 64, 'planted'), (33, 32, 'benign'), (225, 64, 'planted')], ids=_pid)
def test_fault_5_two_heads_exchanged_in_dk(point):
    _caught(point, A.fault_dk_heads_exchanged, 'slice/dk')


@pytest.mark.parametrize('point', [(225, 32, 'benign'), (225, 64, 'planted'), (255, 32, 'planted'), (256, 64, 'benign')], ids=_pid)
def test_fault_6_dq_of_the_eighth_block_left_out(point):
    _caught(point, A.fault_dq_last_block_left_out, 'slice/dq')


# ----------------------------------------------------------------------------------------------------------------------
# the gap
# ----------------------------------------------------------------------------------------------------------------------
def _old_asserts(got, ref):
    """the whole-tensor asserts of tests/test_gpu_vit.py::test_attn_small (o) and of
    tests/test_gpu_vit_train.py::test_attn_small_bwd_against_fp64_autograd (dq, dk, dv) -> (passes, figures)"""
    e_o = float((got[0] - ref[0]).abs().max() / ref[0].abs().max())
    ok, figs = e_o < 1e-2, [f'o {e_o:.2e} (< 1e-2)']
    for tag, t, r in zip(('dq', 'dk', 'dv'), got[2:], ref[2:]):
        e_max, e_norm = float((t - r).abs().max() / r.abs().max()), float((t - r).norm() / r.norm())
        ok = ok and e_max <= 2e-2 and e_norm <= 1e-2
        figs.append(f'{tag} max {e_max:.2e} (<= 2e-2) norm {e_norm:.2e} (<= 1e-2)')
    return ok, '; '.join(figs)


def test_whole_tensor_asserts_let_fault_1_pass_behind_the_last_image_at_197_tokens():
    """(2, 12, 197, 64) with randn * 1.2 inputs, the ViT-B/16 shape of the two present tests.  The row behind the LAST image lies
    outside every tensor those tests allocate; with the zeros fresh device memory usually holds it is a key of score 0 and value 0,
    and fault 1 there passes every whole-tensor assert by a factor of eight or more (o 7.8e-4; gradients 1.2e-3).  That is the gap.
    The row behind image 0 is image 1's first row, a real key: over 2 x 12 x 197 rows one of them scores it near the top, and the
    worst-element assert on o does see that (0.58; on average the row moves o by the 1 / L the slice norm would not show).  The
    figures of this file catch the fault behind either image: the canary rows stand where the zeros were."""
    n, H, L, dh = 2, 12, 197, 64
    d = H * dh
    g = torch.Generator().manual_seed(L)
    qkv = (torch.randn(n * L + 1, 3 * d, generator=g) * 1.2).bfloat16()
    do = torch.randn(n * L + 1, d, generator=g).bfloat16()
    qkv[n * L:] = 0
    do[n * L:] = 0
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    ref = R.reference(q[:n * L], k[:n * L], v[:n * L], do[:n * L], None, None, 0.0, (n, H, L, L, dh))
    ok_last, figs_last = _old_asserts(A.key_mask_off_by_one(q, k, v, do, n, H, L, dh, images=(n - 1,)), ref)
    ok_first, figs_first = _old_asserts(A.key_mask_off_by_one(q, k, v, do, n, H, L, dh, images=(0,)), ref)
    print(f'fault 1 behind the last image: {figs_last}')
    print(f'fault 1 behind image 0: {figs_first}')
    assert ok_last and not ok_first
    # the same fault under this file's figures, behind either image: the nearest case, L = 225 at dh = 64, in both families
    for fam in A.FAMILIES:
        c = A.make_case(225, 64, fam)
        ref = A.reference(225, 64, fam)
        for images in ((0,), (1,)):
            got = A.key_mask_off_by_one(c['q'], c['k'], c['v'], c['do'], *c['dims'], images=images)
            assert A.failing(A.figures(c, got, ref, BARS)), (fam, images)
