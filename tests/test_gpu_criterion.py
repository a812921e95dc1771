"""The three kernels of csrc/criterion.hip — match_cost_kernel, lsap_kernel (all three solver paths), set_loss_kernel with its
hand-derived GIoU gradient — against fp64 runs of oracle/svol_oracle.py and scipy, through the C ABI with hand-built problem tables
and match arrays (tests/criterion_cases.py), at the geometries where they can go wrong: ties, clamp boundaries, zero-extent boxes,
empty problems, flagged problems, non-finite costs.  Then the same conventions through SetCriterion / the matcher modules."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import criterion_cases as CC

pytestmark = pytest.mark.gpu

SENT = 64                    # sentinel floats on either side of a cost buffer
SENT_BITS = 0x4B1D5EA7       # their bit pattern (a finite float no cost takes)
# svol_match_cost bar: a block's error against fp64 may be COST_MARGIN x the fp32 oracle's own error on that block, floored at
# COST_FLOOR (both relative to max(1, max |C64|)): the kernel mirrors torch's separate fp32 ops, expf and the divisions may differ by
# an ulp or two.  Measured on the MI355X (printed by the test), kernel error / fp32-oracle error per block, 12 blocks per launch:
#   weights (5, 1, 2):   ratio 0.93 .. 1.00, largest error 2.0e-7 of the block's scale (4 x 40)
#   weights (1, 2, 0.5): ratio 1.00 in every block (the kernel's costs ARE torch's fp32 costs), largest error 2.2e-7 (4 x 40)
# so the floor is what binds, with a factor 4.5 to spare.
COST_MARGIN = 4.0
COST_FLOOR = 1e-6


def _lib():
    from svol_amd import _lib
    return _lib


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------
# 1. svol_match_cost
def _run_match_cost(ps, w, with_status):
    L = _lib()
    buf = torch.full((SENT + ps.numel + SENT,), SENT_BITS, dtype=torch.int32, device='cuda')
    st = torch.full((ps.n,), 7, dtype=torch.int32, device='cuda') if with_status else None
    t = [_d(a) for a in (ps.logits, ps.boxes, ps.tgt, ps.pred_off, ps.pred_cnt, ps.tgt_off, ps.tgt_cnt, ps.cost_off)]
    rc = L.lib().svol_match_cost(*[x.data_ptr() for x in t], buf.data_ptr() + 4 * SENT, ps.n, *w, st.data_ptr() if with_status else None,
                                 _stream())
    L.check(rc, 'svol_match_cost')
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:SENT] == SENT_BITS).all() and (raw[-SENT:] == SENT_BITS).all(), 'a cost was written outside the cost buffer'
    body = raw[SENT:SENT + ps.numel]
    return body, (st.cpu().numpy() if with_status else None)


def _blocks(ps):
    for p in range(ps.n):
        po, pc, to, tc, co = (int(x[p]) for x in (ps.pred_off, ps.pred_cnt, ps.tgt_off, ps.tgt_cnt, ps.cost_off))
        yield p, slice(po, po + pc), slice(to, to + tc), slice(co, co + pc * tc), (pc, tc)


def _cost_block_errors(ps, body, w, skip=()):
    out = {}
    for p, pr, tr, cr, shape in _blocks(ps):
        if shape[0] * shape[1] == 0 or p in skip:
            continue
        got = body[cr].view(np.float32).reshape(shape).astype(np.float64)
        c64 = CC.cost_block_reference(ps.logits[pr], ps.boxes[pr], ps.tgt[tr], *w)
        c32 = CC.cost_block_reference(ps.logits[pr], ps.boxes[pr], ps.tgt[tr], *w, dtype=torch.float32).astype(np.float64)
        scale = max(1.0, float(np.abs(c64).max()))
        err = float(np.abs(got - c64).max()) / scale if np.isfinite(got).all() else float('inf')
        out[p] = (shape, err, float(np.abs(c32 - c64).max()) / scale)
    return out


@pytest.mark.parametrize('w', CC.COST_WEIGHTS, ids=['w5_1_2', 'w1_2_0.5'])
def test_match_cost_blocks_against_fp64(w):
    ps = CC.match_cost_problem_set(bad=False)
    body, st = _run_match_cost(ps, w, True)
    assert (body != SENT_BITS).all(), 'a cost inside a block was never written'   # numel = the sum of the blocks: empty ones own no float
    assert (st == 0).all(), st
    body_null, _ = _run_match_cost(ps, w, False)
    assert np.array_equal(body, body_null), 'box_status = NULL changed the costs'
    bad = []
    for p, (shape, err, err32) in _cost_block_errors(ps, body, w).items():
        bar = max(COST_FLOOR, COST_MARGIN * err32)
        print(f'match_cost w={w} problem {p:2d} {shape[0]:2d}x{shape[1]:2d}: err {err:.2e}  fp32 oracle {err32:.2e}  '
              f'ratio {err / max(err32, 1e-30):.2f}  bar {bar:.2e}')
        if not err <= bar:
            bad.append((p, shape, err, bar))
    assert not bad, bad


def test_match_cost_flags_exactly_the_problems_with_a_degenerate_box():
    w = CC.COST_WEIGHTS[0]
    ps = CC.match_cost_problem_set(bad=True)
    want = CC.expected_box_status(ps)
    assert np.nonzero(want)[0].tolist() == [3, 5, 6]
    body, st = _run_match_cost(ps, w, True)
    assert st.tolist() == want.tolist(), st
    body_null, _ = _run_match_cost(ps, w, False)
    assert np.array_equal(body, body_null), 'box_status = NULL changed the costs'   # bit patterns: NaN costs compare too
    # the healthy problems beside the flagged ones still hold the fp64 costs
    for p, (shape, err, err32) in _cost_block_errors(ps, body, w, skip=(3, 5, 6)).items():
        assert err <= max(COST_FLOOR, COST_MARGIN * err32), (p, shape, err, err32)


# ---------------------------------------------------------------------------
# 2. svol_lsap_batched
MATCH_SENT = -7


def _run_lsap(probs, gap=5):
    """one launch over `probs` = [(label, cost, expected status)]; `gap` prediction rows that belong to no problem sit in front of
    every problem's rows and 64 behind the last."""
    L = _lib()
    pred_cnt = np.array([c.shape[0] for _, c, _ in probs], np.int32)
    tgt_cnt = np.array([c.shape[1] for _, c, _ in probs], np.int32)
    pred_off = (np.concatenate([[0], np.cumsum(pred_cnt)[:-1]]) + gap * (1 + np.arange(len(probs)))).astype(np.int32)
    tgt_off = np.concatenate([[0], np.cumsum(tgt_cnt)[:-1]]).astype(np.int32)
    cost_off = np.concatenate([[0], np.cumsum(pred_cnt.astype(np.int64) * tgt_cnt)[:-1]]).astype(np.int64)
    flat = _d(np.concatenate([c.reshape(-1) for _, c, _ in probs]).astype(np.float32))
    n_rows = int(pred_off[-1] + pred_cnt[-1]) + 64
    match = torch.full((n_rows,), MATCH_SENT, dtype=torch.int32, device='cuda')
    status = torch.full((len(probs),), 9, dtype=torch.int32, device='cuda')
    t = [_d(a) for a in (cost_off, pred_off, pred_cnt, tgt_off, tgt_cnt)]
    rc = L.lib().svol_lsap_batched(flat.data_ptr(), *[x.data_ptr() for x in t], match.data_ptr(), status.data_ptr(), len(probs),
                                   CC.LSAP_MAX_DIM, _stream())
    L.check(rc, 'svol_lsap_batched')
    torch.cuda.synchronize()
    return match.cpu().numpy(), status.cpu().numpy(), pred_off, pred_cnt, tgt_off, tgt_cnt


@pytest.mark.parametrize('launch', [n for n, _ in CC.lsap_launches()])
def test_lsap_status_and_nonfinite_costs_on_every_path(launch):
    probs = dict(CC.lsap_launches())[launch]
    assert {CC.lsap_path(*c.shape) for _, c, _ in probs} == {'reg', 'lds', 'global'}
    m, st, pred_off, pred_cnt, tgt_off, tgt_cnt = _run_lsap(probs)
    owned = np.zeros(len(m), bool)
    bad = []
    for i, (label, c, want) in enumerate(probs):
        rows = slice(pred_off[i], pred_off[i] + pred_cnt[i])
        owned[rows] = True
        mm = m[rows]
        sst, r, cc = CC.scipy_status(c)
        assert sst == want
        if st[i] != want:
            bad.append((label, 'status', int(st[i]), want))
            continue
        if want == 0:
            gr = np.nonzero(mm >= 0)[0]
            if gr.tolist() != r.tolist() or (mm[gr] - tgt_off[i]).tolist() != cc.tolist() or (mm[mm < 0] != -1).any():
                bad.append((label, 'assignment differs from scipy'))
        else:   # unspecified, but inside {-1} U the problem's own target range
            ok = (mm == -1) | ((mm >= tgt_off[i]) & (mm < tgt_off[i] + tgt_cnt[i]))
            if not ok.all():
                bad.append((label, 'match row outside the problem', mm[~ok][:4].tolist()))
    assert not bad, bad
    assert (m[~owned] == MATCH_SENT).all(), 'a match row that belongs to no problem was written'


# ---------------------------------------------------------------------------
# 3. svol_set_loss
def _run_set_loss(logits, boxes, tgt, match, eos, vid_off=None, rows_per_video=0, status=None, box_status=None, ppl=0):
    L = _lib()
    NL, R = logits.shape[:2]
    lg, bx, tg, mt = _d(logits.astype(np.float32)), _d(boxes.astype(np.float32)), _d(tgt.astype(np.float32)), _d(match.astype(np.int32))
    nanf = float('nan')   # outputs start as NaN: whatever the kernel does not write shows
    losses = torch.full((NL, 4), nanf, device='cuda')
    gl, gb, gg = torch.full((NL, R, 2), nanf, device='cuda'), torch.full((NL, R, 4), nanf, device='cuda'), torch.full((NL, R, 4), nanf, device='cuda')
    vo = _d(vid_off.astype(np.int32)) if vid_off is not None else None
    s1 = _d(status.astype(np.int32)) if status is not None else None
    s2 = _d(box_status.astype(np.int32)) if box_status is not None else None
    P = lambda x: x.data_ptr() if x is not None else None
    rc = L.lib().svol_set_loss(P(lg), P(bx), P(tg), P(mt), P(losses), P(gl), P(gb), P(gg), NL, R, float(eos), P(vo), rows_per_video,
                               P(s1), P(s2), ppl, _stream())
    L.check(rc, 'svol_set_loss')
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (losses, gl, gb, gg)]


def _compare_layer(tag, got, lg, bx, tg, m, cls, eos, videos=None):
    """got = (losses[4], g_label, g_bbox, g_giou) of one layer against the fp64 oracle, per class.  Returns the failures."""
    K = int((m >= 0).sum())
    ref = CC.set_loss_reference(lg, bx, tg, m, eos, torch.float64, videos)
    f32 = CC.set_loss_reference(lg, bx, tg, m, eos, torch.float32, videos)
    bad = []
    for k, name in enumerate(('loss_label', 'loss_bbox', 'loss_giou', 'class_error')):
        e = abs(float(got[0][k]) - ref[0][k]) / max(1.0, abs(ref[0][k]))
        if not e <= CC.LOSS_BAR:
            bad.append((tag, name, float(got[0][k]), ref[0][k]))
    for which, g, g64, g32 in zip(('g_label', 'g_bbox', 'g_giou'), got[1:], ref[1:], f32[1:]):
        e32 = CC.per_class_errors(g32, g64, cls)
        for cname, (err, ref_max) in CC.per_class_errors(g, g64, cls).items():
            bar = CC.grad_bar(cname, ref_max, K, e32[cname][0])
            if cname == 'random':
                print(f'set_loss {tag} {which} random: err {err:.2e}  fp32 oracle {e32[cname][0]:.2e}  '
                      f'ratio {err / max(e32[cname][0], 1e-30):.2f}  rel {err / ref_max:.2e}  bar {bar:.2e}')
            elif ref_max >= 1e-12:
                print(f'set_loss {tag} {which} {cname}: rel err {err / ref_max:.2e}  (bar {CC.DYADIC_BAR:.0e})')
            elif cname != 'background':
                print(f'set_loss {tag} {which} {cname}: zero reference, abs err {err:.2e}  (bar {bar:.2e})')
            if not err <= bar:
                bad.append((tag, which, cname, err, bar))
    return bad


# Measured on the MI355X (printed by the tests).  Dyadic classes, largest error relative to the class's own max |reference| over every
# class, layer and layout (bar 1e-5): g_label 1.6e-6 (zero_w_edge, R = 300 layer 1), g_bbox 1.5e-8, g_giou 5.2e-7 (tgt_inside);
# identical boxes: g_bbox and g_giou exactly 0 (bar 1e-6 / K).  Random class, kernel error / fp32-oracle error: g_label 0.96 .. 2.56,
# g_bbox 0 .. 1.00, g_giou 0.59 .. 1.00; largest relative error 6.7e-7, so the 1e-5 floor binds and the 4x margin never does.
@pytest.mark.parametrize('R,eos', [(7, 0.1), (256, 0.25), (300, 0.1)])
def test_set_loss_against_fp64_autograd_by_geometry_class(R, eos):
    logits, boxes, tgt, match, cls = CC.set_loss_layout(R)
    assert not np.array_equal(match[0], match[1]) and (match[2] < 0).all()
    losses, gl, gb, gg = _run_set_loss(logits, boxes, tgt, match, eos)
    bad = []
    for layer in range(3):
        bad += _compare_layer(f'R={R}/layer{layer}', (losses[layer], gl[layer], gb[layer], gg[layer]), logits[layer], boxes[layer], tgt,
                              match[layer], cls[layer], eos)
    assert not bad, bad
    # class_error counts l0 == l1 on a matched row as correct
    r0 = int(np.nonzero(match[0] >= 0)[0][0])
    assert logits[0, r0, 0] == logits[0, r0, 1]
    # the layer without a match: defined as zero box losses, zero class_error, zero box gradients — exactly
    assert losses[2, 1] == 0 and losses[2, 2] == 0 and losses[2, 3] == 0 and not gb[2].any() and not gg[2].any()
    # off a match there is no box gradient, exactly
    for layer in range(2):
        un = match[layer] < 0
        assert not gb[layer][un].any() and not gg[layer][un].any()


def test_set_loss_rebased_targets_of_the_per_frame_matcher():
    lg, bx, tg, match, loss_match, vid_off, videos, cls = CC.rebase_layout()
    assert (match[100:200][match[100:200] >= 0] - vid_off[1]).min() == 2 and (match[200:] < 0).all()
    got = _run_set_loss(lg[None], bx[None], tg, match[None], 0.1, vid_off=vid_off, rows_per_video=100)
    bad = _compare_layer('rebase', [g[0] for g in got], lg, bx, tg, loss_match, cls, 0.1, videos)
    assert not bad, bad
    # without the re-basing the kernel reads other boxes: the case can tell
    plain = _run_set_loss(lg[None], bx[None], tg, match[None], 0.1)
    assert abs(float(plain[0][0, 1]) - float(got[0][0, 1])) > 1e-3


def test_set_loss_flags_poison_their_own_layer_only():
    R = 300
    logits, boxes, tgt, match, _ = CC.set_loss_layout(R)
    match[2] = match[0][::-1]     # every layer healthy and matched here
    boxes[2] = boxes[0][::-1]
    clean = _run_set_loss(logits, boxes, tgt, match, 0.1)
    assert all(np.isfinite(a).all() for a in clean)
    zeros = np.zeros(3 * R, np.int32)
    for s1, s2 in ((zeros, zeros), (None, zeros), (zeros, None)):
        out = _run_set_loss(logits, boxes, tgt, match, 0.1, status=s1, box_status=s2, ppl=R)
        assert all(np.array_equal(a, b) for a, b in zip(out, clean))
    st = zeros.copy()
    st[R - 1] = 1                 # the last problem of layer 0, past the 256-thread loop's first trip
    bs = zeros.copy()
    bs[R + 7] = 1                 # a problem of layer 1
    for flagged, kw in ((0, dict(status=st, box_status=zeros)), (0, dict(status=st, box_status=None)),
                        (1, dict(status=zeros, box_status=bs)), (1, dict(status=None, box_status=bs)),
                        (0, dict(status=2 * st, box_status=None))):
        out = _run_set_loss(logits, boxes, tgt, match, 0.1, ppl=R, **kw)
        for layer in range(3):
            for a, b in zip(out, clean):
                if layer == flagged:
                    assert np.isnan(a[layer]).all(), (flagged, layer)
                else:
                    assert np.array_equal(a[layer], b[layer]), (flagged, layer)


# ---------------------------------------------------------------------------
# 4. through the modules
B_, N_, T_, Q_ = 2, 10, 5, 2


def _crit(kind, NL):
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    args = syn.head_args(num_layers=NL, aux_loss=NL > 1, num_queries=N_, num_queries_per_frame=Q_, num_frames=T_, matcher=kind)
    return build_loss(args).cuda(), syn.synth_targets(B_, T_, seed=2, max_per_frame=2)


def _outputs(NL, seed=1, bad_box=False, nan_logit=False):
    """hand-made outputs dict (aux layers first, the last layer last); faults go into the LAST layer, row 0 of video 0 (its frame
    0 always has a box)."""
    from svol_amd import synthetic as syn
    leaves = []
    for l_ in range(NL):
        lg, bx = syn.synth_head_outputs(B_, N_, seed=seed + l_)
        if l_ == NL - 1 and bad_box:
            bx[0, 0, 2] = -2.0 ** -6
        if l_ == NL - 1 and nan_logit:
            lg[0, 0, 1] = float('nan')
        leaves.append((lg.cuda().requires_grad_(True), bx.cuda().requires_grad_(True)))
    out = {'pred_logits': leaves[-1][0], 'pred_boxes': leaves[-1][1]}
    if NL > 1:
        out['aux_outputs'] = [{'pred_logits': a, 'pred_boxes': b} for a, b in leaves[:-1]]
    return out, leaves


def _step(crit, out, tg):
    ld = crit(out, tg)
    tot = sum(ld[k] * crit.weight_dict[k] for k in ld if k in crit.weight_dict)
    tot.backward()
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in ld.items()}


def _assert_last_layer_poisoned(ld, leaves, NL):
    for k in ('loss_label', 'loss_bbox', 'loss_giou', 'class_error'):
        assert np.isnan(ld[k]), (k, ld[k])
        for i in range(NL - 1):
            assert np.isfinite(ld[f'{k}_{i}']), (k, i)
    assert torch.isnan(leaves[-1][0].grad).all() and torch.isnan(leaves[-1][1].grad).all()
    for lg, bx in leaves[:-1]:
        assert torch.isfinite(lg.grad).all() and torch.isfinite(bx.grad).all()


@pytest.mark.parametrize('NL', [1, 3], ids=['one_layer', 'aux_loss'])
@pytest.mark.parametrize('kind', ['video_matcher', 'per_frame_matcher'])
def test_modules_raise_what_the_reference_raises(kind, NL):
    crit, tg = _crit(kind, NL)
    last = lambda o: {'pred_logits': o['pred_logits'].detach(), 'pred_boxes': o['pred_boxes'].detach()}
    # a degenerate prediction box: NaN losses and gradients, AssertionError from everything that hands out indices
    out, leaves = _outputs(NL, bad_box=True)
    _assert_last_layer_poisoned(_step(crit, out, tg), leaves, NL)
    with pytest.raises(AssertionError):
        crit.last_indices()
    with pytest.raises(AssertionError):
        crit.matcher(last(out), tg)
    # a NaN logit, healthy boxes: scipy's ValueError
    out, leaves = _outputs(NL, nan_logit=True)
    _assert_last_layer_poisoned(_step(crit, out, tg), leaves, NL)
    with pytest.raises(ValueError, match='matrix contains invalid numeric entries'):
        crit.last_indices()
    with pytest.raises(ValueError, match='matrix contains invalid numeric entries'):
        crit.matcher(last(out), tg)
    # both: the box check comes first in the reference, AssertionError wins
    out, leaves = _outputs(NL, bad_box=True, nan_logit=True)
    _assert_last_layer_poisoned(_step(crit, out, tg), leaves, NL)
    with pytest.raises(AssertionError):
        crit.last_indices()
    with pytest.raises(AssertionError):
        crit.matcher(last(out), tg)
    # a healthy batch straight after
    out, leaves = _outputs(NL)
    ld = _step(crit, out, tg)
    assert all(np.isfinite(v) for v in ld.values()), ld
    assert len(crit.last_indices()) == NL and len(crit.matcher(last(out), tg)) == B_
    assert all(torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all() for a, b in leaves)


def _negate_first_box_height(tg):
    import copy
    bad = copy.deepcopy(tg)
    frame = next(f for f in bad[1]['bboxes'].values() if f)
    frame[0]['bbox'] = frame[0]['bbox'] * torch.tensor([1.0, 1.0, 1.0, -1.0])
    return bad


@pytest.mark.parametrize('kind', ['video_matcher', 'per_frame_matcher'])
def test_static_packed_targets_recover_after_a_bad_batch(kind):
    """The kernels rewrite every flag on every launch: a flagged batch in the fixed-capacity buffers (the ones a captured step
    replays) leaves nothing behind for the next one."""
    from svol_amd.modeling.matcher import StaticPackedTargets
    NL = 3
    crit, tg = _crit(kind, NL)
    sp = StaticPackedTargets(kind, NL, B_, N_, T_, Q_, torch.device('cuda'), max_boxes_per_video=16)
    crit.static_packed = sp
    sp.load(_negate_first_box_height(tg))
    out, _ = _outputs(NL)
    ld = _step(crit, out, tg)
    assert all(np.isnan(v) for v in ld.values()), ld   # the target is shared by every layer's problems: all of them flagged
    with pytest.raises(AssertionError):
        crit.last_indices()
    sp.load(tg)
    out, leaves = _outputs(NL)
    ld = _step(crit, out, tg)
    match = crit.last_match.clone()
    idx = crit.last_indices()
    assert all(np.isfinite(v) for v in ld.values()), ld
    fresh, _ = _crit(kind, NL)
    out2, leaves2 = _outputs(NL)
    ld2 = _step(fresh, out2, tg)
    assert ld == ld2                                     # bit for bit
    assert torch.equal(match, fresh.last_match)
    assert all(torch.equal(a.grad, c.grad) and torch.equal(b.grad, d.grad) for (a, b), (c, d) in zip(leaves, leaves2))
    assert str(idx) == str(fresh.last_indices())


def _empty_video(tv):
    return dict(tv, bboxes=OrderedDict((k, []) for k in tv['bboxes']), num_boxes_per_frame=[0] * len(tv['num_boxes_per_frame']),
                total_boxes=0)


def _cost_with_sentinels(crit, packed, lg, bx):
    """svol_match_cost over `packed`'s tables into a buffer of packed.last_cost's size with sentinels around it."""
    L = _lib()
    n = packed.last_cost.numel()
    buf = torch.full((SENT + n + SENT,), SENT_BITS, dtype=torch.int32, device='cuda')
    m = crit.matcher
    rc = L.lib().svol_match_cost(lg.data_ptr(), bx.data_ptr(), packed.tgt_boxes.data_ptr(), packed.pred_off.data_ptr(),
                                 packed.pred_cnt.data_ptr(), packed.tgt_off.data_ptr(), packed.tgt_cnt.data_ptr(), packed.cost_off.data_ptr(),
                                 buf.data_ptr() + 4 * SENT, packed.n_problems, float(m.cost_bbox), float(m.cost_giou), float(m.cost_class),
                                 None, _stream())
    L.check(rc, 'svol_match_cost')
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:SENT] == SENT_BITS).all() and (raw[-SENT:] == SENT_BITS).all(), 'a cost was written outside the cost buffer'
    body = raw[SENT:SENT + n]
    assert (body[packed.cost_numel:] == SENT_BITS).all()
    assert np.array_equal(body[:packed.cost_numel], packed.last_cost.view(torch.int32).cpu().numpy()[:packed.cost_numel])


@pytest.mark.parametrize('empty', ['one_video', 'whole_batch'])
@pytest.mark.parametrize('kind', ['video_matcher', 'per_frame_matcher'])
def test_videos_without_boxes(kind, empty):
    """A video without a single box, and a batch without one: the reference cannot run either (torch.stack([]) raises in its matcher),
    this build packs them, writes nothing out of range, matches nothing there, and scores what is left against fp64."""
    from types import SimpleNamespace
    from oracle import svol_oracle as O
    NL = 3
    crit, tg = _crit(kind, NL)
    tg = [tg[0] if empty == 'one_video' else _empty_video(tg[0]), _empty_video(tg[1])]
    out, leaves = _outputs(NL)
    ld = crit(out, tg)
    packed = crit.last_packed
    match = crit.last_match.view(NL, B_ * N_).cpu().numpy()
    losses = crit.last_losses.cpu().numpy()
    assert packed.total_boxes == (0 if empty == 'whole_batch' else sum(tg[0]['num_boxes_per_frame']))
    assert (packed._flags.cpu().numpy() == 0).all()
    crit.last_indices()
    assert (match[:, N_:] == -1).all()
    logits = np.stack([a.detach().cpu().numpy().reshape(-1, 2) for a, _ in leaves])
    boxes = np.stack([b.detach().cpu().numpy().reshape(-1, 4) for _, b in leaves])
    _cost_with_sentinels(crit, packed, _d(logits), _d(boxes))
    tgt = packed.tgt_boxes.cpu().numpy()
    margs = SimpleNamespace(set_cost_bbox=crit.matcher.cost_bbox, set_cost_giou=crit.matcher.cost_giou,
                            set_cost_class=crit.matcher.cost_class, matcher=kind, num_frames=T_, num_queries_per_frame=Q_)
    # unit gradients of the same inputs, through the ABI (the module keeps them inside its autograd node)
    got = _run_set_loss(logits, boxes, tgt, match, crit.eos_coef,
                        vid_off=packed.vid_off if kind == 'per_frame_matcher' else None, rows_per_video=N_)
    assert np.array_equal(got[0], losses)
    bad = []
    for layer in range(NL):
        m = match[layer]
        if empty == 'whole_batch':
            assert (m == -1).all()
        else:   # video 0 is matched as the oracle matches it alone
            ref_idx = O.match(margs, torch.from_numpy(logits[layer, :N_][None]), torch.from_numpy(boxes[layer, :N_][None]), tg[:1])[0]
            dev_idx = packed.indices_from_match(crit.last_match, layer)[0]
            assert dev_idx[0].tolist() == ref_idx[0].tolist() and dev_idx[1].tolist() == ref_idx[1].tolist()
            assert len(packed.indices_from_match(crit.last_match, layer)[1][0]) == 0
        lm = m.copy()   # the rows the loss reads (the per-frame matcher's ids are re-based per video)
        if kind == 'per_frame_matcher' and (m >= 0).any():
            lm[m >= 0] = m[m >= 0] - m[m >= 0].min()
        cls = ['matched' if x >= 0 else 'background' for x in m]
        bad += _compare_layer(f'{kind}/{empty}/layer{layer}', [g[layer] for g in got], logits[layer], boxes[layer], tgt, lm,
                              ['random' if c == 'matched' else c for c in cls], crit.eos_coef)
        if empty == 'whole_batch':
            assert losses[layer, 1] == 0 and losses[layer, 2] == 0 and losses[layer, 3] == 0
            assert not got[2][layer].any() and not got[3][layer].any()
    assert not bad, bad
    tot = sum(ld[k] * crit.weight_dict[k] for k in ld if k in crit.weight_dict)
    tot.backward()
    assert all(torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all() for a, b in leaves)
