"""The matcher / criterion case tables (tests/criterion_cases.py) checked against themselves, on the CPU: the classes are what their
names say in fp32 and in fp64 alike, the fp64 references are finite, the fp32 oracle alone stays well inside every bar the GPU tests
apply, the tie classes really tell a kernel that picks a side from torch's split, and the LSAP blocks are labelled as scipy sees them."""
import numpy as np
import pytest
import torch

from tests import criterion_cases as CC


def test_every_class_has_at_least_three_dyadic_pairs():
    for name, c in CC.CLASSES.items():
        assert len(c.pairs) >= 3, name
        for b, t in c.pairs:
            for box in (b, t):
                e = np.array(CC.edges(np.asarray(box, np.float64), np.float64)) * 64
                assert np.array_equal(e, np.round(e)) and e.min() >= 0 and e.max() <= 64, (name, box)
                assert np.array_equal(np.asarray(box, np.float32).astype(np.float64), np.asarray(box, np.float64)), (name, box)
    assert sum(1 for n, _, _ in CC.all_pairs() if n == 'random') == 40


@pytest.mark.parametrize('name', list(CC.CLASSES))
def test_class_predicate_holds_in_fp32_and_fp64(name):
    c = CC.CLASSES[name]
    for b, t in c.pairs:
        assert CC.predicate_holds(c, b, t, np.float32), (name, b, t)
        assert CC.predicate_holds(c, b, t, np.float64), (name, b, t)
    # and the predicate is not vacuous: no pair of any OTHER template satisfies all of them at once
    other = [p for n, cc in CC.CLASSES.items() if n != name for p in cc.pairs[:1]]
    assert not all(CC.predicate_holds(c, b, t, np.float64) for b, t in other)


def _layers(R):
    logits, boxes, tgt, match, cls = CC.set_loss_layout(R)
    for layer in range(3):
        yield layer, logits[layer], boxes[layer], tgt, match[layer], cls[layer], None
    if R == 300:
        lg, bx, tg, _, loss_match, _, videos, cl = CC.rebase_layout()
        yield 'rebase', lg, bx, tg, loss_match, cl, videos


@pytest.mark.parametrize('R', [7, 256, 300])
def test_fp64_references_are_finite_and_the_fp32_oracle_stays_inside_a_quarter_of_every_bar(R):
    seen = set()
    for layer, lg, bx, tg, m, cls, videos in _layers(R):
        K = int((m >= 0).sum())
        ref = CC.set_loss_reference(lg, bx, tg, m, 0.1, torch.float64, videos)
        f32 = CC.set_loss_reference(lg, bx, tg, m, 0.1, torch.float32, videos)
        for a in ref:
            assert np.isfinite(a).all(), (R, layer)
        for v32, v64 in zip(f32[0], ref[0]):
            assert abs(v32 - v64) <= 0.25 * CC.LOSS_BAR * max(1.0, abs(v64)), (R, layer, v32, v64)
        for which, g32, g64 in zip(('g_label', 'g_bbox', 'g_giou'), f32[1:], ref[1:]):
            for cname, (err, ref_max) in CC.per_class_errors(g32, g64, cls).items():
                seen.add(cname)
                if ref_max < 1e-12:   # only what must be zero is zero: no box gradient off a match, none at all on identical boxes
                    assert cname in CC.ZERO_GRAD_CLASSES + ('background',) and which != 'g_label', (R, layer, which, cname)
                if cname == 'random':
                    continue          # its bar IS this error, x4
                bar = CC.grad_bar(cname, ref_max, K)
                print(f'R={R} layer={layer} {which:8s} {cname:20s} fp32 oracle err {err:.2e}  bar {bar:.2e}  ratio {err / bar:.3f}')
                assert err <= 0.25 * bar, (R, layer, which, cname, err, bar)
    if R >= 256:
        assert seen == set(CC.CLASSES) | {'random', 'background'}


@pytest.mark.parametrize('name', CC.TIE_CLASSES)
def test_tie_classes_tell_a_kernel_that_picks_a_side(name):
    """fp64 gradients with the tied prediction coordinate nudged by +-2^-20: the two differ by >= 1e-2 of max |g| and the tie
    gradient (torch's even split, or the clamp's closed side) lies between them — so a kernel that takes either side fails the 1e-5
    bar by three orders of magnitude."""
    c = CC.CLASSES[name]
    for b, t in c.pairs:
        g0 = np.concatenate(CC.pair_gradients(b, t))
        side = []
        for s in (+1, -1):
            bn = np.asarray(b, np.float64).copy()
            bn[c.nudge] += s * CC.NUDGE
            side.append(np.concatenate(CC.pair_gradients(bn, t)))
        gmax = max(np.abs(side[0]).max(), np.abs(side[1]).max())
        gap = np.abs(side[0] - side[1]).max()
        assert gap >= 1e-2 * gmax, (name, b, gap, gmax)
        lo, hi = np.minimum(side[0], side[1]), np.maximum(side[0], side[1])
        assert (g0 >= lo - 1e-4 * gmax).all() and (g0 <= hi + 1e-4 * gmax).all(), (name, b, g0, lo, hi)
        # ... and it is neither side: at least 1e-2 of max |g| (x 1/2) from one of them, hence 1e-5 catches a kernel taking that one
        assert max(np.abs(g0 - side[0]).max(), np.abs(g0 - side[1]).max()) >= 0.5e-2 * gmax


def test_touching_corner_is_a_tie_without_sides():
    """why touch_corner has no nudge: the gradient is continuous across that double boundary."""
    c = CC.CLASSES['touch_corner']
    for b, t in c.pairs:
        g0 = np.concatenate(CC.pair_gradients(b, t))
        for k in (0, 1):
            for s in (+1, -1):
                bn = np.asarray(b, np.float64).copy()
                bn[k] += s * CC.NUDGE
                assert np.abs(np.concatenate(CC.pair_gradients(bn, t)) - g0).max() <= 1e-3 * np.abs(g0).max()


def test_match_cost_problem_set():
    clean, bad = CC.match_cost_problem_set(False), CC.match_cost_problem_set(True)
    assert not CC.expected_box_status(clean).any()
    assert np.nonzero(CC.expected_box_status(bad))[0].tolist() == sorted(CC.COST_BAD) == [3, 5, 6]
    sizes = (clean.pred_cnt * clean.tgt_cnt).tolist()
    assert 333 in sizes and 256 in sizes and sizes[2] == 0 and sizes[-1] == 0 and (4, 40) in CC.COST_SHAPES
    lg = clean.logits
    assert ((lg[:, 0] == 80) & (lg[:, 1] == -80)).any() and ((lg[:, 0] == -80) & (lg[:, 1] == 80)).any() and (lg[:, 0] == lg[:, 1]).any()
    for w in CC.COST_WEIGHTS:
        for p in range(clean.n):
            if sizes[p] == 0:
                continue
            po, pc, to, tc = clean.pred_off[p], clean.pred_cnt[p], clean.tgt_off[p], clean.tgt_cnt[p]
            C = CC.cost_block_reference(lg[po:po + pc], clean.boxes[po:po + pc], clean.tgt[to:to + tc], *w)
            assert C.shape == (pc, tc) and np.isfinite(C).all(), p


def test_lsap_blocks_reach_the_paths_and_are_labelled_as_scipy_sees_them():
    assert CC.lsap_path(1, 1) == 'reg'
    for path, a, b in CC.LSAP_SHAPES:
        assert CC.lsap_path(a, b) == path, (path, a, b)
    assert {(p, a > b) for p, a, b in CC.LSAP_SHAPES} == {(p, t) for p in ('reg', 'lds', 'global') for t in (False, True)}
    n = {0: 0, 1: 0, 2: 0}
    for lname, probs in CC.lsap_launches():
        assert max(max(c.shape) for _, c, _ in probs) == CC.LSAP_MAX_DIM
        for label, c, st in probs:
            got, r, _ = CC.scipy_status(c)
            assert got == st, (lname, label, got, st)
            n[st] += 1
            if 'inf_feasible' in label:
                assert 0.05 < np.isinf(c).mean() < 0.15 and np.isfinite(c[r, _]).all()
        if lname != 'healthy':
            assert [st for _, _, st in probs][1::2] == [0] * 6 and all(st != 0 for _, _, st in probs[0::2])
    assert n[1] == 12 and n[2] == 6 and n[0] >= 30
