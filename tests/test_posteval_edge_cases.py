"""The evaluation / post-processing edge cases (tests/posteval_edge_cases.py) on the CPU:

* the oracle reproduces, bit for bit, what the reference itself computed on every record set (tests/golden/posteval_edges.json);
* every case reaches what it is for -- term counts of the AP sum in each regime of numpy's pairwise summation, NaN IoUs, IoU ties and
  score ties that change the AP when the rule is flipped, an all-NaN AP row, a tie inside every chunk -- computed from the oracle,
  not assumed;
* the reference order of the post-processing inputs is unambiguous: fp64 and fp32 scores sort the grid the same way, saturated
  pairs are exactly 1.0 / 0.0.
"""
import contextlib
import copy
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import posteval as O
from tests import posteval_edge_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, 'golden', 'posteval_edges.json')))


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        yield


@contextlib.contextmanager
def spy():
    """record, while the oracle runs, the terms of every AP sum and every IoU row of the AP path"""
    log = {'terms': [], 'ious': []}
    ipr, cross = O.interpolated_precision_recall, O.compute_iou_batch_cross

    def ipr_spy(precision, recall):
        mprecision = np.hstack([[0], precision, [0]])
        mrecall = np.hstack([[0], recall, [1]])
        for i in range(len(mprecision) - 1)[::-1]:
            mprecision[i] = max(mprecision[i], mprecision[i + 1])
        idx = np.where(mrecall[1::] != mrecall[0:-1])[0] + 1
        log['terms'].append((mrecall[idx] - mrecall[idx - 1]) * mprecision[idx])
        out = ipr(precision, recall)
        assert np.array_equal(np.sum(log['terms'][-1]), out, equal_nan=True)
        return out

    def cross_spy(b1, b2):
        out = cross(b1, b2)
        log['ious'].append(out)
        return out

    O.interpolated_precision_recall, O.compute_iou_batch_cross = ipr_spy, cross_spy
    try:
        yield log
    finally:
        O.interpolated_precision_recall, O.compute_iou_batch_cross = ipr, cross


def oracle_ap(results):
    with quiet():
        _, ap = O.compute_ap(copy.deepcopy(results), iou_thds=C.AP_THDS)
    return ap


def groups_of(results):
    seen = []
    for r in results:
        k = r['video'] + r['sketch']
        if r['pred_boxes'] and k not in seen:
            seen.append(k)
    return seen


# ---- the oracle against the reference's numbers --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(C.RECORD_SETS))
def test_oracle_matches_reference_on_the_edges(name):
    build, ks = C.RECORD_SETS[name]
    results, fx = build(), FX[name]
    assert all(float(f'{e:.4f}') == e for r in results for row in r['pred_boxes'] + [g['bbox'] for g in r['gt_boxes']] for e in row)
    assert groups_of(results) == fx['groups']
    C.assert_same_bits(oracle_ap(results), fx['ap'], f'{name}: AP')
    assert sorted(fx['max_ious']) == sorted(str(k) for k in ks)
    for k in ks:
        want = fx['max_ious'][str(k)]
        if isinstance(want, dict):
            with pytest.raises(Exception) as e:
                O.compute_recall_at_k(results, k=k)
            assert type(e.value).__name__ == want['raises']
        else:
            with quiet():
                _, _, mi = O.compute_recall_at_k(results, k=k)
            C.assert_same_bits(np.asarray(mi, dtype=np.float64), want, f'{name}: max IoU, k={k}')
    if 'raises' in fx['metrics']:
        with pytest.raises(Exception) as e, quiet():
            O.eval_results(copy.deepcopy(results))
        assert type(e.value).__name__ == fx['metrics']['raises']
    else:
        with quiet():
            got = O.eval_results(copy.deepcopy(results))
        assert C.null(json.loads(json.dumps(got))) == fx['metrics']
        assert list(got.keys()) == list(fx['metrics'].keys()) and list(got['brief'].keys()) == list(fx['metrics']['brief'].keys())


def test_fixture_is_small_and_holds_no_records():
    assert os.path.getsize(os.path.join(HERE, 'golden', 'posteval_edges.json')) < 100_000
    assert set(FX) == set(C.RECORD_SETS)
    assert all(set(v) == {'groups', 'ap', 'max_ious', 'metrics'} for v in FX.values())


# ---- every case reaches what it is for -----------------------------------------------------------------------------------------
def _pairwise(a):
    """numpy's pairwise summation, restated: the order the kernel must reproduce"""
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res += v
        return res
    if n <= 128:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] += a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            res += v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:n2]) + _pairwise(a[n2:])


def test_many_positives_reaches_every_regime_of_the_sum():
    results = C.many_positives()
    assert groups_of(results) == ['mp200sk', 'mp003sk', 'mp020sk', 'mp320sk']
    n_gt = {}
    for r in results:
        n_gt[r['video']] = n_gt.get(r['video'], 0) + len(r['gt_boxes'])
    assert n_gt == {'mp200': 200, 'mp003': 3, 'mp020': 20, 'mp320': 320}
    with spy() as log:
        oracle_ap(results)
    terms = log['terms']                          # [group][threshold]
    assert len(terms) == 4 * len(C.AP_THDS)
    counts = np.array([len(t) for t in terms]).reshape(4, -1)
    print('AP term counts per (group, threshold):', counts.tolist())
    assert (counts < 8).any() and (counts[0] > 128).any() and (counts > 256).any()
    assert ((counts >= 8) & (counts <= 128) & (counts % 8 != 0)).any()
    assert counts.max() <= 600                    # at most 3 levels of the recursion: the branch, not the stack limit
    assert ((counts > 128) & (counts <= 256)).any()   # one level and two levels
    differs = 0
    for t in terms:
        assert _pairwise(list(t)) == np.sum(t)    # the restatement above IS numpy's order
        if len(t) > 128:
            left = 0.0
            for v in t:
                left += v
            differs += left != np.sum(t)
    assert differs >= 1, 'a left-to-right sum gives the same bits everywhere: a wrong summation order would not show'
    print('pairs above 128 terms whose left-to-right sum differs from np.sum:', differs)


def test_degenerate_reaches_nan_ious():
    results = C.degenerate()
    with spy() as log:
        oracle_ap(results)
    n_nan = sum(int(np.isnan(i).sum()) for i in log['ious'])
    n_zero_valid = 0
    for r in results:       # touching pairs: valid with intersection 0 over a non-zero union
        for p in r['pred_boxes']:
            for g in r['gt_boxes']:
                a, b = np.array(p[:4]), np.array(g['bbox'])
                xmin, ymin, xmax, ymax = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
                union = O.box_area(a) + O.box_area(b)
                n_zero_valid += bool(xmin <= xmax and ymin <= ymax and (xmax - xmin) * (ymax - ymin) == 0 and union > 0)
    assert n_nan >= 1 and n_zero_valid >= 1
    # the NaN candidate that is already locked: frame 3, the second prediction sees NaN against ground truth 0 and is a false positive
    assert any(np.isnan(i).sum() >= 2 for i in log['ious'])
    for k in (1, 5):
        with quiet():
            _, _, mi = O.compute_recall_at_k(results, k=k)
        assert np.isnan(mi).any() and not np.isnan(mi).all()
    assert not np.isnan(oracle_ap(results)).any()


def private_ap(ground_truth, prediction, thds, later_gt_first=True, earlier_pred_first=True):
    """the oracle's matching loop with its two tie rules as switches (the flipped rules are what a wrong kernel would do).  The
    candidates are ordered by an explicitly STABLE argsort, reversed: the rule the kernel implements, on any numpy build."""
    K, N, M = len(thds), len(ground_truth), len(prediction)
    prediction = list(prediction) if earlier_pred_first else list(prediction)[::-1]
    prediction.sort(key=lambda x: -x['score'])
    lock = np.ones((K, N)) * -1
    tp, fp = np.zeros((K, M)), np.zeros((K, M))
    by_frame = {}
    for i, g in enumerate(ground_truth):
        by_frame.setdefault(g['frame'], []).append((i, g))
    box = lambda d: [d['top-left-x'], d['top-left-y'], d['bot-right-x'], d['bot-right-y']]       # noqa: E731
    for idx, p in enumerate(prediction):
        gts = by_frame.get(p['frame'])
        if gts is None:
            fp[:, idx] = 1
            continue
        iou = O.compute_iou_batch_cross(np.array([box(p)]), np.array([box(g) for _, g in gts])).reshape(-1)
        order = iou.argsort(kind='stable')[::-1] if later_gt_first else np.argsort(-iou, kind='stable')
        for t, thr in enumerate(thds):
            for j in order:
                if iou[j] < thr:
                    break
                if lock[t, gts[j][0]] >= 0:
                    continue
                tp[t, idx] = 1
                lock[t, gts[j][0]] = idx
                break
            fp[t, idx] = 1 - tp[t, idx]
    tp_c, fp_c = np.cumsum(tp, axis=1), np.cumsum(fp, axis=1)
    with np.errstate(all='ignore'):
        return np.array([O.interpolated_precision_recall((tp_c / (tp_c + fp_c))[t], (tp_c / float(N))[t]) for t in range(K)])


def _private(results, thds=C.AP_THDS, **kw):
    preds, gts = C.grouped(results)
    return np.array([private_ap(gts[k], preds[k], thds, **kw) for k in preds])


@pytest.mark.parametrize('name', list(C.RECORD_SETS))
def test_no_record_set_depends_on_how_numpy_orders_equal_ious(name):
    """the private copy (explicitly stable order) is the oracle (numpy's default argsort, whatever this build dispatches it to) on
    every record set, at the ten AP thresholds and at the 64 of the GPU test: the expected values hold on any machine"""
    results = C.RECORD_SETS[name][0]()
    C.assert_same_bits(_private(results), oracle_ap(results), name)
    if name in C.K64_SETS:
        preds, gts = C.grouped(results)
        with quiet():
            want = np.array([O.compute_average_precision_detection(gts[k], preds[k], iou_thresholds=C.K64) for k in preds])
        C.assert_same_bits(_private(results, C.K64), want, f'{name}, 64 thresholds')


def test_iou_ties_change_the_ap_when_the_rule_is_flipped():
    results = C.iou_ties()
    assert max(len(r['gt_boxes']) for r in results) <= C.MAX_TIED_GT <= 16
    assert all(float(e * 64).is_integer() for r in results for row in [p[:4] for p in r['pred_boxes']] + [g['bbox'] for g in r['gt_boxes']]
               for e in row)
    with spy() as log:
        ap = oracle_ap(results)
    n_ties = sum(int(len(i.reshape(-1)) - len(np.unique(i[i >= 0.5]))) - int((i < 0.5).sum()) for i in log['ious'])
    assert n_ties >= 12, 'equal IoUs at or above the lowest threshold'
    flipped = _private(results, later_gt_first=False)
    assert (flipped != ap).any(axis=1).all(), 'every group must notice the flipped rule'
    assert (flipped[:, :4] < ap[:, :4]).all()      # B is lost at 0.5 .. 0.65


def test_score_ties_change_the_ap_under_a_reversed_stable_order():
    results = C.score_ties()
    for key in ('st', 'st2'):
        assert len({p[4] for r in results if r['video'] == key for p in r['pred_boxes']}) == 1
    assert len({r['frame'] for r in results if r['video'] == 'st'}) < sum(r['video'] == 'st' for r in results)   # a frame in two records
    ap = oracle_ap(results)
    assert (_private(results, earlier_pred_first=False) != ap).any(axis=1).all()


def test_wide_frame_shapes():
    results = C.wide_frame()
    assert [len(r['gt_boxes']) for r in results] == [7] * 4 and tuple(len(r['pred_boxes']) for r in results) == C.WIDE_N
    assert C.RECORD_SETS['wide_frame'][1] == (1, 5, 50)
    mi = {k: np.asarray(O.compute_recall_at_k(results, k=k)[2]) for k in (1, 5, 50)}
    assert not np.array_equal(mi[1], mi[5]) and not np.array_equal(mi[5], mi[50])
    # the reference's pair layout is NOT the plain (prediction, ground truth) matrix once n > 1: a kernel computing that one differs
    plain = np.concatenate([np.max([[O.compute_iou_batch_paired(np.array(p[:4]), np.array(g['bbox'])) for g in r['gt_boxes']]
                                    for p in r['pred_boxes'][:50]], axis=0) for r in results])
    assert not np.array_equal(plain, mi[50])


def test_no_gt_group_has_an_all_nan_row_and_late_group_order():
    results = C.no_gt_group()
    assert results[0]['video'] == 'late' and not results[0]['pred_boxes'] and groups_of(results)[-1] == 'lates'
    ap = oracle_ap(results)
    g = groups_of(results)
    assert np.isnan(ap[g.index('nogts')]).all()
    assert (ap[g.index('onlys')] == 0).all()       # ground truth exists, every prediction sits in a frame without any
    assert np.isfinite(ap[g.index('plains')]).all() and (ap[g.index('plains')] > 0).any()
    only = [r for r in results if r['video'] == 'only']
    assert all(not (r['gt_boxes'] and r['pred_boxes']) for r in only) and any(r['gt_boxes'] for r in only)
    with pytest.raises(IndexError):                # ground truth without predictions: the reference's recall@k dies in numpy
        O.compute_recall_at_k(results, k=1)
    assert all(r['pred_boxes'] for r in C.no_gt_group_recall() if r['gt_boxes'])
    g0 = C.no_gt_group_g0()
    assert sum(len(r['gt_boxes']) for r in g0) == 0 and np.isnan(oracle_ap(g0)).all()


def test_many_groups_sizes():
    results = C.many_groups()
    n_pred, n_gt, first, last = {}, {}, {}, {}
    for i, r in enumerate(results):
        k = r['video'] + r['sketch']
        n_pred[k] = n_pred.get(k, 0) + len(r['pred_boxes'])
        n_gt[k] = n_gt.get(k, 0) + len(r['gt_boxes'])
        first.setdefault(k, i)
        last[k] = i
    assert len(n_pred) == 70 and len(set(n_pred.values())) >= 8
    assert 1 in n_pred.values() and 1 in n_gt.values()
    n_rec = {k: sum(1 for r in results if r['video'] + r['sketch'] == k) for k in n_pred}
    assert sum(last[k] - first[k] + 1 > n_rec[k] for k in n_pred) >= 40, 'groups are interleaved in record order'
    assert all(r['pred_boxes'] for r in results if r['gt_boxes'])


# ---- post-processing inputs ------------------------------------------------------------------------------------------------------
def test_grid_scores_are_unambiguous():
    g = torch.from_numpy(C.GRID)
    s64 = torch.sigmoid(g)
    assert float((s64[1:] - s64[:-1]).min()) >= 1.31e-6
    lg = torch.stack([g.float(), torch.zeros(4096)], -1)
    s32 = torch.softmax(lg, -1)[:, 0]
    assert bool((s32[1:] > s32[:-1]).all()) and float((s32.double() - torch.softmax(lg.double(), -1)[:, 0]).abs().max()) < 9e-8
    # the kernel's own formula in numpy fp32
    l0 = lg[:, 0].numpy()
    m = np.maximum(l0, np.float32(0))
    e0, e1 = np.exp(l0 - m, dtype=np.float32), np.exp(np.float32(0) - m, dtype=np.float32)
    sk = e0 / (e0 + e1)
    assert sk.dtype == np.float32 and (sk[1:] > sk[:-1]).all() and np.abs(sk.astype(np.float64) - s64.numpy()).max() < 9e-8


def test_saturated_pairs_are_exact_in_fp32():
    one, zero = torch.tensor(C.SAT_ONE), torch.tensor(C.SAT_ZERO)
    assert {float(a - b) for a, b in C.SAT_ONE} == {30.0, 40.0, 200.0} and {float(a - b) for a, b in C.SAT_ZERO} == {-110.0, -200.0}
    assert bool((torch.softmax(one, -1)[:, 0] == 1.0).all()) and bool((torch.softmax(zero, -1)[:, 0] == 0.0).all())
    for a, b in C.SAT_ONE + C.SAT_ZERO:            # the kernel's formula, fp32: exactly 1.0 / 0.0 with or without denormals
        a, b = np.float32(a), np.float32(b)
        m = max(a, b)
        with np.errstate(under='ignore'):
            e0, e1 = np.exp(a - m, dtype=np.float32), np.exp(b - m, dtype=np.float32)
        assert e0 / (e0 + e1) == (1.0 if a > b else 0.0)
        assert not (-104.0 <= min(a - m, b - m) <= -87.0)


@pytest.mark.parametrize('case,build,chunk', C.PP_CASES, ids=[f'{n}-{c}' for n, _, c in C.PP_CASES])
def test_postprocess_inputs(case, build, chunk):
    logits, boxes, T = build(chunk)
    Bn, N = logits.shape[:2]
    assert Bn == C.B and logits.dtype == boxes.dtype == torch.float32
    assert -(-N // T) == chunk and (N % chunk != 0 or chunk == 1), 'the chunk size the launcher sees, a ragged last chunk'
    ref, perm = C.pp_reference(logits, boxes, T, 'fp32' if case == 'saturated' else 'fp64')
    assert all(sorted(perm[b].tolist()) == list(range(N)) for b in range(Bn))
    xy = ref[..., :4]
    assert bool((xy == 0).any()) and bool((xy == 1).any()) and bool(((xy > 0) & (xy < 1)).any()), 'the clamp cuts at 0 and at 1'
    assert all(len({tuple(r) for r in xy[b].tolist()}) == N for b in range(Bn)), 'the rows of a batch entry are told apart by their boxes'
    s32 = torch.softmax(logits, -1)[..., 0]
    if case != 'saturated':
        _, perm32 = C.pp_reference(logits, boxes, T, 'fp32')
        assert torch.equal(perm, perm32), "torch's fp32 softmax gives the same order"
        assert bool((logits[..., 1] == 0).all())
    else:
        sat = (s32 == 1.0) | (s32 == 0.0)
        assert 0.3 < float(sat.float().mean()) < 0.7 or N < 16
        pairs = {tuple(p) for p in logits[s32 == 1.0].tolist()}
        assert len(pairs) >= 2 or N < 16, 'several distinct logit pairs tie'
    if N > 1:
        assert any(len(set(logits[b, :, 0].tolist())) < N for b in range(Bn)) or case == 'saturated', 'drawn with repetition'
    if case == 'ties_inside_chunks':
        for b in range(Bn):
            for c0 in range(0, N, chunk):
                rows = [tuple(r) for r in logits[b, c0:c0 + chunk].tolist()]
                assert len(set(rows)) < len(rows), f'chunk at {c0} holds no exact tie'
                assert float(s32[b, c0]) == float(s32[b, c0 + len(rows) - 1])


def test_postprocess_chunk_sizes_cover_both_launch_shapes():
    assert C.CHUNKS == (1, 3, 63, 64, 65, 255, 256, 257, 1000, 12288) and C.CHUNK_LIMIT == 12288
    lasts = {c: C.pp_shape(c)[0] % c for c in C.CHUNKS}
    assert lasts[3] == 1, 'a last chunk of one row'
    lg, _, T = C.grid_one_row_tail()
    assert lg.shape[1] % 63 == 1 and -(-lg.shape[1] // T) == 63
