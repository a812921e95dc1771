"""Edge cases for the post-processing / evaluation kernels (svol_amd/csrc/posteval.hip) that the three synthetic fixtures never reach.

Pure CPU, seeded, no GPU import.  tests/test_posteval_edge_cases.py proves on the oracle that every case reaches the branch it is
for and pins the oracle to the reference's own numbers (tests/golden/posteval_edges.json, written by
tests/golden/make_golden_posteval_edges.py); tests/test_gpu_posteval_edges.py holds the kernels to the same numbers bit for bit.

Evaluation record sets: functions returning ``results``, the list of records of the JSONL wire format with every number already
rounded to 4 decimals.  RECORD_SETS maps a name to (builder, the k values of recall@k stored for it).

    many_positives      groups of 200, 3, 20 and 320 ground-truth boxes: every regime of numpy's pairwise sum in one launch.  (The
                        AP sum has at most #ground truth + 1 terms, so the 200-box group reaches one level of the recursion and
                        the 320-box group the second.)
    degenerate          zero-width predictions and ground truth, 0/0 IoUs, a touching pair, a NaN candidate that is already locked
    iou_ties            one prediction with exactly equal IoU against two ground-truth boxes of its frame (dyadic coordinates)
    score_ties          every prediction of a group has the same score
    wide_frame          7 ground-truth boxes against 1, 3, 5 and 9 predictions (the tile / repeat pair layout), k = 1, 5, 50
    no_gt_group         a group without ground truth, a group that predicts only where there is none (its ground truth sits in a
                        record without predictions: recall@k raises there, as in the reference), a group whose first record has no
                        predictions; no_gt_group_recall is the same without that one record, no_gt_group_g0 has no ground truth
    many_groups         70 interleaved groups of uneven size, some of one prediction, some of one ground-truth box

Post-processing inputs: functions of the chunk size returning (logits [2, N, 2], boxes [2, N, 4], num_frames), fp32, with
ceil(N / num_frames) == chunk and a ragged last chunk.

    grid                l1 = 0, l0 drawn with repetition from linspace(-8, 8, 4096): neighbouring scores are >= 1.31e-6 apart, so
                        the order is unambiguous in fp32 and equal logits are exact ties
    saturated           grid rows mixed with logit pairs whose score is exactly 1.0 or 0.0 in fp32: distinct pairs that tie
    ties_inside_chunks  grid rows with duplicated logit pairs inside every chunk, the ragged one included
"""
import numpy as np
import torch

AP_THDS = [float(f'{e:.2f}') for e in np.linspace(0.5, 0.95, 10)]
K64 = [i / 64 for i in range(1, 65)]       # 1/64 .. 1.0, with 0.5 and 0.75 (the tied IoUs themselves); not 0.0: every box of a frame would tie there
K64_SETS = ('many_positives', 'degenerate', 'iou_ties', 'score_ties', 'no_gt_group')


def r4(x):
    return float(f'{float(x):.4f}')


def rec(video, sketch, frame, gts, preds):
    return dict(video=video, sketch=sketch, shape=[1, 1], frame=frame,
                gt_boxes=[{'track_id': i, 'bbox': [r4(e) for e in g]} for i, g in enumerate(gts)],
                pred_boxes=[[r4(e) for e in p] for p in preds])


def _by_score(preds):
    """the wire format carries each record's predictions in descending score order (stable)"""
    return sorted(preds, key=lambda p: p[4], reverse=True)


def _rand_boxes(rng, n):
    c = rng.uniform(0.2, 0.8, (n, 2))
    wh = rng.uniform(0.08, 0.3, (n, 2))
    return np.round(np.concatenate([c - wh / 2, c + wh / 2], 1), 4)


def _jitter(rng, boxes, amp):
    b = np.clip(boxes + rng.uniform(-amp, amp, boxes.shape), 0.0, 1.0)
    lo, hi = np.minimum(b[:, :2], b[:, 2:]), np.maximum(b[:, :2], b[:, 2:])
    return np.round(np.concatenate([lo, hi], 1), 4)


def _interleave(groups):
    out = []
    for i in range(max(len(g) for g in groups)):
        out.extend(g[i] for g in groups if i < len(g))
    return out


def _dense_group(rng, video, n_frames, per_frame):
    """per ground-truth box two predictions: one within +-0.01 of it, one within +-0.2; random scores"""
    recs = []
    for f in range(n_frames):
        gt = _rand_boxes(rng, per_frame)
        pb = np.concatenate([_jitter(rng, gt, 0.01), _jitter(rng, gt, 0.2)], 0)
        sc = np.round(rng.uniform(0.0, 1.0, len(pb)), 4)
        recs.append(rec(video, 'sk', f, gt.tolist(), _by_score([list(b) + [s] for b, s in zip(pb.tolist(), sc.tolist())])))
    return recs


# ---- evaluation record sets ------------------------------------------------------------------------------------------------------
def many_positives():
    rng = np.random.default_rng(20260)
    return _interleave([_dense_group(rng, 'mp200', 40, 5), _dense_group(rng, 'mp003', 1, 3), _dense_group(rng, 'mp020', 4, 5),
                        _dense_group(rng, 'mp320', 64, 5)])


def degenerate():
    Z = [1.0, 0.2, 1.0, 0.6]                     # zero width at the clamp
    return [
        # the top prediction coincides with a zero-area ground truth: 0/0.  The second is a valid box whose edge touches Z
        # (intersection 0, IoU 0.0), so ground truth 0 sees NaN then 0.0 and ground truth 1 sees 0.0 then a real IoU.
        rec('dg', 's', 0, [Z, [0.6, 0.2, 0.9, 0.6]], [Z + [0.95], [0.6, 0.2, 1.0, 0.6, 0.9], [0.62, 0.2, 0.9, 0.58, 0.4]]),
        # a value first, the NaN second (np.max propagates it whatever the order); a zero-width pair that does not overlap (invalid: 0)
        rec('dg', 's', 1, [[1.0, 0.4, 1.0, 0.8], [1.0, 0.7, 1.0, 0.9]], [[0.5, 0.3, 1.0, 0.9, 0.85], Z + [0.8]]),
        # a touching pair, valid with intersection 0, beside an ordinary match
        rec('dg', 's', 2, [[0.3, 0.1, 0.5, 0.3], [0.1, 0.5, 0.4, 0.9]], [[0.1, 0.1, 0.3, 0.3, 0.7], [0.1, 0.5, 0.4, 0.88, 0.65]]),
        # the NaN candidate is already locked when the second prediction arrives: both coincide with ground truth 0, the third
        # prediction matches ground truth 1
        rec('dg', 's', 3, [Z, [0.2, 0.2, 0.6, 0.6]], [Z + [0.6], Z + [0.55], [0.2, 0.2, 0.6, 0.58, 0.5]]),
        # two zero-area ground truths coincident with one prediction: two NaN candidates, the later index is taken first
        rec('dg', 's', 4, [Z, Z, [0.0, 0.0, 0.0, 0.0]], [Z + [0.45], Z + [0.35], [0.0, 0.0, 0.0, 0.0, 0.3]]),
        # an ordinary group beside it
        rec('ok', 's', 0, [[0.1, 0.1, 0.5, 0.5]], [[0.1, 0.1, 0.5, 0.52, 0.9], [0.3, 0.3, 0.7, 0.7, 0.2]]),
    ]


MAX_TIED_GT = 3


def iou_ties():
    """coordinates are multiples of 1/16 (dyadic and 4-decimal at once): every IoU below is exact.
    A = [1/4, 1/4, 3/4, 3/4] contains ground truths 1 and 2, each 3/4 of it: IoU 0.75 with both.  B covers the half of A that lies
    in ground truth 1: IoU 2/3 with it and 1/4 with ground truth 2.  B is a true positive at 0.5 .. 0.65 exactly when A locked
    ground truth 2, the later index.

    No frame has more than MAX_TIED_GT = 3 ground-truth boxes.  The reference orders the candidates with numpy's default argsort,
    reversed.  Where that is an insertion sort (up to 16 elements in numpy's scalar quicksort) equal IoUs come out later index
    first, the rule the kernel implements; numpy builds that dispatch argsort to their AVX-512 / AVX2 sorting networks return
    equal keys in another order from 4 elements on (measured: never for 2 or 3 elements, 9 % of tied 4-element arrays, every
    16-element one), so above 3 boxes the reference's own tie order depends on the machine it runs on."""
    far = [0.0, 0.0, 0.125, 0.125]
    recs = [
        rec('it', 's', 0, [far, [0.25, 0.25, 0.625, 0.75], [0.375, 0.25, 0.75, 0.75]],
            [[0.25, 0.25, 0.75, 0.75, 0.9], [0.25, 0.25, 0.5, 0.75, 0.8]]),
        # the same, transposed, with the ground truths at indices 0 and 2 and a bystander between them
        rec('it', 's', 1, [[0.25, 0.25, 0.75, 0.625], far, [0.25, 0.375, 0.75, 0.75]],
            [[0.25, 0.25, 0.75, 0.75, 0.7], [0.25, 0.25, 0.75, 0.5, 0.6]]),
        # a three-way tie: A against three ground truths of IoU 0.5 each (halves of A); B is the left half itself
        rec('it', 's', 2, [[0.25, 0.25, 0.5, 0.75], [0.5, 0.25, 0.75, 0.75], [0.25, 0.25, 0.75, 0.5]],
            [[0.25, 0.25, 0.75, 0.75, 0.5], [0.25, 0.25, 0.5, 0.75, 0.4]]),
    ]
    # a second group: the tied pair at eight heights, one frame each, ground truth in both index orders around a bystander
    for i in range(8):
        y = 0.125 * i
        ga, gb = [0.0, y, 0.375, y + 0.0625], [0.125, y, 0.5, y + 0.0625]
        gts = [[0.75, 0.75, 0.875, 0.875], ga, gb] if i % 2 else [ga, [0.75, 0.75, 0.875, 0.875], gb]
        recs.append(rec('it3', 's', i, gts, [[0.0, y, 0.5, y + 0.0625, r4(0.95 - 0.1 * i)], [0.0, y, 0.25, y + 0.0625, r4(0.9 - 0.1 * i)]]))
    return recs


def score_ties():
    """one ground truth per frame, two or three predictions of score 0.5 on it: the first in record order takes it"""
    def frame(x, order):
        g = [x, 0.2, x + 0.4, 0.6]
        cand = [[x, 0.2, x + 0.4, 0.44, 0.5],     # IoU 0.6
                [x, 0.2, x + 0.4, 0.56, 0.5],     # IoU 0.9
                [x, 0.2, x + 0.4, 0.5, 0.5]]      # IoU 0.75
        return [g], [cand[i] for i in order]
    a = [rec('st', 's', f, *frame(0.05 * f, o)) for f, o in enumerate([(0, 1), (1, 0), (0, 2, 1), (2, 0), (1, 2, 0), (0, 1)])]
    a.append(rec('st', 's', 2, [[0.5, 0.7, 0.9, 0.9]], [[0.5, 0.7, 0.9, 0.88, 0.5], [0.5, 0.7, 0.9, 0.9, 0.5]]))   # frame 2 again
    b = [rec('st2', 's', f, *frame(0.1 * f, o)) for f, o in enumerate([(1, 0), (0, 1), (0, 1, 2)])]
    for r in b:
        for p in r['pred_boxes']:
            p[4] = 0.25
    return _interleave([a, b])


WIDE_N = (1, 3, 5, 9)


def wide_frame():
    rng = np.random.default_rng(7)
    recs = []
    for f, n in enumerate(WIDE_N):
        gt = _rand_boxes(rng, 7)
        pb = _jitter(rng, gt[rng.integers(0, 7, n)], 0.06)
        sc = np.round(rng.uniform(0.0, 1.0, n), 4)
        recs.append(rec('wfa' if f % 2 == 0 else 'wfb', 's', f, gt.tolist(),
                        _by_score([list(b) + [s] for b, s in zip(pb.tolist(), sc.tolist())])))
    return recs


def no_gt_group(unpredicted_gt=True, ground_truth=True):
    g = [0.2, 0.2, 0.6, 0.6]
    near, off = [0.2, 0.2, 0.6, 0.58], [0.5, 0.5, 0.9, 0.9]
    recs = [
        rec('late', 's', 0, [g] if unpredicted_gt else [], []),              # 'late' is seen first and becomes the LAST group
        rec('nogt', 's', 0, [], [near + [0.9], off + [0.3]]),                # no ground truth anywhere in this group
        rec('only', 's', 0, [], [near + [0.8]]),                             # predicts only where there is no ground truth ...
        rec('only', 's', 1, [g, off], []) if unpredicted_gt else None,       # ... and has ground truth where it does not predict
        rec('nogt', 's', 1, [], [off + [0.5]]),
        rec('plain', 's', 0, [g, off], [near + [0.7], off + [0.6], [0.0, 0.0, 0.1, 0.1, 0.1]]),
        rec('late', 's', 1, [g], [near + [0.4], off + [0.2]]),
        rec('only', 's', 2, [], [off + [0.2], near + [0.1]]),
    ]
    recs = [r for r in recs if r is not None]
    if not ground_truth:
        for r in recs:
            r['gt_boxes'] = []
    return recs


def no_gt_group_recall():
    return no_gt_group(unpredicted_gt=False)


def no_gt_group_g0():
    return no_gt_group(unpredicted_gt=False, ground_truth=False)


def many_groups():
    rng = np.random.default_rng(70)
    groups = []
    for i in range(70):
        if i % 10 == 3:
            shape = [(1, 1)]                      # one ground-truth box, one prediction
        elif i % 10 == 7:
            shape = [(2, 1)]                      # one prediction
        elif i % 10 == 5:
            shape = [(1, 4)]                      # one ground-truth box
        else:
            shape = [(1 + (i + f) % 3, 1 + (3 * i + f + i // 10) % 6) for f in range(1 + (i * 7 + i // 10) % 5)]
        recs = []
        for f, (m, n) in enumerate(shape):
            gt = _rand_boxes(rng, m)
            pb = _jitter(rng, gt[np.arange(n) % m], 0.04 if (i + f) % 2 else 0.12)
            sc = np.round(rng.uniform(0.0, 1.0, n), 4)
            recs.append(rec(f'v{i:02d}', f's{i % 4}', f, gt.tolist(), _by_score([list(b) + [s] for b, s in zip(pb.tolist(), sc.tolist())])))
        groups.append(recs)
    return _interleave(groups)


RECORD_SETS = {   # name: (builder, k values of recall@k)
    'many_positives': (many_positives, (1, 5)),
    'degenerate': (degenerate, (1, 5)),
    'iou_ties': (iou_ties, (1, 5)),
    'score_ties': (score_ties, (1, 5)),
    'wide_frame': (wide_frame, (1, 5, 50)),
    'no_gt_group': (no_gt_group, (1, 5)),
    'no_gt_group_recall': (no_gt_group_recall, (1, 5)),
    'no_gt_group_g0': (no_gt_group_g0, (1, 5)),
    'many_groups': (many_groups, (1, 5)),
}


# ---- post-processing inputs --------------------------------------------------------------------------------------------------------
CHUNKS = (1, 3, 63, 64, 65, 255, 256, 257, 1000, 12288)
CHUNK_LIMIT = 12288
GRID = np.linspace(-8.0, 8.0, 4096)
SAT_ONE = ((30.0, 0.0), (15.0, -15.0), (20.0, -10.0), (40.0, 0.0), (0.0, -40.0), (200.0, 0.0), (100.0, -100.0))     # l0 - l1 in {30, 40, 200}
SAT_ZERO = ((-110.0, 0.0), (0.0, 110.0), (-55.0, 55.0), (-200.0, 0.0), (-100.0, 100.0))                            # l0 - l1 in {-110, -200}
B = 2


def pp_shape(chunk, last=None):
    """(N, num_frames) with ceil(N / num_frames) == chunk and a last chunk of `last` rows (default: chunk - 2, or one row)"""
    if chunk == 1:
        return 5, 5
    if last is None:
        last = max(chunk - 2, 1)
    T = max(3, chunk - last + 1)                 # ceil(N / T) == chunk needs last > chunk - T
    N = (T - 1) * chunk + last
    assert 0 < last < chunk and -(-N // T) == chunk
    return N, T


def _pp_boxes(rng, N):
    cxcy = rng.uniform(-0.05, 1.05, (B, N, 2))        # every box keeps one unclamped coordinate per axis: rows stay distinguishable
    wh = rng.uniform(0.12, 0.6, (B, N, 2))
    boxes = torch.from_numpy(np.concatenate([cxcy, wh], -1)).float()
    boxes[:, 0] = torch.tensor([0.05, 0.5, 0.3, 0.2])        # x0 = -0.1: cut at 0
    boxes[:, -1] = torch.tensor([0.95, 0.5, 0.3, 0.2])       # x1 = 1.1: cut at 1
    return boxes


def _grid_rows(rng, N):
    pool = rng.choice(4096, size=max(1, min(4096, N // 2)), replace=False)      # fewer values than rows: repetition is certain
    return rng.choice(pool, size=(B, N))


def grid(chunk, last=None):
    N, T = pp_shape(chunk, last)
    rng = np.random.default_rng(1000 + chunk)
    logits = torch.zeros((B, N, 2), dtype=torch.float32)
    logits[..., 0] = torch.from_numpy(GRID[_grid_rows(rng, N)]).float()
    return logits, _pp_boxes(rng, N), T


def saturated(chunk):
    N, T = pp_shape(chunk)
    rng = np.random.default_rng(2000 + chunk)
    logits = torch.zeros((B, N, 2), dtype=torch.float32)
    logits[..., 0] = torch.from_numpy(GRID[_grid_rows(rng, N)]).float()
    pairs = torch.tensor(SAT_ONE + SAT_ZERO, dtype=torch.float32)
    kind = torch.from_numpy(rng.integers(0, 2 * len(pairs), (B, N)))             # half the rows stay grid rows
    sat = kind < len(pairs)
    logits[sat] = pairs[kind[sat]]
    return logits, _pp_boxes(rng, N), T


def ties_inside_chunks(chunk):
    """every chunk, the ragged last one included, holds duplicated logit pairs: neighbours and rows far apart.  (A chunk of one row
    cannot hold a tie: chunk >= 3 here, with a last chunk of chunk - 1 >= 2 rows.)"""
    assert chunk >= 3
    N, T = pp_shape(chunk, chunk - 1)
    rng = np.random.default_rng(3000 + chunk)
    logits = torch.zeros((B, N, 2), dtype=torch.float32)
    logits[..., 0] = torch.from_numpy(GRID[_grid_rows(rng, N)]).float()
    for c0 in range(0, N, chunk):
        n = min(chunk, N - c0)
        logits[:, c0 + n - 1] = logits[:, c0]                  # first and last row of the chunk
        if n >= 4:
            logits[:, c0 + n // 2 + 1] = logits[:, c0 + n // 2]    # neighbours
        if n >= 130:
            logits[:, c0 + 129] = logits[:, c0 + 1]            # in different 64-row strides of a block
    return logits, _pp_boxes(rng, N), T


PP_CASES = [('grid', grid, c) for c in CHUNKS] + [('saturated', saturated, c) for c in CHUNKS] + \
           [('ties_inside_chunks', ties_inside_chunks, c) for c in CHUNKS if c >= 3]


def grid_one_row_tail():
    """chunk 63 with a last chunk of one row"""
    return grid(63, last=1)


def pp_reference(logits, boxes, T, scores='fp64'):
    """[B, N, 5] fp64: clamped fp32 xyxy and the fp64 score, rows of every chunk in the reference order -- descending score with
    the row index breaking ties, the score being the fp64 one ('fp64') or torch's fp32 softmax ('fp32') -- and the permutation."""
    from oracle import posteval as O
    N = logits.shape[1]
    chunk = -(-N // T)
    s64 = torch.softmax(logits.double(), -1)[..., 0]
    key = s64 if scores == 'fp64' else torch.softmax(logits, -1)[..., 0].double()
    xyxy = torch.clamp(O.box_cxcywh_to_xyxy(boxes), min=0, max=1)
    perm = torch.empty((logits.shape[0], N), dtype=torch.int64)
    for b in range(logits.shape[0]):
        for c0 in range(0, N, chunk):
            k = key[b, c0:c0 + chunk]
            perm[b, c0:c0 + chunk] = c0 + torch.argsort(-k, stable=True)
    ref = torch.cat([xyxy.double(), s64[..., None]], -1)
    return torch.gather(ref, 1, perm[..., None].expand(-1, -1, 5)), perm


def grouped(results):
    """predictions and ground truth per (video, sketch) key, as compute_ap builds them (eval.py:22-50): keys in order of first prediction"""
    preds, gts = {}, {}
    for res in results:
        key = res['video'] + res['sketch']
        for p in res['pred_boxes']:
            preds.setdefault(key, []).append({'frame': res['frame'], 'top-left-x': p[0], 'top-left-y': p[1], 'bot-right-x': p[2],
                                              'bot-right-y': p[3], 'score': p[4]})
        for g in res['gt_boxes']:
            gts.setdefault(key, []).append({'frame': res['frame'], 'top-left-x': g['bbox'][0], 'top-left-y': g['bbox'][1],
                                            'bot-right-x': g['bbox'][2], 'bot-right-y': g['bbox'][3]})
    return preds, {k: gts.get(k, []) for k in preds}


# ---- comparisons shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def null(x):
    """NaN -> None, recursively; numpy scalars -> Python floats (the fixture's encoding)"""
    if isinstance(x, dict):
        return {k: null(v) for k, v in x.items()}
    if isinstance(x, (list, tuple, np.ndarray)):
        return [null(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return None if x != x else float(x)
    return x


def f64(x):
    """a fixture list (None for NaN) or an array -> float64 array"""
    if isinstance(x, np.ndarray):
        return x.astype(np.float64)
    return np.array([[np.nan if v is None else v for v in row] if isinstance(row, list) else (np.nan if row is None else row)
                     for row in x], dtype=np.float64)


def assert_same_bits(got, want, what):
    """float64 bit patterns equal, NaN exactly where the other has NaN"""
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f'{what}: NaN at {np.argwhere(gn != wn)[:4].tolist()} on one side only'
    g, w = np.ascontiguousarray(got[~gn]).view(np.uint64), np.ascontiguousarray(want[~wn]).view(np.uint64)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f'{what}: {bad.size} of {g.size} values differ in bits, first {got[~gn][bad[0]]!r} != {want[~wn][bad[0]]!r}'
