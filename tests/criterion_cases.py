"""Case tables and fp64 references for the matcher / criterion kernels (csrc/criterion.hip): CPU only.

Everything here is numpy / torch on the host plus ``oracle.svol_oracle`` and scipy.  tests/test_criterion_cases.py checks the
tables against themselves on the CPU, tests/test_gpu_criterion.py feeds them to the kernels through the C ABI.

Geometry classes.  Every class pair (prediction, target) is DYADIC: box edges are whole multiples of 2^-6 in [0, 1] and widths
are even multiples, so cx, cy, w, h, cx -+ w/2 and every difference the GIoU forms are exact in fp32 and in fp64 alike — the
kernel and the reference take the same side of every comparison, and sit on the same tie, by construction.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import svol_oracle as O

U = 2.0 ** -6
NUDGE = 2.0 ** -20


def _bx(x0, y0, x1, y1, s=1, dx=0, dy=0):
    """cxcywh of the box with edges (x0, y0, x1, y1) * s + (dx, dy), in units of 2^-6."""
    x0, x1 = x0 * s + dx, x1 * s + dx
    y0, y1 = y0 * s + dy, y1 * s + dy
    assert 0 <= x0 <= x1 <= 64 and 0 <= y0 <= y1 <= 64 and (x1 - x0) % 2 == 0 and (y1 - y0) % 2 == 0
    return ((x0 + x1) // 2 * U, (y0 + y1) // 2 * U, (x1 - x0) * U, (y1 - y0) * U)


VARIANTS = [(1, 0, 0), (1, 9, 5), (2, 0, 0), (2, 3, 1)]   # (scale, shift x, shift y) of a template: four pairs per template
_T = (6, 6, 20, 20)                                       # the target most templates share

# name -> (templates [(pred edges, target edges)], predicate over the xyxy edges, cxcywh coordinate to nudge off the tie or None)
# predicate arguments: p = (x0, y0, x1, y1) of the prediction, t = the same of the target, b / g = their cxcywh
_CLASS_DEFS = {
    'generic': ([((4, 6, 14, 14), (8, 10, 20, 20))],
                lambda p, t, b, g: p[0] < t[0] < p[2] < t[2] and p[1] < t[1] < p[3] < t[3], None),
    'disjoint_x': ([((2, 6, 8, 16), (12, 8, 20, 20))],
                   lambda p, t, b, g: p[2] < t[0] and p[3] > t[1] and t[3] > p[1], None),
    'disjoint_y': ([((6, 2, 16, 8), (8, 12, 20, 20))],
                   lambda p, t, b, g: p[3] < t[1] and p[2] > t[0] and t[2] > p[0], None),
    'disjoint_both': ([((2, 2, 8, 6), (12, 10, 20, 20))],
                      lambda p, t, b, g: p[2] < t[0] and p[3] < t[1], None),
    'pred_inside': ([((10, 10, 18, 14), _T)],
                    lambda p, t, b, g: p[0] > t[0] and p[2] < t[2] and p[1] > t[1] and p[3] < t[3], None),
    'tgt_inside': ([(_T, (10, 10, 18, 14))],
                   lambda p, t, b, g: t[0] > p[0] and t[2] < p[2] and t[1] > p[1] and t[3] < p[3], None),
    'identical': ([((6, 8, 20, 18), (6, 8, 20, 18))],
                  lambda p, t, b, g: p[0] == t[0] and p[1] == t[1] and p[2] == t[2] and p[3] == t[3], 0),
    'shared_edge_x0': ([((6, 10, 14, 18), _T)],
                       lambda p, t, b, g: p[0] == t[0] and p[2] < t[2] and p[1] > t[1] and p[3] < t[3], 0),
    'shared_edge_x1': ([((12, 10, 20, 18), _T)],
                       lambda p, t, b, g: p[2] == t[2] and p[0] > t[0] and p[1] > t[1] and p[3] < t[3], 0),
    'shared_edge_y1': ([((10, 12, 18, 20), _T)],
                       lambda p, t, b, g: p[3] == t[3] and p[1] > t[1] and p[0] > t[0] and p[2] < t[2], 1),
    'shared_edge_partial': ([((6, 2, 14, 12), _T)],
                            lambda p, t, b, g: p[0] == t[0] and p[2] < t[2] and p[1] < t[1] < p[3] < t[3], 0),
    'touch_x': ([((0, 8, 6, 16), _T)],
                lambda p, t, b, g: p[2] == t[0] and p[1] > t[1] and p[3] < t[3], 0),
    'touch_corner': ([((0, 0, 6, 6), _T)],
                     lambda p, t, b, g: p[2] == t[0] and p[3] == t[1], None),
    'same_centre_crossed': ([((10, 4, 16, 22), (6, 8, 20, 18))],
                            lambda p, t, b, g: b[0] == g[0] and b[1] == g[1] and p[0] > t[0] and p[2] < t[2]
                            and p[1] < t[1] and p[3] > t[3], 0),
    'zero_w_overlap': ([((12, 8, 12, 16), _T)],
                       lambda p, t, b, g: p[0] == p[2] and t[0] < p[0] < t[2] and p[1] > t[1] and p[3] < t[3], None),
    'zero_w_edge': ([((6, 8, 6, 16), _T)],
                    lambda p, t, b, g: p[0] == p[2] == t[0] and p[1] > t[1] and p[3] < t[3], 0),
    'zero_area_disjoint': ([((2, 8, 2, 16), _T), ((2, 2, 2, 2), _T)],
                           lambda p, t, b, g: (p[2] - p[0]) * (p[3] - p[1]) == 0 and p[2] < t[0], None),
    'l1_tie_cx': ([((8, 4, 18, 12), _T)], lambda p, t, b, g: b[0] == g[0] and b[1] != g[1] and b[2] != g[2] and b[3] != g[3], 0),
    'l1_tie_cy': ([((4, 8, 12, 18), _T)], lambda p, t, b, g: b[1] == g[1] and b[0] != g[0] and b[2] != g[2] and b[3] != g[3], 1),
    'l1_tie_w': ([((2, 4, 16, 12), _T)], lambda p, t, b, g: b[2] == g[2] and b[0] != g[0] and b[1] != g[1] and b[3] != g[3], 2),
    'l1_tie_h': ([((4, 2, 12, 16), _T)], lambda p, t, b, g: b[3] == g[3] and b[0] != g[0] and b[1] != g[1] and b[2] != g[2], 3),
}
# touch_corner sits on two clamp boundaries at once, but the gradient is CONTINUOUS there (iw = ih = 0 on the tie, so either clamp's
# share is multiplied by the other's zero): there is no wrong side to pick, and the class has no nudge.  It still pins the values.
# classes whose giou / L1 gradient is exactly zero in exact arithmetic: absolute bar (1e-6 / K), there is no scale to be relative to
ZERO_GRAD_CLASSES = ('identical',)


def _build_classes():
    out = {}
    for name, (templates, pred, nudge) in _CLASS_DEFS.items():
        pairs = []
        for pe, te in templates:
            for s, dx, dy in VARIANTS:
                pairs.append((_bx(*pe, s=s, dx=dx, dy=dy), _bx(*te, s=s, dx=dx, dy=dy)))
        out[name] = SimpleNamespace(name=name, pairs=pairs, predicate=pred, nudge=nudge)
    return out


CLASSES = _build_classes()
TIE_CLASSES = [n for n, c in CLASSES.items() if c.nudge is not None]
N_RANDOM = 40


def _random_boxes(rng, n):
    return np.concatenate([rng.uniform(0.2, 0.8, size=(n, 2)), rng.uniform(0.05, 0.4, size=(n, 2))], -1).astype(np.float32)


def all_pairs():
    """[(class name, pred cxcywh float32[4], target cxcywh float32[4])]: every class pair, then the 40 random non-dyadic ones."""
    out = []
    for name, c in CLASSES.items():
        for b, t in c.pairs:
            out.append((name, np.asarray(b, np.float32), np.asarray(t, np.float32)))
    rng = np.random.RandomState(11)
    pb, tb = _random_boxes(rng, N_RANDOM), _random_boxes(rng, N_RANDOM)
    for i in range(N_RANDOM):
        out.append(('random', pb[i], tb[i]))
    return out


def edges(box, dtype):
    """(x0, y0, x1, y1) of a cxcywh box in `dtype` arithmetic, as box_utils.py:9-13 forms them."""
    b = np.asarray(box).astype(dtype)
    h = dtype(0.5)
    return (b[0] - h * b[2], b[1] - h * b[3], b[0] + h * b[2], b[1] + h * b[3])


def predicate_holds(cls, b, t, dtype):
    bb, tt = np.asarray(b).astype(dtype), np.asarray(t).astype(dtype)
    return bool(cls.predicate(edges(bb, dtype), edges(tt, dtype), bb, tt))


# ---------------------------------------------------------------------------
# references: oracle/svol_oracle.py on float64 (or float32) tensors with autograd
def cost_block_reference(logits, boxes, tgt, w_bbox, w_giou, w_class, dtype=torch.float64):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return O.cost_matrix_block(f(logits), f(boxes), f(tgt), w_bbox, w_giou, w_class).numpy()


def set_loss_reference(logits, boxes, tgt, match, eos, dtype=torch.float64, videos=None):
    """One layer of svol_set_loss from the oracle: logits [R,2], boxes [R,4], tgt [M,4], match [R] (-1, or the tgt row the LOSS
    uses for that prediction row).  `videos`: [(first tgt row, number of tgt rows)] of equally many prediction rows each (default:
    one video holding everything) — the reference indexes each video's own box list with video-local ids (loss.py:87).
    Returns (losses[4] = label, bbox, giou, class_error; g_label [R,2]; g_bbox [R,4]; g_giou [R,4]) as float64 numpy arrays.
    No matched row at all: the reference cannot express it (torch.stack([]) raises); this build defines loss_bbox = loss_giou =
    class_error = 0 with zero box gradients, and the label loss is the all-background cross-entropy, written out here."""
    R = logits.shape[0]
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(dtype).requires_grad_(True)
    bx = torch.from_numpy(np.ascontiguousarray(boxes)).to(dtype).requires_grad_(True)
    match = np.asarray(match)
    if not (match >= 0).any():
        nll = -torch.log_softmax(lg, -1)[:, 1] * eos
        ll = nll.mean()
        gl, = torch.autograd.grad(ll, lg)
        z = np.zeros((R, 4))
        return np.array([float(ll.detach()), 0.0, 0.0, 0.0]), gl.double().numpy(), z, z.copy()
    videos = videos or [(0, tgt.shape[0])]
    B = len(videos)
    N = R // B
    targets, idx = [], []
    for b, (lo, n) in enumerate(videos):
        targets.append({'bboxes': {0: [{'bbox': torch.from_numpy(np.ascontiguousarray(tgt[lo + j]))} for j in range(n)]}})
        m = match[b * N:(b + 1) * N]
        rows = np.nonzero(m >= 0)[0]
        idx.append((rows, m[rows] - lo))
    ld = O.set_criterion(SimpleNamespace(eos_coef=eos), {'pred_logits': lg.view(B, N, 2), 'pred_boxes': bx.view(B, N, 4)}, targets,
                         indices=[idx])
    gl, = torch.autograd.grad(ld['loss_label'], lg)
    gb, = torch.autograd.grad(ld['loss_bbox'], bx, retain_graph=True)
    gg, = torch.autograd.grad(ld['loss_giou'], bx)
    losses = np.array([float(ld[k].detach()) for k in ('loss_label', 'loss_bbox', 'loss_giou', 'class_error')])
    return losses, gl.double().numpy(), gb.double().numpy(), gg.double().numpy()


def pair_gradients(b, t, dtype=torch.float64):
    """(d L1 / d b, d (1 - giou) / d b) of ONE pair, float64 numpy [4] each: loss_boxes with K = 1."""
    _, _, gb, gg = set_loss_reference(np.zeros((1, 2)), np.asarray(b, np.float64)[None], np.asarray(t, np.float64)[None],
                                      np.array([0]), 0.1, dtype)
    return gb[0], gg[0]


# ---------------------------------------------------------------------------
# svol_set_loss layouts
def set_loss_layout(R, seed=0):
    """Three layers of R prediction rows over ONE target table (row i = the target of pair i of all_pairs()):
    layer 0 matches as many pairs as fit (all of them from R = 104 up) on scattered rows, layer 1 a different subset on
    different rows (so K and every row's role differ between the layers), layer 2 matches nothing.
    Returns logits [3,R,2], boxes [3,R,4], tgt [M,4] float32, match [3,R] int32, cls [3][R] (class name | 'background')."""
    pairs = all_pairs()
    rng = np.random.RandomState(100 + seed)
    tgt = np.stack([t for _, _, t in pairs]).astype(np.float32)
    logits = (rng.standard_normal((3, R, 2)) * 2).astype(np.float32)
    boxes = np.stack([_random_boxes(rng, R) for _ in range(3)])
    match = np.full((3, R), -1, np.int32)
    cls = [['background'] * R for _ in range(3)]
    if R >= len(pairs):
        chosen = [list(range(len(pairs))), list(range(1, len(pairs), 2))]
    else:   # a handful: one tie, one clamp boundary, one zero gradient, one plain, one random
        names = [n for n, _, _ in pairs]
        pick = [names.index(n) for n in ('touch_x', 'identical', 'generic', 'zero_w_edge', 'random', 'shared_edge_x0', 'pred_inside')]
        assert R >= 5
        chosen = [pick[:5], pick[3:7]]
    for layer, ids in enumerate(chosen):
        rows = np.sort(rng.permutation(R)[:len(ids)]) if layer == 0 else rng.permutation(R)[:len(ids)]
        if R > 256 and layer == 0:
            rows[-1] = R - 1   # a matched row in the tail of the 256-thread loop
            rows = np.unique(rows)
            ids = ids[:len(rows)]
        for r, i in zip(rows, ids):
            match[layer, r] = i
            boxes[layer, r] = pairs[i][1]
            cls[layer][r] = pairs[i][0]
    # logits: a matched row with l0 == l1 (counts as correct, by >=), saturated pairs on a matched random row and on background rows
    m0 = np.nonzero(match[0] >= 0)[0]
    logits[0, m0[0]] = (0.75, 0.75)
    logits[1, np.nonzero(match[1] >= 0)[0][0]] = (-1.5, -1.5)
    rnd = [r for r in m0 if cls[0][r] == 'random']
    if len(rnd) >= 2:
        logits[0, rnd[0]] = (80.0, -80.0)
        logits[0, rnd[1]] = (-80.0, 80.0)
    bg = np.nonzero(match[0] < 0)[0]
    if len(bg) >= 2:
        logits[0, bg[0]] = (80.0, -80.0)
        logits[0, bg[1]] = (-80.0, 80.0)
    logits[2, 0] = (80.0, -80.0)
    logits[2, R - 1] = (-80.0, 80.0)
    logits[2, R // 2] = (0.5, 0.5)
    return logits, boxes, tgt, match, cls


def rebase_layout():
    """PerFrameMatcher's re-basing (matcher.py:114-115 + loss.py:87), 3 videos x 100 rows, one layer.  `match` holds what the LSAP
    leaves (global target rows); the loss target of match m in video b is row vid_off[b] + (m - smallest matched m of the video).
    Video 0's first box is matched (re-basing is the identity), video 1's first TWO boxes are unmatched (every loss target moves),
    video 2 has boxes and no match.  Returns logits, boxes, tgt, match (device), loss_match (the rows the loss uses), vid_off,
    videos [(first row, count)], cls."""
    pairs = all_pairs()
    rng = np.random.RandomState(7)
    N, counts = 100, (12, 14, 5)
    vid_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    tgt = _random_boxes(rng, sum(counts))
    logits = (rng.standard_normal((300, 2)) * 2).astype(np.float32)
    boxes = _random_boxes(rng, 300)
    match = np.full(300, -1, np.int32)
    loss_match = match.copy()
    cls = ['background'] * 300
    names = [n for n, _, _ in pairs]
    plan = {0: ([0, 3, 4, 7, 11], ['generic', 'random', 'touch_x', 'identical', 'random']),
            1: ([2, 3, 5, 9, 13], ['shared_edge_x0', 'random', 'zero_w_edge', 'random', 'disjoint_x'])}
    used = set()
    for b, (ids, kinds) in plan.items():
        rows = b * N + rng.permutation(N)[:len(ids)]
        for r, m, kind in zip(rows, ids, kinds):
            i = next(k for k in range(len(pairs)) if names[k] == kind and k not in used)
            used.add(i)
            lt = int(vid_off[b]) + (m - min(ids))
            match[r], loss_match[r] = vid_off[b] + m, lt
            boxes[r], tgt[lt], cls[r] = pairs[i][1], pairs[i][2], kind
    videos = [(int(vid_off[b]), counts[b]) for b in range(3)]
    return logits, boxes, tgt, match, loss_match, vid_off, videos, cls


# ---------------------------------------------------------------------------
# svol_match_cost: one launch, two layers of eight problems
COST_SHAPES = [(3, 2), (1, 1), (5, 0), (37, 9), (16, 16), (4, 40), (2, 3), (6, 0)]   # (np, nt) per layer; 37 x 9 = 333 = 256 + a tail
COST_WEIGHTS = [(5.0, 1.0, 2.0), (1.0, 2.0, 0.5)]                                      # (w_bbox, w_giou, w_class)
COST_BAD = {3: 'pred_w', 5: 'tgt_h', 6: 'nan'}                                          # problem -> the fault of the flagged launch


def match_cost_problem_set(bad=False):
    """Problem tables as PackedTargets lays them out for two layers (layer-major; prediction rows of layer l start at l * R), except
    that each layer owns a COPY of the target table — so that a fault planted in one problem's boxes is that problem's alone.
    Boxes: the class predictions / targets (every cross pair is then some tie or boundary geometry; all targets are proper boxes, so
    every cost is finite) and random ones; logits include (+-80, -+80) and equal pairs.  bad=True plants COST_BAD."""
    pairs = all_pairs()
    rng = np.random.RandomState(3)
    P1 = len(COST_SHAPES)
    R, M = sum(s[0] for s in COST_SHAPES), sum(s[1] for s in COST_SHAPES)
    p_off = np.concatenate([[0], np.cumsum([s[0] for s in COST_SHAPES])[:-1]])
    t_off = np.concatenate([[0], np.cumsum([s[1] for s in COST_SHAPES])[:-1]])
    pred_off = np.concatenate([p_off, p_off + R]).astype(np.int32)
    tgt_off = np.concatenate([t_off, t_off + M]).astype(np.int32)
    pred_cnt = np.tile([s[0] for s in COST_SHAPES], 2).astype(np.int32)
    tgt_cnt = np.tile([s[1] for s in COST_SHAPES], 2).astype(np.int32)
    cost_off = np.concatenate([[0], np.cumsum(pred_cnt.astype(np.int64) * tgt_cnt)[:-1]]).astype(np.int64)
    dy = [p for p in pairs if p[0] != 'random']
    boxes = _random_boxes(rng, 2 * R)
    tgt1 = _random_boxes(rng, M)
    for layer in range(2):
        k = 17 * layer
        for q in (0, 3, 4):   # 3x2, 37x9, 16x16: class boxes
            for i in range(COST_SHAPES[q][0]):
                boxes[layer * R + p_off[q] + i] = dy[(k + i * 4) % len(dy)][1] if q == 4 else dy[(k + i) % len(dy)][1]
            k += 37
    for q in (0, 3, 4):
        for j in range(COST_SHAPES[q][1]):
            tgt1[t_off[q] + j] = dy[(j * 4) % len(dy)][2] if q == 4 else dy[(j * 9 + q) % len(dy)][2]
    tgt = np.concatenate([tgt1, tgt1])
    logits = (rng.standard_normal((2 * R, 2)) * 2).astype(np.float32)
    logits[0], logits[1], logits[2] = (80.0, -80.0), (-80.0, 80.0), (1.25, 1.25)
    logits[p_off[3] + 5], logits[p_off[3] + 300 // 9], logits[R + p_off[4] + 15] = (-80.0, 80.0), (80.0, -80.0), (0.0, 0.0)
    if bad:
        boxes[pred_off[3] + 36, 2] = -U                      # a prediction with w = -2^-6, the last row of the 37 x 9 block
        tgt[tgt_off[5] + 39, 3] = -tgt[tgt_off[5] + 39, 3]   # a target with h < 0
        boxes[pred_off[6] + 1, 1] = np.nan                   # one NaN coordinate
    return SimpleNamespace(logits=logits, boxes=boxes, tgt=tgt, pred_off=pred_off, pred_cnt=pred_cnt, tgt_off=tgt_off, tgt_cnt=tgt_cnt,
                           cost_off=cost_off, n=2 * P1, numel=int((pred_cnt.astype(np.int64) * tgt_cnt).sum()))


def expected_box_status(ps):
    """generalized_box_iou's early check (box_utils.py:51-52) per problem, in fp32 numpy: 1 where any box fails x1 >= x0, y1 >= y0."""
    out = np.zeros(ps.n, np.int32)
    for p in range(ps.n):
        for arr, off, cnt in ((ps.boxes, ps.pred_off[p], ps.pred_cnt[p]), (ps.tgt, ps.tgt_off[p], ps.tgt_cnt[p])):
            b = arr[off:off + cnt].astype(np.float32)
            h = np.float32(0.5)
            ok = (b[:, 0] + h * b[:, 2] >= b[:, 0] - h * b[:, 2]) & (b[:, 1] + h * b[:, 3] >= b[:, 1] - h * b[:, 3])
            out[p] |= int(not ok.all())
    return out


# ---------------------------------------------------------------------------
# svol_lsap_batched: which (np, nt) reach which solver path at max_dim = 130
#
#   md = max_dim rounded up to 16 = 144; solver arrays = md * (3*8 + 4*4 + 2) = 6048 bytes; pad = 512 bytes.
#   A max_dim x max_dim block would need 130 * 130 * 4 = 67600 bytes: with the arrays that is over the 64 KiB of LDS, so the staging
#   area is capped at (65536 - 6048 - 512) rounded down to 16 = 58976 bytes = 14744 floats.
#   staged   <=> np * nt <= 14744;   after the transpose of a tall block nr = min(np, nt), nc = max(np, nt);
#   register-resident path  <=> staged and nr <= 64 and nc <= 128:   40 x 100 (4000 floats), and tall 100 x 40
#   staged LDS path         <=> staged and (nr > 64 or nc > 128):     70 x 130 (9100 floats, nr = 70), and tall 130 x 70
#   unstaged (global) path  <=> np * nt > 14744:                      120 x 130 (15600 floats), and tall 130 x 120
#   (the unstaged path exists only from max_dim = 123 up — below that a max_dim^2 block always fits — so these are about the
#   smallest blocks that reach it.)
LSAP_MAX_DIM = 130
LSAP_STAGE_FLOATS = 14744
LSAP_SHAPES = [('reg', 40, 100), ('reg', 100, 40), ('lds', 70, 130), ('lds', 130, 70), ('global', 120, 130), ('global', 130, 120)]
LSAP_KINDS = ('finite', 'inf_feasible', 'inf_line', 'inf_row_tall', 'nan', 'neg_inf')


def lsap_path(np_, nt, max_dim=LSAP_MAX_DIM):
    """The path svol_lsap_batched's sizing sends an np x nt block down, restated from its launcher."""
    md = max(16, (max_dim + 15) // 16 * 16)
    base, pad = md * (3 * 8 + 4 * 4 + 2), 512
    stage = max_dim * max_dim * 4
    if base + stage + pad > 65536:
        stage = (65536 - base - pad) // 16 * 16 if base + pad < 65536 else 0
    if np_ * nt > stage // 4:
        return 'global'
    nr, nc = min(np_, nt), max(np_, nt)
    return 'reg' if nr <= 64 and nc <= 128 else 'lds'


def lsap_cost(np_, nt, kind, seed):
    """float32 [np, nt] cost block and the status scipy's answer maps to (0 solved, 1 invalid entries, 2 infeasible).
    inf_feasible: ~10 % of the entries +inf around a planted finite perfect matching, rows and columns then permuted.
    inf_line: the short side's line all +inf (a row of a wide block, a column of a tall one): infeasible.
    inf_row_tall: a ROW of a tall block all +inf — that prediction simply stays unmatched: feasible."""
    rng = np.random.RandomState(seed)
    c = rng.random_sample((np_, nt)).astype(np.float32)
    k = min(np_, nt)
    if kind == 'inf_feasible':
        mask = rng.random_sample((np_, nt)) < 0.10
        mask[np.arange(k), np.arange(k)] = False
        c[mask] = np.inf
        c = c[rng.permutation(np_)][:, rng.permutation(nt)]
    elif kind == 'inf_line':
        if np_ <= nt:
            c[rng.randint(np_), :] = np.inf
        else:
            c[:, rng.randint(nt)] = np.inf
        return np.ascontiguousarray(c), 2
    elif kind == 'inf_row_tall':
        assert np_ > nt
        c[rng.randint(np_), :] = np.inf
    elif kind == 'nan':
        c[rng.randint(np_), rng.randint(nt)] = np.nan
        return c, 1
    elif kind == 'neg_inf':
        c[rng.randint(np_), rng.randint(nt)] = -np.inf
        return c, 1
    else:
        assert kind == 'finite'
    return np.ascontiguousarray(c), 0


def lsap_launches():
    """[(launch name, [(label, cost, expected status)])]: the finite controls and the +inf blocks in one launch; then one launch per
    kind of flagged problem, each flagged block with a healthy block of the same path next to it."""
    healthy, launches = [], []
    for i, (path, a, b) in enumerate(LSAP_SHAPES):
        for kind in ('finite', 'inf_feasible') + (('inf_row_tall',) if a > b else ()):
            c, st = lsap_cost(a, b, kind, 1000 + 10 * i + len(kind))
            healthy.append((f'{path}/{a}x{b}/{kind}', c, st))
    launches.append(('healthy', healthy))
    for kind in ('inf_line', 'nan', 'neg_inf'):
        probs = []
        for i, (path, a, b) in enumerate(LSAP_SHAPES):
            c, st = lsap_cost(a, b, kind, 2000 + 10 * i + len(kind))
            probs.append((f'{path}/{a}x{b}/{kind}', c, st))
            c, st = lsap_cost(a, b, 'inf_feasible' if i % 2 else 'finite', 3000 + 10 * i + len(kind))
            probs.append((f'{path}/{a}x{b}/beside_{kind}', c, st))
        launches.append((kind, probs))
    return launches


def scipy_status(cost):
    """(status, rows, cols) of scipy.optimize.linear_sum_assignment on the block."""
    from scipy.optimize import linear_sum_assignment
    try:
        r, c = linear_sum_assignment(cost)
        return 0, r, c
    except ValueError as e:
        if 'invalid numeric entries' in str(e):
            return 1, None, None
        if 'infeasible' in str(e):
            return 2, None, None
        raise


# ---------------------------------------------------------------------------
# the per-class metric and its bars (shared by the CPU self-check and the GPU tests)
DYADIC_BAR = 1e-5      # ~30 fp32 operations without cancellation at dyadic coordinates
ZERO_GRAD_ABS = 1e-6   # / K: classes whose fp64 gradient is exactly zero have no scale to be relative to
RANDOM_FLOOR = 1e-5
RANDOM_MARGIN = 4.0    # x the fp32 oracle's own error against fp64 on the same rows
LOSS_BAR = 1e-5        # of max(1, |v|): the project's bar on losses


def class_rows(cls_layer):
    out = {}
    for r, c in enumerate(cls_layer):
        out.setdefault(c, []).append(r)
    return out


def per_class_errors(got, ref, cls_layer):
    """{class: (max |got - ref| over the class's rows, max |ref| over the same rows)}; a non-finite `got` counts as inf."""
    out = {}
    for c, rows in class_rows(cls_layer).items():
        g, r = np.asarray(got, np.float64)[rows], np.asarray(ref, np.float64)[rows]
        out[c] = (float(np.abs(g - r).max()) if np.isfinite(g).all() else float('inf'), float(np.abs(r).max()))
    return out


def grad_bar(cname, ref_max, K, fp32_err=None):
    """Absolute bar on max |got - ref| over one class's rows of one gradient array."""
    if ref_max < 1e-12:
        return ZERO_GRAD_ABS / max(K, 1)
    if cname == 'random':
        return max(RANDOM_FLOOR * ref_max, RANDOM_MARGIN * fp32_err)
    return DYADIC_BAR * ref_max
