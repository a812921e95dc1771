"""svol_postprocess / svol_eval_ap / svol_eval_max_iou on the MI355X at the edges the synthetic fixtures never reach
(tests/posteval_edge_cases.py; tests/test_posteval_edge_cases.py proves on the CPU that each case reaches its branch):

* post-processing at chunk sizes 1 .. 12288 with ragged last chunks, both launch shapes, more rows than threads: box columns
  bit-equal to the clamped fp32 xyxy of the reference order (no escape clause), scores within 2e-7 of fp64, rows of equal score in
  input order, two runs bit-identical, chunk 12289 refused;
* evaluation: AP arrays and max-IoU vectors bit-equal (float64 patterns, NaN where the reference has NaN) to what the reference
  itself computed (tests/golden/posteval_edges.json) -- AP sums of up to 320 terms (numpy's pairwise recursion, two levels), NaN
  IoUs, IoU and score ties, groups without ground truth, 70 groups, K = 1 and K = 64 thresholds; K = 65 refused;
* every operand, output and workspace carved out of guard arenas under the three fills, the workspaces pre-filled with the fill
  word: nothing outside is touched, no result depends on a workspace word the kernel did not write.
"""
import copy
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import posteval_edge_cases as C
from tests.guard_arena import FILLS, GuardArena, _i32

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, 'golden', 'posteval_edges.json')))
SVOL_E_UNSUPPORTED = -2
K64 = C.K64


def _bits32(t):
    return t.contiguous().view(torch.int32)


# ---- post-processing -------------------------------------------------------------------------------------------------------------
def _check_postprocess(case, logits, boxes, T, got, what):
    """got [B, N, 5] (CPU) against the reference order"""
    ref, perm = C.pp_reference(logits, boxes, T, 'fp32' if case == 'saturated' else 'fp64')
    N = logits.shape[1]
    chunk = -(-N // T)
    assert torch.equal(_bits32(got[..., :4]), _bits32(ref[..., :4].float())), f'{what}: box columns differ from the reference order'
    err = float((got[..., 4].double() - ref[..., 4]).abs().max())
    assert err <= 2e-7, f'{what}: score error {err:.3e}'
    xyxy = ref[..., :4].float()
    n_tied = 0
    for b in range(logits.shape[0]):
        row_of = {tuple(r): int(i) for r, i in zip(xyxy[b].tolist(), perm[b].tolist())}      # clamped box -> input row
        rows = torch.tensor([row_of[tuple(r)] for r in got[b, :, :4].tolist()])
        assert torch.equal(rows, perm[b])
        same = (got[b, 1:, 4] == got[b, :-1, 4]) & (torch.arange(1, N) % chunk != 0)           # neighbours of one chunk, equal score
        assert bool((rows[1:][same] > rows[:-1][same]).all()), f'{what}: rows of equal score left their input order'
        lg = logits[b][rows]
        same_lg = (lg[1:] == lg[:-1]).all(-1) & (torch.arange(1, N) % chunk != 0)
        assert bool((~same_lg | same).all()), f'{what}: equal logits, different scores'
        n_tied += int(same.sum())
    return n_tied


@pytest.mark.parametrize('case,build,chunk', C.PP_CASES, ids=[f'{n}-{c}' for n, _, c in C.PP_CASES])
def test_postprocess_edges(case, build, chunk):
    from svol_amd import postprocess as PP
    logits, boxes, T = build(chunk)
    lg, bx = logits.cuda(), boxes.cuda()
    a = PP.postprocess(lg, bx, T)
    b = PP.postprocess(lg, bx, T)
    torch.cuda.synchronize()
    assert torch.equal(_bits32(a), _bits32(b)), 'two runs differ in bits'
    n_tied = _check_postprocess(case, logits, boxes, T, a.cpu(), f'{case}, chunk {chunk}')
    if chunk > 1:
        assert n_tied > 0


def test_postprocess_last_chunk_of_one_row():
    from svol_amd import postprocess as PP
    logits, boxes, T = C.grid_one_row_tail()
    got = PP.postprocess(logits.cuda(), boxes.cuda(), T).cpu()
    _check_postprocess('grid', logits, boxes, T, got, 'grid, chunk 63, last chunk of one row')


def test_postprocess_refuses_chunks_above_its_limit():
    from svol_amd import _lib, postprocess as PP
    from svol_amd.ops import _ptr, _stream
    n = C.CHUNK_LIMIT + 1
    lg = torch.zeros((1, n, 2), device='cuda')
    bx = torch.zeros((1, n, 4), device='cuda')
    out = torch.full((1, n, 5), 7.0, device='cuda')
    assert _lib.lib().svol_postprocess(_ptr(lg), _ptr(bx), _ptr(out), 1, n, n, _stream()) == SVOL_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'a refused call wrote'
    with pytest.raises(_lib.SvolHipError):
        PP.postprocess(lg, bx, 1)
    assert _lib.lib().svol_postprocess(_ptr(lg), _ptr(bx), _ptr(out), 1, n, C.CHUNK_LIMIT, _stream()) == 0      # the limit itself runs
    torch.cuda.synchronize()


# ---- evaluation ------------------------------------------------------------------------------------------------------------------
def _raises_like(fx_entry, fn):
    with pytest.raises(Exception) as e:
        fn()
    assert type(e.value).__name__ == fx_entry['raises']


@pytest.mark.parametrize('name', list(C.RECORD_SETS))
def test_eval_edges_bit_exact_vs_reference(name):
    from svol_amd.evaluate import eval as E
    build, ks = C.RECORD_SETS[name]
    results, fx = build(), FX[name]
    pk = E._Packed(results)
    assert pk.groups == fx['groups']
    C.assert_same_bits(E._ap_arrays(pk, C.AP_THDS), fx['ap'], f'{name}: AP')
    for k in ks:
        want = fx['max_ious'][str(k)]
        if isinstance(want, dict):
            _raises_like(want, lambda: E._max_ious(pk, k))
        else:
            C.assert_same_bits(E._max_ious(pk, k), want, f'{name}: max IoU, k={k}')
    if 'raises' in fx['metrics']:
        _raises_like(fx['metrics'], lambda: E.eval_results(copy.deepcopy(results), verbose=False))
    else:
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')        # means over NaN / over nothing, as in the reference
            got = E.eval_results(copy.deepcopy(results), verbose=False)
        assert C.null(json.loads(json.dumps(got))) == fx['metrics']
        assert list(got.keys()) == list(fx['metrics'].keys()) and list(got['brief'].keys()) == list(fx['metrics']['brief'].keys())


@pytest.mark.parametrize('name', C.K64_SETS)
def test_eval_ap_at_1_and_64_thresholds(name):
    from oracle import posteval as O
    from svol_amd import _lib
    from svol_amd.evaluate import eval as E
    results = C.RECORD_SETS[name][0]()
    pk = E._Packed(results)
    for thds in ([0.5], K64):
        preds, gts = C.grouped(results)
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            want = np.array([O.compute_average_precision_detection(gts[k], preds[k], iou_thresholds=thds) for k in preds])
        C.assert_same_bits(E._ap_arrays(pk, thds), want, f'{name}: AP at {len(thds)} thresholds')
    with pytest.raises(_lib.SvolHipError, match=r'code -2'):
        E._ap_arrays(pk, K64 + [0.99])


def test_ground_truth_without_predictions_raises_as_the_oracle_does():
    from oracle import posteval as O
    from svol_amd.evaluate import eval as E
    results = C.no_gt_group()
    with pytest.raises(Exception) as want:
        O.compute_recall_at_k(results, k=1)
    with pytest.raises(Exception) as got:
        E._max_ious(E._Packed(results), 1)
    assert type(got.value) is type(want.value) is IndexError and str(got.value) == str(want.value)


# ---- guards ----------------------------------------------------------------------------------------------------------------------
def _fill_words(t, word):
    """the fill word's bytes over every byte of a dense slot"""
    raw = t.view(-1).view(torch.uint8)
    pat = torch.tensor([_i32(word)], dtype=torch.int32).view(torch.uint8)
    raw.copy_(pat.repeat((raw.numel() + 3) // 4)[:raw.numel()])


def _arena(slots):
    ar = GuardArena()
    for name, a in slots.items():
        ar.plan(name, tuple(a.shape), a.dtype)
    return ar, ar.build()


@pytest.mark.parametrize('name', ['many_groups', 'many_positives'])
def test_eval_kernels_stay_inside_their_operands(name):
    """svol_eval_ap with its outputs and all three workspaces, svol_eval_max_iou with its output, every operand: slots of two arenas"""
    from svol_amd import _lib
    from svol_amd.evaluate import eval as E
    from svol_amd.ops import _ptr, _stream
    L = _lib.lib()
    results, fx = C.RECORD_SETS[name][0](), FX[name]
    pk = E._Packed(results)
    K, NG, P, G, GT = len(C.AP_THDS), len(pk.groups), len(pk.ap_pred), len(pk.ap_gt), len(pk.gt)
    assert NG == len(fx['groups']) and P > 0 and G > 0 and GT > 0
    host = {
        'box': pk.ap_pred[:, :4], 'score': pk.ap_pred[:, 4], 'pf': pk.ap_pred_frame, 'po': pk.ap_pred_off, 'gt': pk.ap_gt,
        'gf': pk.ap_gt_frame, 'go': pk.ap_gt_off, 'thr': np.asarray(C.AP_THDS, dtype=np.float64),
        'mi_pred': pk.pred[:, :4], 'mi_po': pk.pred_off, 'mi_gt': pk.gt, 'mi_go': pk.gt_off, 'mi_rec': pk.gt_rec,
    }
    host = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in host.items()}
    assert {v.dtype for v in host.values()} == {torch.float64, torch.int32}
    ain, tin = _arena(host)
    for k, v in host.items():
        tin[k].copy_(v)
    e = torch.empty
    ws = {'ws_order': e((max(P, 1),), dtype=torch.int32), 'ws_u8': e((K * (P + G),), dtype=torch.uint8),
          'ws_f64': e((2 * K * (P + 2 * NG),), dtype=torch.float64)}
    outs = {'ap': e((NG, K), dtype=torch.float64), 'mi1': e((GT,), dtype=torch.float64), 'mi5': e((GT,), dtype=torch.float64)}
    aout, tout = _arena({**ws, **outs})
    first = {}
    for fill_name, word in FILLS:
        what = f'{name} [{fill_name}]'
        ain.refill(word)
        aout.refill(word)
        for k in ws:
            _fill_words(tout[k], word)           # a workspace word read before it is written would change the result with the fill
        for k in outs:
            tout[k].fill_(float('nan'))          # an output the call must write: poisoned
        t = tin
        rc = L.svol_eval_ap(_ptr(t['box']), _ptr(t['score']), _ptr(t['pf']), _ptr(t['po']), _ptr(t['gt']), _ptr(t['gf']), _ptr(t['go']),
                            _ptr(t['thr']), K, _ptr(tout['ws_order']), _ptr(tout['ws_u8']), _ptr(tout['ws_f64']), _ptr(tout['ap']), P, G, NG,
                            _stream())
        assert rc == 0, f'{what}: svol_eval_ap returned {rc}'
        for k, slot in ((1, 'mi1'), (5, 'mi5')):
            rc = L.svol_eval_max_iou(_ptr(t['mi_pred']), _ptr(t['mi_po']), _ptr(t['mi_gt']), _ptr(t['mi_go']), _ptr(t['mi_rec']),
                                     _ptr(tout[slot]), GT, k, _stream())
            assert rc == 0, f'{what}: svol_eval_max_iou returned {rc}'
        torch.cuda.synchronize()
        ain.check(what + ', input arena')
        aout.check(what + ', output arena')
        for k, v in host.items():
            assert torch.equal(tin[k].cpu(), v), f'{what}: input {k} was written'
        C.assert_same_bits(tout['ap'].cpu().numpy(), fx['ap'], f'{what}: AP')
        C.assert_same_bits(tout['mi1'].cpu().numpy(), fx['max_ious']['1'], f'{what}: max IoU, k=1')
        C.assert_same_bits(tout['mi5'].cpu().numpy(), fx['max_ious']['5'], f'{what}: max IoU, k=5')
        for k in outs:
            bits = tout[k].cpu().view(torch.int64).clone()
            assert torch.equal(first.setdefault(k, bits), bits), f'{what}: output {k} differs in bits from the first fill'


def test_postprocess_stays_inside_its_operands():
    """chunk 257: the 256-thread shape with more rows than threads, a ragged last chunk"""
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    logits, boxes, T = C.ties_inside_chunks(257)
    Bn, N = logits.shape[:2]
    chunk = -(-N // T)
    ain, tin = _arena({'logits': logits, 'boxes': boxes})
    tin['logits'].copy_(logits)
    tin['boxes'].copy_(boxes)
    aout, tout = _arena({'out': torch.empty((Bn, N, 5), dtype=torch.float32)})
    first = None
    for fill_name, word in FILLS:
        what = f'svol_postprocess [{fill_name}]'
        ain.refill(word)
        aout.refill(word)
        tout['out'].fill_(float('nan'))
        rc = _lib.lib().svol_postprocess(_ptr(tin['logits']), _ptr(tin['boxes']), _ptr(tout['out']), Bn, N, chunk, _stream())
        torch.cuda.synchronize()
        assert rc == 0, f'{what}: return code {rc}'
        ain.check(what + ', input arena')
        aout.check(what + ', output arena')
        assert torch.equal(tin['logits'].cpu(), logits) and torch.equal(tin['boxes'].cpu(), boxes), f'{what}: an input was written'
        got = tout['out'].cpu()
        _check_postprocess('ties_inside_chunks', logits, boxes, T, got, what)
        first = got if first is None else first
        assert torch.equal(_bits32(first), _bits32(got)), f'{what}: output differs in bits from the first fill'
