#!/usr/bin/env python3
"""Golden fixture for the evaluation edge cases (tests/posteval_edge_cases.py), generated FROM THE REFERENCE.

Runs only where the reference is present.  Imports the reference's ``lib.evaluate.eval`` / ``lib.evaluate.utils`` behind the same
torchvision stub as make_golden_posteval.py and stores DATA ONLY, per record set of ``posteval_edge_cases.RECORD_SETS``:

* ``groups`` / ``ap``: the (video, sketch) keys in the order ``compute_ap`` creates them and the AP array
  ``compute_average_precision_detection`` returns for each;
* ``max_ious``: per k, the per-box max-IoU vector obtained by running ``compute_iou_batch_cross`` exactly as
  ``compute_recall_at_k`` does;
* ``metrics``: the dictionary ``eval_results`` returns.

NaN is stored as ``null``.  Where the reference raises (a record with ground truth and no predictions), the entry is
``{"raises": "<exception class>"}``.  The records themselves are NOT stored: the tests regenerate them.

    SVOL_REFERENCE=<checkout of the reference> python tests/golden/make_golden_posteval_edges.py
"""
import copy
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = os.environ.get('SVOL_REFERENCE') or sys.exit('SVOL_REFERENCE must name a checkout of the reference')
sys.path.insert(0, REF)
_tv = types.ModuleType('torchvision'); _ops = types.ModuleType('torchvision.ops'); _boxes = types.ModuleType('torchvision.ops.boxes')
_boxes.box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
_tv.ops = _ops; _ops.boxes = _boxes
for k, v in (('torchvision', _tv), ('torchvision.ops', _ops), ('torchvision.ops.boxes', _boxes)):
    sys.modules.setdefault(k, v)

from lib.evaluate import eval as ref_eval          # noqa: E402
from lib.evaluate import utils as ref_utils        # noqa: E402

from tests import posteval_edge_cases as C         # noqa: E402


class _Log:
    def info(self, *a, **k):
        pass


def _or_raises(fn):
    try:
        return C.null(fn())
    except Exception as e:      # noqa: BLE001  (the class is the datum)
        return {'raises': type(e).__name__}


def _max_ious(results, k):
    out = []
    for res in results:
        g = [e['bbox'] for e in res['gt_boxes']]
        if not g:
            continue
        iou = ref_utils.compute_iou_batch_cross(np.array(res['pred_boxes'][:k]), np.array(g))
        out.extend(iou.max(axis=0).tolist())
    return out


def main():
    fx = {}
    for name, (build, ks) in C.RECORD_SETS.items():
        results = build()
        preds, gts = C.grouped(results)      # grouped exactly as compute_ap does (eval.py:22-50)
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            ap = [ref_utils.compute_average_precision_detection(gts[k], preds[k], iou_thresholds=C.AP_THDS) for k in preds]
            fx[name] = {
                'groups': list(preds.keys()),
                'ap': C.null(ap),
                'max_ious': {str(k): _or_raises(lambda k=k: _max_ious(results, k)) for k in ks},
                'metrics': _or_raises(lambda: ref_eval.eval_results(copy.deepcopy(results), verbose=False, logger=_Log())),
            }
        n_nan = sum(v is None for row in fx[name]['ap'] for v in row)
        print(f'{name}: {len(results)} records, {len(preds)} groups, {n_nan} NaN AP entries, metrics',
              fx[name]['metrics'].get('raises') or fx[name]['metrics']['brief']['SVOL-full-mAP'])
    path = os.path.join(HERE, 'posteval_edges.json')
    with open(path, 'w') as f:
        json.dump(fx, f, allow_nan=False, separators=(',', ':'))
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
