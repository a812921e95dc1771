#!/usr/bin/env python3
"""Generate the head-width 64 / 48 fixtures FROM THE REFERENCE ITSELF (--nheads / --hidden_dim choices whose heads are wider than 32).

Runs only in the build container (needs the reference, see make_golden.py).  The recipes are make_golden.py's run_head_case and
make_golden_encdec.py's run with two heads of 64 (hidden_dim 128) or of 48 (hidden_dim 96): toy sizes, data only.

    python tests/golden/make_golden_dh64.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_golden import run_head_case  # noqa: E402
from tests.golden.make_golden_encdec import run as run_encdec  # noqa: E402

_HEAD = dict(nheads=2, num_layers=2, num_queries=16, num_queries_per_frame=2, num_frames=8, input_vid_dim=64, input_skch_dim=48)
HEAD_CASES = {
    # name (the file is head_<name>.npz): (args overrides, B, T, P, pad_frames)
    'dh64_video': (dict(_HEAD, hidden_dim=128, matcher='video_matcher'), 2, 8, 20, 2),
    'dh48_frame': (dict(_HEAD, hidden_dim=96, matcher='per_frame_matcher'), 2, 8, 20, 2),
}
ENCDEC_CASES = {
    # 40 queries: with encdec_args' 8, the box head's bias gradients are sums over B N dec_layers = 32 rows and one ReLU mask that flips
    # under bf16 rounding moves an element by 0.4 of the largest -- at four heads of 32 as much as at two heads of 64
    'encdec_dh64_append_post': dict(head='variants', over=dict(mode='append_to_seq', pre_norm=False, hidden_dim=128, nheads=2,
                                                               dim_feedforward=128, num_queries=40), B=2, L=150, Ls=2, pad=37),
    'encdec_train_dh64_qry_pre': dict(head='variants', over=dict(mode='concat_to_qry', pre_norm=True, hidden_dim=128, nheads=2,
                                                                 dim_feedforward=128, dropout=0.25, input_dropout=0.0),
                                      B=2, L=40, Ls=1, pad=0, train=True),
}

if __name__ == '__main__':
    only = sys.argv[1:]
    for n, c in HEAD_CASES.items():
        if not only or 'head_' + n in only:
            run_head_case(n, *c)
    for n, c in ENCDEC_CASES.items():
        if not only or n in only:
            run_encdec(n, c)
