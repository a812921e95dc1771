#!/usr/bin/env python3
"""Generate the SVANet head fixtures with MORE THAN EIGHT heads FROM THE REFERENCE ITSELF (--nheads 9 ... 32: the head counts at which
the sketch -> video gate works in more than one group of eight heads, csrc/gate.hip).

Runs only in the build container (needs the reference, see make_golden.py).  The recipe is make_golden.py's run_head_case at toy
sizes, data only: hidden_dim / nheads = 72 / 9 (one head in the second group; not a multiple of 32, so the per-Linear heads path
runs), 96 / 12, 128 / 16 and 256 / 32 (four full groups).

    python tests/golden/make_golden_heads.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_golden import run_head_case  # noqa: E402

_HEAD = dict(num_layers=2, num_queries=16, num_queries_per_frame=2, num_frames=8, input_vid_dim=64, input_skch_dim=48)
HEAD_CASES = {
    # name (the file is head_<name>.npz): (args overrides, B, T, P, pad_frames)
    'h9_video': (dict(_HEAD, hidden_dim=72, nheads=9, matcher='video_matcher'), 2, 8, 20, 2),
    'h12_frame': (dict(_HEAD, hidden_dim=96, nheads=12, matcher='per_frame_matcher'), 2, 8, 20, 2),
    'h16_video': (dict(_HEAD, hidden_dim=128, nheads=16, matcher='video_matcher'), 2, 8, 20, 2),
    'h32_frame': (dict(_HEAD, hidden_dim=256, nheads=32, matcher='per_frame_matcher'), 2, 8, 20, 2),
}

if __name__ == '__main__':
    only = sys.argv[1:]
    for n, c in HEAD_CASES.items():
        if not only or 'head_' + n in only:
            run_head_case(n, *c)
