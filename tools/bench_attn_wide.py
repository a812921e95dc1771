#!/usr/bin/env python3
"""Attention at head width 64 (csrc/attention.hip's generic template at two d-tiles) beside the same build's head width 32 launches of
equal FLOPs.

Forward and backward alone, device events, warm, the median of repeated blocks; a wide block and a narrow block alternate so that
both see the same machine state.  Shapes: video self-attention (B = 8, L = 6272) and the object queries' cross-attention (100 queries
against 6272 keys), H x dh = 4 x 64 against 8 x 32, fp32, bf16 and fp16.  One JSON line per launch pair.  In fp32 the two columns are
the template's two instances (<float, 2> and <float, 1>); at 16 bits the 8 x 32 column is csrc/attention_bf16.hip.

--tree DIR times the svol_amd (and its built library) of another checkout, e.g. a parent commit's, with this same script.

    python tools/bench_attn_wide.py [--blocks 7] [--iters 10] [--tree DIR]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

LOG2E = 1.4426950408889634
ops = None   # svol_amd.ops of the chosen checkout (main)


def make(B, H, Lq, Lk, dh, dtype):
    g = torch.Generator(device='cuda').manual_seed(1)
    d = H * dh
    pm = LOG2E / math.sqrt(dh)
    q = (torch.randn((B * Lq, d), generator=g, device='cuda') * pm).to(dtype)
    k, v = (torch.randn((B * Lk, d), generator=g, device='cuda').to(dtype) for _ in range(2))
    do = torch.randn((B * Lq, d), generator=g, device='cuda').to(dtype)
    o, lse2 = ops.attn_fwd(q, k, v, B, H, Lq, Lk, dh, None, pm)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    dims = (B, H, Lq, Lk, dh)
    fwd = lambda: ops.attn_fwd(q, k, v, *dims, None, pm)
    bwd = lambda: ops.attn_bwd(q, k, v, o, do, lse2, *dims, dq, dk, dv, None, pm)
    return fwd, bwd


def block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def pair(wide, narrow, blocks, iters):
    """median ms per call of the two launches, their blocks alternating"""
    for fn in (wide, narrow):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    tw, tn = [], []
    for _ in range(blocks):
        tw.append(block(wide, iters))
        tn.append(block(narrow, iters))
    return statistics.median(tw), statistics.median(tn), (min(tw), max(tw)), (min(tn), max(tn))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the checkout whose svol_amd is imported (default: this one)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    global ops
    sys.path.insert(0, os.path.abspath(a.tree))
    from svol_amd import ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(a.tree) + os.sep), ops.__file__
    for dtype, dn in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16'), (torch.float16, 'fp16')):
        for tag, B, Lq, Lk in (('self', 8, 6272, 6272), ('cross', 8, 100, 6272)):
            wf, wb = make(B, 4, Lq, Lk, 64, dtype)
            nf, nb = make(B, 8, Lq, Lk, 32, dtype)
            for what, w, n, mult in (('fwd', wf, nf, 4), ('bwd', wb, nb, 10)):
                tw, tn, rw, rn = pair(w, n, a.blocks, a.iters)
                flop = mult * B * 256 * Lq * Lk   # H dh = 256 on both sides
                print(json.dumps(dict(dtype=dn, shape=tag, B=B, Lq=Lq, Lk=Lk, what=what, ms_h4_dh64=round(tw, 4), ms_h8_dh32=round(tn, 4),
                                      ratio=round(tw / tn, 3), tflops_dh64=round(flop / tw / 1e9, 1), tflops_dh32=round(flop / tn / 1e9, 1),
                                      range_dh64=[round(x, 4) for x in rw], range_dh32=[round(x, 4) for x in rn])), flush=True)


if __name__ == '__main__':
    main()
