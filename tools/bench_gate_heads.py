#!/usr/bin/env python3
"""The sketch -> video gate at 8, 16 and 32 heads (csrc/gate.hip: above eight heads the score pass and the backward apply pass run once
per group of eight), and what 16 heads buy at hidden_dim 512: attention as 16 x 32 (csrc/attention_bf16.hip) beside 8 x 64 (the
generic template).

The protocol of tools/bench_attn_wide.py: whole launches (svol_gate_fwd: scores + statistics + apply; svol_gate_bwd: its memset and
two or more kernels) through the C ABI between device events, warm; the head counts' blocks alternate, so that all see the same machine
state; the median of --blocks blocks of --iters launches.  B = 8, L = 6272, bf16 pos, D = 256 and 512.  One JSON line per (D, launch)
with the times per head count and time(H) / (ceil(H / 8) time(8)); then one per attention launch pair.  A head count the library
refuses (a tree from before the change, --tree) is reported as null.

--heads 8 times the eight-head launches alone: the comparison of two trees at H = 8.  (With the other head counts' blocks in between,
the eight-head forward at D = 512 measured 4 - 7 % slower than alone, profiles/gate_heads.md; a tree that refuses them would be
favoured.)

    python tools/bench_gate_heads.py [--blocks 7] [--iters 10] [--tree DIR] [--no-attn] [--heads 8,16,32]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

LOG2E = 1.4426950408889634
ops = _lib = None   # svol_amd.ops / ._lib of the chosen checkout (main)


def make_gate(B, L, D, H, dtype):
    g = torch.Generator(device='cuda').manual_seed(1)
    r = lambda *sh: torch.randn(sh, generator=g, device='cuda')   # noqa: E731
    M = B * L
    x, pos, u = r(M, D), r(M, D).to(dtype), r(B, H, D) * 0.2
    gamma, beta = 1 + 0.1 * r(D), 0.1 * r(D)
    dy32, dy = r(M, D), r(M, D).to(dtype)
    y32, y, ypos = torch.empty_like(x), torch.empty_like(pos), torch.empty_like(pos)
    a, mean, rstd = (torch.empty((M,), device='cuda') for _ in range(3))
    ws, ws2 = torch.empty((B * H * (L + 2),), device='cuda'), torch.empty((M + B * H,), device='cuda')
    dx, du, dg, db = torch.empty_like(x), torch.zeros((B, H, D), device='cuda'), torch.zeros((D,), device='cuda'), torch.zeros((D,), device='cuda')
    L_, P, dt, st = _lib.lib(), ops._ptr, ops._DT[dtype], ops._stream()
    keep = (x, pos, u, gamma, beta, dy32, dy, y32, y, ypos, a, mean, rstd, ws, ws2, dx, du, dg, db)

    def fwd(keep=keep):
        return L_.svol_gate_fwd(P(x), P(pos), P(u), P(gamma), P(beta), P(y32), P(y), P(ypos), P(a), P(mean), P(rstd), P(ws), B, L, D, H, dt, st)

    def bwd(keep=keep):
        return L_.svol_gate_bwd(P(dy32), P(dy), None, P(x), P(pos), P(u), P(gamma), P(a), P(mean), P(rstd), P(ws), P(ws2), P(dx), P(du), P(dg),
                                P(db), B, L, D, H, dt, st)
    if fwd() != 0 or bwd() != 0:
        return None, None
    return fwd, bwd


def make_attn(B, H, Lq, Lk, dh, dtype):
    g = torch.Generator(device='cuda').manual_seed(1)
    d = H * dh
    pm = LOG2E / math.sqrt(dh)
    q = (torch.randn((B * Lq, d), generator=g, device='cuda') * pm).to(dtype)
    k, v = (torch.randn((B * Lk, d), generator=g, device='cuda').to(dtype) for _ in range(2))
    do = torch.randn((B * Lq, d), generator=g, device='cuda').to(dtype)
    o, lse2 = ops.attn_fwd(q, k, v, B, H, Lq, Lk, dh, None, pm)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    dims = (B, H, Lq, Lk, dh)
    return (lambda: ops.attn_fwd(q, k, v, *dims, None, pm)), (lambda: ops.attn_bwd(q, k, v, o, do, lse2, *dims, dq, dk, dv, None, pm))


def block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, blocks, iters):
    """{name: (median, min, max)} ms per call, the launches' blocks alternating"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in fns}
    for _ in range(blocks):
        for n, fn in fns.items():
            t[n].append(block(fn, iters))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--no-attn', action='store_true', help='the gate only')
    ap.add_argument('--heads', default='8,16,32', help='head counts whose blocks alternate (8 is always among them)')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the checkout whose svol_amd is imported (default: this one)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    global ops, _lib
    sys.path.insert(0, os.path.abspath(a.tree))
    from svol_amd import _lib, ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(a.tree) + os.sep), ops.__file__
    B, L, dtype = 8, 6272, torch.bfloat16
    heads = sorted({8} | {int(h) for h in a.heads.split(',')})
    for D in (256, 512):
        made = {H: make_gate(B, L, D, H, dtype) for H in heads}
        for i, what in enumerate(('fwd', 'bwd')):
            t = alternate({H: m[i] for H, m in made.items() if m[i] is not None}, a.blocks, a.iters)
            rec = dict(op='gate', what=what, B=B, L=L, D=D, dtype='bf16')
            for H in made:
                rec[f'ms_h{H}'] = round(t[H][0], 4) if H in t else None
                rec[f'range_h{H}'] = [round(t[H][1], 4), round(t[H][2], 4)] if H in t else None
                if H > 8 and H in t:
                    rec[f'h{H}_over_groups_x_h8'] = round(t[H][0] / (-(-H // 8) * t[8][0]), 3)   # the bound: <= 1.1
            print(json.dumps(rec), flush=True)
        del made
    if a.no_attn:
        return
    for tag, Lq, Lk in (('self', 6272, 6272), ('cross', 100, 6272)):
        narrow, wide = make_attn(B, 16, Lq, Lk, 32, dtype), make_attn(B, 8, Lq, Lk, 64, dtype)
        for i, what in enumerate(('fwd', 'bwd')):
            t = alternate({'h16_dh32': narrow[i], 'h8_dh64': wide[i]}, a.blocks, a.iters)
            print(json.dumps(dict(op='attn', shape=tag, what=what, B=B, Lq=Lq, Lk=Lk, dtype='bf16', ms_h16_dh32=round(t['h16_dh32'][0], 4),
                                  ms_h8_dh64=round(t['h8_dh64'][0], 4), ratio_dh64_over_dh32=round(t['h8_dh64'][0] / t['h16_dh32'][0], 3),
                                  range_h16_dh32=[round(x, 4) for x in t['h16_dh32'][1:]], range_h8_dh64=[round(x, 4) for x in t['h8_dh64'][1:]])),
                  flush=True)


if __name__ == '__main__':
    main()
