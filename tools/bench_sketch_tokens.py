#!/usr/bin/env python
"""Video -> sketch attention (many queries, few keys): svol_attn_fewkeys_fwd / _bwd beside svol_attn_fwd / _bwd on the same operands, and
one SVANet training step in --sketch_attn tokens mode with the attention core forced to each family.

    python tools/bench_sketch_tokens.py [--blocks 5] [--iters 20] [--no-step]

Method: device events around `iters` back-to-back launches per timed block; every shape and family warmed up first; the two families
ALTERNATE block by block inside this one process; per cell the median over the blocks and their spread (max - min) are printed, in
microseconds per launch, with the bytes one launch must move as computed from the shapes (operands read once, results written once,
the few-keys backward's fp32 partials written and read once) and the resulting GB/s at the median.  One JSON line at the end.
Needs the device: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [   # (B, H, Lq, Lk, dh, what)
    (8, 8, 6272, 49, 32, 'ViT video tokens, ResNet sketch grid'),
    (8, 8, 1568, 49, 32, 'ResNet video tokens, ResNet sketch grid'),
    (8, 8, 6272, 197, 32, 'ViT video tokens, ViT sketch tokens'),
    (8, 8, 6272, 98, 64, 'two sketches, hidden_dim 512'),
]
LOG2E = 1.4426950408889634


def launch_bytes(B, H, Lq, Lk, dh, family):
    """(forward, backward) bytes one launch must move, from the shapes: 16-bit operands, fp32 lse2 (and the generic backward's delta)"""
    from svol_amd import ops
    q, kv, lse = B * Lq * H * dh * 2, B * Lk * H * dh * 2, B * H * Lq * 4
    fwd = q + 2 * kv + q + lse                               # q, k, v read; o, lse2 written
    bwd = 3 * q + 2 * kv + lse + q + 2 * kv                  # q, o, do, k, v, lse2 read; dq, dk, dv written
    if family == 'fewkeys':
        bwd += 2 * ops.attn_fewkeys_ws_bytes(B, H, Lq, Lk, dh)
    else:
        bwd += 2 * 3 * lse                                   # the delta scratch, written and read
    return fwd, bwd


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters     # us per launch


def bench_kernels(dtype, blocks, iters):
    from svol_amd import ops
    rows = []
    for B, H, Lq, Lk, dh, what in SHAPES:
        d = H * dh
        g = torch.Generator(device='cuda').manual_seed(Lq + Lk)
        rnd = lambda n: torch.randn((n, d), generator=g, device='cuda', dtype=torch.float32)   # noqa: E731
        premul = LOG2E / dh ** 0.5
        q = (rnd(B * Lq) * premul).to(dtype)
        kv = torch.cat([rnd(B * Lk), rnd(B * Lk)], 1).to(dtype)
        k, v = kv[:, :d], kv[:, d:]
        do = rnd(B * Lq).to(dtype)
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        fams = {'fewkeys': (ops.attn_fewkeys_fwd, ops.attn_fewkeys_bwd), 'generic': (ops.attn_fwd, ops.attn_bwd)}
        saved, cells = {}, {}
        for name, (fwd, bwd) in fams.items():   # warm-up; keep each family's own o / lse2 for its backward
            saved[name] = fwd(q, k, v, B, H, Lq, Lk, dh, None, premul)
            bwd(q, k, v, *saved[name][:1], do, saved[name][1], B, H, Lq, Lk, dh, dq, dkv[:, :d], dkv[:, d:], None, premul)
            cells[name] = {'fwd': [], 'bwd': []}
        torch.cuda.synchronize()
        o_f, o_g = saved['fewkeys'][0].float(), saved['generic'][0].float()
        agree = float((o_f - o_g).abs().max())
        for _ in range(blocks):
            for name, (fwd, bwd) in fams.items():
                o, lse2 = saved[name]
                cells[name]['fwd'].append(timed(lambda: fwd(q, k, v, B, H, Lq, Lk, dh, None, premul), iters))
                cells[name]['bwd'].append(timed(lambda: bwd(q, k, v, o, do, lse2, B, H, Lq, Lk, dh, dq, dkv[:, :d], dkv[:, d:], None, premul), iters))
        for name in fams:
            nb = launch_bytes(B, H, Lq, Lk, dh, name)
            for way, nbytes in zip(('fwd', 'bwd'), nb):
                t = cells[name][way]
                med = statistics.median(t)
                rows.append(dict(dtype=str(dtype).split('.')[-1], B=B, H=H, Lq=Lq, Lk=Lk, dh=dh, family=name, way=way, us_median=round(med, 1),
                                 us_spread=round(max(t) - min(t), 1), bytes=nbytes, gbps=round(nbytes / med / 1e3, 1), o_max_diff=agree))
                print(f'{rows[-1]["dtype"]:8s} B{B} H{H} Lq{Lq} Lk{Lk} dh{dh} {name:8s} {way}: {med:9.1f} us (spread {max(t) - min(t):7.1f}) '
                      f'{nbytes / 1e6:8.1f} MB {nbytes / med / 1e3:7.1f} GB/s   [{what}]', flush=True)
    return rows


def bench_step(dtype, blocks, iters):
    """one training step (forward, criterion, backward; no optimizer) of a mid32-like head in tokens mode: d = 256, 8 heads, 2 layers,
    L = 1568 video tokens (32 frames x 49), Ls = 49, batch 8, the core forced to each family"""
    from svol_amd import synthetic as syn
    from svol_amd.modeling import cross_modal_transformer as cmt
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.model import build_model
    B, T, P, Ls = 8, 32, 49, 49
    args = syn.head_args(hidden_dim=256, nheads=8, num_layers=2, num_queries=100, num_frames=T, backbone='features', sketch_attn='tokens',
                         input_dropout=0.0, compute_dtype={torch.bfloat16: 'bf16', torch.float16: 'fp16'}[dtype])
    model = build_model(args).cuda().train()
    crit = build_loss(args).cuda()
    g = torch.Generator(device='cuda').manual_seed(3)
    sk = torch.randn((B, Ls, args.input_skch_dim), generator=g, device='cuda')
    vd = torch.randn((B, T, P, args.input_vid_dim), generator=g, device='cuda')
    skm, vdm = torch.ones((B, Ls), device='cuda'), torch.ones((B, T), device='cuda')
    tg = syn.synth_targets(B, T, seed=1)
    scale = 4096.0 if dtype == torch.float16 else 1.0

    def step():
        for p_ in model.parameters():
            p_.grad = None
        out = model(sk, vd, skm, vdm)
        ld = crit(out, tg)
        (sum(ld[k] * crit.weight_dict[k] for k in ld.keys() if k in crit.weight_dict) * scale).backward()

    rows, cells = [], {'fewkeys': [], 'generic': []}
    for name in cells:
        cmt.TOKENS_CORE = 'fewkeys!' if name == 'fewkeys' else None
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name in cells:
            cmt.TOKENS_CORE = 'fewkeys!' if name == 'fewkeys' else None
            cells[name].append(timed(step, iters))
    cmt.TOKENS_CORE = 'fewkeys'
    for name, t in cells.items():
        med = statistics.median(t)
        rows.append(dict(dtype=str(dtype).split('.')[-1], step='svanet tokens d256 L1568 Ls49 B8 2 layers', core=name, us_median=round(med, 1),
                         us_spread=round(max(t) - min(t), 1)))
        print(f'{rows[-1]["dtype"]:8s} training step, core {name:8s}: {med / 1e3:8.3f} ms (spread {(max(t) - min(t)) / 1e3:6.3f})', flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sketch_tokens needs the device (no CPU path)')
    rows = []
    for dtype in (torch.bfloat16, torch.float16):
        rows += bench_kernels(dtype, a.blocks, a.iters)
    if not a.no_step:
        for dtype in (torch.bfloat16, torch.float16):
            rows += bench_step(dtype, a.blocks, max(2, a.iters // 4))
    print(json.dumps({'bench_sketch_tokens': rows}))


if __name__ == '__main__':
    main()
