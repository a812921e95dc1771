#!/usr/bin/env python3
"""Trainable ViT-B/16 extractor at BASELINE configs[3] (cfg4) size: 256 frames + 8 sketches at 224x224.

Times (device events, after a warm-up, median of --iters):
  frozen        the frozen extractors' forward (video on the frames, sketch on the sketches)
  train_all     the trainable extractors' forward + backward, every parameter trained
  train_last2   the same with train_layers=2 (preprocess/sketch_vit_finetune.py)
and the short-sequence attention kernels alone at (n=256, H=12, L=197, dh=64): svol_attn_small_fwd / _fwd_lse / _bwd.
Algorithmic GFLOP (no recomputation counted; attention backward = 5 products of the forward's 2) and the share of the
2.5 PFLOP/s dense bf16 peak.  Usage: python tools/bench_vit_train.py [--iters 10] [--frames 256] [--sketches 8]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

PEAK = 2.5e15


def timeit(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def vit_fwd_flops(cfg, n, layers=None):
    d, f, p = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    P = (cfg.image_size // p) ** 2
    L = P + 1
    layers = cfg.num_hidden_layers if layers is None else layers
    per_layer = 2 * L * (4 * d * d + 2 * d * f) + 4 * L * L * d
    return n * (2 * P * cfg.num_channels * p * p * d + layers * per_layer), per_layer


def line(name, ms, flop):
    print(f'{name:34s} {ms:9.3f} ms  {flop / 1e9:9.1f} GFLOP  {flop / (ms * 1e-3) / 1e12:7.1f} TFLOP/s  '
          f'{flop / (ms * 1e-3) / PEAK:6.3f} of peak', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--sketches', type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_vit_train needs the MI355X')
    from svol_amd import ops
    from svol_amd import synthetic as syn
    from svol_amd.modeling.backbone import ViTExtractor
    dev = 'cuda'
    cfg = syn.vit_config()
    d = cfg.hidden_size

    # ---- the attention kernels alone
    n, H, L, dh = 256, 12, 197, 64
    torch.manual_seed(0)
    qkv = (torch.randn(n * L, 3 * d, device=dev)).bfloat16()
    do = torch.randn(n * L, d, device=dev).bfloat16()
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    o, lse2 = ops.attn_small_fwd(q, k, v, n, H, L, dh, want_lse=True)
    dqkv = torch.empty_like(qkv)
    f_fwd = 4.0 * n * H * L * L * dh
    print(f'# attention alone (n={n}, H={H}, L={L}, dh={dh})')
    line('svol_attn_small_fwd', timeit(lambda: ops.attn_small_fwd(q, k, v, n, H, L, dh), a.iters), f_fwd)
    line('svol_attn_small_fwd_lse', timeit(lambda: ops.attn_small_fwd(q, k, v, n, H, L, dh, want_lse=True), a.iters), f_fwd)
    line('svol_attn_small_bwd', timeit(lambda: ops.attn_small_bwd(q, k, v, o, do, lse2, n, H, L, dh, dqkv[:, :d], dqkv[:, d:2 * d],
                                                                  dqkv[:, 2 * d:]), a.iters), 2.5 * f_fwd)
    del qkv, do, o, lse2, dqkv

    # ---- the extractors
    sd_v, sd_s = syn.synth_vit_state_dict(cfg, seed=1), syn.synth_vit_state_dict(cfg, seed=2)
    frames = syn.synth_images(a.frames, cfg, seed=3).to(dev)
    sketches = syn.synth_images(a.sketches, cfg, seed=4).to(dev)
    nimg = a.frames + a.sketches
    fwd_all, per_layer = vit_fwd_flops(cfg, nimg)
    print(f'# extractors ({a.frames} frames + {a.sketches} sketches at {cfg.image_size}^2)')

    def pair(**kw):
        vb, sb = ViTExtractor(cfg, **kw), ViTExtractor(cfg, **kw)
        vb.load_state_dict(sd_v)
        sb.load_state_dict(sd_s)
        return vb.to(dev), sb.to(dev)

    vb, sb = pair()
    vb.eval(), sb.eval()

    def frozen():
        with torch.no_grad():
            vb(frames)
            sb(sketches)
    t_frozen = timeit(frozen, a.iters)
    line('frozen forward', t_frozen, fwd_all)
    del vb, sb
    res = {}
    for name, tl in (('train_all', None), ('train_last2', 2)):
        vb, sb = pair(trainable=True, train_layers=tl)
        vb.train(), sb.train()

        def step():
            lv = vb(frames)
            ls = sb(sketches)
            (lv[:, 1:].sum() + ls[:, 0].sum()).backward()
        res[name] = timeit(step, a.iters)
        bwd_layers = cfg.num_hidden_layers if tl is None else tl
        flop = fwd_all + 2 * nimg * bwd_layers * per_layer + ((fwd_all - cfg.num_hidden_layers * per_layer * nimg) if tl is None else 0)
        line(f'trainable fwd+bwd ({name})', res[name], flop)
        del vb, sb
        torch.cuda.empty_cache()
    print(f'# train_all / frozen = {res["train_all"] / t_frozen:.2f}x (target <= 3.5x); '
          f'train_last2 / frozen = {res["train_last2"] / t_frozen:.2f}x')


if __name__ == '__main__':
    main()
