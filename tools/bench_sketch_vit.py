#!/usr/bin/env python3
"""Sketch-ViT classification fine-tuning step on the MI355X (preprocess/sketch_vit_finetune.py:118-143 at its defaults: batch 32,
ViT-B/16, finetune_layers = 1, AdamW): ms per step and per phase (forward, loss, backward, FlatAdamW incl. the reducer's finish).

    python tools/bench_sketch_vit.py --path cls         SketchViTClassifier.loss: the [CLS]-only last block (cls_logits)
    python tools/bench_sketch_vit.py --path full        the same loss taken from forward()'s full last block
    python tools/bench_sketch_vit.py --path extractor   ViTExtractor(trainable=True, train_layers=1) with a loss on last[:, 0] only
                                                        (what a user could run before the classifier existed; --root selects the
                                                        tree whose svol_amd is imported, so a checkout of an older commit can be timed)

--dtype {bf16,fp16}: the extractor's operand type (compute_dtype); fp16 multiplies the loss by --loss_scale (4096) and hands the same
factor to FlatAdamW, which divides it out inside the update.

Timing: --blocks blocks of --steps steps after --warmup steps; a block's step time is a host clock around the block, ending in a
device synchronise; the phase times are device events inside the steps.  Reported: the median block, every block, and the shader clock
the chip held under --steps more untimed steps (csrc/clock_probe.hip, bench.py's `sclk_ghz`).  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--path', choices=('cls', 'full', 'extractor'), default='cls')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--finetune_layers', type=int, default=1)
    ap.add_argument('--num_labels', type=int, default=19)
    ap.add_argument('--dtype', choices=('bf16', 'fp16'), default='bf16')
    ap.add_argument('--loss_scale', type=float, default=4096.0)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_sketch_vit.py measures on the MI355X: no GPU, no number')
    from svol_amd import parallel
    from svol_amd import synthetic as syn
    dev = torch.device('cuda', 0)
    cfg = syn.vit_config(num_hidden_layers=a.layers)
    x = syn.synth_images(a.n, cfg, seed=2).to(dev)
    targets = (torch.arange(a.n) % a.num_labels).to(dev)
    kw = {} if a.dtype == 'bf16' else {'compute_dtype': a.dtype}   # (an older tree under --root has no such argument)
    scale = a.loss_scale if a.dtype == 'fp16' else 1.0
    if a.path == 'extractor':
        from svol_amd.modeling.backbone import ViTExtractor
        m = ViTExtractor(cfg, trainable=True, train_layers=a.finetune_layers, **kw)
        m.load_state_dict(syn.synth_vit_state_dict(cfg, seed=1))
        m.to(dev).train()
        R = torch.randn(a.n, cfg.hidden_size, device=dev)
        fwd = lambda: m(x)[:, 0]                       # noqa: E731
        lossfn = lambda t: (t * R).sum()               # noqa: E731
    else:
        from svol_amd.modeling.sketch_vit import SketchViTClassifier, _XentFn
        m = SketchViTClassifier(cfg, a.num_labels, a.finetune_layers, **kw)
        m.load_state_dict(syn.synth_classifier(cfg, a.num_labels, seed=1))
        m.to(dev).train()
        fwd = (lambda: m.cls_logits(x)) if a.path == 'cls' else (lambda: m(x)[2])
        lossfn = lambda t: _XentFn.apply(t, targets)[0]   # noqa: E731
    params = [p for p in m.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(m), ordered=True)
    opt = parallel.FlatAdamW(red, lr=1e-4, weight_decay=1e-4, params=params)
    opt.loss_scale = scale
    marks = []

    def step(timed=False):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timed else None
        red.zero_grad()
        if timed:
            ev[0].record()
        out = fwd()
        if timed:
            ev[1].record()
        loss = lossfn(out)
        if timed:
            ev[2].record()
        (loss * scale if scale != 1.0 else loss).backward()
        if timed:
            ev[3].record()
        red.finish()
        opt.step()
        if timed:
            ev[4].record()
            marks.append(ev)
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    blocks, phases = [], []
    for _ in range(a.blocks):
        marks.clear()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step(True)
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) / a.steps * 1e3)
        phases.append([sum(ev[i].elapsed_time(ev[i + 1]) for ev in marks) / a.steps for i in range(4)])
    mid = sorted(range(a.blocks), key=lambda i: blocks[i])[a.blocks // 2]
    res = {'path': a.path, 'dtype': a.dtype, 'n': a.n, 'layers': a.layers, 'finetune_layers': a.finetune_layers, 'steps': a.steps,
           'ms_per_step': round(statistics.median(blocks), 4), 'ms_per_step_blocks': [round(b, 4) for b in blocks],
           'phase_ms': dict(zip(('forward', 'loss', 'backward', 'optimizer'), (round(v, 4) for v in phases[mid]))),
           'loss': round(float(loss), 5), 'sclk_ghz': shader_clock(torch, dev, step, a.steps)}
    print(json.dumps(res))


def shader_clock(torch, dev, step, steps):
    """the shader clock the chip holds under `steps` more (untimed) steps: bench.py's probe"""
    import ctypes
    from svol_amd import _lib
    cap = 8192
    samples = torch.zeros(2 * cap, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    khz = ctypes.c_int32(0)
    ps = torch.cuda.Stream()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().svol_clock_probe(samples.data_ptr(), count.data_ptr(), cap, stop.data_ptr(), 200, 20000, ctypes.byref(khz),
                                           ps.cuda_stream), 'svol_clock_probe')
    try:
        for _ in range(steps):
            step()
    finally:
        stop.fill_(1)            # stream-ordered behind the steps: the probe leaves at its next window
        torch.cuda.synchronize()
    n = int(count.item())
    if n < 8:
        return None
    w = samples[:2 * n].view(n, 2).cpu().double()
    ghz = (w[:, 0] / w[:, 1] * (khz.value / 1e6)).sort().values
    pick = lambda q: round(float(ghz[min(n - 1, int(q * n))]), 3)   # noqa: E731
    return {'p10': pick(0.1), 'median': pick(0.5), 'p90': pick(0.9), 'windows': n}


if __name__ == '__main__':
    main()
