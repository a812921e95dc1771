"""Timings for profiles/resnet50.md and profiles/layernorm_wide.md (records, not bars; bench.py is the flagship yardstick).

    python tools/bench_resnet50.py step       [--B 8 --T 32 --dtype bf16 --warmup 3 --steps 30]
        ms per training step (forward, criterion, backward, FlatAdamW) of build_model(--backbone X) for X = resnet50 and resnet,
        each with the extractors frozen and trained, synthetic weights and pixels, one process, the variants alternated in rounds so that a
        drift of the box shows in all of them.  Host clock around `steps` steps that end in a device synchronise.
    python tools/bench_resnet50.py layernorm  [--iters 3000]
        us per launch of svol_layernorm_fwd / _bwd at the wide shapes, device events around `iters` back-to-back launches that rotate
        through so many input sets that the x buffers ALONE are more than twice the 256 MB last-level cache (the forward reads nothing
        else that rotates); bytes = what the launch must move (below), TB/s = bytes / time.

One JSON line per figure.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

DEV = 'cuda'


def ln_bytes(M, D, esize, fwd):
    """forward: read x, write y (+ gamma, beta, mean, rstd); backward: read dy and x, write dx (+ gamma, mean, rstd, the three [D] sinks)"""
    if fwd:
        return M * D * 2 * esize + 2 * D * 4 + 2 * M * 4
    return M * D * 3 * esize + D * 4 + 2 * M * 4 + 3 * D * 4


def bench_layernorm(a):
    from svol_amd import ops
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}[a.dtype]
    es = torch.empty((), dtype=dt).element_size()
    for M, D in ((12544, 2048), (50176, 1536), (12544, 4096), (50176, 1024)):
        sets = int(600e6 // (M * D * es)) + 1   # the rotating x buffers alone: > 2 x the last-level cache, for the forward too
        g = torch.Generator(device=DEV).manual_seed(1)
        xs = [torch.randn((M, D), device=DEV, generator=g).to(dt) for _ in range(sets)]
        dys = [torch.randn((M, D), device=DEV, generator=g).to(dt) for _ in range(sets)]
        gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
        sinks = [torch.zeros(D, device=DEV) for _ in range(3)]
        _, _, _, mean, rstd = ops.layernorm_fwd(xs[0], gamma, beta, dt)
        stats = [ops.layernorm_fwd(x, gamma, beta, dt)[3:] for x in xs]

        def fwd(i):
            ops.layernorm_fwd(xs[i % sets], gamma, beta, dt)

        def bwd(i):
            mean, rstd = stats[i % sets]
            ops.layernorm_bwd(None, dys[i % sets], None, xs[i % sets], gamma, mean, rstd, dt, want_colsum=True, dg_out=sinks[0], db_out=sinks[1],
                              cs_out=sinks[2])
        for name, fn in (('fwd', fwd), ('bwd', bwd)):
            for i in range(2 * sets):
                fn(i)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            runs = []
            for _ in range(3):
                e0.record()
                for i in range(a.iters):
                    fn(i)
                e1.record()
                torch.cuda.synchronize()
                runs.append(e0.elapsed_time(e1) * 1e3 / a.iters)
            us = sorted(runs)[1]
            b = ln_bytes(M, D, es, name == 'fwd')
            print(json.dumps(dict(what='layernorm_' + name, M=M, D=D, dtype=a.dtype, kernel='wide' if D > 1024 else 'one-wave-per-row',
                                  us_per_launch=round(us, 2), us_runs=[round(r, 2) for r in runs], bytes=b, TB_per_s=round(b / us / 1e6, 3),
                                  buffer_sets=sets, iters=a.iters, note='includes the host-side allocation of the outputs per call')), flush=True)
        del xs, dys, stats


def synth_bottleneck_weights(ext, seed):
    """He-scaled convolutions, BatchNorm weight 1 (0.1 on a block's last BatchNorm, so that 16 residual adds keep the scale), zero shifts
    and means, unit variances: the IMAGENET1K weights cannot be fetched where this runs, and timings do not depend on the values"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in ext.state_dict().items():
        if v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5
        elif k.endswith(('running_var', 'weight')):
            sd[k] = torch.full_like(v, 0.1 if '.bn3.weight' in k else 1.0)
        else:
            sd[k] = torch.zeros_like(v)
    return sd


def make_step(backbone, train_backbone, a):
    from svol_amd import parallel
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.model import build_model
    args = syn.head_args(backbone=backbone, compute_dtype=a.dtype, num_frames=a.T)
    args.train_backbone = int(train_backbone)
    torch.manual_seed(1)
    model = build_model(args)
    if backbone == 'resnet50':
        for seed, ext in ((1, model.backbone.video_backbone), (2, model.backbone.sketch_backbone)):
            ext.load_state_dict(synth_bottleneck_weights(ext, seed))
    else:
        model.backbone.video_backbone.load_state_dict(syn.synth_resnet_state_dict(syn.resnet_param_shapes((3, 4, 6, 3)), seed=1))
        model.backbone.sketch_backbone.load_state_dict(syn.synth_resnet_state_dict(syn.resnet_param_shapes((2, 2, 2, 2)), seed=2))
    model.to(DEV).train()
    if not train_backbone:
        model.backbone.eval()
    crit = build_loss(args).to(DEV).train()
    params = [p for p in model.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
    opt = parallel.FlatAdamW(red, lr=1e-4, weight_decay=1e-4, params=params)
    g = torch.Generator(device=DEV).manual_seed(1)
    vid = torch.randn((a.B, a.T, 3, 224, 224), device=DEV, generator=g)
    sk = torch.randn((a.B, 1, 3, 224, 224), device=DEV, generator=g)
    ms, mv = torch.ones(a.B, 1, device=DEV), torch.ones(a.B, a.T, device=DEV)
    tg = syn.synth_targets(a.B, a.T, seed=1)

    def step():
        red.zero_grad()
        out = model(sk, vid, ms, mv)
        crit(out, tg)
        loss = crit.weighted_total()
        loss.backward()
        red.finish()
        opt.step()
        return loss
    return step, sum(p.numel() for p in params)


def bench_step(a):
    variants = [(bb, tb) for bb in ('resnet50', 'resnet') for tb in (0, 1)]
    if a.only:
        variants = [v for v in variants if f'{v[0]}:{v[1]}' in a.only.split(',')]
    times = {v: [] for v in variants}
    for rnd in range(a.rounds):
        for v in variants:   # (a fresh model per visit: the trained variants hold tens of GB of activations)
            step, n_params = make_step(*v, a)
            for _ in range(a.warmup):
                loss = step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            times[v].append(ms)
            print(json.dumps(dict(what='step', backbone=v[0], train_backbone=v[1], round=rnd, B=a.B, T=a.T, dtype=a.dtype, ms_per_step=round(ms, 2),
                                  steps=a.steps, warmup=a.warmup, trainable_params=n_params, loss=float(loss),
                                  peak_GB=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))), flush=True)
            del step
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
    for v, t in times.items():
        print(json.dumps(dict(what='step_summary', backbone=v[0], train_backbone=v[1], ms_per_step_runs=[round(x, 2) for x in t],
                              ms_per_step_min=round(min(t), 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['step', 'layernorm'])
    ap.add_argument('--B', type=int, default=8)
    ap.add_argument('--T', type=int, default=32)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16', 'fp32'])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--iters', type=int, default=3000)
    ap.add_argument('--only', default='', help='comma list of backbone:train_backbone, e.g. resnet50:0,resnet:0')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resnet50.py measures on the MI355X: no device found')
    torch.cuda.set_device(0)
    (bench_step if a.what == 'step' else bench_layernorm)(a)


if __name__ == '__main__':
    main()
