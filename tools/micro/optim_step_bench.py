"""Time of one optimizer step on the parameter list of the benchmark model (bench.py's configs[1] head: d = 256, 6 layers, the
reducer's 16 MiB buckets in arrival order), in ONE process with device events:

    flat AdamW   parallel.FlatAdamW   svol_adamw_flat   28 B / parameter   (the yardstick: the kernel bench.py times)
    flat Adam    parallel.FlatAdam    svol_adam_flat    28 B / parameter
    flat SGD     parallel.FlatSGD     svol_sgd_flat     20 B / parameter
    torch Adam   torch.optim.Adam at its defaults (multi-tensor)
    torch SGD    torch.optim.SGD(momentum=0.9) otherwise at its defaults

All five read the SAME gradient buffers: the three flat optimizers share one reducer (each keeps flat parameters and state of
its own; the gradient buckets are the reducer's), the torch optimizers step the same parameters, whose .grad are views into those
buckets.  Per optimizer: warm-up, then blocks of --block steps between two events, the five taking turns (alternating blocks,
so that a clock or temperature drift hits all alike), --blocks blocks each = blocks * block timed steps; the whole sequence --reps
times for the spread.  Achieved bytes/s = bytes per parameter * flat length / time per step, also as a share of the HBM peak
(MI355X: 8.0 TB/s spec; 6.29 TB/s is what a float4 copy reaches).  After the timed sequence each flat optimizer runs once more,
untimed, beside bench.py's clock probe: the shader clock the chip held under it.

    python tools/micro/optim_step_bench.py [--block 100] [--blocks 5] [--reps 3] [--out FILE.json]

--clip times the clipped step instead (max_grad_norm, parallel.py), same protocol, five other rows on the same gradient buffers:

    (a) flat AdamW                       the row above
    (b) flat AdamW + scaler              svol_grad_finite per bucket + svol_adamw_flat_scaled + svol_loss_scaler_update: the launch
                                         structure of the clipped step, 32 B / parameter
    (c) clipped AdamW                    svol_grad_sqnorm per bucket + svol_grad_clip_state + svol_adamw_flat_scaled
    (d) clipped AdamW + scaler           (c) + svol_loss_scaler_update
    (e) clip_grad_norm_ + flat AdamW     torch.nn.utils.clip_grad_norm_ over the gradient views, then (a)

--groups times the grouped / capturable step (svol_adamw_flat_grouped + svol_flat_step_advance, parallel.py), same protocol:

    (a) flat AdamW                       the row above
    (b) grouped, one group               capturable=True: one run per bucket
    (c) two groups, contiguous           split by name (what the forward uses first — input projections, embeddings, layer 0 —
                                         against the rest): the groups are contiguous in the arrival-order buckets, a handful of runs
    (d) two groups, alternating          weights against biases and norms: the groups alternate parameter by parameter, the
                                         worst run count
    (e) torch AdamW fused capturable     torch.optim.AdamW(fused=True, capturable=True): what a captured step uses today

The run count per bucket of (b), (c), (d) is printed and stored with the result.

--ema times the weight average (ema_decay, parallel.py: one svol_ema_flat launch per bucket behind the update, 12 B / parameter),
same protocol, six rows: flat AdamW, flat Adam and flat SGD without an average (the rows of the plain run) and each with
ema_decay=0.999.  Printed besides: the time the average adds per step and the bytes/s of that added time at 12 B / parameter.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

HBM_PEAK = 8.0e12       # bytes/s, spec
HBM_COPY = 6.29e12      # bytes/s, measured float4 copy


def shader_clock(dev, opt, steps):
    """The shader clock the chip holds under `steps` more (untimed) steps of `opt`: bench.py's probe (csrc/clock_probe.hip), one wave on
    a stream of its own sampling shader-clock ticks against the constant wall counter in 200 us windows."""
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
            opt.step()
    finally:
        stop.fill_(1)            # stream-ordered behind the steps: the probe leaves at its next window
        torch.cuda.synchronize()
    n = int(count.item())
    if n < 8:
        return None
    w = samples[:2 * n].view(n, 2).cpu().double()
    ghz = (w[:, 0] / w[:, 1] * (khz.value / 1e6)).sort().values
    pick = lambda q: round(float(ghz[min(n - 1, int(q * n))]), 3)
    return {'p10': pick(0.1), 'median': pick(0.5), 'p90': pick(0.9), 'windows': n, 'window_us': 200}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--block', type=int, default=100)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--clip', action='store_true', help='time the clipped step: rows (a) to (e) of the module docstring')
    ap.add_argument('--groups', action='store_true', help='time the grouped / capturable step: rows (a) to (e) of the module docstring')
    ap.add_argument('--ema', action='store_true', help='time the weight average: the three flat optimizers without and with ema_decay')
    a = ap.parse_args()
    assert a.clip + a.groups + a.ema <= 1, '--clip, --groups or --ema'
    assert a.block * a.blocks >= 500, 'at least 500 timed steps per optimizer'
    from svol_amd import parallel
    from svol_amd import synthetic as syn
    from svol_amd.modeling.svanet import build_svanet
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    args = syn.cfg2_args('video_matcher')
    args.compute_dtype = 'bf16'
    torch.manual_seed(1)
    model = build_svanet(args).to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    reducer = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
    kw = dict(lr=1e-4, weight_decay=1e-4, params=params)
    live = [p for b in reducer.buckets for p in b['params']]     # (the torch optimizers skip a parameter without .grad anyway)
    if a.clip:
        # the gradients below have norm 1e-3 * sqrt(19.1e6) = 4.4: max_grad_norm 1 clips every step.  The scalers never grow
        # (growth_interval past the run), so (b) and (d) do the same work every step.
        scaler = lambda: parallel.DynamicLossScaler(dev, init_scale=1.0, growth_interval=10 ** 9)
        opts = {'(a) flat AdamW': parallel.FlatAdamW(reducer, **kw), '(b) flat AdamW + scaler': parallel.FlatAdamW(reducer, **kw),
                '(c) clipped AdamW': parallel.FlatAdamW(reducer, max_grad_norm=1.0, **kw),
                '(d) clipped AdamW + scaler': parallel.FlatAdamW(reducer, max_grad_norm=1.0, **kw)}
        opts['(b) flat AdamW + scaler'].scaler = scaler()
        opts['(d) clipped AdamW + scaler'].scaler = scaler()

        class ClipThenStep:     # what INTEGRATION.md used to advise: ~150 gradient views through torch's multi-tensor norm and scale
            def __init__(self, opt):
                self.flat = opt.flat
                self.opt = opt

            def step(self):
                torch.nn.utils.clip_grad_norm_(live, 1.0)
                self.opt.step()
        opts['(e) clip_grad_norm_ + flat AdamW'] = ClipThenStep(parallel.FlatAdamW(reducer, **kw))
        bytes_per = {k: 28 if k.startswith('(a)') else 32 for k in opts}   # one more read of the gradient ((e): the same minimum)
        probed = list(opts)[:4]
    elif a.groups:
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        late = lambda n: any(t in n for t in parallel._LATE + ('layers.0.',))   # (a boundary inside a bucket, not only between buckets)
        split = {'(c) two groups, contiguous': [[p for n, p in named if late(n)], [p for n, p in named if not late(n)]],
                 '(d) two groups, alternating': [[p for _, p in named if p.dim() >= 2], [p for _, p in named if p.dim() < 2]]}
        assert all(len(g) > 0 for gs in split.values() for g in gs)
        gkw = dict(lr=1e-4, weight_decay=1e-4)
        opts = {'(a) flat AdamW': parallel.FlatAdamW(reducer, **kw),
                '(b) grouped, one group': parallel.FlatAdamW(reducer, capturable=True, **kw)}
        for k, (g0, g1) in split.items():     # group 1 at 10x the lr and without decay: the rows differ, the work does not
            opts[k] = parallel.FlatAdamW(reducer, params=[{'params': g0}, {'params': g1, 'lr': 1e-3, 'weight_decay': 0.0}], **gkw)
        runs = {k: [len(e) for e, _ in o.seg_tables] for k, o in opts.items() if getattr(o, '_grouped', False)}
        opts['(e) torch AdamW fused capturable'] = torch.optim.AdamW(live, lr=1e-4, weight_decay=1e-4, fused=True, capturable=True)
        bytes_per = {k: 28 for k in opts}
        probed = list(opts)[:4]
    elif a.ema:
        mk = {'flat AdamW': lambda **e: parallel.FlatAdamW(reducer, **kw, **e), 'flat Adam': lambda **e: parallel.FlatAdam(reducer, **kw, **e),
              'flat SGD': lambda **e: parallel.FlatSGD(reducer, momentum=0.9, **kw, **e)}
        opts, bytes_per = {}, {}
        for k, f in mk.items():     # (off and on next to each other in the turn order)
            opts[k], opts[k + ' + ema'] = f(), f(ema_decay=0.999)
            bytes_per[k] = 20 if 'SGD' in k else 28
            bytes_per[k + ' + ema'] = bytes_per[k] + 12
        assert all(('ema' in st) == k.endswith('+ ema') for k, o in opts.items() for st in o.flat)
        probed = list(opts)
    else:
        opts = {'flat AdamW': parallel.FlatAdamW(reducer, **kw), 'flat Adam': parallel.FlatAdam(reducer, **kw),
                'flat SGD': parallel.FlatSGD(reducer, momentum=0.9, **kw)}
        opts['torch Adam'] = torch.optim.Adam(live, lr=1e-4, weight_decay=1e-4)
        opts['torch SGD'] = torch.optim.SGD(live, lr=1e-4, momentum=0.9, weight_decay=1e-4)
        bytes_per = {'flat AdamW': 28, 'flat Adam': 28, 'flat SGD': 20, 'torch Adam': 28, 'torch SGD': 20}   # (torch: the same minimum)
        probed = ['flat AdamW', 'flat Adam', 'flat SGD']
    n_flat = sum(b['flat'].numel() for b in reducer.buckets)
    gen = torch.Generator(device=dev).manual_seed(7)
    for b in reducer.buckets:
        b['flat'].copy_(torch.randn(b['flat'].numel(), device=dev, generator=gen) * 1e-3)
    for o in opts.values():
        for _ in range(a.warmup):
            o.step()
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.reps):
        spans = {k: [] for k in opts}
        for _ in range(a.blocks):
            for name, o in opts.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.block):
                    o.step()
                e1.record()
                spans[name].append((e0, e1))
        torch.cuda.synchronize()
        reps.append({k: sum(e0.elapsed_time(e1) for e0, e1 in v) / (a.block * a.blocks) for k, v in spans.items()})
    sclk = {k: shader_clock(dev, opts[k], a.block * a.blocks) for k in probed}
    assert all(bool(torch.isfinite(st['p']).all()) for o in opts.values() if hasattr(o, 'flat') for st in o.flat)
    if a.clip:
        norms = {k: float(o.grad_norm) for k, o in opts.items() if getattr(o, 'grad_norm', None) is not None}
        print('grad_norm after the run:', norms)
    res = {'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__, 'parameters': sum(p.numel() for p in live),
           'flat_floats': n_flat, 'buckets': len(reducer.buckets), 'steps_per_rep': a.block * a.blocks, 'reps': a.reps,
           'argv': ' '.join(sys.argv[1:]), 'sclk_ghz': sclk, 'rows': {}}
    if a.groups:
        res['runs_per_bucket'] = runs
        assert all(o.steps_taken() == opts['(a) flat AdamW'].steps_taken() for k, o in opts.items() if k in runs)
        for k, r in runs.items():
            print(f'runs per bucket, {k}: {r}')
    print(f'{res["device"]}: {res["parameters"]} parameters in {res["buckets"]} buckets ({n_flat * 4 / 2 ** 20:.1f} MiB flat), '
          f'{a.reps} x {a.block * a.blocks} steps each')
    wid = max(12, max(len(k) for k in opts))
    print(f'{"":{wid}s} {"ms/step (reps)":28s} {"median":>8s} {"spread":>8s} {"B/param":>8s} {"TB/s":>7s} {"of 8.0":>7s} {"of 6.29":>8s}')
    for k in opts:
        ms = [r[k] for r in reps]
        med = statistics.median(ms)
        bw = bytes_per[k] * n_flat / (med * 1e-3)
        res['rows'][k] = {'ms_per_step': ms, 'median_ms': med, 'spread_ms': max(ms) - min(ms), 'bytes_per_param': bytes_per[k],
                          'bytes_per_s': bw, 'share_of_hbm_peak': bw / HBM_PEAK, 'share_of_hbm_copy': bw / HBM_COPY}
        print(f'{k:{wid}s} {" ".join(f"{x:.4f}" for x in ms):28s} {med:8.4f} {max(ms) - min(ms):8.4f} {bytes_per[k]:8d} {bw / 1e12:7.2f} '
              f'{bw / HBM_PEAK:7.1%} {bw / HBM_COPY:8.1%}')
    if a.ema:
        res['ema_added'] = {}
        for k in [k for k in opts if not k.endswith('+ ema')]:
            add = res['rows'][k + ' + ema']['median_ms'] - res['rows'][k]['median_ms']
            bw = 12 * n_flat / (add * 1e-3) if add > 0 else float('inf')
            res['ema_added'][k] = {'added_ms': add, 'bytes_per_s': bw, 'share_of_hbm_copy': bw / HBM_COPY}
            print(f'{k}: the average adds {add:.4f} ms per step = {bw / 1e12:.2f} TB/s at 12 B / parameter ({bw / HBM_COPY:.1%} of 6.29)')
    for k, c in sclk.items():
        print(f'shader clock under {k}: ' + (f'{c["median"]:.3f} GHz median (p10 {c["p10"]:.3f}, p90 {c["p90"]:.3f}, {c["windows"]} windows '
                                             f'of {c["window_us"]} us)' if c else 'not sampled'))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
