"""Data-parallel gradient exchange on the real device: two ranks share the one MI355X of the test box (gloo backend,
the functional stand-in for RCCL, which needs one GPU per rank) and run the product model with
BucketedGradAllReduce; see tests/dp_gpu_worker.py for what is asserted."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize('case', ['small', 'full'])
def test_two_ranks_on_one_gpu(case):
    """small: fp32 toy model, 64 KiB buckets.  full: the benchmark's model (L = 6272, 6 layers, bf16, 16 MiB buckets, B = 8 per
    rank) — the GPU lags the host and a bucket boundary falls inside a query half (the all-reduce launched from a
    side-stream hook must also wait for the main stream)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', SVOL_DP_CASE=case)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(HERE, 'dp_gpu_worker.py')]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.count('reducer == mean of per-rank gradients') == 2, p.stdout[-2000:]


def test_sync_bn_two_ranks_equal_the_global_batch():
    """--sync_bn (train.py:65-68: apex convert_syncbn_model) on the trainable ResNet extractor: two ranks with half a batch each
    give the statistics, features and (summed) gradients of one process on the whole batch; without the flag they do not
    (tests/syncbn_gpu_worker.py).  ADVICE r5: the flag used to be parsed and ignored."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(HERE, 'syncbn_gpu_worker.py')]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.count('sync_bn == one process on the global batch') == 2, p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


def test_rccl_world1_forced_allreduce():
    """the RCCL path executes.  One rank, backend nccl, SVOL_FORCE_ALLREDUCE=1: every bucket of the full cfg2 step is
    all-reduced by RCCL on the communication stream behind the producer-stream waits (tests/rccl_world1_worker.py); gradients equal the
    un-reduced run, buckets complete in order, no deadlock with the weight-gradient gate (the worker runs under a timeout)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', SVOL_PORT=str(_free_port()))
    p = subprocess.run([sys.executable, os.path.join(HERE, 'rccl_world1_worker.py')], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert 'rccl world-1:' in p.stdout and 'all-reduced on the communication stream' in p.stdout, p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


def test_bench_reports_allreduce_spans_with_rccl_at_world1():
    """bench.py under SVOL_FORCE_ALLREDUCE=1: a 1-rank RCCL communicator, `allreduce_exposed_ms` and the per-bucket spans in the line."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', SVOL_FORCE_ALLREDUCE='1')
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), 'bench.py'), '--steps', '4', '--warmup', '2', '--no-cpu-baseline'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line['allreduce_backend'].startswith('nccl') and line['allreduce_exposed_ms'] >= 0.0
    assert len(line['allreduce_buckets']) >= 4 and all(b['ms'] > 0 for b in line['allreduce_buckets']), line['allreduce_buckets']


def test_bench_hides_a_collective_that_costs_time_behind_backward():
    """rehearse, on ONE GPU, an all-reduce that takes time.  SVOL_FORCE_ALLREDUCE=1 runs every bucket through a
    one-rank RCCL communicator; SVOL_ALLREDUCE_SPIN=ring follows each collective with a spin kernel of the exchange's modelled
    8-rank xGMI duration (ring: 2 (7/8) bytes / 153 GB/s — 0.19 ms for a 16 MiB bucket, 0.89 ms for the step's 74 MiB).  Asserted: the
    buckets fire in arrival order (0, 1, 2, ...), every bucket but the last is hidden behind backward — the step grows by no more
    than the LAST bucket's span (+ noise) although the exchange as a whole is several times longer —, and finish() waits about that
    last span."""
    import json
    bench = os.path.join(os.path.dirname(HERE), 'bench.py')
    lines = {}
    for spin in (None, 'ring'):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', SVOL_FORCE_ALLREDUCE='1')
        if spin:
            env['SVOL_ALLREDUCE_SPIN'] = spin
        p = subprocess.run([sys.executable, bench, '--steps', '10', '--warmup', '4', '--blocks', '3', '--no-cpu-baseline'], env=env,
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        lines[spin] = json.loads(p.stdout.strip().splitlines()[-1])
    base, spun = lines[None], lines['ring']
    bk = spun['allreduce_buckets']
    assert spun['allreduce_launch_order'] == list(range(len(bk))) and len(bk) >= 4
    total = sum(b['ms'] for b in bk)
    last = bk[-1]['ms']
    assert all(abs(b['ms'] - m) <= 0.25 * m + 0.05 for b, m in zip(bk, spun['allreduce_modelled_ms'])), (bk, spun['allreduce_modelled_ms'])
    growth = spun['ms_per_step'] - base['ms_per_step']
    print(f'spin rehearsal: exchange {total:.2f} ms in {len(bk)} buckets (last {last:.3f} ms), step {base["ms_per_step"]:.2f} -> '
          f'{spun["ms_per_step"]:.2f} ms (+{growth:.2f}), exposed in finish() {spun["allreduce_exposed_ms"]:.3f} ms')
    assert total > 0.6
    assert growth <= last + 0.25, (growth, last)               # (0.25 ms: run-to-run noise of two bench processes on one box)
    assert spun['allreduce_exposed_ms'] <= last + 0.1


@pytest.mark.gpu
def test_flat_adamw_matches_torch_adamw():
    """svol_amd.parallel.FlatAdamW (one kernel per gradient bucket) against torch.optim.AdamW on the same gradients, 4 steps;
    a parameter the reducer skips stays untouched, a bucket boundary falls inside the list."""
    import torch
    from svol_amd import parallel
    torch.manual_seed(0)
    shapes = [(64, 33), (33,), (7,), (128, 128), (5, 3, 2), (1,)]
    pa = [torch.nn.Parameter(torch.randn(s, device='cuda')) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    skip = [pa[2]]
    red = parallel.BucketedGradAllReduce(pa, bucket_bytes=40000, skip=skip)
    opt_a = parallel.FlatAdamW(red, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    opt_b = torch.optim.AdamW([p for i, p in enumerate(pb) if i != 2], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    for step in range(4):
        red.zero_grad()
        opt_b.zero_grad()
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i == 2:
                continue
            g = torch.randn(a.shape, device='cuda') * (1.0 + step)
            a.grad.copy_(g)
            b.grad = g.clone()
        opt_a.step()
        opt_b.step()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert float((a.detach() - b.detach()).abs().max()) <= 2e-6 * max(1.0, float(b.detach().abs().max())), i
    assert torch.equal(pa[2].detach(), pb[2].detach())


@pytest.mark.gpu
def test_dynamic_loss_scaler_skips_overflowed_steps_and_follows_torch_adamw():
    """fp16 training used a static loss scale and never checked for overflow — one inf gradient went straight into p, m and
    v.  DynamicLossScaler (apex-amp semantics, state on the device): gradients arrive multiplied by the scale; a clean step equals
    torch.optim.AdamW on the unscaled gradients; a step with an inf / NaN anywhere in any bucket changes NOTHING (parameters, both
    moments, the bias-correction step count) and halves the scale; the scale grows after `growth_interval` clean steps."""
    import torch
    from svol_amd import parallel
    torch.manual_seed(0)
    shapes = [(64, 33), (33,), (128, 128), (5, 3, 2), (1,)]
    pa = [torch.nn.Parameter(torch.randn(s, device='cuda')) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    red = parallel.BucketedGradAllReduce(pa, bucket_bytes=40000)
    assert len(red.buckets) >= 2
    opt_a = parallel.FlatAdamW(red, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    sc = opt_a.scaler = parallel.DynamicLossScaler(torch.device('cuda'), init_scale=1024.0, growth_interval=3)
    opt_b = torch.optim.AdamW(pb, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    scale = 1024.0
    clean_run = 0
    for step in range(9):
        red.zero_grad()
        opt_b.zero_grad()
        overflow = step in (2, 6)
        gs = [torch.randn(a.shape, device='cuda') * (1.0 + step) for a in pa]
        for i, (a, g) in enumerate(zip(pa, gs)):
            a.grad.copy_(g * scale)                      # what backward of (loss * scale) leaves in the buckets
        if overflow:
            pa[3].grad.view(-1)[7] = float('inf') if step == 2 else float('nan')
        before = [p.detach().clone() for p in pa]
        mom = [(st['m'].clone(), st['v'].clone()) for st in opt_a.flat]
        opt_a.step()
        torch.cuda.synchronize()
        st_host = sc.state.tolist()
        if overflow:
            assert all(torch.equal(a, b) for a, b in zip(before, pa))
            assert all(torch.equal(m, st['m']) and torch.equal(v, st['v']) for (m, v), st in zip(mom, opt_a.flat))
            scale *= 0.5
            clean_run = 0
        else:
            for b, g in zip(pb, gs):
                b.grad = g.clone()
            opt_b.step()
            clean_run += 1
            if clean_run == 3:
                scale *= 2.0
                clean_run = 0
            for a, b in zip(pa, pb):
                assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max())), (step, float((a - b).abs().max()))
        assert st_host[0] == scale and st_host[1] == 0.0, (step, st_host, scale)
    assert sc.state.tolist()[3] == 7.0                  # 9 calls, 2 skipped
    sd = sc.state_dict()
    assert sd['loss_scaler0']['loss_scale'] == scale
    sc2 = parallel.DynamicLossScaler(torch.device('cuda'))
    sc2.load_state_dict(sd)
    assert sc2.state.tolist()[0] == scale


@pytest.mark.gpu
@pytest.mark.parametrize('attach_first', [True, False])
def test_scaled_adamw_resume_keeps_the_bias_correction_step(attach_first):
    """with a DynamicLossScaler the bias-correction step count lives on the device (scaler.state[3]) and was neither saved
    nor restored — a resumed fp16 run restarted it at 1 under warm moments (bc1 = 0.1, bc2 = 0.001: updates ~0.3x mis-scaled).
    An uninterrupted run of 8 steps (step 2 overflows and is skipped) must equal 4 steps + state_dict -> fresh optimizer + scaler ->
    load_state_dict -> 4 more steps, bit for bit, whichever of {attach the scaler, load the state} happens first; and the saved
    'step' is the count of updates TAKEN (3 after four calls with one skip), which is what torch / apex write."""
    import torch
    from svol_amd import parallel
    shapes = [(64, 33), (33,), (128, 128), (5, 3, 2), (1,)]
    dev = torch.device('cuda')

    def grads(step, scale):
        g = torch.Generator(device='cuda').manual_seed(500 + step)
        out = [torch.randn(s, device='cuda', generator=g) * (1.0 + step) * scale for s in shapes]
        if step == 2:
            out[1][5] = float('inf')
        return out

    def make(src):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in src]
        red = parallel.BucketedGradAllReduce(ps, bucket_bytes=40000)
        opt = parallel.FlatAdamW(red, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, params=ps)
        return ps, red, opt

    def run(ps, red, opt, steps):
        for st in steps:
            red.zero_grad()
            scale = float(opt.scaler.state[0].item())
            for p, g in zip(ps, grads(st, scale)):
                p.grad.copy_(g)
            opt.step()
        torch.cuda.synchronize()

    torch.manual_seed(3)
    p0 = [torch.randn(s, device='cuda') for s in shapes]
    pa, ra, oa = make(p0)
    oa.scaler = parallel.DynamicLossScaler(dev, init_scale=256.0, growth_interval=1000)
    run(pa, ra, oa, range(8))
    assert oa.steps_taken() == 7

    pb, rb, ob = make(p0)
    ob.scaler = parallel.DynamicLossScaler(dev, init_scale=256.0, growth_interval=1000)
    run(pb, rb, ob, range(4))
    sd_opt, sd_amp = ob.state_dict(), ob.scaler.state_dict()
    assert {int(float(e['step'])) for e in sd_opt['state'].values()} == {3}   # four calls, one skipped
    pc, rc, oc = make([p.detach() for p in pb])
    sc = parallel.DynamicLossScaler(dev)
    sc.load_state_dict(sd_amp)
    if attach_first:
        oc.scaler = sc
        oc.load_state_dict(sd_opt)
    else:
        oc.load_state_dict(sd_opt)
        oc.scaler = sc
    assert oc.steps_taken() == 3
    run(pc, rc, oc, range(4, 8))
    assert oc.steps_taken() == 7
    for a, c in zip(pa, pc):
        assert torch.equal(a.detach(), c.detach())


@pytest.mark.gpu
def test_flat_adamw_checkpoints_interoperate_with_torch_adamw():
    """FlatAdamW speaks torch.optim.AdamW's state-dict schema.  torch AdamW, 2 steps -> state_dict ->
    FlatAdamW.load_state_dict -> 2 more steps on both == same weights; and back: FlatAdamW.state_dict() resumes a fresh
    torch AdamW.  The parameter list is in the reference's order (every trainable parameter, train.py:72), one of them never
    gets a gradient (no state entry), and a StepLR drives both."""
    import torch
    from svol_amd import parallel
    torch.manual_seed(1)
    shapes = [(64, 33), (33,), (7,), (128, 128), (5, 3, 2), (1,)]
    dead = 2
    mk = lambda src: [torch.nn.Parameter(p.detach().clone()) for p in src]
    p0 = [torch.nn.Parameter(torch.randn(s, device='cuda')) for s in shapes]
    kw = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)

    def grads(step):
        g = torch.Generator(device='cuda').manual_seed(100 + step)
        return [torch.randn(s, device='cuda', generator=g) * (1.0 + step) for s in shapes]

    def torch_steps(params, opt, sched, steps):
        for st in steps:
            opt.zero_grad()
            for i, (p, g) in enumerate(zip(params, grads(st))):
                if i != dead:
                    p.grad = g.clone()
            opt.step()
            sched.step()

    def flat_steps(params, red, opt, sched, steps):
        for st in steps:
            opt.zero_grad()
            for i, (p, g) in enumerate(zip(params, grads(st))):
                if i != dead:
                    p.grad.copy_(g)
            opt.step()
            sched.step()

    # reference run: torch AdamW for 4 steps
    pr = mk(p0)
    o_r = torch.optim.AdamW(pr, **kw)
    s_r = torch.optim.lr_scheduler.StepLR(o_r, step_size=3, gamma=0.5)
    torch_steps(pr, o_r, s_r, range(4))

    # torch (2 steps) -> FlatAdamW (2 steps)
    pa = mk(p0)
    o_a = torch.optim.AdamW(pa, **kw)
    s_a = torch.optim.lr_scheduler.StepLR(o_a, step_size=3, gamma=0.5)
    torch_steps(pa, o_a, s_a, range(2))
    sd_opt, sd_sched = o_a.state_dict(), s_a.state_dict()
    assert dead not in sd_opt['state'] and len(sd_opt['state']) == len(shapes) - 1
    pb = mk(pa)
    red = parallel.BucketedGradAllReduce(pb, bucket_bytes=40000, skip=[pb[dead]])
    o_b = parallel.FlatAdamW(red, params=pb, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0)  # all overwritten by the load
    s_b = torch.optim.lr_scheduler.StepLR(o_b, step_size=3, gamma=0.5)
    o_b.load_state_dict(sd_opt)
    s_b.load_state_dict(sd_sched)
    assert o_b.t == 2 and o_b.betas == (0.9, 0.99) and o_b.weight_decay == 0.05
    flat_steps(pb, red, o_b, s_b, range(2, 4))
    for i, (a, b) in enumerate(zip(pb, pr)):
        assert float((a.detach() - b.detach()).abs().max()) <= 2e-6 * max(1.0, float(b.detach().abs().max())), i
    assert abs(o_b.lr - o_r.param_groups[0]['lr']) < 1e-12 and o_b.lr == 1.5e-3   # StepLR halved it after step 3

    # FlatAdamW state -> fresh torch AdamW, one more step on both
    sd_b = o_b.state_dict()
    assert sorted(sd_b['state']) == [i for i in range(len(shapes)) if i != dead]
    assert sd_b['param_groups'][0]['params'] == list(range(len(shapes)))
    pc = mk(pb)
    o_c = torch.optim.AdamW(pc, **kw)
    o_c.load_state_dict(sd_b)
    s_c = torch.optim.lr_scheduler.StepLR(o_c, step_size=3, gamma=0.5)
    s_c.load_state_dict(s_b.state_dict())
    torch_steps(pc, o_c, s_c, [4])
    torch_steps(pr, o_r, s_r, [4])
    for i, (a, b) in enumerate(zip(pc, pr)):
        assert float((a.detach() - b.detach()).abs().max()) <= 4e-6 * max(1.0, float(b.detach().abs().max())), i

    # a state dict that does not fit is refused, not silently mis-aligned
    bad = o_a.state_dict()
    bad['state'][0]['exp_avg'] = bad['state'][0]['exp_avg'][:10]
    with pytest.raises(ValueError):
        o_b.load_state_dict(bad)


@pytest.mark.gpu
def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: the parent starts the ranks itself before
    touching the GPU, rank 0 prints the one JSON line with the rank count the communicator really had, a failing child makes
    the parent fail.  gloo lets both ranks share the test box's single card (RCCL wants one GPU per rank)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY='0', SVOL_DIST_BACKEND='gloo')
    root = os.path.dirname(HERE)
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
                        '--no-cpu-baseline'], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l_ for l_ in p.stdout.splitlines() if l_.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res['n_gpus'] == 2 and res['n_ranks_seen'] == 2 and res['config']['global_batch'] == 16
    assert res['value'] > 0 and res['scaling'] == 'weak' and res['dist_backend'] == 'gloo'
    # a failing child (a batch size no rank can build) must fail the parent too
    q = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--batch', '-1'], env=env,
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert q.returncode != 0


def test_bench_world4_gloo_rehearsal_reports_per_rank_issue_time():
    """the N > 1 bench path rehearsed at world 4 with the FULL cfg2 model on the one card (gloo; RCCL wants one GPU
    per rank): every rank pins itself to its own slice of the host cores and rank 0 reports each rank's host issue time — at N = 8
    eight Python issuers share one host, and whether they keep their GPUs fed is what decides the scaling curve."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY='0', SVOL_DIST_BACKEND='gloo')
    root = os.path.dirname(HERE)
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '4', '--steps', '2', '--warmup', '1',
                        '--full', '--no-cpu-baseline'], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l_ for l_ in p.stdout.splitlines() if l_.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res['n_gpus'] == 4 and res['n_ranks_seen'] == 4 and res['config']['global_batch'] == 32
    assert len(res['host_issue_ms_per_rank']) == 4 and all(0 < x < 1000 for x in res['host_issue_ms_per_rank'])
    assert res['host_cores_per_rank'] >= 1
    print('world-4 gloo rehearsal: ms/step', res['ms_per_step'], 'issue per rank', res['host_issue_ms_per_rank'],
          'cores per rank', res['host_cores_per_rank'])


@pytest.mark.gpu
def test_step_fence_bounds_the_host_run_ahead():
    """parallel.StepFence: after tick() at most ``max_inflight`` steps are unfinished on the device (profiles/round3_summary.md, "host
    run-ahead": the unfenced loop stalled 1 s in hipMalloc).  A spin kernel of ~20 ms per step stands in for the training step."""
    import time
    import torch
    from svol_amd import parallel
    x = torch.randn(8192, 8192, device='cuda')
    torch.cuda.synchronize()
    t0 = time.perf_counter(); (x @ x); torch.cuda.synchronize(); one = time.perf_counter() - t0
    fence = parallel.StepFence(2)
    evs = []
    for i in range(8):
        for _ in range(3):
            x @ x
        e = torch.cuda.Event(); e.record(); evs.append(e)
        fence.tick()
        # everything older than the two newest steps has finished when tick() returns
        assert all(ev.query() for ev in evs[:-2]), i
    assert len(fence._q) == 2
    fence.drain()
    assert not fence._q and all(ev.query() for ev in evs) and one > 0
