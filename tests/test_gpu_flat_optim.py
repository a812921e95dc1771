"""parallel.FlatSGD / parallel.FlatAdam on the device (the reference's --optimizer sgd | adam, train.py:94-97): parity with
torch.optim.SGD / torch.optim.Adam, the zeroing and issued-during-backward variants, dynamic loss scaling, checkpoints both ways,
two ranks on one GPU, and a short training run through parallel.build_optimizer.

The parity bar is the project's own for this comparison (tests/test_gpu_parallel.py): max|a - b| <= 2e-6 * max(1, max|b|), and 4e-6
after a checkpoint round trip plus further steps.  On these shapes with lr 3e-3, wd 0.05 and gradient scale 1 + step, torch's own fp32
SGD and Adam (foreach and single-tensor) stay within 2.3e-7 of an fp64 run over 8 steps, so two correct fp32 implementations have
about 4x headroom under it."""
import argparse
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# the shapes of test_flat_adamw_matches_torch_adamw; (5, 3, 2) and (33,) end a bucket with numel % 4 != 0.  The reducer pads every
# tensor to a 16-byte boundary, so a bucket's flat length is always a multiple of 4 and the classes never reach the kernels' scalar
# tail: test_update_kernels_stay_inside_their_ranges runs it through the C entries (n % 4 = 1, 2, 3) against fp64 arithmetic.
SHAPES = [(64, 33), (33,), (7,), (128, 128), (5, 3, 2), (1,)]
DEAD = 2
KW = {'sgd': dict(lr=3e-3, momentum=0.9, weight_decay=0.05), 'sgd0': dict(lr=3e-3, momentum=0.0, weight_decay=0.05),
      'adam': dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)}


def _classes(kind):
    from svol_amd import parallel
    return (parallel.FlatAdam, torch.optim.Adam) if kind == 'adam' else (parallel.FlatSGD, torch.optim.SGD)


def _close(a, b, bar, what):
    err, ref = float((a.detach() - b.detach()).abs().max()), max(1.0, float(b.detach().abs().max()))
    print(f'{what}: max|a-b| = {err:.3e} (bar {bar * ref:.3e})')
    assert err <= bar * ref, (what, err, bar * ref)


def _grads(step, seed=100, scale=1.0):
    g = torch.Generator(device='cuda').manual_seed(seed + step)
    return [torch.randn(s, device='cuda', generator=g) * (1.0 + step) * scale for s in SHAPES]


def _mk(src):
    return [torch.nn.Parameter(p.detach().clone()) for p in src]


def _p0(seed=0):
    torch.manual_seed(seed)
    return [torch.randn(s, device='cuda') for s in SHAPES]


def _flat(kind, src, skip_dead=True, **kw):
    from svol_amd import parallel
    ps = _mk(src)
    red = parallel.BucketedGradAllReduce(ps, bucket_bytes=40000, skip=[ps[DEAD]] if skip_dead else None)
    assert len(red.buckets) >= 2
    return ps, red, _classes(kind)[0](red, params=ps, **dict(KW[kind], **kw))


def _flat_steps(ps, red, opt, steps, sched=None, **gkw):
    for st in steps:
        opt.zero_grad()
        for i, (p, g) in enumerate(zip(ps, _grads(st, **gkw))):
            if i != DEAD:
                p.grad.copy_(g)
        opt.step()
        if sched is not None:
            sched.step()


def _torch_steps(ps, opt, steps, sched=None, **gkw):
    for st in steps:
        opt.zero_grad()
        for i, (p, g) in enumerate(zip(ps, _grads(st, **gkw))):
            if i != DEAD:
                p.grad = g.clone()
        opt.step()
        if sched is not None:
            sched.step()


@pytest.mark.parametrize('kind', ['sgd', 'sgd0', 'adam'])
def test_flat_optimizer_matches_torch(kind):
    """5 steps on identical gradients; a bucket boundary falls inside the list, a parameter the reducer skips stays untouched."""
    p0 = _p0()
    pa, red, oa = _flat(kind, p0)
    pb = _mk(p0)
    ob = _classes(kind)[1]([p for i, p in enumerate(pb) if i != DEAD], **KW[kind])
    _flat_steps(pa, red, oa, range(5))
    _torch_steps(pb, ob, range(5))
    for i, (a, b) in enumerate(zip(pa, pb)):
        _close(a, b, 2e-6, f'{kind} parameter {i}')
    assert torch.equal(pa[DEAD].detach(), p0[DEAD])
    if kind == 'sgd0':      # plain SGD: torch keeps no buffer and writes no state
        assert oa.state_dict()['state'] == {} == ob.state_dict()['state']


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_flat_checkpoints_interoperate_with_torch(kind):
    """torch, 2 steps -> state_dict -> flat.load_state_dict -> 2 more steps on both == the same weights; and back: what the flat class
    writes resumes a fresh torch optimizer.  The parameter list is in the reference's order with one dead parameter; a StepLR drives both."""
    Flat, Torch = _classes(kind)
    p0 = _p0(1)
    pr = _mk(p0)
    o_r = Torch(pr, **KW[kind])
    s_r = torch.optim.lr_scheduler.StepLR(o_r, step_size=3, gamma=0.5)
    _torch_steps(pr, o_r, range(4), s_r)

    pa = _mk(p0)
    o_a = Torch(pa, **KW[kind])
    s_a = torch.optim.lr_scheduler.StepLR(o_a, step_size=3, gamma=0.5)
    _torch_steps(pa, o_a, range(2), s_a)
    sd_opt, sd_sched = o_a.state_dict(), s_a.state_dict()
    assert DEAD not in sd_opt['state'] and len(sd_opt['state']) == len(SHAPES) - 1
    other = dict(lr=1.0, momentum=0.5, weight_decay=0.0) if kind == 'sgd' else dict(lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0)
    pb, red, o_b = _flat(kind, pa, **other)                 # all overwritten by the load
    s_b = torch.optim.lr_scheduler.StepLR(o_b, step_size=3, gamma=0.5)
    o_b.load_state_dict(sd_opt)
    s_b.load_state_dict(sd_sched)
    assert all(o_b.param_groups[0][k] == v for k, v in KW[kind].items())
    _flat_steps(pb, red, o_b, range(2, 4), s_b)
    for i, (a, b) in enumerate(zip(pb, pr)):
        _close(a, b, 2e-6, f'{kind} torch -> flat, parameter {i}')
    assert o_b.lr == 1.5e-3 == o_r.param_groups[0]['lr']    # StepLR halved it after step 3

    sd_b = o_b.state_dict()
    assert sorted(sd_b['state']) == [i for i in range(len(SHAPES)) if i != DEAD]
    assert all(set(e) == ({'momentum_buffer'} if kind == 'sgd' else {'step', 'exp_avg', 'exp_avg_sq'}) for e in sd_b['state'].values())
    pc = _mk(pb)
    o_c = Torch(pc, **KW[kind])
    o_c.load_state_dict(sd_b)
    s_c = torch.optim.lr_scheduler.StepLR(o_c, step_size=3, gamma=0.5)
    s_c.load_state_dict(s_b.state_dict())
    _torch_steps(pc, o_c, [4], s_c)
    _torch_steps(pr, o_r, [4], s_r)
    for i, (a, b) in enumerate(zip(pc, pr)):
        _close(a, b, 4e-6, f'{kind} flat -> torch, parameter {i}')


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_zero_grads_changes_nothing_and_leaves_clean_buckets(kind):
    p0 = _p0(2)
    pa, ra, oa = _flat(kind, p0)
    pz, rz, oz = _flat(kind, p0, zero_grads=True)
    for st in range(4):
        _flat_steps(pa, ra, oa, [st])
        _flat_steps(pz, rz, oz, [st])
        assert all(bool((b['flat'] == 0).all()) and b.get('clean') for b in rz.buckets), st
        assert any(bool((b['flat'] != 0).any()) for b in ra.buckets)
    for a, z in zip(pa, pz):
        assert torch.equal(a.detach(), z.detach())
    for sa, sz in zip(oa.flat, oz.flat):
        assert all(torch.equal(sa[k], sz[k]) for k in sa)


@pytest.mark.parametrize('n', [4096 + 3, 1024, 2, 4 * 256 * 3 + 1])
def test_update_kernels_stay_inside_their_ranges(n):
    """Every entry over ranges carved out of one arena of -0.0 words (tests/test_gpu_guards.py): the words in front of and behind each
    range come back bit-identical, the zeroing entries equal the plain ones bit for bit and leave the gradient range all zero, and
    a scaled entry writes nothing on an overflowed step.  n % 4 != 0 runs the scalar tail; the result is held against the update
    written out in fp64 at the parity bar."""
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    from tests.test_gpu_guards import GuardArena
    L = _lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(n)
    src = {k: torch.randn(n, device='cuda', generator=gen) for k in ('p', 'g', 'a', 'b')}
    src['b'] = src['b'].abs()

    def arena():
        ar = GuardArena(guard_bytes=1 << 12)
        for k in ('p', 'g', 'a', 'b', 'state'):
            ar.plan(k, (4,) if k == 'state' else (n,), torch.float32)
        t = ar.build()
        for k in src:
            t[k].copy_(src[k])
        return ar, t

    def run(name, overflow=False):
        ar, t = arena()
        t['state'].copy_(torch.tensor([4.0, 1.0 if overflow else 0.0, 0.0, 2.0]))
        sgd = 'sgd' in name
        args = [_ptr(t['p']), _ptr(t['g']), _ptr(t['a'])] + ([] if sgd else [_ptr(t['b'])]) + [n, 3e-3]
        args += [0.9, 0.05] if sgd else [0.9, 0.999, 1e-8, 0.05]
        if name.endswith('_scaled'):
            args += [4.0, _ptr(t['state'])]          # gradient factor 4 / scale 4
        else:
            args += ([] if sgd else [3]) + [1.0]     # Adam: step 3 == state[3] + 1
        _lib.check(getattr(L, name)(*args, _stream()), name)
        torch.cuda.synchronize()
        ar.check(f'{name} n={n}')
        return t

    for base in ('svol_sgd_flat', 'svol_adam_flat', 'svol_adamw_flat'):
        plain, zero, scaled, skipped = run(base), run(base + '_zero'), run(base + '_scaled'), run(base + '_scaled', overflow=True)
        keys = ('p', 'a') if 'sgd' in base else ('p', 'a', 'b')
        assert all(torch.equal(plain[k], zero[k]) for k in keys)
        assert not torch.equal(plain['p'], src['p']) and torch.equal(plain['g'], src['g'])
        assert bool((zero['g'] == 0).all())
        assert all(torch.equal(skipped[k], src[k]) for k in ('p', 'g', 'a', 'b'))
        for k in keys:      # on-device float bias corrections against the host's double ones
            _close(scaled[k], plain[k], 2e-6, f'{base}_scaled {k}')
        p, g, a, b = (src[k].double() for k in ('p', 'g', 'a', 'b'))
        d = g + 0.05 * p
        if 'adamw' in base:     # decoupled decay: the parameter shrinks, the bare gradient feeds the moments
            p, d = p * (1 - 3e-3 * 0.05), g
        if 'sgd' in base:
            want = {'a': 0.9 * a + d}
            want['p'] = p - 3e-3 * want['a']
        else:
            want = {'a': a + (d - a) * (1 - 0.9), 'b': b * 0.999 + (1 - 0.999) * d * d}
            want['p'] = p - 3e-3 / (1 - 0.9 ** 3) * want['a'] / (want['b'].sqrt() / (1 - 0.999 ** 3) ** 0.5 + 1e-8)
        for k in keys:
            _close(plain[k], want[k].float(), 2e-6, f'{base} n={n} {k} against fp64')
            if n % 4:
                assert float((plain[k][n - n % 4:] - want[k].float()[n - n % 4:]).abs().max()) <= 2e-6 * max(1.0, float(want[k].abs().max()))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.l = torch.nn.ModuleList([torch.nn.Linear(32, 67), torch.nn.Linear(67, 67), torch.nn.Linear(67, 67), torch.nn.Linear(67, 5)])

    def forward(self, x):
        for lin in self.l[:-1]:
            x = torch.tanh(lin(x))
        return self.l[-1](x)


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_updates_issued_during_backward_change_nothing(kind):
    """step_in_backward (with zero_grads, the pair the benchmark's lab switch uses): real autograd on a small module, the reducer's
    on_bucket_reduced hook issues each bucket's update when its last gradient has arrived.  Same kernels on the same values in
    another order: parameters and state bit-identical to the plain optimizer, every bucket went early, zero_grad() had no fills left."""
    from svol_amd import parallel
    torch.manual_seed(4)
    ref = _Net().cuda()
    x = torch.randn(16, 32, device='cuda')
    y = torch.randn(16, 5, device='cuda')

    def run(early):
        net = _Net().cuda()
        net.load_state_dict(ref.state_dict())
        ps = list(net.parameters())
        red = parallel.BucketedGradAllReduce(ps, bucket_bytes=20000, tail_bytes=0)
        assert len(red.buckets) >= 3
        opt = _classes(kind)[0](red, params=ps, zero_grads=early, step_in_backward=early, **KW[kind])
        assert (red.on_bucket_reduced is not None) == early
        went, losses = [], []
        for _ in range(5):
            skipped = sum(1 for b in red.buckets if b.get('clean'))
            opt.zero_grad()
            loss = ((net(x) - y) ** 2).mean()
            loss.backward()
            red.finish(mean=False)
            went.append((sum(opt._stepped), skipped))
            opt.step()
            losses.append(loss.detach())
        torch.cuda.synchronize()
        return ps, opt, went, [float(v) for v in losses], len(red.buckets)

    pa, oa, wa, la, nb = run(False)
    pb, ob, wb, lb, _ = run(True)
    assert all(w == (0, 0) for w in wa)
    assert all(e >= nb - 1 for e, _ in wb) and [s for _, s in wb] == [0] + [nb] * 4, wb   # every bucket but (at most) the last went early
    assert la == lb and la[-1] < la[0]
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    for sa, sb in zip(oa.flat, ob.flat):
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert oa.steps_taken() == ob.steps_taken() == 5


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_dynamic_loss_scaler_skips_overflowed_steps_and_follows_torch(kind):
    """Gradients arrive multiplied by the scale; a clean step equals torch on the unscaled gradients; a step with an inf (step 2) or a
    NaN (step 6) anywhere in any bucket changes NOTHING — parameters, state buffers, the count of updates taken — and halves the
    scale; the scale grows after `growth_interval` clean steps."""
    from svol_amd import parallel
    p0 = _p0()
    pa, red, oa = _flat(kind, p0, skip_dead=False)
    sc = oa.scaler = parallel.DynamicLossScaler(torch.device('cuda'), init_scale=1024.0, growth_interval=3)
    pb = _mk(p0)
    ob = _classes(kind)[1](pb, **KW[kind])
    scale, clean_run, taken = 1024.0, 0, 0
    for step in range(9):
        red.zero_grad()
        ob.zero_grad()
        overflow = step in (2, 6)
        gs = _grads(step, seed=300)
        for a, g in zip(pa, gs):
            a.grad.copy_(g * scale)                      # what backward of (loss * scale) leaves in the buckets
        if overflow:
            pa[4].grad.view(-1)[7] = float('inf') if step == 2 else float('nan')
        before = [p.detach().clone() for p in pa]
        state = [{k: v.clone() for k, v in st.items()} for st in oa.flat]
        oa.step()
        torch.cuda.synchronize()
        st_host = sc.state.tolist()
        if overflow:
            assert all(torch.equal(a, b) for a, b in zip(before, pa))
            assert all(torch.equal(old[k], st[k]) for old, st in zip(state, oa.flat) for k in st)
            scale *= 0.5
            clean_run = 0
        else:
            for b, g in zip(pb, gs):
                b.grad = g.clone()
            ob.step()
            taken += 1
            clean_run += 1
            if clean_run == 3:
                scale *= 2.0
                clean_run = 0
            for i, (a, b) in enumerate(zip(pa, pb)):
                _close(a, b, 2e-6, f'{kind} scaled step {step} parameter {i}')
        assert st_host[0] == scale and st_host[1] == 0.0 and st_host[3] == float(taken), (step, st_host, scale, taken)
    assert sc.state.tolist()[3] == 7.0 and oa.steps_taken() == 7      # 9 calls, 2 skipped


def test_scaled_sgd_writes_no_state_for_a_skipped_first_step():
    from svol_amd import parallel
    pa, red, oa = _flat('sgd', _p0())
    oa.scaler = parallel.DynamicLossScaler(torch.device('cuda'), init_scale=8.0)
    red.zero_grad()
    pa[0].grad.view(-1)[0] = float('inf')
    oa.step()
    assert oa.state_dict()['state'] == {} and oa.steps_taken() == 0
    _flat_steps(pa, red, oa, [1])
    sd = oa.state_dict()['state']
    assert sorted(sd) == [i for i in range(len(SHAPES)) if i != DEAD] and all(set(e) == {'momentum_buffer'} for e in sd.values())


@pytest.mark.parametrize('attach_first', [True, False])
def test_scaled_adam_resume_keeps_the_bias_correction_step(attach_first):
    """8 uninterrupted steps (step 2 overflows and is skipped) == 4 steps + state_dict -> fresh optimizer + scaler -> load_state_dict ->
    4 more, bit for bit, whichever of {attach the scaler, load the state} happens first; the saved 'step' counts updates TAKEN."""
    from svol_amd import parallel
    dev = torch.device('cuda')

    def run(ps, red, opt, steps):
        for st in steps:
            red.zero_grad()
            gs = _grads(st, seed=500, scale=float(opt.scaler.state[0].item()))
            if st == 2:
                gs[1][5] = float('inf')
            for p, g in zip(ps, gs):
                p.grad.copy_(g)
            opt.step()
        torch.cuda.synchronize()

    p0 = _p0(3)
    pa, ra, oa = _flat('adam', p0, skip_dead=False)
    oa.scaler = parallel.DynamicLossScaler(dev, init_scale=256.0, growth_interval=1000)
    run(pa, ra, oa, range(8))
    assert oa.steps_taken() == 7
    pb, rb, ob = _flat('adam', p0, skip_dead=False)
    ob.scaler = parallel.DynamicLossScaler(dev, init_scale=256.0, growth_interval=1000)
    run(pb, rb, ob, range(4))
    sd_opt, sd_amp = ob.state_dict(), ob.scaler.state_dict()
    assert {int(float(e['step'])) for e in sd_opt['state'].values()} == {3}   # four calls, one skipped
    pc, rc, oc = _flat('adam', [p.detach() for p in pb], skip_dead=False)
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


def test_two_ranks_sum_and_the_update_kernel_takes_the_mean():
    """World size 2 on one GPU (gloo, as tests/test_gpu_parallel.py): finish(mean=False) leaves sums in the buckets and the update
    kernel applies 1 / world — the result equals torch's optimizer on the averaged gradients (tests/flat_optim_dp_worker.py)."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(HERE, 'flat_optim_dp_worker.py')]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.count('flat optimizers == torch on the averaged gradients') == 2, p.stdout[-2000:]
    print('\n'.join(ln for ln in p.stdout.splitlines() if 'flat optimizers' in ln))


def _torch_opt(name, params, a):
    if name == 'sgd':
        return torch.optim.SGD(params, lr=a.lr, momentum=0.9, weight_decay=a.wd)     # train.py:94-95
    return torch.optim.Adam(params, lr=a.lr, weight_decay=a.wd)                      # train.py:96-97


def _train(name, flat, steps=20, shadow_steps=3):
    from svol_amd import parallel
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.svanet import build_svanet
    args = syn.head_args(hidden_dim=128, nheads=8, num_layers=2, num_queries=20, num_frames=8, input_vid_dim=64, input_skch_dim=64,
                         input_dropout=0.0, matcher='video_matcher')
    args.compute_dtype = 'bf16'
    opt_args = argparse.Namespace(optimizer=name, lr=2e-3, wd=1e-4)
    torch.manual_seed(1)
    model = build_svanet(args).cuda().train()
    crit = build_loss(args).cuda().train()
    params = [p for p in model.parameters() if p.requires_grad]
    if flat:
        red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
        opt = parallel.build_optimizer(opt_args, red, params)
        assert type(opt) is {'sgd': parallel.FlatSGD, 'adam': parallel.FlatAdam}[name]
        # torch's optimizer of the same name riding along on copies of the parameters, fed THIS run's gradients
        shadow = [torch.nn.Parameter(p.detach().clone()) for p in params]
        shadow_opt = _torch_opt(name, shadow, opt_args)
    else:
        opt = _torch_opt(name, params, opt_args)
    B, T, P = 2, 8, 32
    inp = {k: v.cuda() for k, v in syn.synth_inputs(args, B, T, P, seed=3).items()}
    tg = syn.synth_targets(B, T, seed=3)
    losses = []
    for k in range(steps):
        opt.zero_grad()
        out = model(inp['src_sketch'], inp['src_sketch_mask'], inp['src_video'], inp['src_video_mask'])
        crit(out, tg)
        loss = crit.weighted_total()
        loss.backward()
        if flat:
            red.finish(mean=False)
            if k < shadow_steps:
                for s, p in zip(shadow, params):
                    s.grad = None if p.grad is None else p.grad.detach().clone()
        opt.step()
        if flat and k < shadow_steps:
            shadow_opt.step()
            assert sum(s.grad is not None for s in shadow) > len(shadow) // 2
            worst = max(zip(params, shadow), key=lambda ab: float((ab[0].detach() - ab[1].detach()).abs().max()))
            _close(worst[0], worst[1], 2e-6, f'{name} step {k + 1}: parameters against torch on the same gradients (worst tensor)')
            for p, s in zip(params, shadow):
                err, ref = float((p.detach() - s.detach()).abs().max()), max(1.0, float(s.detach().abs().max()))
                assert err <= 2e-6 * ref, (name, k, tuple(p.shape), err, ref)
        losses.append(float(loss))
    return losses


@pytest.mark.parametrize('name', ['sgd', 'adam'])
def test_short_training_run_through_build_optimizer(name):
    """20 steps on one fixed synthetic batch (the model and batch of tests/test_gpu_training.py) with the optimizer build_optimizer
    returns for --optimizer sgd | adam: the loss goes down, and the run follows the same loop under torch's optimizer on ordinary
    per-parameter gradients by that file's bar for the same comparison — equal first loss to 1e-4, loss curves within 3 % over the
    first 8 steps (later, flipped Hungarian assignments amplify rounding noise between two runs of even the same variant).

    A loss curve barely moves under a slightly wrong update, so the PARAMETERS are compared too, over the first three steps, against
    torch's optimizer stepping copies of them on the gradients this very run produced (_train).  Not against the second run's
    parameters: the backward's atomics make two runs' gradients differ in their last bits, and Adam's first updates are
    lr * g / (|g| + eps) ~ lr * sign(g), so an element whose gradient is at that noise level may move by up to 2 * lr = 4e-3 in
    either run — no bound on that comparison separates a right update from a wrong one.  On the same gradients the bar is the
    parity bar of this file, 2e-6 * max(1, max|b|) per tensor (module docstring: about 4x what two correct fp32 implementations
    need over 8 steps; here 3 steps at a smaller lr and wd)."""
    a = _train(name, flat=True)
    b = _train(name, flat=False)
    print(name, 'flat ', ' '.join(f'{x:.4f}' for x in a))
    print(name, 'torch', ' '.join(f'{x:.4f}' for x in b))
    assert all(x == x and abs(x) < 1e4 for x in a + b)
    assert a[-1] < a[0] and b[-1] < b[0], (a[0], a[-1], b[0], b[-1])
    assert abs(a[0] - b[0]) <= 1e-4 * abs(b[0])
    for k in range(8):
        assert abs(a[k] - b[k]) <= 0.03 * abs(b[k]), (k, a[k], b[k])
