"""Global gradient-norm clipping inside the flat optimizers' step on the device (max_grad_norm / --clip_max_norm: what
torch.nn.utils.clip_grad_norm_ does between backward and step in a DETR-style loop): the sum-of-squares kernel through its C entry,
parity of the clipped step with clip_grad_norm_ + the torch optimizer of the same name, the pending 1 / world and the loss scale,
the dynamic loss scaler, step_in_backward, clipping off, and a short training run.

Shapes, bucket size and gradients are those of tests/test_gpu_flat_optim.py (helpers copied, not imported).  The live gradient has
18 560 elements, so its norm is about 136 * (1 + step): with max_norm = 200 step 0 is NOT clipped and steps 1-4 are, and every parity
test asserts from opt.grad_norm that both regimes occurred.

The parity bar is the project's own, max|a - b| <= 2e-6 * max(1, max|b|), for the parameters and for grad_norm against the norm torch
returns.  Measured for THIS pipeline (clip_grad_norm_(live, 200) then SGD / Adam / AdamW with lr 3e-3, wd 0.05, 5 steps, these shapes
and gradient scales, three parameter seeds, foreach and single-tensor alike): torch's fp32 run stays within 1.6e-7 (SGD), 1.0e-7 (Adam)
and 2.5e-7 (AdamW) of the same run in fp64 by that measure, and its returned norm within 1.2e-7 relative — 8x and 16x headroom under
2e-6, so the bar stands as it is.  The sum-of-squares kernel is held to 1e-5 relative on the norm: for sums of non-negative terms the
relative error is at most (longest adder chain) * 2^-24; the kernel's fp32 chain is ceil(n / 2^21) + 12 <= 128 (the rest runs in
double), which bounds the sum at 7.6e-6 and the square root at half of it."""
import argparse
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 33), (33,), (7,), (128, 128), (5, 3, 2), (1,)]
DEAD = 2
MAX_NORM = 200.0
KW = {'sgd': dict(lr=3e-3, momentum=0.9, weight_decay=0.05), 'adam': dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05),
      'adamw': dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)}


def _classes(kind):
    from svol_amd import parallel
    return {'sgd': (parallel.FlatSGD, torch.optim.SGD), 'adam': (parallel.FlatAdam, torch.optim.Adam),
            'adamw': (parallel.FlatAdamW, torch.optim.AdamW)}[kind]


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


def _flat(kind, src, **kw):
    from svol_amd import parallel
    ps = _mk(src)
    red = parallel.BucketedGradAllReduce(ps, bucket_bytes=40000, skip=[ps[DEAD]])
    assert len(red.buckets) >= 2
    return ps, red, _classes(kind)[0](red, params=ps, **dict(KW[kind], **kw))


def _flat_steps(ps, red, opt, steps, scale=1.0, before_step=None):
    """-> the grad_norm of every step (None where clipping is off)"""
    norms = []
    for st in steps:
        opt.zero_grad()
        for i, (p, g) in enumerate(zip(ps, _grads(st, scale=scale))):
            if i != DEAD:
                p.grad.copy_(g)
        if before_step is not None:
            before_step()
        opt.step()
        norms.append(None if opt.grad_norm is None else opt.grad_norm.clone())
    return norms


@functools.lru_cache(maxsize=None)
def _torch_clipped(kind, steps=(0, 1, 2, 3, 4)):
    """The reference, computed once per (kind, steps) and never written to: clip_grad_norm_(live, 200) then the torch optimizer, fp32, on
    the plain gradients -> (parameters, the norms torch returned)."""
    ps = _mk(_p0())
    live = [p for i, p in enumerate(ps) if i != DEAD]
    opt = _classes(kind)[1](live, **KW[kind])
    norms = []
    for st in steps:
        opt.zero_grad()
        for i, (p, g) in enumerate(zip(ps, _grads(st))):
            if i != DEAD:
                p.grad = g.clone()
        norms.append(torch.nn.utils.clip_grad_norm_(live, MAX_NORM).detach().clone())
        opt.step()
    return [p.detach().clone() for p in ps], torch.stack(norms)


def _both_regimes(norms):
    assert float(norms[0]) < MAX_NORM and all(float(v) > MAX_NORM for v in norms[1:]), [float(v) for v in norms]


def _against_torch(kind, pa, norms, what, steps=(0, 1, 2, 3, 4)):
    pb, nb = _torch_clipped(kind, steps)
    norms = torch.stack(norms)
    _both_regimes(norms)
    _both_regimes(nb)
    for i, (a, b) in enumerate(zip(pa, pb)):
        _close(a, b, 2e-6, f'{kind} {what}: parameter {i}')
    _close(norms, nb, 2e-6, f'{kind} {what}: grad_norm')
    assert torch.equal(pa[DEAD].detach(), _p0()[DEAD])


CAP_PASS = 2048 * 256 * 4     # floats one pass of the capped grid covers


@pytest.mark.parametrize('n', [1, 3, 4, 5, 4 * 256 * 3 + 1, 65536 + 3, CAP_PASS + 4 * 256 + 3])
def test_sum_of_squares_kernel_reads_its_range_once_and_repeats_its_bits(n):
    """svol_grad_sqnorm over a range carved out of an arena of -0.0 words (tests/test_gpu_guards.py), with 64 floats of 1e30 directly
    in front of and behind g inside its slot: a read outside [0, n) makes the sum inf.  The padding, the gradient range and every guard
    word (around the range, the workspace and the result) come back bit-identical; two runs give the same bits; sqrt(sum) is within
    1e-5 relative of the fp64 norm (module docstring).  n % 4 != 0 runs the scalar tail, the last n a second grid-stride pass."""
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    from tests.test_gpu_guards import GuardArena
    L = _lib.lib()
    PAD = 64
    ws_floats = int(L.svol_grad_sqnorm_ws_bytes(n)) // 4
    assert ws_floats * 256 * 4 > min(n, CAP_PASS - 1) and ws_floats <= 2048
    gen = torch.Generator(device='cuda').manual_seed(n)
    cases = {'randn': torch.randn(n, device='cuda', generator=gen)}
    if n == 65536 + 3:
        cases['one 1e4 among 1e-4s'] = torch.full((n,), 1e-4, device='cuda')
        cases['one 1e4 among 1e-4s'][n // 3] = 1e4
    for what, src in cases.items():
        ar = GuardArena(guard_bytes=1 << 12)
        ar.plan('gpad', (n + 2 * PAD,), torch.float32)
        ar.plan('ws', (ws_floats,), torch.float32)
        ar.plan('out', (2,), torch.float32)
        t = ar.build()
        t['gpad'].fill_(1e30)
        g = t['gpad'][PAD:PAD + n]
        g.copy_(src)
        assert _ptr(g) % 16 == 0
        held = t['gpad'].view(torch.int32).clone()
        for k in range(2):
            _lib.check(L.svol_grad_sqnorm(_ptr(g), n, _ptr(t['ws']), _ptr(t['out'][k:]), _stream()), 'svol_grad_sqnorm')
        torch.cuda.synchronize()
        ar.check(f'svol_grad_sqnorm n={n} {what}')
        assert torch.equal(t['gpad'].view(torch.int32), held)
        assert torch.equal(t['out'][0], t['out'][1]) and bool(torch.isfinite(t['out'][0]))
        got, want = float(t['out'][0].double().sqrt()), float(src.double().norm())
        print(f'n={n} {what}: sqrt(sum) = {got!r}, fp64 norm = {want!r}, relative error {abs(got - want) / want:.2e}')
        assert abs(got - want) <= 1e-5 * want


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'adamw'])
def test_clipped_step_matches_clip_grad_norm_and_the_torch_optimizer(kind):
    """5 steps on identical gradients, step 0 below max_norm and steps 1-4 above it."""
    pa, red, oa = _flat(kind, _p0(), max_grad_norm=MAX_NORM)
    norms = _flat_steps(pa, red, oa, range(5))
    assert all(v.shape == () and v.dtype == torch.float32 and v.is_cuda for v in norms)
    _against_torch(kind, pa, norms, 'clipped')
    assert oa.steps_taken() == 5 and 'max_grad_norm' not in oa.state_dict()['param_groups'][0]


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'adamw'])
def test_sums_over_ranks_and_a_loss_scale_do_not_reach_the_norm(kind):
    """The two traps of clip_grad_norm_ over the gradient views: the buckets hold 4 ranks' SUMS (finish(mean=False): pending_scale =
    0.25) of gradients multiplied by a loss scale of 1024 — 4096 times the true gradient.  Parameters and grad_norm equal the torch
    reference on the plain gradients."""
    pa, red, oa = _flat(kind, _p0(), max_grad_norm=MAX_NORM)
    oa.loss_scale = 1024.0

    def pending():
        red.pending_scale = 0.25
    norms = _flat_steps(pa, red, oa, range(5), scale=1024.0 * 4.0, before_step=pending)
    assert red.pending_scale == 1.0      # consumed, as without clipping
    _against_torch(kind, pa, norms, 'summed and scaled')


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_clipping_under_the_dynamic_loss_scaler(kind, monkeypatch):
    """Gradients arrive multiplied by the current scale; step 2 has an inf in the second bucket: parameters and state stay bit-identical,
    the scale is halved, the count of updates is not advanced, grad_norm is not finite — and the other four steps match a torch run
    that never saw step 2.  The sum of squares is the overflow check: svol_grad_finite is not called."""
    from svol_amd import _lib, parallel

    def not_needed(*a):
        raise AssertionError('svol_grad_finite called on the clipped path')
    monkeypatch.setattr(_lib.lib(), 'svol_grad_finite', not_needed)
    pa, red, oa = _flat(kind, _p0(), max_grad_norm=MAX_NORM)
    sc = oa.scaler = parallel.DynamicLossScaler(torch.device('cuda'), init_scale=2.0 ** 10)
    scale, norms = 2.0 ** 10, []
    for step in range(5):
        red.zero_grad()
        for i, (a, g) in enumerate(zip(pa, _grads(step, scale=scale))):
            if i != DEAD:
                a.grad.copy_(g)
        if step == 2:
            red.buckets[1]['flat'][5] = float('inf')
            before = [p.detach().clone() for p in pa]
            state = [{k: v.clone() for k, v in st.items()} for st in oa.flat]
        oa.step()
        if step == 2:
            assert all(torch.equal(a, b) for a, b in zip(before, pa))
            assert all(torch.equal(old[k], st[k]) for old, st in zip(state, oa.flat) for k in st)
            assert not bool(torch.isfinite(oa.grad_norm))
            scale *= 0.5
            assert sc.state.tolist() == [scale, 0.0, 0.0, 2.0] and oa.steps_taken() == 2
        else:
            norms.append(oa.grad_norm.clone())
    assert sc.state.tolist() == [512.0, 0.0, 2.0, 4.0] and oa.steps_taken() == 4
    _against_torch(kind, pa, norms, 'under the scaler', steps=(0, 1, 3, 4))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.l = torch.nn.ModuleList([torch.nn.Linear(32, 67), torch.nn.Linear(67, 67), torch.nn.Linear(67, 67), torch.nn.Linear(67, 5)])

    def forward(self, x):
        for lin in self.l[:-1]:
            x = torch.tanh(lin(x))
        return self.l[-1](x)


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_step_in_backward_is_ignored_while_clipping(kind):
    """step_in_backward=True, zero_grads=True with clipping on, real autograd on a small module: no bucket is updated during backward
    (the norm spans all of them), the reducer's own fill runs, and parameters, state and norms are bit-identical to the plain clipped
    optimizer's."""
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
        opt = _classes(kind)[0](red, params=ps, zero_grads=early, step_in_backward=early, max_grad_norm=0.05, **KW[kind])
        norms = []
        for _ in range(5):
            assert not any(b.get('clean') for b in red.buckets)
            opt.zero_grad()
            ((net(x) - y) ** 2).mean().backward()
            red.finish(mean=False)
            assert sum(opt._stepped) == 0
            opt.step()
            norms.append(opt.grad_norm.clone())
        torch.cuda.synchronize()
        return ps, opt, torch.stack(norms)

    pa, oa, na = run(False)
    pb, ob, nb = run(True)
    print('norms', na.tolist())
    assert torch.equal(na, nb) and bool((na > 0.05).any())      # clipping was at work
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    for sa, sb in zip(oa.flat, ob.flat):
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert oa.steps_taken() == ob.steps_taken() == 5


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'adamw'])
def test_off_means_untouched(kind):
    p0 = _p0(2)
    runs = []
    for how in ('no keyword', 'None', 'set and reset'):
        pa, red, oa = _flat(kind, p0, **({} if how == 'no keyword' else dict(max_grad_norm=None)))
        if how == 'set and reset':
            oa.max_grad_norm = 1.0
            assert oa.grad_norm is not None
            oa.max_grad_norm = None
        assert oa.max_grad_norm is None and oa.grad_norm is None
        assert _flat_steps(pa, red, oa, range(3)) == [None] * 3
        runs.append((pa, oa))
    for pa, oa in runs[1:]:
        assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(pa, runs[0][0]))
        assert all(torch.equal(sa[k], sb[k]) for sa, sb in zip(oa.flat, runs[0][1].flat) for k in sa)


def test_short_training_run_with_clip_max_norm():
    """20 steps of the tiny head of tests/test_gpu_flat_optim.py::test_short_training_run_through_build_optimizer with --clip_max_norm
    0.1 through build_optimizer: at three steps the fp64 norm of the live param.grad views, taken between finish(mean=False) and
    step(), equals grad_norm after the step to 1e-5 relative; the loss ends finite and below where it began."""
    from svol_amd import parallel
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.svanet import build_svanet
    args = syn.head_args(hidden_dim=128, nheads=8, num_layers=2, num_queries=20, num_frames=8, input_vid_dim=64, input_skch_dim=64,
                         input_dropout=0.0, matcher='video_matcher')
    args.compute_dtype = 'bf16'
    opt_args = argparse.Namespace(optimizer='adamw', lr=2e-3, wd=1e-4, clip_max_norm=0.1)
    torch.manual_seed(1)
    model = build_svanet(args).cuda().train()
    crit = build_loss(args).cuda().train()
    params = [p for p in model.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
    opt = parallel.build_optimizer(opt_args, red, params)
    assert type(opt) is parallel.FlatAdamW and opt.max_grad_norm == 0.1
    live = [p for b in red.buckets for p in b['params']]
    B, T, P = 2, 8, 32
    inp = {k: v.cuda() for k, v in syn.synth_inputs(args, B, T, P, seed=3).items()}
    tg = syn.synth_targets(B, T, seed=3)
    losses, pairs = [], []
    for k in range(20):
        opt.zero_grad()
        out = model(inp['src_sketch'], inp['src_sketch_mask'], inp['src_video'], inp['src_video_mask'])
        crit(out, tg)
        loss = crit.weighted_total()
        loss.backward()
        red.finish(mean=False)
        want = torch.stack([p.grad.double().pow(2).sum() for p in live]).sum().sqrt() if k in (0, 7, 19) else None
        opt.step()
        if want is not None:
            pairs.append((k, float(opt.grad_norm), float(want)))
        losses.append(float(loss))
    print('losses', ' '.join(f'{x:.4f}' for x in losses))
    for k, got, want in pairs:
        print(f'step {k}: grad_norm = {got!r}, fp64 norm of param.grad = {want!r}, relative error {abs(got - want) / want:.2e}')
        assert abs(got - want) <= 1e-5 * want
    assert len(pairs) == 3 and any(want > 0.1 for _, _, want in pairs)
    assert losses[-1] == losses[-1] and abs(losses[-1]) < 1e4 and losses[-1] < losses[0], (losses[0], losses[-1])
