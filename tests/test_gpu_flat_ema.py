"""The flat optimizers' weight average on the device (ema_decay=...; svol_ema_flat): the kernel alone in a guard arena against the
fp64 twin of tests/ema_ref.py, then through FlatSGD / FlatAdam / FlatAdamW on every path that issues an update — plain, zeroing,
clipped, grouped, during backward, under the dynamic loss scaler, captured into a graph —, the exchange of averaged_weights()
through a real head, and checkpoints.

The bar (tests/ema_ref.py, derived there): |got - ref| <= 2^-23 * (|ref| + 2 * (1 - d) * |p - ema_prev|) per element, ref one
fp64 application to the device's own previous average.  Everything the average must NOT touch is compared bit for bit: the
parameters and optimizer state against an optimizer without an average on the same gradients, the average itself over a skipped
step, parameters and average around averaged_weights()."""
import argparse
import warnings

import pytest
import torch

from tests import ema_ref
from tests.guard_arena import GuardArena

pytestmark = pytest.mark.gpu

KINDS = ['sgd', 'adam', 'adamw']
KW = {'sgd': dict(lr=3e-2, momentum=0.9, weight_decay=0.05), 'adam': dict(lr=3e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05),
      'adamw': dict(lr=3e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)}
DECAY = 0.99


def _cls(kind):
    from svol_amd import parallel
    return {'sgd': parallel.FlatSGD, 'adam': parallel.FlatAdam, 'adamw': parallel.FlatAdamW}[kind]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- the kernel alone --------------------------------------------------------------------------------------------------------------
# one float4 per thread, 256 threads per workgroup: one vector, exactly one workgroup, one workgroup plus one vector, several
# workgroups plus one vector
SIZES = [4, 1024, 1028, 4 * 256 * 3 + 4]


def _src(n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    ema, p = torch.randn(n, device='cuda', generator=g), torch.randn(n, device='cuda', generator=g)
    p[1::2] = ema[1::2]                 # every other element: p == ema exactly
    return ema, p


def _kernel(ema, p, decay, warmup, step=1, state=None, count=None):
    """one launch over copies of ema and p inside red zones; returns the new average after checking that nothing else changed"""
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    n = ema.numel()
    ar = GuardArena(guard_bytes=1 << 12)
    ar.plan('ema', (n,), torch.float32)
    ar.plan('p', (n,), torch.float32)
    ar.plan('state', (4,), torch.float32)
    ar.plan('count', (1,), torch.float32)
    t = ar.build()
    t['ema'].copy_(ema)
    t['p'].copy_(p)
    t['state'].copy_(torch.tensor(state if state is not None else [0.0] * 4))
    t['count'].fill_(count if count is not None else 0.0)
    keep = {k: t[k].clone() for k in ('p', 'state', 'count')}
    rc = _lib.lib().svol_ema_flat(_ptr(t['ema']), _ptr(t['p']), n, decay, int(warmup), step, _ptr(t['state']) if state is not None else 0,
                                  _ptr(t['count']) if count is not None else 0, _stream())
    _lib.check(rc, 'svol_ema_flat')
    torch.cuda.synchronize()
    ar.check(f'svol_ema_flat n={n}')                                     # nothing outside [0, n) of ema
    assert all(_same(t[k], keep[k]) for k in keep)                       # p, the state vector and the count are only read
    return t['ema'].clone()


@pytest.mark.parametrize('decay', [0.9, DECAY, 0.0, 1.0])
@pytest.mark.parametrize('n', SIZES)
def test_kernel_meets_the_bar_and_stays_inside_its_range(n, decay):
    ema, p = _src(n, 10 + n)
    got = _kernel(ema, p, decay, warmup=False, step=1)
    ema_ref.check(got, ema, p, ema_ref.decay_at(decay, False, 1), f'n={n} decay={decay}')
    assert torch.equal(got[1::2], ema[1::2])                             # p == ema: exactly ema
    if decay == 1.0:
        assert torch.equal(got, ema)
    else:
        assert not torch.equal(got[0::2], ema[0::2])


@pytest.mark.parametrize('n', [4, 1028])
def test_kernel_writes_nothing_on_an_overflowed_step(n):
    ema, p = _src(n, 20 + n)
    for count in (None, 4.0):
        got = _kernel(ema, p, 0.5, warmup=True, state=[1024.0, 1.0, 0.0, 4.0], count=count)
        assert _same(got, ema)
    assert not _same(_kernel(ema, p, 0.5, warmup=True, state=[1024.0, 0.0, 0.0, 4.0]), ema)


@pytest.mark.parametrize('source', ['state', 'count', 'count_beside_state', 'host'])
def test_warmup_index_comes_from_where_the_update_read_its_count(source):
    """four updates taken so far: the one being averaged is the fifth, d = min(decay, 6 / 15) = 0.4 — solved from one element."""
    n = 1028
    ema, p = _src(n, 31)
    kw = {'state': dict(step=0, state=[1.0, 0.0, 9.0, 4.0]), 'count': dict(step=0, count=4.0),
          'count_beside_state': dict(step=77, state=[1.0, 0.0, 9.0, 77.0], count=4.0), 'host': dict(step=5)}[source]
    got = _kernel(ema, p, DECAY, warmup=True, **kw)
    ema_ref.check(got, ema, p, 0.4, source)
    i = int((p - ema).abs().argmax())
    delta = float(p[i].double() - ema[i].double())
    d = 1.0 - float(got[i].double() - ema[i].double()) / delta
    tol = 2.0 ** -23 * (abs(float(got[i])) / abs(delta) + 2 * 0.6)       # the element's bar, divided by |p - ema|
    print(f'{source}: solved d = {d:.9f} (0.4 +- {tol:.2e})')
    assert abs(d - 0.4) <= tol
    # past the warm-up, and with the warm-up off, it is the decay itself
    kw_late = {k: ([1.0, 0.0, 0.0, 5000.0] if k == 'state' else 5000.0 if k == 'count' else 5001) for k in kw}
    d32 = ema_ref.decay_at(DECAY, False, 1)
    ema_ref.check(_kernel(ema, p, DECAY, warmup=True, **kw_late), ema, p, d32, source + ' late')
    ema_ref.check(_kernel(ema, p, DECAY, warmup=False, **kw), ema, p, d32, source + ' no warm-up')


# ---- through the optimizers --------------------------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.l = torch.nn.ModuleList([torch.nn.Linear(6, 8), torch.nn.Linear(8, 12), torch.nn.Linear(12, 4)])

    def forward(self, x):
        for lin in self.l[:-1]:
            x = torch.tanh(lin(x))
        return self.l[-1](x)


def _toy(kind, seed=0, groups=False, **kw):
    from svol_amd import parallel
    torch.manual_seed(seed)
    net = _Toy().cuda()
    ps = list(net.parameters())
    red = parallel.BucketedGradAllReduce(ps, bucket_bytes=256, tail_bytes=0)
    assert len(red.buckets) >= 2
    params = [{'params': [p for p in ps if p.dim() == 2], 'lr': 3e-3}, {'params': [p for p in ps if p.dim() == 1]}] if groups else ps
    opt = _cls(kind)(red, params=params, **dict(KW[kind], **kw))
    return net, ps, red, opt


def _feed(ps, step, scale=1.0, seed=500):
    g = torch.Generator(device='cuda').manual_seed(seed + step)
    for p in ps:
        p.grad.copy_(torch.randn(p.shape, device='cuda', generator=g) * scale)


def _check_step(opt, ps, prev, d, what):
    for i, (p, e) in enumerate(zip(ps, prev)):
        ema_ref.check(opt.ema_views(p), e, p.detach(), d, f'{what} parameter {i}')


VARIANTS = {'plain': {}, 'zero_grads': dict(zero_grads=True), 'clip': dict(max_grad_norm=1.0), 'groups': dict(groups=True),
            'early': dict(step_in_backward=True)}


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_average_follows_every_update_and_changes_none(kind, variant):
    """Five steps of two optimizers on the same gradients, one with an average and one without: after every step each average is
    one twin application to the device's previous average and the parameters that step produced, at the step's warm-up decay;
    parameters and optimizer state of the two are bit-identical throughout.  'early': real autograd, each bucket's update (and
    its average) issued by the reducer during backward."""
    kw = VARIANTS[variant]
    neta, pa, reda, oa = _toy(kind, ema_decay=DECAY, **kw)
    netb, pb, redb, ob = _toy(kind, **kw)
    assert all('ema' in st for st in oa.flat) and not any('ema' in st for st in ob.flat)
    assert all(_same(st['ema'], st['p']) for st in oa.flat)              # seeded from the re-homed parameters
    assert oa._grouped == (variant == 'groups')
    early = variant == 'early'
    x, y = torch.randn(16, 6, device='cuda'), torch.randn(16, 4, device='cuda')
    for t in range(1, 6):
        prev = [oa.ema_views(p).clone() for p in pa]
        for net, ps, red, opt in ((neta, pa, reda, oa), (netb, pb, redb, ob)):
            opt.zero_grad()
            if early:
                ((net(x) - y) ** 2).mean().backward()
                red.finish(mean=False)
                assert sum(opt._stepped) >= len(red.buckets) - 1         # the updates went during backward
            else:
                _feed(ps, t)
            opt.step()
        torch.cuda.synchronize()
        _check_step(oa, pa, prev, ema_ref.decay_at(DECAY, True, t), f'{kind} {variant} step {t}')
        assert not any(_same(oa.ema_views(p), e) for p, e in zip(pa, prev))
        assert all(_same(a, b) for a, b in zip(pa, pb)), t
        assert all(_same(sa[k], sb[k]) for sa, sb in zip(oa.flat, ob.flat) for k in sb), t
        assert all(set(sa) == set(sb) | {'ema'} for sa, sb in zip(oa.flat, ob.flat))
    assert oa.steps_taken() == ob.steps_taken() == 5
    sda, sdb = oa.state_dict(), ob.state_dict()
    assert sda['param_groups'] == sdb['param_groups'] and sda['state'].keys() == sdb['state'].keys()
    for b in reda.buckets:                                               # the padding floats of the average stayed what they were
        pad = torch.ones_like(b['flat'], dtype=torch.bool)
        for p, off in zip(b['params'], b['offsets']):
            pad[off:off + p.numel()] = False
        assert bool((oa.flat[b['index']]['ema'][pad] == 0).all())


@pytest.mark.parametrize('capturable', [False, True], ids=['plain', 'capturable'])
@pytest.mark.parametrize('kind', KINDS)
def test_a_step_the_loss_scaler_skips_moves_neither_the_average_nor_its_warmup(kind, capturable):
    from svol_amd import parallel
    _, ps, red, opt = _toy(kind, ema_decay=DECAY, capturable=capturable)
    sc = opt.scaler = parallel.DynamicLossScaler(torch.device('cuda'), init_scale=1024.0)
    scale, taken = 1024.0, 0
    for step in range(1, 6):
        prev = [opt.ema_views(p).clone() for p in ps]
        before = [p.detach().clone() for p in ps]
        red.zero_grad()
        _feed(ps, step, scale=scale)
        if step == 3:
            ps[2].grad.view(-1)[5] = float('inf')
        opt.step()
        torch.cuda.synchronize()
        if step == 3:
            assert all(_same(opt.ema_views(p), e) for p, e in zip(ps, prev))          # the average after step 3 IS the one after step 2
            assert all(_same(p, b) for p, b in zip(ps, before))
            scale *= 0.5
        else:
            taken += 1
            _check_step(opt, ps, prev, ema_ref.decay_at(DECAY, True, taken), f'{kind} scaled step {step}')
        if step == 4:                                                    # its index is 3, not 4: d = 4 / 13, not 5 / 14
            assert taken == 3
            with pytest.raises(AssertionError):
                _check_step(opt, ps, prev, ema_ref.decay_at(DECAY, True, 4), 'the index a call count would give')
        st = sc.state.tolist()
        assert (st[0], st[1], st[3]) == (scale, 0.0, float(taken))
    assert opt.steps_taken() == 4


@pytest.mark.parametrize('kind', KINDS)
def test_captured_step_replays_the_average(kind, monkeypatch):
    """capturable=True: one step() captured on a side stream and replayed four times over refreshed gradients equals four eager
    steps of a second optimizer bit for bit, parameters and average.  Every launch of the captured step goes to the one capture
    stream: the graph is a single chain, it has no parallel branches."""
    from svol_amd import parallel
    _, pw, _, ow = _toy(kind, ema_decay=DECAY, capturable=True)          # a third optimizer takes the kernels' first launches
    _feed(pw, 0)
    ow.step()
    _, pa, reda, oa = _toy(kind, ema_decay=DECAY, capturable=True)
    _, pb, redb, ob = _toy(kind, ema_decay=DECAY, capturable=True)
    oa.push_hyper()
    torch.cuda.synchronize()
    used = []
    real = parallel._stream
    monkeypatch.setattr(parallel, '_stream', lambda: used.append(real()) or used[-1])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        oa.step()
    torch.cuda.current_stream().wait_stream(side)
    monkeypatch.undo()
    assert used and all(s == side.cuda_stream for s in used)
    assert oa.steps_taken() == 0 and all(_same(st['ema'], st['p']) for st in oa.flat)     # capturing ran nothing
    for t in range(1, 5):
        prev = [oa.ema_views(p).clone() for p in pa]
        _feed(pa, t)
        graph.replay()
        redb.zero_grad()
        _feed(pb, t)
        ob.step()
        torch.cuda.synchronize()
        _check_step(oa, pa, prev, ema_ref.decay_at(DECAY, True, t), f'{kind} replay {t}')
        assert all(_same(a, b) for a, b in zip(pa, pb)), t
        assert all(_same(sa[k], sb[k]) for sa, sb in zip(oa.flat, ob.flat) for k in sa), t
    assert oa.steps_taken() == ob.steps_taken() == 4
    assert not any(_same(st['ema'], st['p']) for st in oa.flat)


# ---- averaged_weights() through a real head ----------------------------------------------------------------------------------------
def test_averaged_weights_through_a_real_head():
    from svol_amd import parallel
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.svanet import build_svanet
    args = syn.head_args(hidden_dim=32, nheads=4, num_layers=1, num_queries=8, num_frames=4, input_vid_dim=32, input_skch_dim=32)
    args.compute_dtype = 'bf16'
    torch.manual_seed(1)
    model = build_svanet(args).cuda().train()
    crit = build_loss(args).cuda().train()
    params = [p for p in model.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), bucket_bytes=1 << 14, skip=parallel.unused_parameters(model),
                                         ordered=True)
    assert len(red.buckets) >= 2
    opt = parallel.FlatAdamW(red, lr=2e-3, weight_decay=1e-4, params=params, ema_decay=0.5)
    B, T, P = 2, 4, 16
    inp = {k: v.cuda() for k, v in syn.synth_inputs(args, B, T, P, seed=3).items()}
    tg = syn.synth_targets(B, T, seed=3)
    for _ in range(2):
        opt.zero_grad()
        crit(model(**inp), tg)
        crit.weighted_total().backward()
        red.finish(mean=False)
        opt.step()
    owned = [p for b in red.buckets for p in b['params']]
    assert not any(_same(opt.ema_views(p), p) for p in owned if p.dim() == 2)       # the average is visibly not the weights

    def forward(m):
        m.eval()
        with torch.no_grad():
            out = m(**inp)
        torch.cuda.synchronize()
        return out['pred_logits'].clone(), out['pred_boxes'].clone()

    fresh = build_svanet(args).cuda()
    fresh.load_state_dict(opt.ema_state_dict(model))
    want = forward(fresh)
    p0, e0 = [st['p'].clone() for st in opt.flat], [st['ema'].clone() for st in opt.flat]
    outside = forward(model)
    with opt.averaged_weights():
        assert all(_same(p, e) for p, e in zip([st['p'] for st in opt.flat], e0))   # every parameter equals its average
        inside = forward(model)
        with pytest.raises(RuntimeError):
            with opt.averaged_weights():
                pass
    assert all(_same(a, b) for a, b in zip(inside, want))
    assert not any(_same(a, b) for a, b in zip(inside, outside))
    assert all(_same(st['p'], p) and _same(st['ema'], e) for st, p, e in zip(opt.flat, p0, e0))
    assert all(_same(a, b) for a, b in zip(forward(model), outside))
    # entering during a stream capture is refused (and leaves nothing exchanged)
    x = torch.zeros(4, device='cuda')
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        x.add_(1.0)
        with pytest.raises(RuntimeError):
            opt.averaged_weights().__enter__()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not opt._ema_swapped and all(_same(st['p'], p) and _same(st['ema'], e) for st, p, e in zip(opt.flat, p0, e0))


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
PARENT_KEYS = ['model', 'optimizer', 'lr_scheduler', 'amp', 'iter', 'args']          # the format's keys before it carried an average


@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_checkpoint_carries_the_average_and_the_warmup_continues(kind, tmp_path):
    from svol_amd.utils import checkpoint
    ns = argparse.Namespace(x=1)
    net, ps, red, opt = _toy(kind, ema_decay=DECAY)
    for t in (1, 2):
        opt.zero_grad()
        _feed(ps, t)
        opt.step()
    path = checkpoint.save_checkpoint(str(tmp_path / 'on.ckpt'), net, opt, None, 2, ns)
    ck = torch.load(path, weights_only=False)
    assert sorted(ck) == sorted(PARENT_KEYS + ['model_ema', 'ema']) and list(ck['model_ema']) == list(ck['model'])
    assert all(not torch.equal(ck['model_ema'][k], ck['model'][k]) for k in ck['model'])

    net2, ps2, red2, opt2 = _toy(kind, seed=5, ema_decay=DECAY)          # constructed anew, from other weights
    _, info = checkpoint.load_checkpoint(path, net2, opt2, resume_all=True, map_location='cuda')
    assert info['ema'] == 'restored' and opt2.steps_taken() == 2
    assert all(_same(a['ema'], b['ema']) and _same(a['p'], b['p']) for a, b in zip(opt.flat, opt2.flat))
    for o, q in ((opt, ps), (opt2, ps2)):                                # the third update on both: its warm-up index is 3
        prev = [o.ema_views(p).clone() for p in q]
        o.zero_grad()
        _feed(q, 3)
        o.step()
        torch.cuda.synchronize()
        _check_step(o, q, prev, ema_ref.decay_at(DECAY, True, 3), f'{kind} step 3')
    assert all(_same(a['ema'], b['ema']) and _same(a['p'], b['p']) for a, b in zip(opt.flat, opt2.flat))

    net3, ps3, red3, opt3 = _toy(kind, seed=6)                           # no average: exactly the keys the format had
    opt3.zero_grad()
    _feed(ps3, 1)
    opt3.step()
    path_off = checkpoint.save_checkpoint(str(tmp_path / 'off.ckpt'), net3, opt3, None, 1, ns)
    assert sorted(torch.load(path_off, weights_only=False)) == sorted(PARENT_KEYS)
    net4, ps4, red4, opt4 = _toy(kind, seed=7, ema_decay=DECAY)
    _, info4 = checkpoint.load_checkpoint(path_off, net4, opt4, resume_all=True, map_location='cuda')
    assert 'reseeded' in info4['ema']
    assert all(_same(st['ema'], st['p']) for st in opt4.flat) and all(_same(a, b) for a, b in zip(ps3, ps4))
