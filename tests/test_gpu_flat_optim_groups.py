"""Parameter groups and the capturable step of the flat optimizers on the device: the ..._grouped C entries in a guard arena against
the three rules written out in fp64, then parallel.FlatSGD / FlatAdam / FlatAdamW with two and three groups against the torch
optimizer of the same name built with the same groups — plain, zeroing, under StepLR, through checkpoints both ways, under the
dynamic loss scaler, clipped, and captured into a graph and replayed.

The parity bar is the project's own for this comparison (tests/test_gpu_flat_optim.py): max|a - b| <= 2e-6 * max(1, max|b|) per
tensor, 4e-6 after a checkpoint round trip plus further steps.  For that bar to SEE a wrong group lookup the groups' learning rates
differ by 10x (3e-3 / 3e-2: Adam moves a parameter by about lr per step, three orders above the bar) and one group is frozen
(lr = 0, weight_decay = 0), which leaves p bit-identical under all three rules (p - 0 * x, p * 1) and so tags every element with the
group the kernel gave it."""
import warnings

import pytest
import torch

from tests.test_gpu_flat_optim import DEAD, SHAPES, _close, _grads, _mk, _p0

pytestmark = pytest.mark.gpu

KINDS = ['sgd', 'adam', 'adamw']
# per group: a tenth of the lr with decay / the lr without (biases and norms) / frozen
GROUP_KW = {'sgd': [dict(lr=3e-3, momentum=0.9, weight_decay=0.05), dict(lr=3e-2, momentum=0.5, weight_decay=0.0),
                    dict(lr=0.0, momentum=0.9, weight_decay=0.0)],
            'adam': [dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05), dict(lr=3e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0),
                     dict(lr=0.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]}
GROUP_KW['adamw'] = GROUP_KW['adam']


def _classes(kind):
    from svol_amd import parallel
    return {'sgd': (parallel.FlatSGD, torch.optim.SGD), 'adam': (parallel.FlatAdam, torch.optim.Adam),
            'adamw': (parallel.FlatAdamW, torch.optim.AdamW)}[kind]


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
# run lengths in float4s against one float4 per thread in 256-thread workgroups: single-vector runs at the very start, a boundary on
# a wave edge (64), on workgroup edges (256, 512), one past a workgroup edge (1025), a run over more than two workgroups, a short
# last run in a partial workgroup
ENDS = [1, 2, 64, 256, 512, 1025, 1028]
GROUPS = [0, 1, 0, 2, 1, 0, 2]
N = 4 * ENDS[-1]
STEP_COUNT = 2.0


def _rows(kind, equal=False):
    rows = []
    for kw in GROUP_KW[kind]:
        kw = GROUP_KW[kind][0] if equal else kw
        mid = [kw['momentum'], 0.0, 0.0] if kind == 'sgd' else [kw['betas'][0], kw['betas'][1], kw['eps']]
        rows.append([kw['lr']] + mid + [kw['weight_decay'], 0.0, 0.0, 0.0])
    return torch.tensor(rows, dtype=torch.float32)


def _per_element(ends, groups, rows, n):
    """the table's row of every element, in double"""
    lens = torch.tensor([4 * (e - s) for s, e in zip([0] + ends[:-1], ends)])
    assert int(lens.sum()) == n
    return rows.double()[torch.tensor(groups)].repeat_interleave(lens, dim=0).cuda()      # [n, 8]


def _rule_fp64(kind, src, per, gscale, step):
    p, g, a, b = (src[k].double() for k in ('p', 'g', 'a', 'b'))
    lr, c1, c2, eps, wd = (per[:, j] for j in range(5))
    g = g * gscale
    if kind == 'sgd':
        buf = c1 * a + (g + wd * p)
        return {'p': p - lr * buf, 'a': buf}
    if kind == 'adamw':
        p, d = p * (1 - lr * wd), g
    else:
        d = g + wd * p
    m, v = a + (d - a) * (1 - c1), b * c2 + (1 - c2) * d * d
    return {'p': p - lr / (1 - c1 ** step) * m / (v.sqrt() / (1 - c2 ** step).sqrt() + eps), 'a': m, 'b': v}


def _entry(kind, src, ends, groups, rows, zero=0, state=None, grad_mul=1.0):
    """one launch over copies of `src` carved out of a guard arena, tables included; returns the arena's tensors after the guard check"""
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    from tests.test_gpu_guards import GuardArena
    n = src['p'].numel()
    ar = GuardArena(guard_bytes=1 << 12)
    for k in ('p', 'g', 'a', 'b'):
        ar.plan(k, (n,), torch.float32)
    ar.plan('state', (4,), torch.float32)
    ar.plan('count', (1,), torch.float32)
    ar.plan('ends', (len(ends),), torch.int32)
    ar.plan('groups', (len(ends),), torch.int32)
    ar.plan('hyper', tuple(rows.shape), torch.float32)
    t = ar.build()
    for k in ('p', 'g', 'a', 'b'):
        t[k].copy_(src[k])
    t['state'].copy_(torch.tensor(state if state is not None else [0.0] * 4))
    t['count'].fill_(STEP_COUNT)
    t['ends'].copy_(torch.tensor(ends, dtype=torch.int32))
    t['groups'].copy_(torch.tensor(groups, dtype=torch.int32))
    t['hyper'].copy_(rows)
    name = f'svol_{kind}_flat_grouped'
    args = [_ptr(t['p']), _ptr(t['g']), _ptr(t['a'])] + ([] if kind == 'sgd' else [_ptr(t['b'])])
    args += [n, _ptr(t['ends']), _ptr(t['groups']), len(ends), _ptr(t['hyper']), rows.shape[0], _ptr(t['state']) if state is not None else 0]
    args += ([] if kind == 'sgd' else [_ptr(t['count'])]) + [grad_mul, zero]
    _lib.check(getattr(_lib.lib(), name)(*args, _stream()), name)
    torch.cuda.synchronize()
    ar.check(f'{name} n={n} nseg={len(ends)} zero={zero}')
    assert float(t['count']) == STEP_COUNT and t['ends'].tolist() == ends        # the entries only read their tables and the count
    return t


def _src(n, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    src = {k: torch.randn(n, device='cuda', generator=gen) for k in ('p', 'g', 'a', 'b')}
    src['b'] = src['b'].abs()
    return src


@pytest.mark.parametrize('kind', KINDS)
def test_grouped_entries_in_a_guard_arena(kind):
    keys = ('p', 'a') if kind == 'sgd' else ('p', 'a', 'b')
    src, rows = _src(N, 11), _rows(kind)
    per = _per_element(ENDS, GROUPS, rows, N)
    frozen = per[:, 0] == 0
    assert 0 < int(frozen.sum()) == 4 * (192 + 3)

    base = _entry(kind, src, ENDS, GROUPS, rows)
    assert torch.equal(base['p'][frozen], src['p'][frozen])                  # frozen runs: exact
    assert bool((base['p'][~frozen] != src['p'][~frozen]).any()) and torch.equal(base['g'], src['g'])
    want = _rule_fp64(kind, src, per, 1.0, STEP_COUNT + 1)
    for k in keys:
        _close(base[k], want[k].float(), 2e-6, f'{kind} seven runs {k} against fp64')
        for s, e in zip([0] + ENDS[:-1], ENDS):                              # run by run: a short run does not hide behind a long one's maximum
            _close(base[k][4 * s:4 * e], want[k][4 * s:4 * e].float(), 2e-6, f'{kind} run [{s}, {e}) {k}')

    zeroed = _entry(kind, src, ENDS, GROUPS, rows, zero=1)
    assert all(torch.equal(zeroed[k], base[k]) for k in keys) and bool((zeroed['g'] == 0).all())

    for zero in (0, 1):                                                      # a set overflow flag: nothing at all is written
        skipped = _entry(kind, src, ENDS, GROUPS, rows, zero=zero, state=[4.0, 1.0, 0.0, 7.0])
        assert all(torch.equal(skipped[k], src[k]) for k in ('p', 'g', 'a', 'b'))

    unit = _entry(kind, src, ENDS, GROUPS, rows, state=[1.0, 0.0, 5.0, 9.0])   # ([3] is not the step: the count is)
    assert all(torch.equal(unit[k], base[k]) for k in keys)
    scaled = _entry(kind, src, ENDS, GROUPS, rows, state=[8.0, 0.0, 0.0, 0.0], grad_mul=2.0)
    want4 = _rule_fp64(kind, src, per, 0.25, STEP_COUNT + 1)
    for k in keys:
        _close(scaled[k], want4[k].float(), 2e-6, f'{kind} grad_mul 2 / scale 8 {k}')
    assert not torch.equal(scaled['p'], base['p'])

    # regrouping invariance: with all rows equal the seven-run and the one-run table are the same arithmetic
    same = _rows(kind, equal=True)
    seven, one = _entry(kind, src, ENDS, GROUPS, same), _entry(kind, src, [N // 4], [1], same)
    assert all(torch.equal(seven[k], one[k]) for k in keys)
    assert not torch.equal(seven['p'][frozen], src['p'][frozen])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [4, 4000])
def test_grouped_entries_with_one_run(kind, n):
    keys = ('p', 'a') if kind == 'sgd' else ('p', 'a', 'b')
    src, rows = _src(n, n), _rows(kind)
    for group in (0, 1):
        got = _entry(kind, src, [n // 4], [group], rows, zero=1)
        want = _rule_fp64(kind, src, _per_element([n // 4], [group], rows, n), 1.0, STEP_COUNT + 1)
        for k in keys:
            _close(got[k], want[k].float(), 2e-6, f'{kind} n={n} group {group} {k}')
        assert bool((got['g'] == 0).all())
    got = _entry(kind, src, [n // 4], [2], rows)
    assert torch.equal(got['p'], src['p'])


def test_flat_step_advance():
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    from tests.test_gpu_guards import GuardArena
    ar = GuardArena(guard_bytes=1 << 12)
    ar.plan('count', (1,), torch.float32)
    ar.plan('state', (4,), torch.float32)
    t = ar.build()
    t['count'].fill_(2.0)
    f = _lib.lib().svol_flat_step_advance
    for state, want in (([4.0, 0.0, 0.0, 0.0], 3.0), ([4.0, 1.0, 0.0, 0.0], 3.0), (None, 4.0), ([1.0, 0.0, 0.0, 0.0], 5.0)):
        if state is not None:
            t['state'].copy_(torch.tensor(state))
        _lib.check(f(_ptr(t['count']), _ptr(t['state']) if state is not None else 0, _stream()), 'svol_flat_step_advance')
        torch.cuda.synchronize()
        assert float(t['count']) == want, (state, float(t['count']))
        assert state is None or t['state'].tolist() == state
    ar.check('svol_flat_step_advance')


# ---- through the classes -----------------------------------------------------------------------------------------------------------
def _groups(ps, kind, ngroups, **override):
    """assigned alternately by parameter index, so that runs alternate inside the buckets"""
    return [dict(GROUP_KW[kind][k], params=[p for i, p in enumerate(ps) if i % ngroups == k], **override) for k in range(ngroups)]


def _flat(kind, src, ngroups, skip_dead=True, **kw):
    from svol_amd import parallel
    ps = _mk(src)
    red = parallel.BucketedGradAllReduce(ps, bucket_bytes=40000, skip=[ps[DEAD]] if skip_dead else None)
    assert len(red.buckets) >= 2
    opt = _classes(kind)[0](red, params=_groups(ps, kind, ngroups), **kw)
    assert opt._grouped and max(len(e) for e, _ in opt.seg_tables) >= 2        # runs alternate inside a bucket
    return ps, red, opt


def _torch(kind, src, ngroups):
    ps = _mk(src)
    return ps, _classes(kind)[1](_groups(ps, kind, ngroups))


def _steps(ps, opt, steps, sched=None, seed=100, skip_dead=True, fill=None):
    """identical gradients into a flat optimizer's bucket views or a torch optimizer's .grad"""
    flat = hasattr(opt, 'reducer')
    for st in steps:
        opt.zero_grad()
        for i, (p, g) in enumerate(zip(ps, _grads(st, seed=seed))):
            if i != DEAD or not skip_dead:
                if flat:
                    p.grad.copy_(g)
                else:
                    p.grad = g.clone()
        opt.step()
        if sched is not None:
            sched.step()


def _all_close(pa, pb, bar, what):
    for i, (a, b) in enumerate(zip(pa, pb)):
        _close(a, b, bar, f'{what} parameter {i}')


@pytest.mark.parametrize('zero_grads', [False, True], ids=['plain', 'zero_grads'])
@pytest.mark.parametrize('ngroups', [2, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_groups_match_torch(kind, ngroups, zero_grads):
    p0 = _p0()
    pa, red, oa = _flat(kind, p0, ngroups, zero_grads=zero_grads)
    pb, ob = _torch(kind, p0, ngroups)
    _steps(pa, oa, range(5))
    _steps(pb, ob, range(5))
    _all_close(pa, pb, 2e-6, f'{kind} {ngroups} groups')
    assert torch.equal(pa[DEAD].detach(), p0[DEAD]) and oa.steps_taken() == 5
    if ngroups == 3:        # group 2 is frozen: exact
        assert all(torch.equal(a.detach(), p) for i, (a, p) in enumerate(zip(pa, p0)) if i % 3 == 2)
    assert all(bool(b.get('clean')) == zero_grads and bool((b['flat'] == 0).all()) == zero_grads for b in red.buckets)
    for b in red.buckets:   # the padding floats of every parameter stayed zero
        pad = torch.ones_like(b['flat'], dtype=torch.bool)
        for p, off in zip(b['params'], b['offsets']):
            pad[off:off + p.numel()] = False
        st = oa.flat[red.buckets.index(b)]
        assert all(bool((st[k][pad] == 0).all()) for k in st)


@pytest.mark.parametrize('kind', KINDS)
def test_step_lr_reaches_the_kernel_on_the_next_step(kind):
    p0 = _p0(5)
    pa, red, oa = _flat(kind, p0, 2)
    pb, ob = _torch(kind, p0, 2)
    sa = torch.optim.lr_scheduler.StepLR(oa, step_size=2, gamma=0.1)
    sb = torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.1)
    for st in range(5):
        _steps(pa, oa, [st], sa)
        _steps(pb, ob, [st], sb)
        _all_close(pa, pb, 2e-6, f'{kind} StepLR step {st}')
    assert [g['lr'] for g in oa.param_groups] == [g['lr'] for g in ob.param_groups] == [pytest.approx(3e-5), pytest.approx(3e-4)]


@pytest.mark.parametrize('kind', KINDS)
def test_two_group_checkpoints_interoperate_with_torch_mid_run(kind):
    """torch, 2 steps -> state_dict -> flat.load_state_dict -> 2 more steps on both == the same weights; and back: what the flat class
    writes resumes a fresh torch optimizer.  The StepLR has already halved both groups' lr when the file is written and halves
    them again in each further leg; the schedulers built on the loading side start from other settings, which the files overwrite."""
    p0 = _p0(1)
    pr, o_r = _torch(kind, p0, 2)
    s_r = torch.optim.lr_scheduler.StepLR(o_r, step_size=2, gamma=0.5)
    _steps(pr, o_r, range(4), s_r)

    pa, o_a = _torch(kind, p0, 2)
    s_a = torch.optim.lr_scheduler.StepLR(o_a, step_size=2, gamma=0.5)
    _steps(pa, o_a, range(2), s_a)
    sd_opt, sd_sched = o_a.state_dict(), s_a.state_dict()
    assert [g['lr'] for g in sd_opt['param_groups']] == [1.5e-3, 1.5e-2]
    from svol_amd import parallel
    pb = _mk(pa)
    red = parallel.BucketedGradAllReduce(pb, bucket_bytes=40000, skip=[pb[DEAD]])
    o_b = _classes(kind)[0](red, params=_groups(pb, kind, 2, lr=1.0, weight_decay=0.5))       # all overwritten by the load
    s_b = torch.optim.lr_scheduler.StepLR(o_b, step_size=1, gamma=0.9)                      # (overwritten by the file's)
    o_b.load_state_dict(sd_opt)
    s_b.load_state_dict(sd_sched)
    assert all(g[k] == v for g, kw in zip(o_b.param_groups, GROUP_KW[kind]) for k, v in kw.items() if k != 'lr')
    assert [(g['lr'], g['initial_lr']) for g in o_b.param_groups] == [(1.5e-3, 3e-3), (1.5e-2, 3e-2)]
    assert o_b.steps_taken() == (2 if kind != 'sgd' else 1)
    _steps(pb, o_b, range(2, 4), s_b)
    _all_close(pb, pr, 2e-6, f'{kind} torch -> flat,')
    assert [g['lr'] for g in o_b.param_groups] == [g['lr'] for g in o_r.param_groups] == [7.5e-4, 7.5e-3]

    sd_b = o_b.state_dict()
    assert [g['params'] for g in sd_b['param_groups']] == [g['params'] for g in sd_opt['param_groups']]
    assert sorted(sd_b['state']) == sorted(sd_opt['state']) and len(sd_b['state']) == len(SHAPES) - 1
    pc = _mk(pb)
    o_c = _classes(kind)[1](_groups(pc, kind, 2, lr=1.0, weight_decay=0.5))
    o_c.load_state_dict(sd_b)
    s_c = torch.optim.lr_scheduler.StepLR(o_c, step_size=1, gamma=0.9)
    s_c.load_state_dict(s_b.state_dict())
    _steps(pc, o_c, [4, 5], s_c)
    _steps(pr, o_r, [4, 5], s_r)
    _all_close(pc, pr, 4e-6, f'{kind} flat -> torch,')


@pytest.mark.parametrize('kind', KINDS)
def test_dynamic_loss_scaler_skips_every_group_and_follows_torch(kind):
    """tests/test_gpu_flat_optim.py's scaler test with three groups: a step with an inf anywhere changes nothing in ANY group and does
    not count; clean steps equal the grouped torch optimizer on the unscaled gradients."""
    from svol_amd import parallel
    p0 = _p0()
    pa, red, oa = _flat(kind, p0, 3, skip_dead=False)
    sc = oa.scaler = parallel.DynamicLossScaler(torch.device('cuda'), init_scale=1024.0, growth_interval=3)
    pb, ob = _torch(kind, p0, 3)
    scale, clean_run, taken = 1024.0, 0, 0
    for step in range(7):
        red.zero_grad()
        ob.zero_grad()
        overflow = step in (0, 3)                   # (step 0: the very first bias-correction step is still 1 afterwards)
        gs = _grads(step, seed=300)
        for a, g in zip(pa, gs):
            a.grad.copy_(g * scale)
        if overflow:
            pa[4].grad.view(-1)[7] = float('inf')
        before = [p.detach().clone() for p in pa]
        state = [{k: v.clone() for k, v in st.items()} for st in oa.flat]
        oa.step()
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
            _all_close(pa, pb, 2e-6, f'{kind} scaled step {step}')
        assert oa.steps_taken() == taken and sc.state.tolist()[:2] == [scale, 0.0], (step, sc.state.tolist(), scale, taken)
    assert oa.steps_taken() == 5


@pytest.mark.parametrize('kind', KINDS)
def test_clipped_groups_match_clip_grad_norm_and_torch(kind):
    """max_grad_norm with a static loss scale and a pending 1 / world: the buckets hold gradient * 8 * 2, the norm and the update are
    those of the true gradient."""
    p0 = _p0(6)
    pa, red, oa = _flat(kind, p0, 2, skip_dead=False, max_grad_norm=5.0)
    oa.loss_scale = 8.0
    pb, ob = _torch(kind, p0, 2)
    for st in range(4):
        red.zero_grad()
        ob.zero_grad()
        gs = _grads(st, seed=700)
        for a, b, g in zip(pa, pb, gs):
            a.grad.copy_(g * 16.0)
            b.grad = g.clone()
        red.pending_scale = 0.5
        oa.step()
        total = torch.nn.utils.clip_grad_norm_(pb, 5.0)
        ob.step()
        assert float(total) > 5.0
        _close(oa.grad_norm, total, 2e-6, f'{kind} step {st}: grad_norm')      # (the bar tests/test_gpu_grad_clip.py holds it to)
        _all_close(pa, pb, 2e-6, f'{kind} clipped step {st}')
    assert oa.steps_taken() == 4
    # the same factors without clipping
    pa, red, oa = _flat(kind, p0, 2, skip_dead=False)
    oa.loss_scale = 8.0
    pb, ob = _torch(kind, p0, 2)
    for st in range(3):
        red.zero_grad()
        for a, g in zip(pa, _grads(st, seed=700)):
            a.grad.copy_(g * 16.0)
        red.pending_scale = 0.5
        oa.step()
    _steps(pb, ob, range(3), seed=700, skip_dead=False)
    _all_close(pa, pb, 2e-6, f'{kind} loss_scale 8, 1 / world')


@pytest.mark.parametrize('ngroups', [1, 2])
@pytest.mark.parametrize('kind', KINDS)
def test_captured_step_replays_with_the_schedule(kind, ngroups):
    """capturable=True: opt.step() alone captured on a side stream (one chain of launches), replayed five times with new gradients
    copied into the buckets, scheduler.step() and push_hyper() between replays — against eager torch over the same gradients and
    schedule.  The bias correction advances and the lr follows the schedule under replay: nothing of either is baked into the graph."""
    from svol_amd import parallel
    p0 = _p0(7)
    pa = _mk(p0)
    red = parallel.BucketedGradAllReduce(pa, bucket_bytes=40000, skip=[pa[DEAD]])
    oa = _classes(kind)[0](red, params=_groups(pa, kind, ngroups), capturable=True)
    assert oa._grouped and len(oa.param_groups) == ngroups
    pb, ob = _torch(kind, p0, ngroups)
    sa = torch.optim.lr_scheduler.StepLR(oa, step_size=2, gamma=0.1)
    sb = torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.1)
    _steps(pa, oa, [0], sa)                          # one eager step: the captured ones continue its device count
    oa.push_hyper()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        oa.step()
    torch.cuda.current_stream().wait_stream(side)
    assert oa.steps_taken() == 1                     # capturing ran nothing
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')              # "lr_scheduler.step() before optimizer.step()": the replays are the steps
        for st in range(1, 6):
            for i, (p, g) in enumerate(zip(pa, _grads(st))):
                if i != DEAD:
                    p.grad.copy_(g)
            graph.replay()
            sa.step()
            oa.push_hyper()
    _steps(pb, ob, range(6), sb)
    torch.cuda.synchronize()
    assert oa.steps_taken() == 6
    assert [g['lr'] for g in oa.param_groups] == pytest.approx([g['lr'] for g in ob.param_groups])
    assert oa.param_groups[0]['lr'] == pytest.approx(3e-6)
    _all_close(pa, pb, 2e-6, f'{kind} {ngroups} group(s) captured')
    assert torch.equal(pa[DEAD].detach(), p0[DEAD])


@pytest.mark.parametrize('kind', KINDS)
def test_one_group_not_capturable_is_the_plain_path(kind):
    """params as a list of ONE dict and capturable=False: launch for launch the plain path, bit-identical to the plain list form."""
    from svol_amd import parallel
    p0 = _p0(8)
    out = []
    for as_dicts in (False, True):
        ps = _mk(p0)
        red = parallel.BucketedGradAllReduce(ps, bucket_bytes=40000, skip=[ps[DEAD]])
        opt = _classes(kind)[0](red, params=[dict(GROUP_KW[kind][0], params=ps)] if as_dicts else ps, **GROUP_KW[kind][0])
        assert not opt._grouped and len(opt.param_groups) == 1
        _steps(ps, opt, range(3))
        assert opt.steps_taken() == opt.t == 3
        out.append((ps, opt))
    (pa, oa), (pb, ob) = out
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(pa, pb))
    assert all(torch.equal(sa[k], sb[k]) for sa, sb in zip(oa.flat, ob.flat) for k in sa)


def test_graphed_train_step_drives_a_two_group_flat_optimizer_and_its_scheduler():
    """graph.GraphedTrainStep over the tiny head of tests/test_gpu_flat_optim.py's training run with the optimizer a reference-style
    driver builds (build_optimizer over two groups, capturable=True) and a StepLR with gamma 0: the whole step is captured once;
    every replay is an update (the device count advances, the parameters of both groups move), and once the scheduler has set
    both groups' lr to 0 the replays leave every parameter bit-identical — the edit reached the captured kernels through
    push_hyper(), which GraphedTrainStep calls itself.  (Weight decay 0, so that lr = 0 freezes AdamW exactly.)"""
    import argparse
    from svol_amd import parallel
    from svol_amd import synthetic as syn
    from svol_amd.graph import GraphedTrainStep
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.svanet import build_svanet
    args = syn.head_args(hidden_dim=128, nheads=8, num_layers=2, num_queries=20, num_frames=8, input_vid_dim=64, input_skch_dim=64,
                         input_dropout=0.0, matcher='video_matcher')
    args.compute_dtype = 'bf16'
    torch.manual_seed(1)
    model = build_svanet(args).cuda().train()
    crit = build_loss(args).cuda().train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{'params': [p for n, p in named if n.endswith('bias')], 'lr': 2e-4}, {'params': [p for n, p in named if not n.endswith('bias')]}]
    assert all(len(g['params']) > 4 for g in groups)
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
    opt = parallel.build_optimizer(argparse.Namespace(optimizer='adamw', lr=2e-3, wd=0.0), red, groups, capturable=True)
    assert type(opt) is parallel.FlatAdamW and opt._grouped and max(len(e) for e, _ in opt.seg_tables) > 10
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.0)
    B, T, P = 2, 8, 32
    inp = {k: v.cuda() for k, v in syn.synth_inputs(args, B, T, P, seed=3).items()}
    tg = syn.synth_targets(B, T, seed=3)
    gstep = GraphedTrainStep(model, crit, opt, red, inp, tg)
    live = [p for b in red.buckets for p in b['params']]
    assert opt.steps_taken() == 3                                  # the eager warm-up steps; the capture itself ran nothing
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                            # "lr_scheduler.step() before optimizer.step()"
        for k in range(5):
            before = [p.detach().clone() for p in live]
            loss, _ = gstep(inp, tg)
            sched.step()
            moved = [not torch.equal(a, p.detach()) for a, p in zip(before, live)]
            assert bool(torch.isfinite(loss)) and opt.steps_taken() == 4 + k
            if k < 3:                                              # lr 2e-4 / 2e-3
                assert sum(moved) > len(moved) // 2 and any(m for m, p in zip(moved, live) if p.dim() == 1), (k, sum(moved))
            else:                                                  # both groups at lr 0 since the third scheduler step
                assert not any(moved), (k, sum(moved))
    assert [g['lr'] for g in opt.param_groups] == [0.0, 0.0]
