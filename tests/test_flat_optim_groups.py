"""CPU half of the flat optimizers' parameter groups and capturable step (the recipe the reference carries commented out at
train.py:76-106: backbone parameters in a group of their own at a tenth of the head's lr): the grouped C entries' surface and
argument validation, the per-bucket run tables, torch's multi-group checkpoint schema both ways, schedulers over several groups,
--lr_backbone and parallel.reference_param_groups.  The kernels themselves are GPU-only: tests/test_gpu_flat_optim_groups.py."""
import argparse
import copy
import os
import re
import warnings

import pytest
import torch

from svol_amd import parallel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['svol_sgd_flat_grouped', 'svol_adam_flat_grouped', 'svol_adamw_flat_grouped', 'svol_flat_step_advance']
CLASSES = {'sgd': (parallel.FlatSGD, torch.optim.SGD), 'adam': (parallel.FlatAdam, torch.optim.Adam),
           'adamw': (parallel.FlatAdamW, torch.optim.AdamW)}


def _lib():
    from svol_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_grouped_entries_are_declared_exported_and_bound():
    L = _lib()
    txt = open(os.path.join(REPO, 'include', 'svol_hip.h')).read()
    decl = set(re.findall(r'\b(svol_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', txt, flags=re.S)))
    for n in NEW:
        assert n in decl, f'{n} not declared in include/svol_hip.h'
        assert n in L.SIGNATURES, f'{n} not in _lib.SIGNATURES'
        assert hasattr(L.lib(), n), f'{n} not exported'
    assert 'train.py:76-106' in txt
    assert L.lib().svol_abi_version() == 7          # new symbols only


def test_grouped_argument_validation_without_gpu():
    """Every check sits in front of the launch, so these calls are safe without a device.  The pointers are made-up addresses: an
    accepted call is only made with n == 0, which returns before anything could touch them."""
    L = _lib().lib()
    A, M = 0x10000, 0x10004                        # 16-byte aligned / misaligned

    def sgd(p=A, g=A, b=A, n=8, ends=A, groups=A, nseg=1, hyper=A, ngroups=1, state=0):
        return L.svol_sgd_flat_grouped(p, g, b, n, ends, groups, nseg, hyper, ngroups, state, 1.0, 0, 0)

    def adam(fn, p=A, g=A, m=A, v=A, n=8, ends=A, groups=A, nseg=1, hyper=A, ngroups=1, state=0, count=A):
        return fn(p, g, m, v, n, ends, groups, nseg, hyper, ngroups, state, count, 1.0, 0, 0)

    assert sgd(p=0) == sgd(g=0) == sgd(b=0) == sgd(ends=0) == sgd(groups=0) == sgd(hyper=0) == -1
    assert sgd(n=-4) == sgd(nseg=0) == sgd(ngroups=0) == sgd(nseg=-1) == -1
    assert sgd(n=0) == sgd(n=0, state=A) == 0
    assert sgd(p=M) == sgd(g=M) == sgd(b=M) == -2
    assert sgd(n=6) == sgd(n=9) == sgd(n=1 << 33) == -2          # no scalar tail: a bucket never has one; seg_end is int32
    for fn in (L.svol_adam_flat_grouped, L.svol_adamw_flat_grouped):
        assert adam(fn, p=0) == adam(fn, g=0) == adam(fn, m=0) == adam(fn, v=0) == -1
        assert adam(fn, ends=0) == adam(fn, groups=0) == adam(fn, hyper=0) == adam(fn, count=0) == -1
        assert adam(fn, n=-4) == adam(fn, nseg=0) == adam(fn, ngroups=0) == adam(fn, n=0, count=0) == -1
        assert adam(fn, n=0) == adam(fn, n=0, state=A) == 0
        assert adam(fn, p=M) == adam(fn, g=M) == adam(fn, m=M) == adam(fn, v=M) == -2
        assert adam(fn, n=6) == adam(fn, n=1 << 33) == -2
    assert L.svol_flat_step_advance(0, 0, 0) == L.svol_flat_step_advance(0, A, 0) == -1


# (17,) and (3,) are padded to a 16-byte boundary; bucket_bytes=160 cuts the list into several buckets
SHAPES = [(6, 5), (5,), (3,), (4, 4), (17,), (2, 2), (8,)]
DEAD = 2


def _params(seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]


def _reducer(ps, **kw):
    return parallel.BucketedGradAllReduce(ps, bucket_bytes=160, skip=[ps[DEAD]], tail_bytes=0, **kw)


def test_run_tables_follow_the_bucket_layout():
    ps = _params()
    red = _reducer(ps)
    assert len(red.buckets) >= 2
    gi = {0: 0, 1: 1, 2: 1, 3: 1, 4: 2, 5: 0, 6: 0}                       # parameter index -> group
    groups = [{'params': [ps[i] for i in gi if gi[i] == k], 'lr': 10.0 ** -k} for k in range(3)]
    fo = parallel.FlatAdamW(red, lr=1.0, params=groups)
    assert fo._grouped and not fo.capturable and len(fo.param_groups) == 3
    assert [g['lr'] for g in fo.param_groups] == [1.0, 0.1, 0.01]
    assert all(g['betas'] == (0.9, 0.999) and g['weight_decay'] == 1e-2 for g in fo.param_groups)      # missing keys: the defaults
    assert len(fo.seg_tables) == len(red.buckets)
    index = {id(p): i for i, p in enumerate(ps)}
    merged = 0
    for b, (ends, grp) in zip(red.buckets, fo.seg_tables):
        assert len(ends) == len(grp) >= 1
        assert all(a < c for a, c in zip(ends, ends[1:])) and ends[0] > 0                                # ascending
        assert ends[-1] * 4 == b['flat'].numel()                                                         # ends at numel / 4
        assert all(a != c for a, c in zip(grp, grp[1:]))                                                 # adjacent equal groups merged
        merged += len(b['params']) - len(ends)
        for p, off in zip(b['params'], b['offsets']):                                                    # every offset maps to its group
            assert off % 4 == 0
            run = next(s for s, e in enumerate(ends) if e > off // 4)
            assert grp[run] == gi[index[id(p)]]
            last = (off + p.numel() - 1) // 4
            assert next(s for s, e in enumerate(ends) if e > last) == run                                # and so does its last vector
        assert fo._seg_dev[red.buckets.index(b)][0].tolist() == ends and fo._seg_dev[red.buckets.index(b)][1].tolist() == grp
        assert fo._seg_dev[0][0].dtype == torch.int32
    assert merged >= 1                                                    # the layout has neighbours of one group
    assert fo._hyper_dev.shape == (3, 8) and fo._hyper_dev[:, 0].tolist() == [1.0, pytest.approx(0.1), pytest.approx(0.01)]
    red.remove()
    # one group + capturable: one run per bucket
    ps = _params()
    red = _reducer(ps)
    fo = parallel.FlatSGD(red, lr=1.0, params=ps, capturable=True)
    assert fo._grouped and all(grp == [0] and ends == [b['flat'].numel() // 4] for b, (ends, grp) in zip(red.buckets, fo.seg_tables))
    assert fo._hyper_dev[0].tolist() == [1.0, pytest.approx(0.9), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    red.remove()
    # one group, not capturable: the plain path, no tables
    ps = _params()
    red = _reducer(ps)
    fo = parallel.FlatAdam(red, params=[{'params': ps}])
    assert not fo._grouped and not hasattr(fo, 'seg_tables') and len(fo.param_groups) == 1
    fo.push_hyper()                                                       # a no-op there
    red.remove()


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'adamw'])
def test_a_missing_or_doubled_parameter_raises(kind):
    Flat = CLASSES[kind][0]
    ps = _params()
    red = _reducer(ps)
    with pytest.raises(ValueError, match='not in `params`'):
        Flat(red, params=[{'params': ps[:3]}, {'params': ps[4:]}])        # ps[3] owns a bucket slot and is in no group
    with pytest.raises(ValueError):
        Flat(red, params=[{'params': ps[:4]}, {'params': ps[3:]}])        # ps[3] in two groups
    with pytest.raises(ValueError):
        Flat(red, params=[{'params': ps[:4] + ps[:1]}, {'params': ps[4:]}])
    Flat(red, params=[{'params': ps[:2] + ps[3:4]}, {'params': ps[4:]}])  # the skipped parameter may be left out, as in the plain form
    red.remove()


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'adamw'])
def test_grouped_path_refuses_step_in_backward(kind):
    Flat = CLASSES[kind][0]
    ps = _params()
    red = _reducer(ps)
    with pytest.raises(ValueError, match='step_in_backward'):
        Flat(red, params=[{'params': ps[:3], 'lr': 1e-3}, {'params': ps[3:]}], step_in_backward=True)
    with pytest.raises(ValueError, match='step_in_backward'):
        Flat(red, params=ps, capturable=True, step_in_backward=True)
    assert red.on_bucket_reduced is None
    red.remove()


KW = {'sgd': (dict(lr=2e-3, momentum=0.8, weight_decay=0.03), dict(lr=2e-2, momentum=0.5, weight_decay=0.0)),
      'adam': (dict(lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.03), dict(lr=2e-2, betas=(0.7, 0.9), eps=1e-6, weight_decay=0.0)),
      'adamw': (dict(lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.03), dict(lr=2e-2, betas=(0.7, 0.9), eps=1e-6, weight_decay=0.0))}
SPLIT = ([0, 2, 4, 6], [1, 3, 5])                  # parameter indices of the two groups: they alternate inside the buckets


def _two_groups(ps, kw0, kw1):
    return [dict(kw0, params=[ps[i] for i in SPLIT[0]]), dict(kw1, params=[ps[i] for i in SPLIT[1]])]


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'adamw'])
def test_two_group_checkpoints_interoperate_with_torch(kind):
    """torch with two groups, stepped on CPU -> flat.load_state_dict -> flat.state_dict() -> a fresh torch optimizer: group 'params'
    lists, per-group hyper-parameters and state tensors round-trip; other group counts or sizes are refused."""
    Flat, Torch = CLASSES[kind]
    kw0, kw1 = KW[kind]
    pt = _params(1)
    opt = Torch(_two_groups(pt, kw0, kw1))
    for _ in range(3):
        opt.zero_grad()
        for i, p in enumerate(pt):
            if i != DEAD:
                p.grad = torch.randn(p.shape)
        opt.step()
    sd = opt.state_dict()
    assert [g['params'] for g in sd['param_groups']] == [[0, 1, 2, 3], [4, 5, 6]]

    pf = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    red = _reducer(pf)
    other = dict(lr=1.0, weight_decay=0.5)
    fo = Flat(red, params=_two_groups(pf, other, other))
    assert fo.state_dict()['state'] == {} and [g['params'] for g in fo.state_dict()['param_groups']] == [[0, 1, 2, 3], [4, 5, 6]]
    fo.load_state_dict(sd)
    for g, kw in zip(fo.param_groups, (kw0, kw1)):
        assert all(g[k] == v for k, v in kw.items()), (g, kw)             # each group's hyper-parameters come from the file
    assert fo.lr == kw0['lr'] and fo.weight_decay == kw0['weight_decay']  # attribute access means group 0
    assert fo._hyper_rows != fo._rows()                                   # the table is stale until push_hyper() (step() calls it)
    fo.push_hyper()
    assert fo._hyper_dev[:, 0].tolist() == [pytest.approx(kw0['lr']), pytest.approx(kw1['lr'])]
    assert fo._hyper_dev[:, 4].tolist() == [pytest.approx(kw0['weight_decay']), pytest.approx(kw1['weight_decay'])]
    if kind != 'sgd':
        assert fo.t == 3 and fo.steps_taken() == 3 and float(fo._step_dev) == 3.0      # the device count the kernels read
    out = fo.state_dict()
    assert [g['params'] for g in out['param_groups']] == [[0, 1, 2, 3], [4, 5, 6]]
    for go, gs in zip(out['param_groups'], sd['param_groups']):
        assert set(go) <= set(gs)          # (FlatAdamW's groups carry no 'decoupled_weight_decay' key, torch AdamW's may)
        assert all(go[k] == gs[k] for k in kw0)
    dead = SPLIT[0].index(DEAD)                                           # position 1 of group 0
    assert sorted(out['state']) == sorted(sd['state']) == [i for i in range(7) if i != dead]
    for i, ent in out['state'].items():
        assert set(ent) == set(sd['state'][i])
        for k in ent:
            assert torch.equal(ent[k], sd['state'][i][k]), (i, k)
    fresh = Torch(_two_groups([torch.nn.Parameter(p.detach().clone()) for p in pt], other, other))
    fresh.load_state_dict(out)                                            # torch accepts what the flat class writes
    back = fresh.state_dict()
    for g, kw in zip(fresh.param_groups, (kw0, kw1)):
        assert all(g[k] == v for k, v in kw.items())
    assert all(torch.equal(back['state'][i][k], sd['state'][i][k]) for i in sd['state'] for k in sd['state'][i])
    # another group count, other group sizes
    g0, g1 = sd['param_groups']
    bad = copy.deepcopy(sd)
    bad['param_groups'] = [dict(g0, params=[0, 1]), dict(g0, params=[2, 3]), g1]
    with pytest.raises(ValueError, match='3 parameter groups'):
        fo.load_state_dict(bad)
    bad = copy.deepcopy(sd)
    bad['param_groups'] = [dict(g0, params=[0, 1, 2, 3, 4, 5, 6])]
    with pytest.raises(ValueError, match='1 parameter groups'):
        fo.load_state_dict(bad)
    bad = copy.deepcopy(sd)
    bad['param_groups'] = [dict(g0, params=[0, 1, 2]), dict(g1, params=[3, 4, 5, 6])]
    with pytest.raises(ValueError, match='sizes'):
        fo.load_state_dict(bad)
    bad = copy.deepcopy(sd)
    bad['param_groups'][1]['maximize'] = True                             # an unsupported option in ANY group
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    red.remove()


def test_sgd_group_without_momentum_keeps_no_buffers():
    """torch SGD keeps a momentum buffer only for the parameters of a group whose momentum is not 0; so does the file written here."""
    pf = _params(2)
    red = _reducer(pf)
    fo = parallel.FlatSGD(red, lr=1e-3, params=_two_groups(pf, dict(momentum=0.0), dict(momentum=0.9)))
    fo.t = 1
    fo._sync_count()
    assert sorted(fo.state_dict()['state']) == [4, 5, 6]
    red.remove()


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'adamw'])
def test_step_lr_scales_every_group(kind):
    pf = _params()
    red = _reducer(pf)
    fo = CLASSES[kind][0](red, params=_two_groups(pf, dict(lr=3e-3), dict(lr=3e-2)))
    sched = torch.optim.lr_scheduler.StepLR(fo, step_size=1, gamma=0.1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')            # "lr_scheduler.step() before optimizer.step()"
        sched.step()
    assert [g['lr'] for g in fo.param_groups] == [pytest.approx(3e-4, rel=1e-12), pytest.approx(3e-3, rel=1e-12)]
    assert fo.lr == fo.param_groups[0]['lr']
    fo.push_hyper()
    assert fo._hyper_dev[:, 0].tolist() == [pytest.approx(3e-4), pytest.approx(3e-3)]
    rows = fo._hyper_rows
    fo.push_hyper()                                # nothing changed: nothing uploaded
    assert fo._hyper_rows is rows
    red.remove()


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.Linear(6, 6))
        self.head = torch.nn.Linear(6, 3)
        self.norm = torch.nn.LayerNorm(3)


def test_lr_backbone_option_and_reference_param_groups():
    from svol_amd import configs
    assert configs.parse_args([]).lr_backbone is None
    a = configs.parse_args(['--optimizer', 'adamw', '--lr', '0.001', '--lr_backbone', '0.0001', '--wd', '0.01'])
    assert a.lr_backbone == 1e-4 and 'lr_backbone' not in configs.reference_defaults()
    model = _Model()
    groups = parallel.reference_param_groups(model, a)
    assert [set(g) for g in groups] == [{'params', 'lr'}] * 2 and [g['lr'] for g in groups] == [1e-4, 1e-3]
    names = {id(p): n for n, p in model.named_parameters()}
    assert [names[id(p)] for p in groups[0]['params']] == ['backbone.0.weight', 'backbone.0.bias', 'backbone.1.weight', 'backbone.1.bias']
    assert [names[id(p)] for p in groups[1]['params']] == ['head.weight', 'head.bias', 'norm.weight', 'norm.bias']
    # build_optimizer hands the groups on
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), bucket_bytes=96, ordered=True, tail_bytes=0)
    opt = parallel.build_optimizer(a, red, groups, capturable=True)
    assert type(opt) is parallel.FlatAdamW and opt.capturable and len(opt.param_groups) == 2
    assert [g['lr'] for g in opt.param_groups] == [1e-4, 1e-3] and all(g['weight_decay'] == 0.01 for g in opt.param_groups)
    assert [len(g['params']) for g in opt.param_groups] == [4, 4]
    assert sum(len(e) for e, _ in opt.seg_tables) >= 2
    red.remove()
    # one group: no --lr_backbone, or nothing of the backbone trains
    one = parallel.reference_param_groups(model, configs.parse_args([]))
    assert len(one) == 1 and set(one[0]) == {'params'} and len(one[0]['params']) == 8
    for p in model.backbone.parameters():
        p.requires_grad_(False)
    one = parallel.reference_param_groups(model, a)
    assert len(one) == 1 and [names[id(p)] for p in one[0]['params']] == ['head.weight', 'head.bias', 'norm.weight', 'norm.bias']
    red = parallel.BucketedGradAllReduce(one[0]['params'])
    opt = parallel.build_optimizer(argparse.Namespace(optimizer='sgd', lr=1e-3, wd=0.0), red, one)
    assert type(opt) is parallel.FlatSGD and not opt._grouped and len(opt.param_groups) == 1
    red.remove()
