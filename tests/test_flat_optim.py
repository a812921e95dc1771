"""CPU half of the flat SGD / Adam optimizers (the reference's --optimizer sgd | adam, train.py:94-97): the C-ABI surface and its
argument validation, the torch checkpoint schema on load and save, and parallel.build_optimizer's dispatch.  The update kernels
themselves are GPU-only: tests/test_gpu_flat_optim.py."""
import argparse
import copy
import os
import re
import warnings

import pytest
import torch

from svol_amd import parallel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['svol_sgd_flat', 'svol_sgd_flat_zero', 'svol_sgd_flat_scaled', 'svol_adam_flat', 'svol_adam_flat_zero', 'svol_adam_flat_scaled']


def _lib():
    from svol_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_new_entries_are_declared_exported_and_bound():
    L = _lib()
    txt = open(os.path.join(REPO, 'include', 'svol_hip.h')).read()
    decl = set(re.findall(r'\b(svol_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', txt, flags=re.S)))
    for n in NEW:
        assert n in decl, f'{n} not declared in include/svol_hip.h'
        assert n in L.SIGNATURES, f'{n} not in _lib.SIGNATURES'
        assert hasattr(L.lib(), n), f'{n} not exported'
    assert 'train.py:94' in txt and 'train.py:96' in txt
    assert L.lib().svol_abi_version() == 7          # new symbols only


def test_argument_validation_without_gpu():
    """Every check sits in front of the launch, so these calls are safe without a device.  The pointers are made-up addresses:
    an accepted call is only made with n == 0, which returns before anything could touch them."""
    L = _lib().lib()
    A, M = 0x10000, 0x10004                        # 16-byte aligned / misaligned
    sgd = lambda fn, p, g, b, n: fn(p, g, b, n, 0.1, 0.9, 0.0, 1.0, 0)
    adam = lambda fn, p, g, m, v, n, step: fn(p, g, m, v, n, 0.1, 0.9, 0.999, 1e-8, 0.0, step, 1.0, 0)
    for fn in (L.svol_sgd_flat, L.svol_sgd_flat_zero):
        assert sgd(fn, 0, A, A, 8) == sgd(fn, A, 0, A, 8) == sgd(fn, A, A, 0, 8) == -1
        assert sgd(fn, A, A, A, -1) == -1
        assert sgd(fn, A, A, A, 0) == 0
        assert sgd(fn, M, A, A, 8) == sgd(fn, A, M, A, 8) == sgd(fn, A, A, M, 8) == -2
    for fn in (L.svol_adam_flat, L.svol_adam_flat_zero):
        assert adam(fn, 0, A, A, A, 8, 1) == adam(fn, A, 0, A, A, 8, 1) == adam(fn, A, A, 0, A, 8, 1) == adam(fn, A, A, A, 0, 8, 1) == -1
        assert adam(fn, A, A, A, A, -1, 1) == -1
        assert adam(fn, A, A, A, A, 8, 0) == adam(fn, A, A, A, A, 8, -3) == adam(fn, A, A, A, A, 0, 0) == -1
        assert adam(fn, A, A, A, A, 0, 1) == 0
        assert adam(fn, M, A, A, A, 8, 1) == adam(fn, A, M, A, A, 8, 1) == adam(fn, A, A, M, A, 8, 1) == adam(fn, A, A, A, M, 8, 1) == -2
    f = L.svol_sgd_flat_scaled
    assert f(0, A, A, 8, 0.1, 0.9, 0.0, 1.0, A, 0) == f(A, A, A, 8, 0.1, 0.9, 0.0, 1.0, 0, 0) == f(A, A, A, -1, 0.1, 0.9, 0.0, 1.0, A, 0) == -1
    assert f(A, A, A, 0, 0.1, 0.9, 0.0, 1.0, A, 0) == 0 and f(A, A, M, 8, 0.1, 0.9, 0.0, 1.0, A, 0) == -2
    f = L.svol_adam_flat_scaled
    assert f(A, A, A, 0, 8, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, A, 0) == f(A, A, A, A, 8, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 0) == -1
    assert f(A, A, A, A, -1, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, A, 0) == -1
    assert f(A, A, A, A, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, A, 0) == 0 and f(A, M, A, A, 8, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, A, 0) == -2


SHAPES = [(6, 5), (5,), (3,), (4, 4)]
DEAD = 2


def _torch_run(cls, **kw):
    torch.manual_seed(0)
    pt = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    opt = cls(pt, **kw)
    for _ in range(3):
        opt.zero_grad()
        for i, p in enumerate(pt):
            if i != DEAD:
                p.grad = torch.randn(p.shape)
        opt.step()
    return pt, opt


def _flat(cls, pt, **kw):
    pf = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    red = parallel.BucketedGradAllReduce(pf, bucket_bytes=64, skip=[pf[DEAD]])
    assert len(red.buckets) > 1
    fo = cls(red, params=pf, **kw)
    assert isinstance(fo, torch.optim.Optimizer) and fo.state_dict()['state'] == {}
    for a, b in zip(pf, pt):                       # re-homed into the flat buffers, values unchanged
        assert torch.equal(a.detach(), b.detach())
    return pf, red, fo


def _step_lr_edits_lr(fo, lr):
    sched = torch.optim.lr_scheduler.StepLR(fo, step_size=1, gamma=0.1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')            # "lr_scheduler.step() before optimizer.step()"
        sched.step()
    assert abs(fo.lr - lr * 0.1) < 1e-12 and fo.param_groups[0]['lr'] == fo.lr


def test_flat_sgd_speaks_the_torch_sgd_schema_on_load_and_save():
    pt, opt = _torch_run(torch.optim.SGD, lr=2e-3, momentum=0.8, weight_decay=0.03)
    sd = opt.state_dict()
    pf, red, fo = _flat(parallel.FlatSGD, pt, lr=1.0)
    assert fo.momentum == 0.9                      # the reference's value is the default
    assert set(fo.param_groups[0]) == set(opt.param_groups[0])
    fo.load_state_dict(sd)
    assert fo.lr == 2e-3 and fo.momentum == 0.8 and fo.weight_decay == 0.03
    out = fo.state_dict()
    assert sorted(out['state']) == sorted(sd['state']) == [0, 1, 3]
    for i in out['state']:
        assert set(out['state'][i]) == {'momentum_buffer'}          # torch SGD keeps no 'step'
        assert torch.equal(out['state'][i]['momentum_buffer'], sd['state'][i]['momentum_buffer'])
        assert out['state'][i]['momentum_buffer'].shape == pt[i].shape
    assert out['param_groups'][0]['params'] == [0, 1, 2, 3]
    fresh = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in pt], lr=1.0)
    fresh.load_state_dict(out)                     # torch accepts what FlatSGD writes
    assert fresh.param_groups[0]['lr'] == 2e-3 and fresh.param_groups[0]['momentum'] == 0.8
    assert torch.equal(fresh.state_dict()['state'][3]['momentum_buffer'], sd['state'][3]['momentum_buffer'])
    _step_lr_edits_lr(fo, 2e-3)
    # malformed or unsupported files are refused
    bad = copy.deepcopy(opt.state_dict())   # (state_dict() hands out the optimizer's own per-parameter dicts)
    bad['param_groups'][0]['params'] = [0, 1, 2]
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    bad = copy.deepcopy(opt.state_dict())
    bad['state'][3]['momentum_buffer'] = torch.zeros(3)
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    bad = copy.deepcopy(opt.state_dict())
    bad['state'][DEAD] = {'momentum_buffer': torch.zeros(SHAPES[DEAD])}      # state for a parameter without a bucket
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    none = copy.deepcopy(opt.state_dict())   # torch SGD's entry before a first update (and at momentum 0): passed over, buffer zero
    none['state'][1] = {'momentum_buffer': None}
    fo.load_state_dict(none)
    assert bool((fo._views(pf[1])[0] == 0).all()) and torch.equal(fo._views(pf[3])[0], sd['state'][3]['momentum_buffer'])
    fo.load_state_dict(sd)
    for key, val in (('nesterov', True), ('dampening', 0.1), ('maximize', True)):
        bad = copy.deepcopy(opt.state_dict())
        bad['param_groups'][0][key] = val
        with pytest.raises(ValueError):
            fo.load_state_dict(bad)
    bad = copy.deepcopy(opt.state_dict())                         # two groups that differ
    g0 = bad['param_groups'][0]
    bad['param_groups'] = [dict(g0, params=[0, 1]), dict(g0, params=[2, 3], momentum=0.5)]
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    same = copy.deepcopy(opt.state_dict())                        # two groups that agree are one group
    same['param_groups'] = [dict(g0, params=[0, 1]), dict(g0, params=[2, 3])]
    fo.load_state_dict(same)
    assert torch.equal(fo.state_dict()['state'][3]['momentum_buffer'], sd['state'][3]['momentum_buffer'])
    red.remove()
    # without params= the positions of a torch checkpoint mean nothing
    pf2 = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    red2 = parallel.BucketedGradAllReduce(pf2, bucket_bytes=64, skip=[pf2[DEAD]])
    with pytest.raises(ValueError):
        parallel.FlatSGD(red2, lr=1.0).load_state_dict(sd)
    red2.remove()


def test_flat_adam_speaks_the_torch_adam_schema_on_load_and_save():
    pt, opt = _torch_run(torch.optim.Adam, lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.03)
    sd = opt.state_dict()
    pf, red, fo = _flat(parallel.FlatAdam, pt, lr=1.0)
    assert set(fo.param_groups[0]) == set(opt.param_groups[0])
    assert fo.weight_decay == 0.0                  # torch Adam's default, not AdamW's
    fo.load_state_dict(sd)
    assert fo.t == 3 and fo.lr == 2e-3 and fo.betas == (0.8, 0.95) and fo.eps == 1e-7 and fo.weight_decay == 0.03
    out = fo.state_dict()
    assert sorted(out['state']) == sorted(sd['state']) == [0, 1, 3]
    for i in out['state']:
        assert set(out['state'][i]) == {'step', 'exp_avg', 'exp_avg_sq'}
        assert float(out['state'][i]['step']) == float(sd['state'][i]['step']) == 3.0
        assert torch.equal(out['state'][i]['exp_avg'], sd['state'][i]['exp_avg'])
        assert torch.equal(out['state'][i]['exp_avg_sq'], sd['state'][i]['exp_avg_sq'])
        assert out['state'][i]['exp_avg'].shape == pt[i].shape
    assert out['param_groups'][0]['params'] == [0, 1, 2, 3]
    fresh = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in pt], lr=1.0)
    fresh.load_state_dict(out)                     # torch accepts what FlatAdam writes
    assert fresh.param_groups[0]['lr'] == 2e-3 and fresh.param_groups[0]['betas'] == (0.8, 0.95)
    _step_lr_edits_lr(fo, 2e-3)
    bad = copy.deepcopy(opt.state_dict())
    bad['param_groups'][0]['params'] = [0, 1, 2]
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    bad = copy.deepcopy(opt.state_dict())
    bad['state'][3]['exp_avg_sq'] = torch.zeros(3)
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    for key in ('exp_avg', 'exp_avg_sq', 'step'):  # an entry that lacks a key is malformed, not "no state yet"
        bad = copy.deepcopy(opt.state_dict())
        del bad['state'][1][key]
        with pytest.raises(ValueError, match=key):
            fo.load_state_dict(bad)
    bad = copy.deepcopy(opt.state_dict())
    bad['state'][1]['exp_avg'] = None
    with pytest.raises(ValueError, match='exp_avg'):
        fo.load_state_dict(bad)
    bad = copy.deepcopy(opt.state_dict())
    bad['state'][0]['step'] = torch.tensor(2.0)    # one step count for all
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    for key in ('amsgrad', 'maximize', 'decoupled_weight_decay'):
        bad = copy.deepcopy(opt.state_dict())
        bad['param_groups'][0][key] = True
        with pytest.raises(ValueError):
            fo.load_state_dict(bad)
    bad = copy.deepcopy(opt.state_dict())
    g0 = bad['param_groups'][0]
    bad['param_groups'] = [dict(g0, params=[0, 1]), dict(g0, params=[2, 3], lr=1e-5)]
    with pytest.raises(ValueError):
        fo.load_state_dict(bad)
    red.remove()
    pf2 = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    red2 = parallel.BucketedGradAllReduce(pf2, bucket_bytes=64, skip=[pf2[DEAD]])
    with pytest.raises(ValueError):
        parallel.FlatAdam(red2, lr=1.0).load_state_dict(sd)
    red2.remove()


def test_flat_adamw_keeps_its_surface_beside_the_new_classes():
    """FlatAdam reuses FlatAdamW's flat layout; FlatAdamW's own attributes and round-1 flat state format stay what they were."""
    pf = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    red = parallel.BucketedGradAllReduce(pf, bucket_bytes=64)
    fo = parallel.FlatAdamW(red, lr=1e-3)
    assert set(fo.flat[0]) == {'p', 'm', 'v'} and fo.t == 0 and fo.betas == (0.9, 0.999) and fo.weight_decay == 1e-2
    assert 'decoupled_weight_decay' not in fo.param_groups[0]
    fo.load_state_dict({'t': 5, 'lr': 3e-4, 'm': [torch.ones_like(st['m']) for st in fo.flat], 'v': [torch.ones_like(st['v']) for st in fo.flat]})
    assert fo.t == 5 and fo.lr == 3e-4 and all(bool((st['m'] == 1).all()) for st in fo.flat)
    red.remove()
    # a torch-schema entry without its moments is refused (it raised before the shared base class, too), not dropped
    pt, opt = _torch_run(torch.optim.AdamW, lr=2e-3)
    pw, redw, fw = _flat(parallel.FlatAdamW, pt, lr=1.0)
    bad = copy.deepcopy(opt.state_dict())
    del bad['state'][1]['exp_avg']
    with pytest.raises(ValueError, match='exp_avg'):
        fw.load_state_dict(bad)
    fw.load_state_dict(opt.state_dict())
    assert fw.t == 3 and torch.equal(fw._views(pw[1])[0], opt.state_dict()['state'][1]['exp_avg'])
    redw.remove()
    sg = parallel.FlatSGD(parallel.BucketedGradAllReduce(pf, bucket_bytes=64), lr=1e-3)
    assert set(sg.flat[0]) == {'p', 'buf'}
    sg.reducer.remove()


def test_build_optimizer_dispatches_like_the_reference():
    """train.py:94-99: sgd -> SGD(lr, momentum=0.9, weight_decay=wd), adam -> Adam(lr, weight_decay=wd), adamw -> AdamW(likewise)."""
    for name, cls in (('sgd', parallel.FlatSGD), ('adam', parallel.FlatAdam), ('adamw', parallel.FlatAdamW)):
        ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
        red = parallel.BucketedGradAllReduce(ps, bucket_bytes=64)
        opt = parallel.build_optimizer(argparse.Namespace(optimizer=name, lr=3e-4, wd=2e-4), red, ps)
        assert type(opt) is cls
        g = opt.param_groups[0]
        assert g['lr'] == 3e-4 and g['weight_decay'] == 2e-4 and g['params'] == ps
        if name == 'sgd':
            assert g['momentum'] == 0.9 and g['dampening'] == 0 and g['nesterov'] is False
        else:
            assert g['betas'] == (0.9, 0.999) and g['eps'] == 1e-8 and g['amsgrad'] is False
        red.remove()
    ps = [torch.nn.Parameter(torch.randn(3))]
    red = parallel.BucketedGradAllReduce(ps)
    with pytest.raises(ValueError, match='sgd.*adam.*adamw'):
        parallel.build_optimizer(argparse.Namespace(optimizer='rmsprop', lr=1e-3, wd=0.0), red, ps)
    red.remove()


def test_build_optimizer_takes_the_project_option_surface():
    from svol_amd import configs
    a = configs.parse_args(['--optimizer', 'sgd', '--lr', '0.01', '--wd', '0.001'])
    ps = [torch.nn.Parameter(torch.randn(5))]
    red = parallel.BucketedGradAllReduce(ps)
    opt = parallel.build_optimizer(a, red, ps)
    assert type(opt) is parallel.FlatSGD and opt.lr == 0.01 and opt.weight_decay == 0.001
    red.remove()
