"""CPU half of the flat optimizers' weight average (ema_decay=...): the C entry svol_ema_flat and every refusal of its table, the
--model_ema_decay option, and the parts of the optimizers' surface that are plain torch (views, state dicts, the exchange of
averaged_weights, the checkpoint entries).  The kernel itself is GPU-only: tests/test_gpu_flat_ema.py."""
import argparse
import os
import re

import pytest
import torch

from svol_amd import configs, parallel
from svol_amd.utils import checkpoint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [('sgd', parallel.FlatSGD), ('adam', parallel.FlatAdam), ('adamw', parallel.FlatAdamW)]


def _lib():
    from svol_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_entry_is_declared_exported_and_bound():
    L = _lib()
    txt = open(os.path.join(REPO, 'include', 'svol_hip.h')).read()
    decl = set(re.findall(r'\b(svol_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', txt, flags=re.S)))
    assert 'svol_ema_flat' in decl and 'svol_ema_flat' in L.SIGNATURES and hasattr(L.lib(), 'svol_ema_flat')
    assert len(L.SIGNATURES['svol_ema_flat']) == 9
    assert 'fmaf(1 - d, p[i] - ema[i], ema[i])' in txt and '(1 + t) / (10 + t)' in txt
    assert L.lib().svol_abi_version() == 7          # a new symbol only


def test_every_refusal_sits_in_front_of_the_launch():
    """No device is touched: each call is refused, or has nothing to do.  The pointers are made-up addresses."""
    f = _lib().lib().svol_ema_flat
    A, B, M, S = 0x10000, 0x20000, 0x10004, 0x30000         # 16-byte aligned (two ranges) / misaligned / a state vector
    ok = dict(ema=A, p=B, n=8, decay=0.9, warmup=1, step=1, state=0, count=0)
    call = lambda **kw: f(*[dict(ok, **kw)[k] for k in ('ema', 'p', 'n', 'decay', 'warmup', 'step', 'state', 'count')], 0)
    INVALID, UNSUPPORTED = -1, -2
    assert call(ema=0) == call(p=0) == call(ema=0, p=0) == INVALID
    assert call(n=-1) == call(n=-4) == INVALID
    for d in (-0.01, 1.01, float('nan'), float('inf'), -float('inf')):
        assert call(decay=d) == INVALID, d
    # the host-count path (neither state nor step_count) counts from 1, warm-up or not
    assert call(step=0) == call(step=-3) == call(step=0, warmup=0) == INVALID
    for n in (1, 2, 3, 7, 1027):
        assert call(n=n) == UNSUPPORTED, n
    assert call(ema=M) == call(p=M) == call(ema=M, p=M + 16) == UNSUPPORTED
    assert call(n=4 * 256 * (1 << 31)) == UNSUPPORTED         # 2^31 workgroups: the grid does not fit
    # an invalid argument is reported before an unsupported one
    assert call(n=3, decay=2.0) == call(ema=M, step=0) == call(ema=M, n=-1) == INVALID
    # nothing to do: SVOL_OK and no launch, on each of the three count paths, at both ends of the decay's range
    assert call(n=0) == call(n=0, decay=0.0) == call(n=0, decay=1.0) == 0
    assert call(n=0, step=0, state=S) == call(n=0, step=0, count=S) == call(n=0, step=0, state=S, count=S + 12) == 0
    # with a device count the host's step is not looked at
    assert call(n=3, step=0, state=S) == call(n=3, step=0, count=S) == UNSUPPORTED


def test_model_ema_decay_is_an_additive_option():
    assert configs.parse_args([]).model_ema_decay is None
    assert configs.parse_args(['--model_ema_decay', '0.999']).model_ema_decay == 0.999
    assert 'model_ema_decay' not in configs.reference_defaults()


SHAPES = [(6, 5), (5,), (3,), (4, 4)]
DEAD = 2


def _reducer(seed=0):
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    red = parallel.BucketedGradAllReduce(ps, bucket_bytes=64, skip=[ps[DEAD]])
    assert len(red.buckets) > 1
    return ps, red


@pytest.mark.parametrize('name,cls', CLASSES)
def test_build_optimizer_hands_model_ema_decay_on(name, cls):
    ns = lambda **kw: argparse.Namespace(optimizer=name, lr=3e-4, wd=2e-4, **kw)
    sds = {}
    for what, args, kw, want in (('no option', ns(), {}, None), ('off', ns(model_ema_decay=None), {}, None),
                                 ('on', ns(model_ema_decay=0.99), {}, 0.99), ('zero is a decay', ns(model_ema_decay=0.0), {}, 0.0),
                                 ('keyword wins', ns(model_ema_decay=0.99), dict(ema_decay=0.5), 0.5),
                                 ('keyword turns it off', ns(model_ema_decay=0.99), dict(ema_decay=None), None),
                                 ('keyword alone', ns(), dict(ema_decay=0.9, ema_warmup=False), 0.9)):
        ps, red = _reducer()
        opt = parallel.build_optimizer(args, red, ps, **kw)
        assert type(opt) is cls and opt.ema_decay == want, what
        assert opt.ema_warmup is (what != 'keyword alone'), what
        assert all(('ema' in st) == (want is not None) for st in opt.flat), what
        if want is not None:
            assert all(torch.equal(st['ema'], st['p']) and st['ema'].data_ptr() != st['p'].data_ptr() for st in opt.flat)
        sds[what] = opt.state_dict()
        assert all('ema' not in k for k in opt.param_groups[0]) and set(sds[what]) == {'state', 'param_groups'}
        red.remove()
    assert all(sd == sds['no option'] for sd in sds.values())      # a setting of the object: torch's schema stays as it is
    a = configs.parse_args(['--optimizer', name, '--model_ema_decay', '0.25'])
    ps, red = _reducer()
    assert parallel.build_optimizer(a, red, ps).ema_decay == 0.25
    red.remove()
    for bad in (-0.1, 1.5, float('nan')):
        ps, red = _reducer()
        with pytest.raises(ValueError):
            cls(red, params=ps, ema_decay=bad)
        red.remove()


def test_an_optimizer_without_an_average_refuses_its_readers():
    ps, red = _reducer()
    opt = parallel.FlatAdamW(red, params=ps)
    for call in (lambda: opt.ema_views(ps[0]), lambda: opt.ema_extra_state(), lambda: opt.load_ema_extra_state(None),
                 lambda: opt.ema_state_dict(torch.nn.Linear(2, 2)), lambda: opt.averaged_weights().__enter__()):
        with pytest.raises(RuntimeError):
            call()
    red.remove()


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.bn, self.b = torch.nn.Linear(8, 12), torch.nn.BatchNorm1d(12), torch.nn.Linear(12, 4)
        self.frozen = torch.nn.Linear(4, 4)
        for p in self.frozen.parameters():
            p.requires_grad_(False)


def _toy(seed, **kw):
    torch.manual_seed(seed)
    net = _Toy()
    skip = [net.b.bias]
    red = parallel.BucketedGradAllReduce([p for p in net.parameters() if p.requires_grad], bucket_bytes=256, skip=skip)
    assert len(red.buckets) > 1
    opt = parallel.FlatAdamW(red, params=[p for p in net.parameters() if p.requires_grad], **kw)
    return net, red, opt


def _drift(opt, seed=9):
    """make the averages differ from the weights without a kernel: write them"""
    g = torch.Generator().manual_seed(seed)
    for st in opt.flat:
        st['ema'].copy_(torch.randn(st['ema'].shape, generator=g))


def test_views_state_dicts_and_the_exchange_on_the_host():
    net, red, opt = _toy(1, ema_decay=0.9)
    _drift(opt)
    owned = {id(p) for b in red.buckets for p in b['params']}
    for p in net.parameters():
        if id(p) in owned:
            v = opt.ema_views(p)
            bi, off, n = opt._slot[id(p)]
            assert v.shape == p.shape and v.data_ptr() == opt.flat[bi]['ema'].data_ptr() + 4 * off       # a view, no copy
    live = {k: v.clone() for k, v in net.state_dict().items()}
    sd = opt.ema_state_dict(net)
    assert list(sd) == list(live)
    names = {id(p): n for n, p in net.named_parameters()}
    for k, v in sd.items():
        p = dict(net.named_parameters()).get(k)
        if p is not None and id(p) in owned:
            assert torch.equal(v, opt.ema_views(p)) and not torch.equal(v, live[k]), k
            assert v.data_ptr() != opt.ema_views(p).data_ptr()                  # a clone
        else:
            assert torch.equal(v, live[k]), k                                   # buffers, the skipped bias, the frozen layer
    assert {'bn.running_mean', 'b.bias', 'frozen.weight'} <= {k for k in sd if k not in
                                                                {names[i] for i in owned}}
    ex = opt.ema_extra_state()
    assert set(ex) == {'decay', 'warmup', 'step', 'params'} and ex['decay'] == 0.9 and ex['warmup'] is True and ex['step'] == 0
    plist = [p for g in opt.param_groups for p in g['params']]
    assert sorted(ex['params']) == [i for i, p in enumerate(plist) if id(p) in owned]
    assert all(torch.equal(ex['params'][i], opt.ema_views(plist[i])) for i in ex['params'])

    before_p = [st['p'].clone() for st in opt.flat]
    before_e = [st['ema'].clone() for st in opt.flat]
    versions = [p._version for p in plist if id(p) in owned]
    with opt.averaged_weights() as same:
        assert same is opt
        for p in plist:
            if id(p) in owned:
                assert torch.equal(p.detach(), sd[names[id(p)]])                # the model IS the averaged model
        assert all(torch.equal(st['ema'], b) for st, b in zip(opt.flat, before_p))
        assert all(p._version > v for p, v in zip([p for p in plist if id(p) in owned], versions))
        inside = opt.ema_state_dict(net)
        assert all(torch.equal(inside[k], sd[k]) for k in sd)                   # the same answer from inside
        with pytest.raises(RuntimeError):
            with opt.averaged_weights():
                pass
        with pytest.raises(RuntimeError):
            opt.step()
        with pytest.raises(RuntimeError):
            opt.load_ema_extra_state(None)
    assert all(torch.equal(st['p'], b) for st, b in zip(opt.flat, before_p))
    assert all(torch.equal(st['ema'], b) for st, b in zip(opt.flat, before_e))
    with pytest.raises(KeyError):                                               # an exception inside still exchanges back
        with opt.averaged_weights():
            raise KeyError('x')
    assert all(torch.equal(st['p'], b) for st, b in zip(opt.flat, before_p)) and not opt._ema_swapped
    opt.load_ema_extra_state(None)
    assert all(torch.equal(st['ema'], st['p']) for st in opt.flat)
    opt.load_ema_extra_state(ex)
    assert all(torch.equal(st['ema'], b) for st, b in zip(opt.flat, before_e))
    short = dict(ex, params={k: v for k, v in ex['params'].items() if k != 0})
    with pytest.raises(ValueError):
        opt.load_ema_extra_state(short)
    red.remove()


PARENT_KEYS = ['model', 'optimizer', 'lr_scheduler', 'amp', 'iter', 'args']      # what the format held before the average


@pytest.mark.parametrize('prefix', [False, True])
def test_checkpoint_entries(tmp_path, prefix):
    args = argparse.Namespace(x=1)
    net, red, opt = _toy(2, ema_decay=0.9)
    _drift(opt)
    path = checkpoint.save_checkpoint(str(tmp_path / 'on.ckpt'), net, opt, None, 7, args, ddp_prefix=prefix)
    ck = torch.load(path, weights_only=False)
    assert sorted(ck) == sorted(PARENT_KEYS + ['model_ema', 'ema'])
    assert list(ck['model_ema']) == list(ck['model']) and all(k.startswith('module.') == prefix for k in ck['model_ema'])
    want = opt.ema_state_dict(net)
    assert all(torch.equal(v, want[k[7:] if prefix else k]) for k, v in ck['model_ema'].items())
    ema_before = [st['ema'].clone() for st in opt.flat]
    red.remove()

    net2, red2, opt2 = _toy(3, ema_decay=0.9)                     # constructed anew, other weights
    _, info = checkpoint.load_checkpoint(path, net2, opt2, resume_all=True)
    assert info['ema'] == 'restored' and info['start_iter'] == 8
    assert all(torch.equal(st['ema'], b) for st, b in zip(opt2.flat, ema_before))
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(net.parameters(), net2.parameters()))
    red2.remove()

    net3, red3, opt3 = _toy(2)                                    # no average: exactly the keys the format had
    path_off = checkpoint.save_checkpoint(str(tmp_path / 'off.ckpt'), net3, opt3, None, 7, args, ddp_prefix=prefix)
    assert sorted(torch.load(path_off, weights_only=False)) == sorted(PARENT_KEYS)
    _, info3 = checkpoint.load_checkpoint(path_off, net3, opt3, resume_all=True)
    assert 'ema' not in info3
    red3.remove()

    net4, red4, opt4 = _toy(4, ema_decay=0.9)                     # that file into an optimizer that keeps an average
    _drift(opt4)
    _, info4 = checkpoint.load_checkpoint(path_off, net4, opt4, resume_all=True)
    assert 'reseeded' in info4['ema']
    assert all(torch.equal(st['ema'], st['p']) for st in opt4.flat)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(net3.parameters(), net4.parameters()))
    red4.remove()
