"""CPU half of global gradient-norm clipping inside the flat optimizers' step (torch.nn.utils.clip_grad_norm_ where a DETR-style
loop calls it, the place of train.py:231-234): the C-ABI surface and its argument validation, the --clip_max_norm option, and how
parallel.build_optimizer hands it on.  The kernels themselves are GPU-only: tests/test_gpu_grad_clip.py."""
import argparse
import os
import re

import pytest
import torch

from svol_amd import configs, parallel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['svol_grad_sqnorm_ws_bytes', 'svol_grad_sqnorm', 'svol_grad_clip_state']
SHAPES = [(6, 5), (5,), (3,), (4, 4)]
DEAD = 2


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
    assert 'train.py:231-234' in txt and 'clip_grad_norm_' in txt
    assert L.lib().svol_abi_version() == 7          # new symbols only


def test_argument_validation_without_gpu():
    """Every check sits in front of the launch, so these calls are safe without a device: each of them is refused.  The pointers
    are made-up addresses.  (No accepted call is made: even n == 0 launches the kernel that writes the zero.)"""
    L = _lib().lib()
    A, M = 0x10000, 0x10004                        # 16-byte aligned / misaligned
    f = L.svol_grad_sqnorm
    assert f(0, 8, A, A, 0) == f(A, 8, 0, A, 0) == f(A, 8, A, 0, 0) == -1
    assert f(A, -1, A, A, 0) == f(M, -1, A, A, 0) == -1
    assert f(M, 8, A, A, 0) == f(A, 8, M, A, 0) == f(M, 0, A, A, 0) == -2
    w = L.svol_grad_sqnorm_ws_bytes
    assert w(-1) == -1
    assert w(0) == w(1) == w(3 * 1024) == 16       # one float per workgroup of 256 threads x 4 floats, in 16-byte units
    assert w(4 * 256 * 4) == 32 and w(4 * 256 * 3 + 1) == 16
    assert w(2048 * 1024) == w(1 << 40) == 2048 * 4   # the grid is capped at 2048 workgroups
    c = L.svol_grad_clip_state
    ok = dict(sq=A, nb=2, gmul=1.0, max_norm=1.0, loss_scale=1.0, steps=0, scaler=0, out=A)
    call = lambda **kw: c(*[dict(ok, **kw)[k] for k in ('sq', 'nb', 'gmul', 'max_norm', 'loss_scale', 'steps', 'scaler', 'out')], 0)
    assert call(sq=0) == call(out=0) == call(nb=0) == call(nb=-3) == call(steps=-1) == -1
    assert call(max_norm=0.0) == call(max_norm=-1.0) == call(max_norm=float('nan')) == -1
    assert call(loss_scale=0.0) == call(loss_scale=float('nan')) == -1     # no scaler state: the static scale divides the norm


def test_clip_max_norm_is_an_additive_option():
    assert configs.parse_args([]).clip_max_norm == 0.0
    assert configs.parse_args(['--clip_max_norm', '0.1']).clip_max_norm == 0.1
    assert 'clip_max_norm' not in configs.reference_defaults()


def _reducer():
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    red = parallel.BucketedGradAllReduce(ps, bucket_bytes=64, skip=[ps[DEAD]])
    assert len(red.buckets) > 1
    return ps, red


@pytest.mark.parametrize('name,cls', [('sgd', parallel.FlatSGD), ('adam', parallel.FlatAdam), ('adamw', parallel.FlatAdamW)])
def test_build_optimizer_hands_clip_max_norm_on(name, cls):
    ns = lambda **kw: argparse.Namespace(optimizer=name, lr=3e-4, wd=2e-4, **kw)
    keys = {}
    for what, args, kw, want in (('no option', ns(), {}, None), ('off', ns(clip_max_norm=0.0), {}, None),
                                 ('on', ns(clip_max_norm=0.1), {}, 0.1), ('keyword wins', ns(clip_max_norm=0.1), dict(max_grad_norm=2.0), 2.0),
                                 ('keyword turns it off', ns(clip_max_norm=0.1), dict(max_grad_norm=None), None),
                                 ('keyword alone', ns(), dict(max_grad_norm=float('inf')), float('inf'))):
        ps, red = _reducer()
        opt = parallel.build_optimizer(args, red, ps, **kw)
        assert type(opt) is cls and opt.max_grad_norm == want, what
        assert (opt.grad_norm is None) == (want is None), what
        if want is not None:
            assert opt.grad_norm.shape == () and opt.grad_norm.dtype == torch.float32 and float(opt.grad_norm) == 0.0
        sd = opt.state_dict()
        keys[what] = set(sd['param_groups'][0].keys())
        assert 'max_grad_norm' not in opt.param_groups[0] and 'max_grad_norm' not in sd and sd['state'] == {}
        red.remove()
    assert all(k == keys['no option'] for k in keys.values()), keys     # a setting of the loop: torch-schema interop stays as it is
    a = configs.parse_args(['--optimizer', name, '--clip_max_norm', '0.25'])
    ps, red = _reducer()
    assert parallel.build_optimizer(a, red, ps).max_grad_norm == 0.25
    red.remove()


def test_max_grad_norm_is_a_property_that_may_be_set_between_steps():
    ps, red = _reducer()
    opt = parallel.FlatAdamW(red, lr=1e-3, params=ps)
    assert opt.max_grad_norm is None and opt.grad_norm is None
    opt.max_grad_norm = 5
    assert opt.max_grad_norm == 5.0 and isinstance(opt.max_grad_norm, float) and opt.grad_norm is not None
    view = opt.grad_norm
    for off in (0, 0.0, None):
        opt.max_grad_norm = 1.0
        assert opt.grad_norm.data_ptr() == view.data_ptr()      # the same state vector every time
        opt.max_grad_norm = off
        assert opt.max_grad_norm is None and opt.grad_norm is None
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError):
            opt.max_grad_norm = bad
    with pytest.raises(ValueError):
        parallel.FlatSGD(red, lr=1e-3, params=ps, max_grad_norm=-0.5)
    red.remove()
