"""The bottleneck extractors (svol_amd/modeling/resnet.py, block='bottleneck': ResNet-50) against the fp64 restatement tests/resnet50_ref.py
(itself pinned to transformers.ResNetModel by tests/test_resnet50_ref.py).

Nets (synthetic weights, resnet50_ref.synth_state_dict):
    A      stem 16, planes (8, 16),   depths (1, 1), 3 images of 32 x 32   channels not a multiple of 32: the explicit im2col matrix
    B      stem 32, planes (32, 64),  depths (2, 1), 2 images of 64 x 64   the implicit-GEMM kernel, a block without downsample
    full   stem 64, planes (64 .. 512), depths (3, 4, 6, 3), 2 images of 64 x 64: 2048 channels on 8 rows at the end
           (last BatchNorm weight of every block 0.1 +- 10 %: torchvision's zero_init_residual is the limit of it; with 0.5 the
           train-mode network on 8 samples amplifies ANY rounding to tens of per cent, the fp64-accumulated emulation included)

Bars: the BasicBlock tests' (test_gpu_resnet.py / test_gpu_resnet_fp16.py), as they stand:
    frozen   max |err| / max |ref| and L2: fp32 1e-3 / 1e-4, bf16 3e-2 / 1e-2, fp16 min(3 x emulation, the bf16 bar)
    train    features L2 2.5e-2, running statistics 1e-2 max(1, |v|), gradients vs fp64 L2 0.6 per parameter, vs the network with the
             product's roundings 0.2 per parameter and 0.12 in the median
The rounding emulation (resnet50_ref.emulate_frozen / emulate_train: fp64 arithmetic, activations and weights rounded where the product
rounds, run on the CPU inside the test) enters fp16's frozen bar as it does in the BasicBlock fp16 test; everywhere else it is only
printed beside the device's figure: it says how close to its bar the deeper stack runs by the roundings alone (frozen full bf16 L2
7.8e-3 of 1e-2, train full bf16 2.45e-2 of 2.5e-2; profiles/resnet50.md).  No figure needed a wider bar.
"""
from __future__ import annotations

import functools

import pytest
import torch

from tests import resnet50_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
NETS = {'A': dict(depths=(1, 1), planes=(8, 16), stem=16, n=3, size=32, gamma3=0.5),
        'B': dict(depths=(2, 1), planes=(32, 64), stem=32, n=2, size=64, gamma3=0.5),
        'full': dict(depths=(3, 4, 6, 3), planes=(64, 128, 256, 512), stem=64, n=2, size=64, gamma3=0.1)}
FROZEN_BARS = {'fp32': (1e-3, 1e-4), 'bf16': (3e-2, 1e-2)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, fp64 net, state dict, pixels, eval-mode feature map) — computed once, never modified"""
    c = NETS[name]
    net = R.RefBottleneckNet(c['depths'], c['planes'], c['stem'])
    sd = R.synth_state_dict(net, seed=7)
    for k in sd:
        if '.bn3.weight' in k:
            sd[k] = sd[k] * (c['gamma3'] / 0.5)
    net.load_state_dict(sd)
    net.eval()
    x = R.synth_pixels(c['n'], c['size'], seed=8)
    with torch.no_grad():
        ref = net(x)
    return c, net, sd, x, ref


def figures(out, ref, scale):
    out, ref = out.double().cpu(), ref.double()
    if not bool(torch.isfinite(out).all()):
        return float('inf'), float('inf')
    return float((out - ref).abs().max()) / scale, float((out - ref).norm() / ref.norm())


@functools.lru_cache(maxsize=None)
def frozen_emulation(name, dtype):
    c, net, sd, x, ref = case(name)
    return R.emulate_frozen(sd, c['depths'], x, TORCH[dtype])


def frozen_bars(name, dtype, avg):
    """(max bar, L2 bar, emulation's figures or None)"""
    c, net, sd, x, ref = case(name)
    if dtype == 'fp32':
        return (*FROZEN_BARS['fp32'], None)
    emu = frozen_emulation(name, dtype)
    scale = float(ref.abs().max())
    ee, el2 = figures(emu.mean((2, 3)), ref.mean((2, 3)), scale) if avg else figures(emu, ref, scale)
    cap_e, cap_l2 = FROZEN_BARS['bf16']
    if dtype == 'fp16':   # test_frozen_extractor_fp16_golden's rule
        return min(3 * ee, cap_e), min(3 * el2, cap_l2), (ee, el2)
    return cap_e, cap_l2, (ee, el2)


def extractor(name, dtype, avg, trainable=False):
    from svol_amd.modeling.resnet import ResNetExtractor
    c, net, sd, x, ref = case(name)
    m = ResNetExtractor(c['depths'], c['planes'], c['stem'], avgpool=avg, compute_dtype=dtype, trainable=trainable, block='bottleneck')
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def check_frozen(name, dtype):
    c, net, sd, x, ref = case(name)
    scale = float(ref.abs().max())
    bad = []
    for avg in (False, True):
        m = extractor(name, dtype, avg).eval()
        out = m(x.to(DEV))
        want = ref.mean((2, 3)) if avg else R.tokens(ref)
        assert out.shape == want.shape and out.dtype == (torch.float32 if avg else TORCH[dtype])
        e, l2 = figures(out, want, scale)
        be, bl2, emu = frozen_bars(name, dtype, avg)
        print(f'frozen {name} {dtype} avgpool={avg}: device max {e:.3e} (<= {be:.3e}) L2 {l2:.3e} (<= {bl2:.3e})'
              + (f'; emulation max {emu[0]:.3e} L2 {emu[1]:.3e}' if emu else ''))
        if not (e <= be and l2 <= bl2):
            bad.append((avg, e, be, l2, bl2))
    assert not bad, bad


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_frozen_features_of_the_tiny_nets(name, dtype):
    check_frozen(name, dtype)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_frozen_features_of_the_full_network(dtype):
    """(3, 4, 6, 3) x 2048 on 2 images of 64 x 64: every unit shape class of ResNet-50, 53 folded convolutions in a row"""
    check_frozen('full', dtype)


def test_fp16_fold_range_check_names_a_bottleneck_unit():
    """refold() covers conv3: a channel with a tiny running variance scales its filter past 65504"""
    m = extractor('A', 'fp16', False)
    with torch.no_grad():
        getattr(m, '5')[0].bn3.running_var[3] = 1e-12
        getattr(m, '5')[0].conv3.weight[3] = 1e3   # x gamma / sqrt(var + eps) ~ 0.5 * 316
    with pytest.raises(ValueError, match=r'5\.0\.conv3'):
        m.refold()


@functools.lru_cache(maxsize=None)
def train_case(name, avg):
    """probe, the fp64 train-mode answers and the emulations' features / statistics for one net, shared by both statistics modes"""
    c, net, sd, x, ref = case(name)
    netp = R.RefBottleneckNet(c['depths'], c['planes'], c['stem'], avgpool=avg)
    netp.load_state_dict(sd)
    n, C, side = ref.shape[0], ref.shape[1], ref.shape[2]
    probe = torch.randn((n, C) if avg else (n, side * side, C), generator=torch.Generator().manual_seed(11))
    probe_fmap = probe.view(n, C, 1, 1) if avg else probe.transpose(1, 2).reshape(n, C, side, side)
    f, grads, stats = R.train_reference(netp, x, probe_fmap.view(n, C) if avg else probe_fmap)
    return probe, probe_fmap, (f if avg else R.tokens(f)), grads, stats


@functools.lru_cache(maxsize=None)
def train_emulation(name, dtype, avg):
    """(feature L2, worst running statistic) of the rounding emulation against fp64"""
    c, net, sd, x, ref = case(name)
    probe, probe_fmap, f, grads, stats = train_case(name, avg)
    fe, _, se = R.emulate_train(sd, c['depths'], x, TORCH[dtype], avg=avg)
    fe = fe.flatten(1) if avg else R.tokens(fe)
    l2 = float((fe - f).norm() / f.norm())
    worst = max(float((se[k] - stats[k]).abs().max()) / max(1.0, float(stats[k].abs().max())) for k in stats)
    return l2, worst


def check_train_forward(m, name, dtype, avg, out):
    """features and updated running statistics against fp64; -> list of failures"""
    probe, probe_fmap, f, grads, stats = train_case(name, avg)
    el2, estat = train_emulation(name, dtype, avg)
    bar_l2, bar_stat = 2.5e-2, 1e-2   # test_resnet_training_mode_gradients' bars; the emulation is printed, not used
    l2 = float((out.detach().double().cpu() - f).norm() / f.norm()) if bool(torch.isfinite(out).all()) else float('inf')
    bufs = dict(m.named_buffers())
    worst, worst_key = 0.0, ''
    for k, v in stats.items():
        e = float((bufs[k].double().cpu() - v).abs().max()) / max(1.0, float(v.abs().max()))
        if not e <= worst:
            worst, worst_key = e, k
    print(f'train {name} {dtype} avgpool={avg}: feature L2 {l2:.3e} (<= {bar_l2:.3e}; emulation {el2:.3e}); running statistics worst '
          f'{worst:.3e} [{worst_key}] (<= {bar_stat:.3e}; emulation {estat:.3e})')
    assert int(bufs['1.num_batches_tracked']) == 1 and int(bufs[f'{3 + len(NETS[name]["depths"])}.0.bn3.num_batches_tracked']) == 1
    bad = []
    if not l2 <= bar_l2:
        bad.append(f'features L2 {l2:.3e} > {bar_l2:.3e}')
    if not worst <= bar_stat:
        bad.append(f'{worst_key} {worst:.3e} > {bar_stat:.3e}')
    return bad


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_full_network_in_train_mode_features_and_running_statistics(dtype):
    """batch-statistics BatchNorm through all 53 units: svol_bn_colstats / _finalize / _apply at C = 2048 on 8 rows"""
    c, net, sd, x, ref = case('full')
    m = extractor('full', dtype, False, trainable=True).train()
    out = m(x.to(DEV))
    assert out.shape == (2, 4, 2048)
    bad = check_train_forward(m, 'full', dtype, False, out)
    assert not bad, bad


@pytest.mark.parametrize('two_pass', [True, False], ids=['two-pass-stats', 'one-pass-stats'])
@pytest.mark.parametrize('avg', [False, True], ids=['tokens', 'pooled'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_training_mode_gradients_of_the_tiny_nets(name, dtype, avg, two_pass, monkeypatch):
    """every parameter gradient, features and running statistics; the bars of test_resnet_training_mode_gradients.  fp16 runs under
    its fp16 twin's loss scale of 4096 on net A; net B takes 256 (both powers of two, taken out exactly): its probe is a SUM over 128
    token rows with N(0,1) weights, and through the residual adds of its three He-scaled blocks the backward signal grows towards the
    stem until the scaled dz passes 65504 — at 4096 the stem's weight gradient came out NaN (profiles/resnet50.md), which the dynamic
    scaler of a real run answers by halving the scale.  SVOL_BN_TWO_PASS is what ops.BN_STATS_TWO_PASS holds: set here for both modes,
    as that test does."""
    from svol_amd import ops
    S = 1.0 if dtype != 'fp16' else (4096.0 if name == 'A' else 256.0)
    monkeypatch.setattr(ops, 'BN_STATS_TWO_PASS', two_pass)
    c, net, sd, x, ref = case(name)
    probe, probe_fmap, f, grads, stats = train_case(name, avg)
    m = extractor(name, dtype, avg, trainable=True).train()
    out = m(x.to(DEV))
    assert out.shape == probe.shape and out.dtype == (torch.float32 if avg else TORCH[dtype])
    (out.float() * (probe.to(DEV) * S)).sum().backward()
    torch.cuda.synchronize()
    bad = check_train_forward(m, name, dtype, avg, out)
    _, ge, _ = R.emulate_train(sd, c['depths'], x, TORCH[dtype], probe_fmap, avg, device=DEV, ftype=torch.float32, loss_scale=S)
    e64, eem = {}, {}
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
        gk = p.grad.double().cpu() / S
        e64[k] = float((gk - grads[k]).norm() / max(float(grads[k].norm()), 1e-12))
        eem[k] = float((gk - ge[k].double().cpu()).norm() / max(float(ge[k].norm()), 1e-12))
    med64, med = sorted(e64.values())[len(e64) // 2], sorted(eem.values())[len(eem) // 2]
    k64, kem = max(e64, key=e64.get), max(eem, key=eem.get)
    print(f'train {name} {dtype} avgpool={avg} two_pass={two_pass}: gradient L2 vs fp64 max {e64[k64]:.2e} [{k64}] median {med64:.2e}; '
          f'vs the rounding reference max {eem[kem]:.2e} [{kem}] median {med:.2e}')
    if not max(e64.values()) <= 0.6:
        bad.append({k: round(v, 3) for k, v in e64.items() if not v <= 0.6})
    if not (max(eem.values()) <= 0.2 and med <= 0.12):
        bad.append(({k: round(v, 4) for k, v in eem.items() if not v <= 0.2}, med))
    assert not bad, bad
