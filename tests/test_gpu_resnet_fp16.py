"""The ResNet extractors on fp16 operands (compute_dtype='fp16'; the reference's apex-amp configuration), frozen and trained:

  1. svol_im2col / svol_maxpool_nhwc / svol_avgpool_nhwc with fp16 data, bit-exact against torch on the same fp16 values, every output
     carved out of a guard arena (tests/test_gpu_guards.py);
  2. svol_conv_nhwc in fp16 against fp64 conv2d and against the explicit im2col + GEMM path;
  3. the frozen extractor against the committed goldens, judged by a torch fp32 emulation with fp16 roundings at the product's
     rounding sites (3 x its error figures, never more than the bf16 test's bars);
  4. training mode (batch-statistics BatchNorm, every parameter gradient) under a loss scale of 4096 against the fp64 oracle and a
     torch fp32 network with fp16 roundings forward and backward;
  5. the fp16 instances of csrc/resnet_train.hip one by one against fp64;
  6. raw uint8 frames through the nhwc_f16 ingest route: the tokens of the float route, bit for bit;
  7. build_model(--backbone resnet --compute_dtype fp16): eval tokens, a clean FlatAdamW step under a DynamicLossScaler and an
     overflowed one that must change nothing but the scale.

Items 3 and 4 print their error figures, bf16 beside fp16 where it costs nothing (profiles/resnet_fp16.md quotes them)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from svol_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H16 = torch.float16
_TORCH = {'fp16': torch.float16, 'bf16': torch.bfloat16}


def _ulp16(v):
    """one fp16 unit in the last place at magnitude v (normal range)"""
    return 2.0 ** (math.floor(math.log2(v)) - 10)


def _pad32(k):
    return (k + 31) // 32 * 32


# ---- 1. data movement ------------------------------------------------------------------------------------------------------------
def _guarded(shape, dtype):
    from tests.test_gpu_guards import GuardArena
    ar = GuardArena(guard_bytes=1 << 14)
    ar.plan('out', shape, dtype)
    return ar, ar.build()['out']


def _unfold_ref(x_nchw, k, s, p):
    """[n, C, H, W] fp32 -> [n*Ho*Wo, k*k*C] in (ky, kx, c) order"""
    n, C = x_nchw.shape[:2]
    ref = F.unfold(x_nchw, k, padding=p, stride=s)
    return ref.view(n, C, k, k, -1).permute(0, 4, 2, 3, 1).reshape(-1, k * k * C)


def _im2col_abi(src, strides, src_dt, N, H, W, C, k, s, p, ld):
    from svol_amd import ops
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    ar, cols = _guarded((N * Ho * Wo, ld), H16)
    rc = ops._lib.lib().svol_im2col(ops._ptr(src), *strides, src_dt, ops._ptr(cols), ld, N, H, W, C, k, k, s, p, 2, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ar.check(f'svol_im2col C={C} k={k} s={s}')
    return cols.cpu()


IM2COL_CASES = [  # (C, k, s, p, source, the path it takes)
    (3, 7, 2, 3, 'nchw_f32', 'stem'), (3, 7, 2, 3, 'nhwc_f16', 'stem'),
    (8, 3, 2, 1, 'nhwc_f16', '16-byte'), (40, 3, 2, 1, 'nhwc_f16', '16-byte'), (8, 1, 2, 0, 'nhwc_f16', '16-byte'), (40, 1, 2, 0, 'nhwc_f16', '16-byte'),
    (5, 3, 1, 1, 'nhwc_f16', 'generic')]


@pytest.mark.parametrize('C,k,s,p,src,path', IM2COL_CASES, ids=[f'C{c[0]}-k{c[1]}s{c[2]}-{c[4]}' for c in IM2COL_CASES])
def test_im2col_fp16_is_bit_exact(C, k, s, p, src, path):
    N, H, W = 2, 13, 9
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C * 10 + k))
    K = k * k * C
    ld = 160 if C == 3 else _pad32(K)
    assert ld > K                                       # every case has a zero tail
    if src == 'nchw_f32':
        got = _im2col_abi(x.to(DEV), (C * H * W, W, 1, H * W), 0, N, H, W, C, k, s, p, ld)
        ref = _unfold_ref(x, k, s, p).to(H16)           # one rounding, fp32 -> fp16
    else:
        x16 = x.to(H16)
        got = _im2col_abi(x16.permute(0, 2, 3, 1).contiguous().to(DEV), (H * W * C, W * C, C, 1), 2, N, H, W, C, k, s, p, ld)
        ref = _unfold_ref(x16.float(), k, s, p).to(H16)   # a copy
    assert got.dtype == H16 and torch.equal(got[:, :K], ref), path
    assert torch.equal(got[:, K:].view(torch.int16), torch.zeros_like(got[:, K:]).view(torch.int16)), 'zero tail (+0.0 bits)'


@pytest.mark.parametrize('C', [8, 64])
def test_maxpool_fp16_is_bit_exact(C):
    from svol_amd import ops
    N, H, W = 2, 13, 9
    x16 = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C)).to(H16)
    nhwc = x16.permute(0, 2, 3, 1).contiguous().to(DEV)
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    ar, y = _guarded((N * Ho * Wo, C), H16)
    rc = ops._lib.lib().svol_maxpool_nhwc(ops._ptr(nhwc), ops._ptr(y), N, H, W, C, 3, 2, 1, 2, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ar.check(f'svol_maxpool_nhwc C={C}')
    ref = F.max_pool2d(x16.float(), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, C).to(H16)
    assert torch.equal(y.cpu(), ref)
    y2, ho, wo = ops.maxpool_nhwc(nhwc, N, H, W, C, 3, 2, 1)
    assert (ho, wo) == (Ho, Wo) and y2.dtype == H16 and torch.equal(y2.cpu(), ref)


@pytest.mark.parametrize('N,HW,C', [(2, 117, 64), (3, 49, 40)])
def test_avgpool_fp16_against_fp64(N, HW, C):
    """mean over the positions to 1e-6 of every mean: the inputs are post-ReLU activations (what the sketch branch pools), so no
    mean is a cancellation; fp16 values of this range are multiples of 2^-24 that an fp32 sum holds almost exactly, which leaves the
    division's rounding (6e-8) and a few last-bit partial sums."""
    from svol_amd import ops
    x16 = torch.relu(torch.randn(N, HW, C, generator=torch.Generator().manual_seed(HW))).to(H16)
    ar, y = _guarded((N, C), torch.float32)
    xd = x16.to(DEV)
    rc = ops._lib.lib().svol_avgpool_nhwc(ops._ptr(xd), ops._ptr(y), N, HW, C, 2, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ar.check(f'svol_avgpool_nhwc C={C}')
    ref = x16.double().mean(1)
    rel = float(((y.cpu().double() - ref).abs() / ref.abs()).max())
    print(f'avgpool fp16 N={N} HW={HW} C={C}: max relative error {rel:.2e}')
    assert rel <= 1e-6
    assert torch.equal(ops.avgpool_nhwc(xd.view(N * HW, C), N, HW, C), y)


# ---- 2. the implicit convolution -------------------------------------------------------------------------------------------------
CONV_CASES = [(2, 14, 14, 64, 64, 3, 1, 1, 'relu', False), (3, 13, 9, 64, 128, 3, 2, 1, 'relu', False), (2, 12, 12, 128, 256, 1, 2, 0, 'none', False),
              (2, 10, 10, 128, 128, 3, 1, 1, 'relu_res', True), (1, 7, 7, 256, 512, 3, 1, 1, 'relu_res', True), (5, 9, 11, 32, 36, 3, 1, 1, 'none', False)]


@pytest.mark.parametrize('case', CONV_CASES, ids=[f'{c[3]}to{c[4]}-k{c[5]}s{c[6]}-{c[8]}' for c in CONV_CASES])
def test_implicit_conv_fp16(case):
    """the geometries of test_implicit_conv_matches_im2col_path on fp16 operands.  Against fp64 conv2d on the same fp16 values:
    1.5e-3 of max|ref| (one output rounding to fp16, 4.9e-4, plus fp32 accumulation over K <= 2304; an eighth of the bf16 bar like
    gpu_checks.TOL).  Against ops.im2col + ops.gemm_nt, called directly: the same products in another order, 2 fp16 ulps of max|ref|."""
    from svol_amd import ops
    N, H, W, C, Cout, k, s, p, act, res = case
    g = torch.Generator().manual_seed(11 + C + Cout)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Cout, C, k, k, generator=g) / (C * k * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    xh, wh = x.to(H16), w.to(H16)
    ref = F.conv2d(xh.double(), wh.double(), b.double(), s, p)
    Ho, Wo = ref.shape[2], ref.shape[3]
    r = torch.randn(N, Cout, Ho, Wo, generator=g).to(H16) if res else None
    if res:
        ref = ref + r.double()
    if act != 'none':
        ref = torch.relu(ref)
    nhwc = xh.permute(0, 2, 3, 1).contiguous().view(-1, C).to(DEV)
    wf = wh.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV)
    rr = r.permute(0, 2, 3, 1).contiguous().view(-1, Cout).to(DEV) if res else None
    code = {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'relu_res': ops.ACT_RELU_RES}[act]
    assert ops._CONV_IMPLICIT
    bd = b.to(DEV)
    Mrows = N * Ho * Wo
    ar, y = _guarded((Mrows, Cout), H16)
    rc = ops._lib.lib().svol_conv_nhwc(ops._ptr(nhwc), ops._ptr(wf), wf.stride(0), ops._ptr(y), ops._ptr(bd), code, ops._ptr(rr), N, H, W, C,
                                       Cout, k, k, s, p, 2, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc                                   # the implicit kernel itself took the call
    ar.check(f'svol_conv_nhwc {case}')
    y2, ho, wo = ops.conv_nhwc(nhwc, wf, bd, code, N, H, W, C, k, k, s, p, residual=rr)
    assert (ho, wo) == (Ho, Wo) and y2.dtype == H16 and torch.equal(y2, y)
    top = float(ref.abs().max())
    got = y.float().cpu().view(N, Ho, Wo, Cout).permute(0, 3, 1, 2).double()
    err = float((got - ref).abs().max()) / top
    cols, _, _ = ops.im2col(nhwc, N, H, W, C, k, k, s, p, H16, ldcols=wf.shape[1])
    ye = ops.gemm_nt(cols, wf, bd, code, residual=rr)
    d = float((ye.float() - y.float()).abs().max())
    print(f'conv fp16 {case}: vs fp64 {err:.2e} of max|ref|; implicit vs explicit {d / _ulp16(top):.2f} ulp16(max|ref|)')
    assert err < 1.5e-3, (case, err)
    assert d <= 2 * _ulp16(top), (case, d, _ulp16(top))


# ---- 3. the frozen extractor against the goldens -----------------------------------------------------------------------------------
def _emulate_frozen(sd, depths, x, dt):
    """torch fp32 on the CPU with roundings to `dt` where the product rounds: the BatchNorm-folded weights (folded in fp32), the stem's
    im2col (= the pixels), every unit's output.  -> feature map [n, C, h, w] fp32."""
    r = lambda t: t.to(dt).float()

    def unit(h, conv, bn, stride, pad, idt=None, relu=True):
        scale = sd[bn + '.weight'].float() / torch.sqrt(sd[bn + '.running_var'].float() + 1e-5)
        shift = sd[bn + '.bias'].float() - sd[bn + '.running_mean'].float() * scale
        z = F.conv2d(h, r(sd[conv + '.weight'].float() * scale[:, None, None, None]), shift, stride, pad)
        if idt is not None:
            z = z + idt
        return r(torch.relu(z) if relu else z)
    h = unit(r(x.float()), '0', '1', 2, 3)
    h = F.max_pool2d(h, 3, 2, 1)
    for li, nb in enumerate(depths):
        for bi in range(nb):
            p, stride = f'{4 + li}.{bi}', (1 if li == 0 else 2) if bi == 0 else 1
            t = unit(h, p + '.conv1', p + '.bn1', stride, 1)
            idt = unit(h, p + '.downsample.0', p + '.downsample.1', stride, 0, relu=False) if (p + '.downsample.0.weight') in sd else h
            h = unit(t, p + '.conv2', p + '.bn2', 1, 1, idt=idt)
    return h


def _figures(out, ref, scale):
    out, ref = out.double(), ref.double()
    return float((out - ref).abs().max()) / scale, float((out - ref).norm() / ref.norm())


def _frozen_rule(dev_fig, emu_fig, what):
    """the device within 3 x the emulation's figures (accumulation order: the margin the ViT fp16 tests use), never above the bf16
    test's bars (test_resnet_extractor_golden: 3e-2 of the feature scale, 1e-2 L2)"""
    (e, l2), (ee, el2) = dev_fig, emu_fig
    assert e <= min(3 * ee, 3e-2) and l2 <= min(3 * el2, 1e-2), f'{what}: device max {e:.3e} L2 {l2:.3e}; emulation max {ee:.3e} L2 {el2:.3e}'


@functools.lru_cache(maxsize=None)
def _golden_case(name):
    from tests.test_oracle_resnet import resnet_case
    z, meta, sd, x = resnet_case(name)
    depths = tuple(meta['depths'])
    emu = {d: _emulate_frozen(sd, depths, x, _TORCH[d]) for d in ('fp16', 'bf16')}
    return z, meta, sd, x, emu


@pytest.mark.parametrize('name', ['resnet_tiny', 'resnet_tiny3', 'resnet18_1img', 'resnet34_1img'])
def test_frozen_extractor_fp16_golden(name):
    from svol_amd.modeling.resnet import ResNetExtractor
    z, meta, sd, x, emu = _golden_case(name)
    scale = float(np.abs(z['tokens']).max())
    for avg in (False, True):
        ref = torch.from_numpy(z['pooled'] if avg else z['tokens'])
        for d in ('fp16', 'bf16'):
            m = ResNetExtractor(tuple(meta['depths']), tuple(meta['widths']), meta['stem'], avgpool=avg, compute_dtype=d)
            m.load_state_dict(sd, strict=True)
            m.to(DEV).eval()
            out = m(x.to(DEV))
            assert out.dtype == (torch.float32 if avg else _TORCH[d]) and out.shape == ref.shape
            e = emu[d].mean((2, 3)) if avg else emu[d].flatten(2).transpose(1, 2)
            dev_fig, emu_fig = _figures(out.float().cpu(), ref, scale), _figures(e, ref, scale)
            print(f'{name} {d} avgpool={avg}: device max {dev_fig[0]:.3e} L2 {dev_fig[1]:.3e}; emulation max {emu_fig[0]:.3e} L2 {emu_fig[1]:.3e}')
            if d == 'fp16':   # (bf16: printed for the profile; its bars are test_resnet_extractor_golden's)
                _frozen_rule(dev_fig, emu_fig, f'{name} avgpool={avg}')


# ---- 4. training mode ------------------------------------------------------------------------------------------------------------
class _RoundF16(torch.autograd.Function):
    """x -> fp16(x) in the forward AND the backward: where the HIP path keeps an activation / its gradient in fp16"""

    @staticmethod
    def forward(ctx, x):
        return x.half().float()

    @staticmethod
    def backward(ctx, g):
        return g.half().float()


def _emulated_f16_reference(sd, depths, x, probe_fmap, avg, loss_scale):
    """the network in torch fp32 on the GPU with the HIP path's fp16 roundings (conv weights; conv output, unit output and the
    gradients of these two), the probe multiplied by the loss scale, the gradients divided by it: -> (features, {key: gradient})"""
    r = _RoundF16.apply
    P = {k: (v.detach().to(DEV).float().requires_grad_('running' not in k) if v.is_floating_point() else v) for k, v in sd.items()}
    # conv weights: rounded in the forward only — the product's weight gradients are fp32 GEMM outputs that never pass through fp16
    # (rounding the SCALED dW to half, as the bf16 twin harmlessly does with bfloat16, overflows 65504)
    w = lambda k: P[k] + (P[k].detach().half().float() - P[k].detach())

    def bn(z, p):
        return F.batch_norm(z, None, None, P[p + '.weight'], P[p + '.bias'], True, 0.1, 1e-5)
    h = r(F.relu(bn(r(F.conv2d(r(x.to(DEV).float()), w('0.weight'), None, 2, 3)), '1')))
    h = F.max_pool2d(h, 3, 2, 1)
    for li, nb in enumerate(depths):
        for bi in range(nb):
            p, stride = f'{4 + li}.{bi}', (1 if li == 0 else 2) if bi == 0 else 1
            t = r(F.relu(bn(r(F.conv2d(h, w(p + '.conv1.weight'), None, stride, 1)), p + '.bn1')))
            idt = h
            if (p + '.downsample.0.weight') in P:
                idt = r(bn(r(F.conv2d(h, w(p + '.downsample.0.weight'), None, stride, 0)), p + '.downsample.1'))
            h = r(F.relu(bn(r(F.conv2d(t, w(p + '.conv2.weight'), None, 1, 1)), p + '.bn2') + idt))
    f = F.adaptive_avg_pool2d(h, 1) if avg else h
    (f * (probe_fmap.to(DEV).float() * loss_scale)).sum().backward()
    return f.detach(), {k: v.grad / loss_scale for k, v in P.items() if torch.is_tensor(v) and v.requires_grad}


@functools.lru_cache(maxsize=None)
def _train_case(name, avg):
    """fixture, probe and the fp64 oracle's answers, computed once for both statistics modes"""
    from oracle import resnet_oracle as R
    from tests.test_oracle_resnet import resnet_case
    z, meta, sd, x = resnet_case(name)
    depths = tuple(meta['depths'])
    fm = R.resnet_features(sd, depths, x, avgpool=avg)
    n, C = fm.shape[:2]
    out_shape = (n, C) if avg else (n, fm.shape[2] * fm.shape[3], C)
    probe = torch.randn(out_shape, generator=torch.Generator().manual_seed(11))
    side = fm.shape[2]
    probe_fmap = probe.view(n, -1, 1, 1) if avg else probe.transpose(1, 2).reshape(n, -1, side, side)
    f, grads, stats = R.resnet_train_grads(sd, depths, x, probe_fmap, avgpool=avg)
    return meta, sd, x, depths, probe, probe_fmap, f, grads, stats


@pytest.mark.parametrize('name', ['resnet_tiny_train', 'resnet_tiny3_train'])
@pytest.mark.parametrize('avg', [False, True], ids=['tokens', 'pooled'])
@pytest.mark.parametrize('two_pass', [True, False], ids=['two-pass-stats', 'one-pass-stats'])
def test_training_mode_gradients_fp16(name, avg, two_pass, monkeypatch):
    """test_resnet_training_mode_gradients with half for bfloat16 and a loss scale of 4096 (a power of two: taken out exactly), its
    bars as caps.  fp16 flips fewer ReLU masks than bf16 (three more mantissa bits), so the figures printed here sit below bf16's."""
    from svol_amd import ops
    from svol_amd.modeling.resnet import ResNetExtractor
    S = 4096.0
    monkeypatch.setattr(ops, 'BN_STATS_TWO_PASS', two_pass)
    meta, sd, x, depths, probe, probe_fmap, f, grads, stats = _train_case(name, avg)
    m = ResNetExtractor(depths, tuple(meta['widths']), meta['stem'], avgpool=avg, compute_dtype='fp16', trainable=True)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    out = m(x.to(DEV))
    assert out.shape == probe.shape and out.dtype == (torch.float32 if avg else H16)
    (out.float() * (probe.to(DEV) * S)).sum().backward()
    torch.cuda.synchronize()
    ref_out = f.flatten(1) if avg else f.flatten(2).transpose(1, 2)
    l2 = float((out.detach().float().cpu().double() - ref_out).norm() / ref_out.norm())
    for k, v in stats.items():
        have = dict(m.named_buffers())[k].double().cpu()
        assert float((have - v.double()).abs().max()) <= 1e-2 * max(1.0, float(v.abs().max())), k
    assert int(dict(m.named_buffers())['1.num_batches_tracked']) == 1
    fe, ge = _emulated_f16_reference(sd, depths, x, probe_fmap, avg, S)
    e64, eem = {}, {}
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
        gk = p.grad.double().cpu() / S
        e64[k] = float((gk - grads[k]).norm() / max(float(grads[k].norm()), 1e-12))
        eem[k] = float((gk - ge[k].double().cpu()).norm() / max(float(ge[k].norm()), 1e-12))
    med64, med = sorted(e64.values())[len(e64) // 2], sorted(eem.values())[len(eem) // 2]
    print(f'{name} fp16 avg={avg} two_pass={two_pass}: feature L2 {l2:.2e}; gradient L2 vs fp64 max {max(e64.values()):.2e} median {med64:.2e}; '
          f'vs the fp16-rounding reference max {max(eem.values()):.2e} median {med:.2e}')
    assert l2 <= 2.5e-2, f'features vs fp64: L2 {l2:.3e}'
    assert max(e64.values()) <= 0.6, {k: round(v, 3) for k, v in e64.items() if v > 0.6}
    bad = {k: round(v, 4) for k, v in eem.items() if not v <= 0.2}
    assert not bad and med <= (0.03 if (name == 'resnet_tiny3_train' and two_pass) else 0.12), (bad, med)


# ---- 5. the training kernels' fp16 instances ---------------------------------------------------------------------------------------
def test_training_kernels_fp16():
    """test_resnet_training_kernels on fp16 values: batch statistics, BatchNorm apply and backward, the weight gradient (svol_gemm_tn on
    the im2col matrix and svol_conv_wgrad_nhwc), weight pack / flip / unpack, col2im, max pooling with index and its backward — the same
    shapes, torch fp64 on the same fp16 values, that test's bars as caps."""
    from svol_amd import ops
    from svol_amd.modeling.resnet import _w16

    def rel(a, b):
        a, b = a.double().cpu(), b.double().cpu()
        return float((a - b).norm() / max(float(b.norm()), 1e-30))
    g = torch.Generator().manual_seed(0)
    dt = H16
    res = {}
    for (n, H, W, C, Cout, k, s, p) in [(3, 8, 8, 16, 32, 3, 2, 1), (2, 16, 16, 32, 32, 3, 1, 1), (2, 8, 8, 64, 128, 1, 2, 0), (2, 14, 14, 64, 64, 3, 1, 1),
                                       (5, 28, 28, 128, 256, 3, 2, 1), (3, 7, 7, 512, 512, 3, 1, 1), (9, 56, 56, 64, 64, 3, 1, 1)]:
        tag = f'{n}x{H}x{W}x{C}->{Cout} k{k}s{s}'
        x = torch.randn(n, C, H, W, generator=g)
        w = torch.randn(Cout, C, k, k, generator=g) * 0.1
        x16 = x.permute(0, 2, 3, 1).reshape(n * H * W, C).to(dt).to(DEV).contiguous()
        xr = x16.double().cpu().view(n, H, W, C).permute(0, 3, 1, 2).requires_grad_(True)
        w16 = _w16(w.to(DEV), dt)
        assert w16.dtype == dt and torch.equal(w16[:, :k * k * C].cpu(), w.permute(0, 2, 3, 1).reshape(Cout, -1).to(dt)), tag + ' weight pack'
        assert float(w16[:, k * k * C:].float().abs().max()) == 0.0 if w16.shape[1] > k * k * C else True
        wr = w16[:, :k * k * C].double().cpu().view(Cout, k, k, C).permute(0, 3, 1, 2).requires_grad_(True)
        z, Ho, Wo = ops.conv_nhwc(x16, w16, None, ops.ACT_NONE, n, H, W, C, k, k, s, p)
        zr = F.conv2d(xr, wr, None, s, p)
        res[tag + ' conv'] = (rel(z, zr.detach().permute(0, 2, 3, 1).reshape(-1, Cout)), 4e-3)
        M = z.shape[0]
        gamma = (1 + 0.1 * torch.randn(Cout, generator=g)).to(DEV)
        beta = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
        rm, rv = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV)
        mean, rstd, scale, shift = ops.bn_train_stats(z, gamma, beta, rm, rv, 0.1, 1e-5)
        zd = z.double().cpu()
        var_ref = zd.var(0, unbiased=False)
        res[tag + ' mean'] = (float(((mean.double().cpu() - zd.mean(0)).abs() / zd.std(0)).max()), 1e-6)   # (in standard deviations)
        res[tag + ' rstd'] = (rel(rstd, 1.0 / torch.sqrt(var_ref + 1e-5)), 1e-5)
        res[tag + ' running_mean'] = (float(((rm.double().cpu() - 0.1 * zd.mean(0)).abs() / zd.std(0)).max()), 1e-6)
        res[tag + ' running_var'] = (rel(rv, 0.9 + 0.1 * zd.var(0, unbiased=True)), 1e-5)
        idt = torch.randn(M, Cout, generator=g).to(dt).to(DEV)
        y = ops.bn_apply(z, scale, shift, idt, True)
        zz, gr, br, rr = zd.clone().requires_grad_(True), gamma.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True), idt.double().cpu().requires_grad_(True)
        pre = F.batch_norm(zz, None, None, gr, br, True, 0.1, 1e-5) + rr
        res[tag + ' bn_apply'] = (rel(y, torch.relu(pre).detach()), 4e-3)
        dy = torch.randn(M, Cout, generator=g).to(dt).to(DEV)
        dz, dres, dgm, dbt = ops.bn_bwd(dy, y, z, mean, rstd, gamma, True)
        (pre * (dy.double().cpu() * (y.double().cpu() > 0).double())).sum().backward()
        res[tag + ' dz'] = (rel(dz, zz.grad), 4e-3)
        res[tag + ' didentity'] = (rel(dres, rr.grad), 1e-6)
        res[tag + ' dgamma'] = (rel(dgm, gr.grad), 1e-5)
        res[tag + ' dbeta'] = (rel(dbt, br.grad), 1e-5)
        zr.backward(dz.double().cpu().view(n, Ho, Wo, Cout).permute(0, 3, 1, 2))
        cols, _, _ = ops.im2col(x16, n, H, W, C, k, k, s, p, dt, ldcols=w16.shape[1])
        dW = ops.gemm_tn(dz, cols)[:, :k * k * C].reshape(Cout, k, k, C).permute(0, 3, 1, 2)
        res[tag + ' dW'] = (rel(dW, wr.grad), 1e-5)
        dwg = ops.conv_wgrad_nhwc(dz, x16, n, H, W, C, k, k, s, p, w16.shape[1])
        assert dwg is not None
        res[tag + ' dW (gathered in the GEMM)'] = (rel(dwg[:, :k * k * C].reshape(Cout, k, k, C).permute(0, 3, 1, 2), wr.grad), 1e-5)
        assert float(dwg[:, k * k * C:].abs().max()) == 0.0 if w16.shape[1] > k * k * C else True
        w32 = wr.detach().float().to(DEV).contiguous()
        res[tag + ' weight pack'] = (rel(ops.conv_weight_pack(w32, dt), w16), 0.0)
        wflip = ops.conv_weight_pack(w32, dt, flip=True)
        ref_flip = w32.flip(2, 3).permute(1, 2, 3, 0).reshape(C, k * k * Cout).to(dt)
        res[tag + ' weight flip'] = (rel(wflip[:, :k * k * Cout], ref_flip), 0.0)
        acc = torch.ones_like(w32)
        ops.conv_weight_unpack_add(ops.gemm_tn(dz, cols), acc)
        res[tag + ' weight unpack-add'] = (rel(acc - 1.0, wr.grad), 1e-5)
        dx = ops.col2im_nhwc(ops.gemm_nt(dz, w16.t().contiguous()), n, H, W, C, k, k, s, p)
        res[tag + ' dx'] = (rel(dx.view(n, H, W, C).permute(0, 3, 1, 2), xr.grad), 5e-3)
        if s == 1:
            dx2 = ops.conv_nhwc(dz, wflip, None, ops.ACT_NONE, n, Ho, Wo, Cout, k, k, 1, p)[0]
            res[tag + ' dx (as a convolution of dz)'] = (rel(dx2.view(n, H, W, C).permute(0, 3, 1, 2), xr.grad), 5e-3)
    n, H, W, C = 2, 9, 9, 16
    x16 = torch.relu(torch.randn(n, C, H, W, generator=g)).permute(0, 2, 3, 1).reshape(-1, C).to(dt).to(DEV).contiguous()
    xr = x16.double().cpu().view(n, H, W, C).permute(0, 3, 1, 2).requires_grad_(True)
    y, idx, Ho, Wo = ops.maxpool_idx_nhwc(x16, n, H, W, C, 3, 2, 1)
    yr = F.max_pool2d(xr, 3, 2, 1)
    dy = torch.randn(n * Ho * Wo, C, generator=g).to(dt).to(DEV)
    yr.backward(dy.double().cpu().view(n, Ho, Wo, C).permute(0, 3, 1, 2))
    res['maxpool fwd'] = (rel(y, yr.detach().permute(0, 2, 3, 1).reshape(-1, C)), 0.0)
    res['maxpool bwd (ties)'] = (rel(ops.maxpool_bwd_nhwc(dy, idx, n, H, W, C, 3, 2, 1).view(n, H, W, C).permute(0, 3, 1, 2), xr.grad), 3e-3)
    bad = {k_: v for k_, v in res.items() if not v[0] <= v[1]}
    assert not bad, bad


# ---- 6. raw frames ---------------------------------------------------------------------------------------------------------------
def _tiny_backbone(trainable=False):
    from svol_amd.modeling.resnet import ResNetBackbone, ResNetExtractor
    vb = ResNetExtractor((1, 1), (16, 32), 16, compute_dtype='fp16', trainable=trainable)
    sb = ResNetExtractor((1, 1), (16, 32), 16, avgpool=True, compute_dtype='fp16', trainable=trainable)
    vb.load_state_dict(syn.synth_resnet_state_dict(syn.resnet_param_shapes((1, 1), (16, 32), 16), seed=1))
    sb.load_state_dict(syn.synth_resnet_state_dict(syn.resnet_param_shapes((1, 1), (16, 32), 16), seed=2))
    return ResNetBackbone(vb, sb).to(DEV)


def test_raw_frames_take_the_nhwc_f16_route():
    """uint8 frames through the backbone's own ingest (resize -> fp16 NHWC -> the stem's im2col through strides) give the tokens of the
    float route (the same resize to fp32 NCHW pixels, passed as floats), bit for bit: one rounding to fp16 either way"""
    from svol_amd.ingest import FrameIngest
    bb = _tiny_backbone().eval()
    assert bb.nhwc and bb.ingest.out == 'nhwc_f16'
    r = np.random.default_rng(5)
    vid = torch.from_numpy(r.integers(0, 256, size=(1, 2, 37, 53, 3), dtype=np.uint8)).to(DEV)
    sk = torch.from_numpy(r.integers(0, 256, size=(1, 1, 41, 29, 3), dtype=np.uint8)).to(DEV)
    s_raw, v_raw = bb(sk, vid)
    to_float = FrameIngest((224, 224), 'totensor', out='nchw_f32')
    s_f, v_f = bb(to_float(sk), to_float(vid))
    assert v_raw.dtype == H16 and v_raw.shape == v_f.shape == (1, 2 * 28 * 28, 32) and s_raw.shape == s_f.shape == (1, 1, 32)
    assert torch.equal(v_raw, v_f) and torch.equal(s_raw, s_f)
    assert bool(torch.isfinite(v_raw.float()).all()) and float(v_raw.float().abs().max()) > 0


# ---- 7. through build_model ------------------------------------------------------------------------------------------------------
def test_build_model_fp16_resnet_eval_and_loss_scaled_steps():
    from oracle import resnet_oracle as R
    from svol_amd import parallel
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.model import build_model
    over = dict(hidden_dim=64, nheads=8, num_layers=1, num_queries=10, num_frames=2, backbone='resnet', compute_dtype='fp16', input_dropout=0.0)
    dv, ds = (3, 4, 6, 3), (2, 2, 2, 2)
    sdv = syn.synth_resnet_state_dict(syn.resnet_param_shapes(dv), seed=1)
    sds = syn.synth_resnet_state_dict(syn.resnet_param_shapes(ds), seed=2)
    vid = syn.synth_images(2, syn.vit_config(image_size=224), seed=4).view(1, 2, 3, 224, 224)
    sk = syn.synth_images(1, syn.vit_config(image_size=224), seed=5).view(1, 1, 3, 224, 224)
    ms, mv = torch.ones(1, 1, device=DEV), torch.ones(1, 2, device=DEV)

    def make(train):
        args = syn.head_args(**over)
        args.train_backbone = train
        torch.manual_seed(1)
        model = build_model(args)
        model.backbone.video_backbone.load_state_dict(sdv)
        model.backbone.sketch_backbone.load_state_dict(sds)
        return args, model.to(DEV)
    # eval: the frozen extractors' tokens under the rule of item 3, against the oracle
    args, model = make(False)
    model.eval()
    assert model.backbone.video_backbone.compute_dtype == H16 and model.backbone.sketch_backbone.compute_dtype == H16
    s, v = model.backbone(sk.to(DEV), vid.to(DEV))
    assert s.shape == (1, 1, 512) and v.shape == (1, 98, 512) and v.dtype == H16
    rs, rv = R.resnet_backbone_forward(sdv, dv, sds, ds, sk, vid)
    ev = _emulate_frozen(sdv, dv, vid[0], H16).flatten(2).transpose(1, 2).reshape(1, 98, 512)
    es = _emulate_frozen(sds, ds, sk[0], H16).mean((2, 3)).view(1, 1, 512)
    for what, got, emu, ref in (('frames', v, ev, rv), ('sketch', s, es, rs)):
        scale = float(ref.abs().max())
        dev_fig, emu_fig = _figures(got.float().cpu(), ref, scale), _figures(emu, ref, scale)
        print(f'build_model fp16 {what}: device max {dev_fig[0]:.3e} L2 {dev_fig[1]:.3e}; emulation max {emu_fig[0]:.3e} L2 {emu_fig[1]:.3e}')
        _frozen_rule(dev_fig, emu_fig, what)
    out = model(sk.to(DEV), vid.to(DEV), ms, mv)
    assert out['pred_boxes'].shape == (1, 10, 4) and bool(torch.isfinite(out['pred_logits'].float()).all())
    del model
    # training: the backbone's parameters sit in the gradient buckets like the head's, so the scaler covers them with nothing added
    args, model = make(True)
    model.train()
    crit = build_loss(args).to(DEV).train()
    params = [p for p in model.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
    opt = parallel.FlatAdamW(red, lr=1e-3, weight_decay=1e-4, params=params)
    sc = opt.scaler = parallel.DynamicLossScaler(torch.device(DEV), init_scale=2.0 ** 12)
    targets = syn.synth_targets(1, 2, seed=1)

    def step(extra):
        red.zero_grad()
        crit(model(sk.to(DEV), vid.to(DEV), ms, mv), targets)
        loss = crit.weighted_total()
        sc.scale(loss * extra if extra != 1.0 else loss).backward()
        red.finish()
        opt.step()
        torch.cuda.synchronize()
        return loss
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss = step(1.0)
    assert bool(torch.isfinite(loss))
    still = [k for k, p in model.backbone.named_parameters() if torch.equal(p.detach(), before['backbone.' + k])]
    assert not still, f'{len(still)} backbone parameters did not move: {still[:5]}'
    assert sc.state.tolist()[0] == 2.0 ** 12
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    step(2.0 ** 30)                                     # scaled gradients overflow fp16: the whole update is skipped
    changed = [k for k, p in model.named_parameters() if not torch.equal(p.detach(), before[k])]
    assert not changed, f'{len(changed)} parameters changed in an overflowed step: {changed[:5]}'
    assert sc.state.tolist()[0] == 2.0 ** 11
