"""``SketchViTClassifier(compute_dtype='fp16')`` on the device at the smallest configuration of tests/test_gpu_sketch_vit.py (d64_dh32,
n = 3, C = 19), against the same fp64 chain (tests/sketch_vit_ref.py) and at that file's bars:

  a. forward's before_norm / after_norm within 1e-2 of their scale; logits and loss of forward and of cls_logits (the [CLS]-only last
     block, svol_attn_cls_fwd_h16) within 3 x the bf16 emulation's figures (EMULATED there: fp16 is held to bf16's bars, which it should
     meet with room); loss() is F.cross_entropy of its own logits.
  b. gradients of loss() through cls_logits against fp64 autograd (3 layers, K = 1 and K = 2), the loss multiplied by
     gpu_checks.FP16_LOSS_SCALE = 4096 and the factor divided out exactly: every trainable parameter <= 3e-2 norm-wise, key biases
     <= 1e-3 of the largest parameter-gradient norm, frozen parameters without a gradient; the L2 error of the whole gradient is no
     larger than the bf16 classifier's on the same case.
  c. the four tensors extract_features saves are [n, d] fp32 and finite, the class tokens bit-equal to forward's.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import sketch_vit_ref as R
from tests.test_gpu_sketch_vit import EMULATED, FACTOR

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAME, N = 'd64_dh32', 3


def _model(cfg, sd, K=1, cd='fp16'):
    from svol_amd.modeling.sketch_vit import SketchViTClassifier
    m = SketchViTClassifier(cfg, R.NUM_LABELS, finetune_layers=K, compute_dtype=cd)
    m.load_state_dict(sd)
    return m.to(DEV)


def test_forward_cls_logits_and_features_against_fp64():
    cfg, sd, x, targets = R.setup(NAME, N)
    ref = R.reference(sd, cfg, x, targets)
    m = _model(cfg, sd).eval()
    assert m.vit.compute_dtype == 'fp16' and m.vit.dtype == torch.float16
    xs, ts = x.to(DEV), targets.to(DEV)
    with torch.no_grad():
        before, after, logits = m(xs)
    for tag, got in (('before_norm', before), ('after_norm', after)):
        e = float((got.cpu().double() - ref[tag]).abs().max() / ref[tag].abs().max())
        print(f'{NAME} n={N} {tag}: {e:.3e}')
        assert e < 1e-2, (tag, e)
    m.train()
    with torch.no_grad():
        logits_c = m.cls_logits(xs)
        loss_c, hits = m.loss(xs, ts)
    torch.cuda.synchronize()
    assert logits.shape == logits_c.shape == (N, R.NUM_LABELS) and logits.dtype == torch.float32
    e_logits, e_loss = EMULATED[(NAME, N)]
    for tag, lg in (('forward', logits), ('cls_logits', logits_c)):
        rows = F.cross_entropy(lg.cpu().double(), targets, reduction='none')
        f = R.figures(lg, rows, ref)
        print(f'{NAME} n={N} {tag}: logits {f.logits:.3e} (<= {FACTOR * e_logits:.3e})  loss {f.loss:.3e} (<= {FACTOR * e_loss:.3e})')
        assert f.logits <= FACTOR * e_logits and f.loss <= FACTOR * e_loss, (tag, f)
    own = F.cross_entropy(logits_c.cpu().double(), targets)
    assert abs(float(loss_c) - float(own)) <= 1e-5 * float(own)
    assert abs(float(loss_c) - float(ref['loss'])) <= FACTOR * e_loss * float(ref['loss'])
    assert int(hits) == int((logits_c.argmax(1).cpu() == targets).sum())
    feats = m.extract_features(xs)
    assert m.training and set(feats) == {'before_norm', 'after_norm'}
    for tag, t in (('before_norm', before), ('after_norm', after)):
        assert set(feats[tag]) == {'class_token', 'feature_avg'}
        for f_ in feats[tag].values():
            assert f_.shape == (N, cfg.hidden_size) and f_.dtype == torch.float32 and bool(torch.isfinite(f_).all())
        assert torch.equal(feats[tag]['class_token'], t[:, 0])


def _device_grads(m, x, targets, scale):
    m.train()
    for p in m.parameters():
        p.grad = None
    loss, _ = m.loss(x.to(DEV), targets.to(DEV))
    (loss * scale).backward()
    torch.cuda.synchronize()
    return {k: (p.grad.detach().cpu().double() / scale if p.grad is not None else None) for k, p in m.named_parameters()}


@pytest.mark.parametrize('K', [1, 2])
def test_gradients_of_the_loss_against_fp64_autograd_and_bf16(K):
    from oracle.vit_oracle import vit_forward
    from tests import gpu_checks as G
    cfg, sd, x, targets = R.setup(NAME, N, layers=3)
    sdr = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    vit, W, b = R.split(sdr)
    last, _ = vit_forward(vit, cfg, x.double())
    R.head(last, W, b, targets)[2].backward()
    trained = {k for k in sd if k.startswith(tuple(f'vit.layers.{i}.' for i in range(3 - K, 3)) + ('vit.layernorm.', 'classifier.'))}
    top = max(float(sdr[k].grad.norm()) for k in trained)
    kb = {k for k in trained if k.endswith('attention.k_proj.bias')}
    ref_norm = sum(float(sdr[k].grad.norm()) ** 2 for k in trained) ** 0.5
    whole = {}
    for cd, scale in (('bf16', 1.0), ('fp16', G.FP16_LOSS_SCALE)):
        grads = _device_grads(_model(cfg, sd, K, cd), x, targets, scale)
        assert {k for k, g in grads.items() if g is not None} == trained
        whole[cd] = sum(float((grads[k] - sdr[k].grad).norm()) ** 2 for k in trained) ** 0.5 / ref_norm
        if cd == 'fp16':
            res = {k: float(grads[k].norm()) / top for k in kb}
            errs = {k: float((grads[k] - sdr[k].grad).norm() / sdr[k].grad.norm()) for k in trained - kb}
    print(f'{NAME} K={K}: whole-gradient L2 error bf16 {whole["bf16"]:.3e} fp16 {whole["fp16"]:.3e}; fp16 worst parameter '
          f'{max(errs.values()):.3e} ({max(errs, key=errs.get)})')
    assert all(v <= 1e-3 for v in res.values()), res
    bad = {k: e for k, e in errs.items() if e > 3e-2}
    assert not bad, bad
    assert whole['fp16'] <= whole['bf16'], whole
