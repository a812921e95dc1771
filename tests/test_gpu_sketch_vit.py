"""svol_amd.modeling.sketch_vit.SketchViTClassifier on the device against fp64 (tests/sketch_vit_ref.py: oracle.vit_oracle.vit_forward ->
F.linear -> F.cross_entropy, the chain of preprocess/sketch_vit_finetune.py:79-85,140-141).

  a. the model at d64_dh32 and d128_dh64, n = 3 and n = 1, C = 19: forward's before_norm / after_norm within 1e-2 of their scale (the bar
     of tests/test_gpu_vit.py); logits and loss of forward AND of cls_logits (the [CLS]-only last block) within 3 x the figures of the
     bf16 emulation (EMULATED; tests/test_sketch_vit_cases.py re-derives them; the factor is that of tests/test_gpu_attn_small.py);
     loss() is F.cross_entropy of its own logits and counts the top-1 hits; extract_features is the four reductions of forward's
     outputs (class tokens bit-equal, patch means within L 2^-24 mean |x| per channel).
  b. gradients of loss() through cls_logits against fp64 autograd, K = 1 and K = 2 on a 3-layer config, both head widths: every
     trainable parameter <= 3e-2 norm-wise (key biases: the rule of test_extractor_gradients_against_fp64_oracle — their exact gradient
     is zero, so <= 1e-3 of the largest parameter-gradient norm), frozen parameters have no gradient; under SVOL_DETERMINISTIC=1, in a
     fresh process, two runs are bit-identical.
  c. 20 FlatAdamW steps on 4 fixed images (lr 1e-3): the loss falls, only trainable parameters move, and the {'model', 'optimizer',
     'epoch'} checkpoint round-trips to bit-equal logits; the ViT-B widths once (2 layers, n = 2, forward and backward).

Emulation figures (logits: max |d| / max |ref|; loss: worst row's |d| / mean loss) and the device's, forward / cls_logits:

    config      n   emulation logits / loss    bar (3 x)              device forward         device cls_logits
    d64_dh32    3   7.17e-3 / 3.01e-3          2.15e-2 / 9.03e-3      4.08e-3 / 1.07e-3      4.77e-3 / 1.48e-3
    d64_dh32    1   7.17e-3 / 3.05e-3          2.15e-2 / 9.15e-3      4.08e-3 / 5.08e-4      4.77e-3 / 1.50e-3
    d128_dh64   3   4.34e-3 / 1.70e-3          1.30e-2 / 5.10e-3      4.56e-3 / 1.29e-3      4.66e-3 / 1.58e-3
    d128_dh64   1   5.87e-3 / 1.65e-3          1.76e-2 / 4.95e-3      5.57e-3 / 1.25e-3      6.32e-3 / 1.30e-3

On the device before_norm / after_norm stand at 4.1e-3 to 6.6e-3 of their scale; the worst parameter gradient is 8.7e-3 / 9.3e-3 (K = 1 /
2, d64_dh32: a k_proj.weight) and 1.15e-2 (d128_dh64, both K: the last block's q_proj.weight) against 3e-2; the 20 steps take the loss
from 3.86 to 2.8e-3.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import sketch_vit_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (config, n) -> (logits figure, loss figure) of sketch_vit_ref.emulation
EMULATED = {('d64_dh32', 3): (7.17e-3, 3.01e-3), ('d64_dh32', 1): (7.17e-3, 3.05e-3),
            ('d128_dh64', 3): (4.34e-3, 1.70e-3), ('d128_dh64', 1): (5.87e-3, 1.65e-3)}
FACTOR = 3.0


def _model(cfg, sd, K=1):
    from svol_amd.modeling.sketch_vit import SketchViTClassifier
    m = SketchViTClassifier(cfg, R.NUM_LABELS, finetune_layers=K)
    m.load_state_dict(sd)
    return m.to(DEV)


@pytest.mark.parametrize('name,n', list(EMULATED))
def test_forward_and_cls_logits_against_fp64(name, n):
    cfg, sd, x, targets = R.setup(name, n)
    ref = R.reference(sd, cfg, x, targets)
    m = _model(cfg, sd).eval()
    xs, ts = x.to(DEV), targets.to(DEV)
    with torch.no_grad():
        before, after, logits = m(xs)
    for tag, got in (('before_norm', before), ('after_norm', after)):
        e = float((got.cpu().double() - ref[tag]).abs().max() / ref[tag].abs().max())
        print(f'{name} n={n} {tag}: {e:.3e}')
        assert e < 1e-2, (tag, e)
    m.train()
    with torch.no_grad():
        logits_c = m.cls_logits(xs)
        loss_c, hits = m.loss(xs, ts)
    torch.cuda.synchronize()
    assert logits.shape == logits_c.shape == (n, R.NUM_LABELS) and logits.dtype == torch.float32
    e_logits, e_loss = EMULATED[(name, n)]
    for tag, lg in (('forward', logits), ('cls_logits', logits_c)):
        rows = F.cross_entropy(lg.cpu().double(), targets, reduction='none')
        f = R.figures(lg, rows, ref)
        print(f'{name} n={n} {tag}: logits {f.logits:.3e} (<= {FACTOR * e_logits:.3e})  loss {f.loss:.3e} (<= {FACTOR * e_loss:.3e})')
        assert f.logits <= FACTOR * e_logits and f.loss <= FACTOR * e_loss, (tag, f)
    own = F.cross_entropy(logits_c.cpu().double(), targets)
    assert abs(float(loss_c) - float(own)) <= 1e-5 * float(own)
    assert abs(float(loss_c) - float(ref['loss'])) <= FACTOR * e_loss * float(ref['loss'])
    assert int(hits) == int((logits_c.argmax(1).cpu() == targets).sum())
    # the four saved features are reductions of forward's outputs
    m.train()
    feats = m.extract_features(xs)
    assert m.training
    L = before.shape[1]
    for tag, t in (('before_norm', before), ('after_norm', after)):
        assert set(feats[tag]) == {'class_token', 'feature_avg'}
        assert torch.equal(feats[tag]['class_token'], t[:, 0])
        mean = t[:, 1:].double().mean(1)
        bound = L * 2.0 ** -24 * t[:, 1:].double().abs().mean(1)
        assert bool(((feats[tag]['feature_avg'].double() - mean).abs() <= bound).all())
        assert feats[tag]['feature_avg'].dtype == torch.float32 and feats[tag]['feature_avg'].shape == (n, cfg.hidden_size)


def _device_grads(m, x, targets):
    m.train()
    for p in m.parameters():
        p.grad = None
    loss, _ = m.loss(x.to(DEV), targets.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in m.named_parameters()}


@pytest.mark.parametrize('K', [1, 2])
@pytest.mark.parametrize('name', list(R.CFGS))
def test_gradients_of_the_loss_against_fp64_autograd(name, K):
    cfg, sd, x, targets = R.setup(name, 3, layers=3)
    m = _model(cfg, sd, K)
    grads = _device_grads(m, x, targets)
    sdr = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    vit, W, b = R.split(sdr)
    from oracle.vit_oracle import vit_forward
    last, _ = vit_forward(vit, cfg, x.double())
    R.head(last, W, b, targets)[2].backward()
    trained = {k for k in sd if k.startswith(tuple(f'vit.layers.{i}.' for i in range(3 - K, 3)) + ('vit.layernorm.', 'classifier.'))}
    assert {k for k, g in grads.items() if g is not None} == trained
    top = max(float(sdr[k].grad.norm()) for k in trained)
    kb = {k for k in trained if k.endswith('attention.k_proj.bias')}
    assert all(float(grads[k].norm()) <= 1e-3 * top for k in kb), {k: float(grads[k].norm()) / top for k in kb}
    errs = {k: float((grads[k].cpu().double() - sdr[k].grad).norm() / sdr[k].grad.norm()) for k in trained - kb}
    print(f'{name} K={K}: worst {max(errs.values()):.3e} ({max(errs, key=errs.get)})')
    bad = {k: e for k, e in errs.items() if e > 3e-2}
    assert not bad, bad


def _deterministic_worker():
    """run in a child process under SVOL_DETERMINISTIC=1 (the weight-gradient GEMMs and LayerNorm column reductions then sum in a fixed
    order): two backward passes of the same model and batch give the same bits"""
    cfg, sd, x, targets = R.setup('d128_dh64', 3, layers=3)
    m = _model(cfg, sd, 2)
    a, b = _device_grads(m, x, targets), _device_grads(m, x, targets)
    assert any(g is not None for g in a.values())
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    print('deterministic OK')


def test_gradients_are_bit_reproducible_in_deterministic_mode():
    env = dict(os.environ, SVOL_DETERMINISTIC='1')
    code = 'import tests.test_gpu_sketch_vit as t; t._deterministic_worker()'
    p = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and 'deterministic OK' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_finetune_loop_and_checkpoint_round_trip(tmp_path):
    from svol_amd import parallel
    from svol_amd.modeling.sketch_vit import SketchViTClassifier
    from svol_amd.utils.checkpoint import load_sketch_vit_checkpoint, save_sketch_vit_checkpoint
    cfg, sd, x, targets = R.setup('d128_dh64', 4)
    m = _model(cfg, sd).train()
    xs, ts = x.to(DEV), targets.to(DEV)
    params = [p for p in m.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(m), ordered=True)
    opt = parallel.FlatAdamW(red, lr=1e-3, weight_decay=1e-4, params=params)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    losses = []
    for step in range(21):
        red.zero_grad()
        loss, _ = m.loss(xs, ts)
        losses.append(float(loss.detach()))
        if step == 20:
            break
        loss.backward()
        red.finish()
        opt.step()
    torch.cuda.synchronize()
    print('loss', ' '.join(f'{v:.4f}' for v in losses))
    assert all(map(lambda v: v == v and abs(v) < 1e30, losses)) and losses[20] < losses[0]
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]) != p.requires_grad, k
    path = str(tmp_path / 'sketch_vit_9.pt')
    save_sketch_vit_checkpoint(path, m, opt, 9)
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    assert set(ckpt) == {'model', 'optimizer', 'epoch'} and ckpt['epoch'] == 9
    assert next(iter(ckpt['model'])).startswith('ViTEmbeddings.') and 'Classifier.weight' in ckpt['model']
    m2 = SketchViTClassifier(cfg, R.NUM_LABELS, finetune_layers=1)
    assert load_sketch_vit_checkpoint(path, m2)['epoch'] == 9
    m2.to(DEV).eval()
    m.eval()
    with torch.no_grad():
        a, b = m(xs), m2(xs)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    m.train()
    m2.train()
    with torch.no_grad():
        assert torch.equal(m.cls_logits(xs), m2.cls_logits(xs))


def test_vit_base_widths_forward_and_backward():
    from svol_amd import synthetic as syn
    cfg = syn.vit_config(num_hidden_layers=2)
    sd = syn.synth_classifier(cfg, 24, seed=3)
    from svol_amd.modeling.sketch_vit import SketchViTClassifier
    m = SketchViTClassifier(cfg, 24, finetune_layers=1)
    m.load_state_dict(sd)
    m.to(DEV).train()
    x = syn.synth_images(2, cfg, seed=4).to(DEV)
    targets = torch.tensor([3, 23], device=DEV)
    loss, hits = m.loss(x, targets)
    loss.backward()
    m.eval()
    with torch.no_grad():
        _, _, logits = m(x)
    torch.cuda.synchronize()
    own = F.cross_entropy(logits.double(), targets)
    assert abs(float(loss.detach()) - float(own)) <= 2e-2 * float(own)      # the two paths round differently: bf16 operands on both
    trained = [p for p in m.parameters() if p.requires_grad]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in trained)
    assert all(p.grad is None for p in m.parameters() if not p.requires_grad)
    assert float(m.classifier.weight.grad.norm()) > 0 and float(m.vit.layers[-1].mlp.fc1.weight.grad.norm()) > 0
