"""The ViT extractor with fp16 operands (``ViTExtractor(compute_dtype='fp16')``, ``--backbone vit --compute_dtype fp16``) on the MI355X:

  1. svol_patchify and svol_vit_embed with SVOL_F16 write ``x.to(float16)`` of their fp32 values, bit for bit.
  2. the frozen extractor on the committed tests/golden/vit_*.npz fixtures (fp32 transformers outputs): below the 1e-2 of
     tests/test_gpu_vit.py, and at most half the bf16 extractor's error on the same fixture, computed here.  fp16 rounds an operand 8 x
     finer than bf16 (11 significant bits against 8); the factor 2 leaves room for what both share: fp32 accumulation order, the fp32
     LayerNorm and GELU arithmetic, eps 1e-5 against 1e-12.
  3. the trainable forward is the frozen forward bit for bit.
  4. parameter gradients against fp64 autograd of oracle.vit_oracle on the three configurations of tests/test_gpu_vit_train.py (n = 2),
     the loss multiplied by gpu_checks.FP16_LOSS_SCALE = 4096 (a power of two: divided out exactly): every parameter within that file's
     3e-2, the key-bias residue <= 1e-3 of the largest gradient norm, and the L2 error of the whole gradient at most half the bf16
     extractor's on the same case.
  5. one training step of build_model(--backbone vit --train_backbone 1 --compute_dtype fp16) at the sizes of
     test_build_model_trains_the_vit_and_round_trips_a_checkpoint, FlatAdamW with loss_scale 4096: the loss is finite, every backbone
     parameter moves, both extractors report fp16.
  6. compute_dtype='fp32' still raises.
"""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from svol_amd import synthetic as syn
from tests.test_gpu_vit_train import CFGS, _loss, _setup

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F16 = torch.float16
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, 'golden', 'vit_*.npz')))


def test_patchify_and_embed_round_once_to_fp16():
    from svol_amd import _lib
    from svol_amd.ops import _DT, _ptr, _stream
    cfg = syn.vit_config(hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128, image_size=48)
    x = syn.synth_images(2, cfg, 4).to(DEV)
    n, C, H, W = x.shape
    p = cfg.patch_size
    P = (H // p) * (W // p)
    lib = _lib.lib()
    out32 = torch.empty((n * P, C * p * p), dtype=torch.float32, device=DEV)
    out16 = torch.zeros((n * P, C * p * p), dtype=F16, device=DEV)
    assert lib.svol_patchify(_ptr(x), _ptr(out32), n, C, H, W, p, _DT[torch.float32], _stream()) == 0
    assert lib.svol_patchify(_ptr(x), _ptr(out16), n, C, H, W, p, _DT[F16], _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out16, out32.to(F16)) and float(out16.float().abs().max()) > 0
    d = cfg.hidden_size
    proj, cls, pos = (torch.randn(s, device=DEV) for s in ((n * P, d), (1, 1, d), (1, P + 1, d)))
    x32 = torch.empty((n * (P + 1), d), device=DEV)
    x16 = torch.zeros((n * (P + 1), d), dtype=F16, device=DEV)
    assert lib.svol_vit_embed(_ptr(proj), _ptr(cls), _ptr(pos), _ptr(x32), _ptr(x16), n, P, d, _DT[F16], _stream()) == 0
    torch.cuda.synchronize()
    ref = torch.cat([cls.expand(n, -1, -1), proj.view(n, P, d)], 1) + pos
    assert torch.equal(x32.view(n, P + 1, d), ref)
    assert torch.equal(x16, x32.to(F16))


def _ext(cfg, sd, **kw):
    from svol_amd.modeling.backbone import ViTExtractor
    m = ViTExtractor(cfg, **kw)
    m.load_state_dict(sd)
    return m.to(DEV)


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(p)[4:-4] for p in FIXTURES])
def test_extractor_vs_transformers_and_vs_bf16(path):
    z = np.load(path)
    cfg = syn.vit_config(**ast.literal_eval(str(z['over'])))
    st = int(z['stride'])
    sd = syn.synth_vit_state_dict(cfg, int(z['seed']))
    x = syn.synth_images(int(z['n']), cfg, int(z['seed'])).to(DEV)
    ref, refp = torch.from_numpy(z['last_hidden_state']), torch.from_numpy(z['pre_norm'])
    errs = {}
    for cd in ('bf16', 'fp16'):
        m = _ext(cfg, sd, compute_dtype=cd).eval()
        assert m.compute_dtype == cd
        last, pre = m(x, return_pre_norm=True)
        assert last.dtype == torch.float32
        errs[cd] = (float((last.cpu()[:, ::st] - ref).abs().max()) / float(ref.abs().max()),
                    float((pre.cpu()[:, ::st] - refp).abs().max()) / float(refp.abs().max()))
        del m
    print(f'vit extractor rel err (last, pre-norm): bf16 {errs["bf16"][0]:.2e} {errs["bf16"][1]:.2e}   '
          f'fp16 {errs["fp16"][0]:.2e} {errs["fp16"][1]:.2e}')
    for e16, eb in zip(errs['fp16'], errs['bf16']):
        assert e16 < 1e-2
        assert e16 <= 0.5 * eb, (e16, eb)


def _grads(m, x, R0, R1, scale=1.0):
    m.train()
    for p in m.parameters():
        p.grad = None
    last = m(x.to(DEV))
    (_loss(last, R0.to(DEV), R1.to(DEV)) * scale).backward()
    torch.cuda.synchronize()
    return last.detach(), {k: p.grad.detach().cpu().double() / scale for k, p in m.named_parameters()}


@pytest.mark.parametrize('name', list(CFGS))
def test_trainable_forward_is_the_frozen_forward(name):
    cfg, sd, x, R0, R1 = _setup(name)
    frozen = _ext(cfg, sd, compute_dtype='fp16').eval()
    with torch.no_grad():
        ref = frozen(x.to(DEV))
    last, _ = _grads(_ext(cfg, sd, compute_dtype='fp16', trainable=True), x, R0, R1)
    assert torch.equal(last, ref)


@pytest.mark.parametrize('name', list(CFGS))
def test_extractor_gradients_against_fp64_oracle_and_bf16(name):
    from oracle.vit_oracle import vit_forward
    from tests import gpu_checks as G
    cfg, sd, x, R0, R1 = _setup(name)
    sdr = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    last, _ = vit_forward(sdr, cfg, x.double())
    _loss(last, R0.double(), R1.double()).backward()
    top = max(float(t.grad.norm()) for t in sdr.values())
    kb = {k for k in sdr if k.endswith('attention.k_proj.bias')}
    ref_norm = sum(float(t.grad.norm()) ** 2 for t in sdr.values()) ** 0.5
    whole = {}
    for cd, scale in (('bf16', 1.0), ('fp16', G.FP16_LOSS_SCALE)):
        _, grads = _grads(_ext(cfg, sd, compute_dtype=cd, trainable=True), x, R0, R1, scale)
        assert set(grads) == set(sdr)
        whole[cd] = sum(float((grads[k] - t.grad).norm()) ** 2 for k, t in sdr.items()) ** 0.5 / ref_norm
        if cd == 'fp16':
            assert all(bool(torch.isfinite(g).all()) for g in grads.values())
            res = {k: float(grads[k].norm()) / top for k in kb}
            errs = {k: float((grads[k] - t.grad).norm() / t.grad.norm()) for k, t in sdr.items() if k not in kb}
    print(f'{name}: whole-gradient L2 error bf16 {whole["bf16"]:.3e} fp16 {whole["fp16"]:.3e}; fp16 worst parameter '
          f'{max(errs.values()):.3e} ({max(errs, key=errs.get)}); key-bias residue {max(res.values()):.2e} of the largest norm')
    assert all(v <= 1e-3 for v in res.values()), res
    bad = {k: e for k, e in errs.items() if e > 3e-2}
    assert not bad, bad
    assert whole['fp16'] <= 0.5 * whole['bf16'], whole


def test_build_model_trains_the_fp16_vit_for_one_step():
    from svol_amd import configs, parallel
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.model import build_model
    from tests import gpu_checks as G
    argv = ['--backbone', 'vit', '--train_backbone', '1', '--compute_dtype', 'fp16', '--hidden_dim', '64', '--nheads', '8',
            '--num_layers', '1', '--num_queries', '10', '--num_frames', '2', '--matcher', 'video_matcher', '--input_dropout', '0.0']
    args = configs.parse_args(argv)
    torch.manual_seed(1)
    model = build_model(args)
    bb = model.backbone
    assert bb.video_backbone.compute_dtype == bb.sketch_backbone.compute_dtype == 'fp16'
    assert bb.video_backbone.dtype == bb.sketch_backbone.dtype == F16
    cfg = syn.vit_config()
    bb.video_backbone.load_state_dict(syn.synth_vit_state_dict(cfg, seed=1))
    bb.sketch_backbone.load_state_dict(syn.synth_vit_state_dict(cfg, seed=2))
    model.to(DEV).train()
    crit = build_loss(args).to(DEV).train()
    params = [p for p in model.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
    opt = parallel.FlatAdamW(red, lr=1e-3, weight_decay=1e-4, params=params)
    opt.loss_scale = G.FP16_LOSS_SCALE
    B, T = 1, 2
    vid = syn.synth_images(B * T, cfg, seed=4).view(B, T, 3, 224, 224).to(DEV)
    sk = syn.synth_images(B, cfg, seed=5).view(B, 1, 3, 224, 224).to(DEV)
    before = {k: v.detach().clone() for k, v in bb.named_parameters()}
    red.zero_grad()
    out = model(sk, vid, torch.ones(B, 1, device=DEV), torch.ones(B, T, device=DEV))
    crit(out, syn.synth_targets(B, T, seed=1))
    loss = crit.weighted_total()
    (loss * G.FP16_LOSS_SCALE).backward()
    red.finish()
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(bool(torch.isfinite(p).all()) for p in bb.parameters())
    still = [k for k, p in bb.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not still, f'{len(still)} backbone parameters did not move: {still[:5]}'


def test_fp32_extractor_still_raises():
    from svol_amd.modeling.backbone import ViTExtractor
    cfg = syn.vit_config(hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128, image_size=32)
    with pytest.raises(NotImplementedError):
        ViTExtractor(cfg, compute_dtype='fp32')
