"""Trainable ViT-B/16 extractor on the MI355X: svol_attn_small_fwd_lse / svol_attn_small_bwd against fp64 math, the extractor's
parameter gradients against fp64 autograd of oracle/vit_oracle.py (HF ViTModel), partial fine-tuning
(preprocess/sketch_vit_finetune.py), weight freshness under fused AdamW, and one reference-style training step through build_model.
Bars are estimates, not measurements: bf16 operands (P and dS rounded to bf16 before their products) against fp64."""
import math
import os
import subprocess
import sys

import pytest
import torch

from svol_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2, 5, 32), (2, 2, 17, 64), (2, 12, 197, 64), (1, 4, 256, 32), (2, 3, 33, 64)]


def _qkv(n, H, L, dh, seed):
    torch.manual_seed(seed)
    d = H * dh
    return (torch.randn(n * L, 3 * d) * 1.2).bfloat16(), (torch.randn(n * L, d)).bfloat16()


def _fwd(g, n, H, L, dh, lse=True):
    from svol_amd import ops
    d = H * dh
    return ops.attn_small_fwd(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], n, H, L, dh, want_lse=lse)


@pytest.mark.parametrize('n,H,L,dh', SHAPES + [(1, 1, 1, 64)])
def test_fwd_lse_matches_the_plain_forward_and_fp64(n, H, L, dh):
    qkv, _ = _qkv(n, H, L, dh, L)
    g = qkv.to(DEV)
    o_plain, _ = _fwd(g, n, H, L, dh, lse=False)
    o, lse2 = _fwd(g, n, H, L, dh)
    torch.cuda.synchronize()
    assert torch.equal(o, o_plain)
    d = H * dh
    sp = lambda t: t.double().view(n, L, H, dh).transpose(1, 2)  # noqa: E731
    s = sp(qkv[:, :d]) @ sp(qkv[:, d:2 * d]).transpose(-1, -2) / math.sqrt(dh)
    ref = torch.logsumexp(s, -1) / math.log(2.0)
    assert float((lse2.cpu().double() - ref).abs().max()) <= 1e-4


def _bwd_ref(qkv, do, n, H, L, dh):
    d = H * dh
    sp = lambda t: t.double().view(n, L, H, dh).transpose(1, 2).detach().requires_grad_(True)  # noqa: E731
    q, k, v = sp(qkv[:, :d]), sp(qkv[:, d:2 * d]), sp(qkv[:, 2 * d:])
    o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), -1) @ v
    o.backward(do.double().view(n, L, H, dh).transpose(1, 2))
    back = lambda t: t.grad.transpose(1, 2).reshape(n * L, d)  # noqa: E731
    return back(q), back(k), back(v)


def _bwd(g, o, lse2, do, n, H, L, dh, out=None):
    from svol_amd import ops
    d = H * dh
    if out is None:
        out = torch.empty((n * L, 3 * d), dtype=torch.bfloat16, device=DEV)
    ops.attn_small_bwd(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], o, do, lse2, n, H, L, dh, out[:, :d], out[:, d:2 * d], out[:, 2 * d:3 * d])
    return out


@pytest.mark.parametrize('n,H,L,dh', SHAPES)
def test_attn_small_bwd_against_fp64_autograd(n, H, L, dh):
    qkv, do = _qkv(n, H, L, dh, L + 1)
    g, dog = qkv.to(DEV), do.to(DEV)
    o, lse2 = _fwd(g, n, H, L, dh)
    out = _bwd(g, o, lse2, dog, n, H, L, dh)
    torch.cuda.synchronize()
    d = H * dh
    for j, ref in enumerate(_bwd_ref(qkv, do, n, H, L, dh)):
        got = out[:, j * d:(j + 1) * d].cpu().double()
        mx = float(ref.abs().max())
        assert float((got - ref).abs().max()) <= 2e-2 * mx, ('dq', 'dk', 'dv')[j]
        assert float((got - ref).norm() / ref.norm()) <= 1e-2, ('dq', 'dk', 'dv')[j]


def test_attn_small_bwd_is_deterministic():
    n, H, L, dh = 2, 12, 197, 64
    qkv, do = _qkv(n, H, L, dh, 7)
    g, dog = qkv.to(DEV), do.to(DEV)
    o, lse2 = _fwd(g, n, H, L, dh)
    a = _bwd(g, o, lse2, dog, n, H, L, dh)
    b = _bwd(g, o, lse2, dog, n, H, L, dh)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize('n,H,L,dh', [(2, 2, 17, 64), (1, 4, 256, 32), (2, 12, 197, 64)])
def test_attn_small_bwd_writes_nothing_outside_its_slices(n, H, L, dh):
    """dq / dk / dv as column slices of a wider buffer with sentinel columns between and after them and sentinel rows past n*L."""
    qkv, do = _qkv(n, H, L, dh, 3)
    g, dog = qkv.to(DEV), do.to(DEV)
    o, lse2 = _fwd(g, n, H, L, dh)
    d = H * dh
    pad = 8
    buf = torch.full((n * L + 5, 3 * (d + pad)), 7.0, dtype=torch.bfloat16, device=DEV)
    from svol_amd import ops
    sl = [buf[:n * L, j * (d + pad):j * (d + pad) + d] for j in range(3)]
    ops.attn_small_bwd(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], o, dog, lse2, n, H, L, dh, *sl)
    ref = _bwd(g, o, lse2, dog, n, H, L, dh)
    torch.cuda.synchronize()
    mask = torch.ones_like(buf, dtype=torch.bool)
    for j in range(3):
        mask[:n * L, j * (d + pad):j * (d + pad) + d] = False
        assert torch.equal(sl[j], ref[:, j * d:(j + 1) * d])
    assert bool((buf[mask] == 7.0).all())


# ---- the extractor ------------------------------------------------------------------------------------------------------------
def _ext(cfg, sd, **kw):
    from svol_amd.modeling.backbone import ViTExtractor
    m = ViTExtractor(cfg, **kw)
    m.load_state_dict(sd)
    return m.to(DEV)


def _loss(last, R0, R1):
    return (last[:, 0] * R0).sum() + (last[:, 1:] * R1).sum()


CFGS = {'d64_dh32': dict(hidden_size=64, num_attention_heads=2, intermediate_size=128, image_size=32, num_hidden_layers=2),
        'd128_dh64': dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_size=48, num_hidden_layers=2),
        'vitb_2layers': dict(num_hidden_layers=2)}


def _setup(name, n=2, seed=1):
    cfg = syn.vit_config(**CFGS[name])
    sd = syn.synth_vit_state_dict(cfg, seed=seed)
    x = syn.synth_images(n, cfg, seed=seed + 1)
    L = (cfg.image_size // cfg.patch_size) ** 2 + 1
    gen = torch.Generator().manual_seed(seed + 2)
    R0 = torch.randn(n, cfg.hidden_size, generator=gen)
    R1 = torch.randn(n, L - 1, cfg.hidden_size, generator=gen)
    return cfg, sd, x, R0, R1


def _grads(m, x, R0, R1):
    m.train()
    for p in m.parameters():
        p.grad = None
    last = m(x.to(DEV))
    _loss(last, R0.to(DEV), R1.to(DEV)).backward()
    torch.cuda.synchronize()
    return last.detach(), {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in m.named_parameters()}


@pytest.mark.parametrize('name', list(CFGS))
def test_trainable_forward_is_the_frozen_forward(name):
    cfg, sd, x, R0, R1 = _setup(name)
    frozen = _ext(cfg, sd).eval()
    with torch.no_grad():
        ref = frozen(x.to(DEV))
    last, _ = _grads(_ext(cfg, sd, trainable=True), x, R0, R1)
    assert torch.equal(last, ref)


@pytest.mark.parametrize('name', list(CFGS))
def test_extractor_gradients_against_fp64_oracle(name):
    """norm-wise <= 3e-2 per parameter.  Except the key biases: their exact gradient is zero (b_k adds q . b_k to every score of
    a row, which the softmax cancels), so the fp64 reference is rounding noise and a relative error means nothing; the first run
    measured the bf16 residue at ~3e-5 of the largest parameter-gradient norm, the bar asks for <= 1e-3 of it."""
    from oracle.vit_oracle import vit_forward
    cfg, sd, x, R0, R1 = _setup(name)
    m = _ext(cfg, sd, trainable=True)
    _, grads = _grads(m, x, R0, R1)
    sdr = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    last, _ = vit_forward(sdr, cfg, x.double())
    _loss(last, R0.double(), R1.double()).backward()
    assert set(grads) == set(sdr) and all(g is not None for g in grads.values())
    top = max(float(t.grad.norm()) for t in sdr.values())
    kb = {k for k in sdr if k.endswith('attention.k_proj.bias')}
    assert all(float(grads[k].norm()) <= 1e-3 * top for k in kb), {k: float(grads[k].norm()) / top for k in kb}
    errs = {k: float((grads[k].cpu().double() - t.grad).norm() / t.grad.norm()) for k, t in sdr.items() if k not in kb}
    bad = {k: e for k, e in errs.items() if e > 3e-2}
    assert not bad, bad


def _partial_worker():
    """run in a child process under SVOL_DETERMINISTIC=1: the weight-gradient GEMMs and LayerNorm column reductions then sum in a
    fixed order (by default they meet through fp32 atomics, whose arrival order varies from launch to launch)."""
    cfg, sd, x, R0, R1 = _setup('d128_dh64', seed=5)
    cfg.num_hidden_layers = 4
    sd = syn.synth_vit_state_dict(cfg, seed=5)
    full = _ext(cfg, sd, trainable=True)
    part = _ext(cfg, sd, trainable=True, train_layers=2)
    _, gf = _grads(full, x, R0, R1)
    _, gp = _grads(part, x, R0, R1)
    trained = {k for k, p in part.named_parameters() if p.requires_grad}
    assert trained == {k for k in gp if k.startswith(('layers.2.', 'layers.3.', 'layernorm.'))}
    for k, g in gp.items():
        if k in trained:
            assert g is not None and torch.equal(g, gf[k]), k
        else:
            assert g is None, k
    print('partial OK')


def test_partial_finetuning_gradients_are_the_full_ones():
    env = dict(os.environ, SVOL_DETERMINISTIC='1')
    code = 'import tests.test_gpu_vit_train as t; t._partial_worker()'
    p = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and 'partial OK' in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_weights_are_fresh_after_fused_adamw_steps():
    """the trainable path casts its bf16 weights every training forward (fused AdamW on ROCm does not bump _version), and the
    frozen path of the same extractor in eval mode does not serve copies from before the steps."""
    cfg, sd, x, R0, R1 = _setup('d128_dh64', seed=9)
    m = _ext(cfg, sd, trainable=True).train()
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, fused=True)
    xs = x.to(DEV)
    with torch.no_grad():
        m.eval()
        m(xs)          # fills the frozen path's weight cache with the step-0 weights
        m.train()
    for step in range(2):
        out = m(xs)
        if step == 1:
            ref_m = _ext(cfg, {k: v.detach().cpu() for k, v in sd1.items()}, trainable=True).train()
            torch.cuda.synchronize()
            assert torch.equal(out, ref_m(xs))
            break
        _loss(out, R0.to(DEV), R1.to(DEV)).backward()
        opt.step()
        opt.zero_grad()
        sd1 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.eval()
    ref_m.eval()
    with torch.no_grad():
        assert torch.equal(m(xs), ref_m(xs))


def test_build_model_trains_the_vit_and_round_trips_a_checkpoint(tmp_path):
    from svol_amd import configs, parallel
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.model import build_model
    from svol_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    argv = ['--backbone', 'vit', '--train_backbone', '1', '--hidden_dim', '64', '--nheads', '8', '--num_layers', '1',
            '--num_queries', '10', '--num_frames', '2', '--matcher', 'video_matcher', '--input_dropout', '0.0']
    args = configs.parse_args(argv)
    torch.manual_seed(1)
    model = build_model(args)
    cfg = syn.vit_config()
    model.backbone.video_backbone.load_state_dict(syn.synth_vit_state_dict(cfg, seed=1))
    model.backbone.sketch_backbone.load_state_dict(syn.synth_vit_state_dict(cfg, seed=2))
    model.to(DEV).train()
    crit = build_loss(args).to(DEV).train()
    assert all(p.requires_grad for p in model.backbone.parameters())
    params = [p for p in model.parameters() if p.requires_grad]
    red = parallel.BucketedGradAllReduce(parallel.arrival_order(model), skip=parallel.unused_parameters(model), ordered=True)
    opt = parallel.FlatAdamW(red, lr=1e-3, weight_decay=1e-4, params=params)
    B, T = 1, 2
    vid = syn.synth_images(B * T, cfg, seed=4).view(B, T, 3, 224, 224).to(DEV)
    sk = syn.synth_images(B, cfg, seed=5).view(B, 1, 3, 224, 224).to(DEV)
    before = {k: v.detach().clone() for k, v in model.backbone.named_parameters()}
    red.zero_grad()
    out = model(sk, vid, torch.ones(B, 1, device=DEV), torch.ones(B, T, device=DEV))
    crit(out, syn.synth_targets(B, T, seed=1))
    loss = crit.weighted_total()
    loss.backward()
    red.finish()
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    still = [k for k, p in model.backbone.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not still, f'{len(still)} backbone parameters did not move: {still[:5]}'
    path = str(tmp_path / 'm.ckpt')
    save_checkpoint(path, model, opt, None, 1, args)
    m2 = build_model(configs.parse_args(argv))
    load_checkpoint(path, m2)
    m2.to(DEV)
    model.eval()
    m2.eval()
    with torch.no_grad():
        o1 = model(sk, vid, torch.ones(B, 1, device=DEV), torch.ones(B, T, device=DEV))
        o2 = m2(sk, vid, torch.ones(B, 1, device=DEV), torch.ones(B, T, device=DEV))
    assert torch.equal(o1['pred_boxes'], o2['pred_boxes']) and torch.equal(o1['pred_logits'], o2['pred_logits'])
