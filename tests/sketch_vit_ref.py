"""References for svol_amd.modeling.sketch_vit.SketchViTClassifier (plain torch on the CPU, importable without the device library).

    reference(sd, cfg, x, targets)   fp64: oracle.vit_oracle.vit_forward -> F.linear on the [CLS] state -> F.cross_entropy, the chain of
                                     preprocess/sketch_vit_finetune.py:79-85,140-141
    emulation(sd, cfg, x, targets)   the same chain in fp64 arithmetic with bf16 roundings where the device rounds: both operands of every
                                     bf16 linear map (patch embedding, q / k / v, out-projection, fc1, fc2: the LayerNorm outputs, the
                                     GELU output and the weights) and the attention output.  The residual stream, the LayerNorms, the
                                     softmax and the classifier (an fp32 GEMM on the device) are not rounded.
    figures(...)                     the error figures the device tests hold the model to, 3 x the emulation's:
                                       logits  max |logits - ref| / max |ref|
                                       loss    the worst row's |loss_i - ref_i| / the mean loss (the mean's own error is a sum of a few
                                               terms of either sign; the worst row bounds it and does not vanish by luck)

sd: the state dict of transformers.ViTForImageClassification (svol_amd.synthetic.synth_classifier).
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle.vit_oracle import vit_forward

BF16 = torch.bfloat16
CFGS = {'d64_dh32': dict(hidden_size=64, num_attention_heads=2, intermediate_size=128, image_size=32, num_hidden_layers=2),
        'd128_dh64': dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_size=48, num_hidden_layers=2)}
NUM_LABELS = 19
SEED = 1


def setup(name, n, layers=None, seed=SEED):
    """-> (cfg, sd, pixel_values [n, 3, S, S], targets [n]) of one named config"""
    from svol_amd import synthetic as syn
    over = dict(CFGS[name])
    if layers is not None:
        over['num_hidden_layers'] = layers
    cfg = syn.vit_config(**over)
    sd = syn.synth_classifier(cfg, NUM_LABELS, seed)
    x = syn.synth_images(n, cfg, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    return cfg, sd, x, torch.randint(0, NUM_LABELS, (n,), generator=g)


def split(sd):
    """-> (the ViT's entries without their prefix, classifier weight, classifier bias)"""
    return {k[4:]: v for k, v in sd.items() if k.startswith('vit.')}, sd['classifier.weight'], sd['classifier.bias']


def head(last, W, b, targets):
    """-> (logits [n, C], row losses [n], mean loss) from the final states [n, L, d]"""
    logits = F.linear(last[:, 0], W, b)
    rows = F.cross_entropy(logits, targets, reduction='none')
    return logits, rows, rows.mean()


def reference(sd, cfg, x, targets):
    """fp64 -> dict(before_norm, after_norm, logits, rows, loss)"""
    vit, W, b = split({k: v.double() for k, v in sd.items()})
    last, pre = vit_forward(vit, cfg, x.double())
    logits, rows, loss = head(last, W, b, targets)
    return dict(before_norm=pre, after_norm=last, logits=logits, rows=rows, loss=loss)


def _r(t):
    return t.to(BF16).double()


def emulation(sd, cfg, x, targets):
    """fp64 arithmetic, bf16 roundings at the device's sites (module docstring) -> the same dict"""
    vit, W, b = split({k: v.double() for k, v in sd.items()})
    d, h = cfg.hidden_size, cfg.num_attention_heads
    dh, eps = d // h, cfg.layer_norm_eps
    lin = lambda t, p: F.linear(_r(t), _r(vit[p + '.weight']), vit[p + '.bias'])   # noqa: E731
    t = F.conv2d(_r(x.double()), _r(vit['embeddings.patch_embeddings.projection.weight']), vit['embeddings.patch_embeddings.projection.bias'],
                 stride=cfg.patch_size)
    t = t.flatten(2).transpose(1, 2)
    n = t.shape[0]
    t = torch.cat([vit['embeddings.cls_token'].expand(n, -1, -1), t], dim=1) + vit['embeddings.position_embeddings']
    for i in range(cfg.num_hidden_layers):
        p = f'layers.{i}.'
        y = F.layer_norm(t, (d,), vit[p + 'layernorm_before.weight'], vit[p + 'layernorm_before.bias'], eps)
        sp = lambda u: u.view(n, -1, h, dh).transpose(1, 2)   # noqa: E731
        q, k, v = (sp(lin(y, p + f'attention.{nm}_proj')) for nm in 'qkv')
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1) @ v
        t = t + lin(a.transpose(1, 2).reshape(n, -1, d), p + 'attention.o_proj')      # (lin rounds its input: the attention output)
        y = F.layer_norm(t, (d,), vit[p + 'layernorm_after.weight'], vit[p + 'layernorm_after.bias'], eps)
        t = t + lin(F.gelu(lin(y, p + 'mlp.fc1')), p + 'mlp.fc2')
    last = F.layer_norm(t, (d,), vit['layernorm.weight'], vit['layernorm.bias'], eps)
    logits, rows, loss = head(last, W, b, targets)
    return dict(before_norm=t, after_norm=last, logits=logits, rows=rows, loss=loss)


def figures(got_logits, got_rows, ref):
    """-> SimpleNamespace(logits, loss): the two error figures of the module docstring"""
    gl, gr = got_logits.detach().double().cpu(), got_rows.detach().double().cpu()
    return SimpleNamespace(logits=float((gl - ref['logits']).abs().max() / ref['logits'].abs().max()),
                           loss=float((gr - ref['rows']).abs().max() / ref['loss'].abs()))
