"""``--sketch_attn tokens`` without a device: the fp64 reference's V2 half against torch.nn.MultiheadAttention running the reference's
commented lines (cross_modal_transformer.py:129-135) literally, and the option's wiring: the flag is additive and defaults to 'gate',
the two modes share their state-dict keys, unused_parameters per mode, the mask expansion for n sketches, the token counts of
sketch_tokens = 'grid'."""
from __future__ import annotations

import torch
from torch import nn

from oracle import svol_oracle as O
from svol_amd import configs, parallel
from svol_amd import synthetic as syn
from tests import sketch_tokens_ref as R


def test_v2_half_is_the_references_commented_lines():
    torch.manual_seed(0)
    d, h, B, L, Ls = 64, 2, 2, 24, 5
    mha, norm1 = nn.MultiheadAttention(d, h).double(), nn.LayerNorm(d).double()
    csa, norm2, norm3 = nn.MultiheadAttention(d, h).double(), nn.LayerNorm(d).double(), nn.LayerNorm(d).double()
    fc1, fc2 = nn.Linear(d, 2048).double(), nn.Linear(2048, d).double()
    for m in (norm1, norm2, norm3):
        nn.init.uniform_(m.weight, 0.9, 1.1)
        nn.init.uniform_(m.bias, -0.1, 0.1)
    for m in (mha, csa):
        nn.init.uniform_(m.in_proj_bias, -0.1, 0.1)
        nn.init.uniform_(m.out_proj.bias, -0.1, 0.1)
    src_vid, vid_pos = torch.randn(L, B, d, dtype=torch.float64), torch.randn(L, B, d, dtype=torch.float64)
    src_skch, skch_pos = torch.randn(Ls, B, d, dtype=torch.float64), torch.randn(Ls, B, d, dtype=torch.float64)
    pad = torch.zeros((B, Ls), dtype=torch.bool)
    pad[1, -2:] = True
    with torch.no_grad():
        # V2 (7x7), sequence-first as the reference runs it
        q = src_vid + vid_pos
        k = src_skch + skch_pos
        v = src_skch
        mem, att1 = mha(q, k, v, key_padding_mask=pad)
        mem = mem + src_vid
        mem = norm1(mem)
        # :137-143
        q = k = mem + vid_pos
        v = mem
        mem, att2 = csa(q, k, v)
        mem = mem + v
        mem = norm2(mem)
        mem = mem + fc2(torch.nn.functional.gelu(fc1(mem)))
        mem = norm3(mem)
        p = 'layer.'
        sd = {}
        for name, m in (('sketch_video_cross_attn', mha), ('content_self_attn', csa)):
            sd.update({p + name + '.in_proj_weight': m.in_proj_weight, p + name + '.in_proj_bias': m.in_proj_bias,
                       p + name + '.out_proj.weight': m.out_proj.weight, p + name + '.out_proj.bias': m.out_proj.bias})
        for name, m in (('norm1', norm1), ('norm2', norm2), ('norm3', norm3), ('mlp1.fc1', fc1), ('mlp1.fc2', fc2)):
            sd.update({p + name + '.weight': m.weight, p + name + '.bias': m.bias})
        bf = lambda t: t.transpose(0, 1)   # noqa: E731
        got = R.video_half_tokens(sd, p, h, bf(src_vid), bf(src_skch), bf(vid_pos), bf(skch_pos), pad)
    assert float((got - bf(mem)).abs().max()) <= 1e-12
    assert float(att1[1, :, -2:].abs().max()) == 0.0     # the padded sketch tokens get no weight


def test_reference_ignores_padded_sketch_tokens_and_sees_the_sketch():
    args = R.case_args()
    inp = R.case_inputs(args)
    sd = {k: v.double() for k, v in syn.synth_state_dict(args, seed=1).items()}
    base = R.model_forward(sd, args, inp)['pred_logits']
    junk = dict(inp, src_sketch=inp['src_sketch'].clone())
    junk['src_sketch'][R.PAD_ROW, R.LS - R.PAD_TOKENS:] = float('nan')
    assert torch.equal(R.model_forward(sd, args, junk)['pred_logits'], base)
    perm = dict(inp, src_sketch=inp['src_sketch'].clone())
    perm['src_sketch'][:, :3] = inp['src_sketch'][:, [2, 0, 1]]
    moved = float((R.model_forward(sd, args, perm)['pred_logits'] - base).abs().max())
    args_np = R.case_args(use_sketch_pos=False)
    still = float((R.model_forward(sd, args_np, perm)['pred_logits'] - R.model_forward(sd, args_np, inp)['pred_logits']).abs().max())
    assert moved > 1e-6 and still <= 1e-12, (moved, still)


def test_sketch_attn_flag_is_additive_and_defaults_to_gate():
    assert 'sketch_attn' not in configs.reference_defaults()
    assert configs.parse_args([]).sketch_attn == 'gate'
    assert configs.parse_args(['--sketch_attn', 'tokens']).sketch_attn == 'tokens'
    try:
        configs.parse_args(['--sketch_attn', 'grid'])
    except SystemExit:
        pass
    else:
        raise AssertionError('--sketch_attn takes gate or tokens only')


def _build(**over):
    from svol_amd.modeling.model import build_model
    return build_model(R.case_args(**over))


def test_modes_share_state_dict_keys_and_differ_in_unused_parameters():
    gate, tokens, default = _build(sketch_attn='gate'), _build(sketch_attn='tokens'), _build()
    assert default.head.transformer.sketch_attn == 'tokens'      # (case_args asks for tokens)
    no_flag = R.case_args()
    del no_flag.sketch_attn
    from svol_amd.modeling.model import build_model
    m = build_model(no_flag)
    assert m.head.transformer.sketch_attn == 'gate' and all(l.sketch_attn == 'gate' for l in m.head.transformer.layers)
    assert list(gate.state_dict().keys()) == list(tokens.state_dict().keys())
    assert [tuple(v.shape) for v in gate.state_dict().values()] == [tuple(v.shape) for v in tokens.state_dict().values()]
    names = lambda mod: {n for n, p in mod.named_parameters() if any(p is q for q in parallel.unused_parameters(mod))}   # noqa: E731
    g, t = names(gate), names(tokens)
    assert any('sketch_video_cross_attn.out_proj' in n for n in g)
    assert not any('sketch_video_cross_attn' in n for n in t)
    assert g - t == {n for n in g if 'sketch_video_cross_attn.out_proj' in n} and t <= g
    try:
        _build(sketch_attn='grid')
    except ValueError:
        pass
    else:
        raise AssertionError("sketch_attn='grid' must be refused")


def test_mask_expansion_for_n_sketches():
    from svol_amd.modeling.model import SketchLocalizationModel

    class Head(nn.Module):
        def forward(self, sk, skm, vd, vdm):
            return skm, vdm

    class Backbone(nn.Module):
        def forward(self, sk, vd):
            return sk, vd.flatten(1, 2)

    m = SketchLocalizationModel(Backbone(), Head())
    vd = torch.zeros((2, 4, 6, 8))
    vmask = torch.ones((2, 4))
    # one sketch of one token / of 49 tokens: the factor is the token count, as it always was
    for Ls in (1, 49):
        skm, vdm = m(torch.zeros((2, Ls, 8)), vd, torch.tensor([[1.0], [0.0]]), vmask)
        assert skm.tolist() == [[1.0] * Ls, [0.0] * Ls] and tuple(vdm.shape) == (2, 24)
    # three sketches of 49 tokens, the third one of row 1 missing
    skm, _ = m(torch.zeros((2, 3 * 49, 8)), vd, torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0]]), vmask)
    assert tuple(skm.shape) == (2, 147) and skm[0].tolist() == [1.0] * 147 and skm[1].tolist() == [1.0] * 98 + [0.0] * 49
    # three pooled sketches
    skm, _ = m(torch.zeros((2, 3, 8)), vd, torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 1.0]]), vmask)
    assert skm.tolist() == [[1.0, 1.0, 1.0], [1.0, 0.0, 1.0]]


def test_grid_sketch_tokens_by_shape_arithmetic():
    from svol_amd.modeling.model import build_backbone
    for backbone, width in (('resnet', 512), ('resnet50', 2048)):
        for st, pooled in (('pooled', True), ('grid', False), (None, True)):
            a = R.case_args(backbone=backbone, compute_dtype='bf16', train_backbone=0)
            if st is not None:
                a.sketch_tokens = st
            bb = build_backbone(a)
            assert bb.sketch_backbone.avgpool is pooled and bb.video_backbone.avgpool is False and a.input_skch_dim == width
    for st, want in (('pooled', 'pooled'), ('grid', 'grid')):
        a = R.case_args(backbone='vit', compute_dtype='bf16')
        a.sketch_tokens = st
        assert build_backbone(a).sketch_tokens == want
    a = R.case_args(backbone='resnet')
    a.sketch_tokens = 'all'
    try:
        build_backbone(a)
    except ValueError:
        pass
    else:
        raise AssertionError("sketch_tokens='all' must be refused")


class _StubResNet(nn.Module):
    """the shapes of ResNetExtractor.forward on 224 x 224 pixels: [n, 7 * 7, C] in the compute dtype, or [n, C] fp32 with avgpool"""
    compute_dtype, out_channels = torch.bfloat16, 16

    def __init__(self, avgpool):
        super().__init__()
        self.avgpool = avgpool

    def forward(self, pix, nhwc=False):
        n, hw = pix.shape[0], (pix.shape[-1] // 32) ** 2
        tok = torch.arange(n * hw * self.out_channels, dtype=torch.float32).view(n, hw, self.out_channels)
        return tok.mean(1) if self.avgpool else tok.to(self.compute_dtype)


class _StubViT(nn.Module):
    """the shapes of ViTExtractor.forward: [n, 1 + (224 / 16)^2, d]"""
    cfg = syn.vit_config(hidden_size=8)

    def uses_autograd(self):
        return False

    def forward(self, pix):
        n, P = pix.shape[0], (pix.shape[-1] // self.cfg.patch_size) ** 2
        return torch.arange(n * (P + 1) * 8, dtype=torch.float32).view(n, P + 1, 8)


def test_backbones_hand_over_the_sketch_grid():
    """what the backbones' forward returns, with stub extractors of the real ones' output shapes (no device): one token per sketch
    when pooled, 49 / 197 per sketch with the grid, n sketches side by side in the token dimension, the frames' tokens as before"""
    from svol_amd.modeling.backbone import ViTBackbone
    from svol_amd.modeling.resnet import ResNetBackbone
    B, T = 2, 3
    frames = torch.zeros((B, T, 3, 224, 224))
    for n_sk in (1, 2):
        sketches = torch.zeros((B, n_sk, 3, 224, 224))
        for pooled, per in ((True, 1), (False, 49)):
            sk, vd = ResNetBackbone(_StubResNet(False), _StubResNet(pooled))(sketches, frames)
            assert tuple(sk.shape) == (B, n_sk * per, 16) and tuple(vd.shape) == (B, T * 49, 16)
            # row b of the result holds sketch b's tokens in order (the view keeps the extractor's row order)
            want = _StubResNet(pooled)(sketches.flatten(0, 1)).reshape(B, n_sk * per, 16)
            assert torch.equal(sk.float(), want.float())
        for st, per in (('pooled', 1), ('grid', 197)):
            sk, vd = ViTBackbone(_StubViT(), _StubViT(), sketch_tokens=st)(sketches, frames)
            assert tuple(sk.shape) == (B, n_sk * per, 8) and tuple(vd.shape) == (B, T * 196, 8)
            full = _StubViT()(sketches.flatten(0, 1))
            assert torch.equal(sk, (full if st == 'grid' else full[:, :1]).reshape(B, n_sk * per, 8))


def test_oracle_pieces_are_imported_not_restated():
    import inspect
    src = inspect.getsource(R)
    for name in ('O.mha', 'O.input_proj', 'O.position_embedding_sine', 'O.query_self', 'O.query_cross', 'O._ln'):
        assert name in src
    assert R.O is O
