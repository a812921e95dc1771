"""Host wiring of the fp16 ViT extractor, without a device: which dtype build_backbone hands the ViT, what the extractor and the
classifier accept, and that ops sends fp16 tensors to the ``_h16`` entry points and bf16 tensors to the entries they always took."""
import pytest
import torch


def _tiny(monkeypatch):
    from svol_amd import synthetic as syn
    from svol_amd.modeling import backbone
    cfg = syn.vit_config(hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128, image_size=32)
    monkeypatch.setattr(backbone, 'vit_base_config', lambda **over: cfg)
    return cfg


@pytest.mark.parametrize('head,vit', [('bf16', 'bf16'), ('fp16', 'fp16'), ('fp32', 'bf16')])
@pytest.mark.parametrize('train', ['0', '1'])
def test_build_backbone_hands_the_vit_fp16_only_under_an_fp16_head(monkeypatch, head, vit, train):
    from svol_amd import configs
    from svol_amd.modeling.model import build_backbone
    _tiny(monkeypatch)
    args = configs.parse_args(['--backbone', 'vit', '--compute_dtype', head, '--train_backbone', train])
    bb = build_backbone(args)
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16}[vit]
    for m in (bb.video_backbone, bb.sketch_backbone):
        assert m.compute_dtype == vit and m.dtype == dt and m.trainable == (train == '1')


def test_extractor_and_classifier_dtypes(monkeypatch):
    from svol_amd.modeling.backbone import ViTExtractor
    from svol_amd.modeling.sketch_vit import SketchViTClassifier
    cfg = _tiny(monkeypatch)
    assert ViTExtractor(cfg).dtype == torch.bfloat16
    assert ViTExtractor(cfg, compute_dtype='fp16').dtype == torch.float16
    for bad in ('fp32', 'fp8'):
        with pytest.raises(NotImplementedError):
            ViTExtractor(cfg, compute_dtype=bad)
    assert SketchViTClassifier(cfg, 19).vit.dtype == torch.bfloat16
    m = SketchViTClassifier(cfg, 19, finetune_layers=1, compute_dtype='fp16')
    assert m.vit.dtype == torch.float16 and m.vit.train_layers == 1
    with pytest.raises(NotImplementedError):
        SketchViTClassifier(cfg, 19, compute_dtype='fp32')


def test_ops_picks_the_h16_entry_for_fp16_tensors_only(monkeypatch):
    from svol_amd import _lib, ops

    class Lib:
        def __getattr__(self, name):
            return name

    monkeypatch.setattr(_lib, 'lib', lambda: Lib())
    for base in ('svol_attn_small_fwd', 'svol_attn_small_fwd_lse', 'svol_attn_small_bwd', 'svol_attn_cls_fwd', 'svol_attn_cls_bwd'):
        assert base in _lib.SIGNATURES and base + '_h16' in _lib.SIGNATURES
        assert _lib.SIGNATURES[base] == _lib.SIGNATURES[base + '_h16']
        assert ops._h16_entry(base, torch.zeros(1, dtype=torch.float16)) == (base + '_h16', base + '_h16')
        assert ops._h16_entry(base, torch.zeros(1, dtype=torch.bfloat16)) == (base, base)
