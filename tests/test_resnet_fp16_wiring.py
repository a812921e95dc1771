"""Host wiring of the fp16 ResNet extractors (no device): --compute_dtype reaches both extractors through build_backbone in the frozen
and the trainable mode, ResNetBackbone asks its FrameIngest for the NHWC image in the extractors' own 16-bit type, the BatchNorm fold
rounds once from fp32, and refold() refuses fp16 weights that a tiny running variance pushed past 65504 (bf16 cannot overflow there)."""
import pytest
import torch

from svol_amd import configs

_TORCH = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}


@pytest.mark.parametrize('train', [0, 1], ids=['frozen', 'trainable'])
@pytest.mark.parametrize('d', ['bf16', 'fp16', 'fp32'])
def test_build_backbone_hands_the_compute_dtype_to_both_extractors(d, train):
    from svol_amd.modeling.model import build_backbone
    from svol_amd.modeling.resnet import ResNetBackbone
    args = configs.parse_args(['--backbone', 'resnet', '--compute_dtype', d, '--train_backbone', str(train)])
    bb = build_backbone(args)
    assert isinstance(bb, ResNetBackbone) and args.input_vid_dim == 512 and args.input_skch_dim == 512
    for ex in (bb.video_backbone, bb.sketch_backbone):
        assert ex.compute_dtype == _TORCH[d]
        assert ex.trainable == bool(train)
        assert all(p.requires_grad == bool(train) for p in ex.parameters())
    assert bb.sketch_backbone.avgpool and not bb.video_backbone.avgpool
    want = {'bf16': (True, 'nhwc_bf16'), 'fp16': (True, 'nhwc_f16'), 'fp32': (False, 'nchw_f32')}[d]
    assert (bb.nhwc, bb.ingest.out) == want


def test_extractor_takes_the_dtype_by_name_or_as_a_torch_dtype():
    from svol_amd.modeling.resnet import ResNetBackbone, ResNetExtractor
    a = ResNetExtractor((1,), (8,), 8, compute_dtype='fp16')
    b = ResNetExtractor((1,), (8,), 8, compute_dtype=torch.float16, avgpool=True)
    assert a.compute_dtype == torch.float16 and b.compute_dtype == torch.float16
    assert ResNetBackbone(a, b).ingest.out == 'nhwc_f16'
    # two different 16-bit types share no NHWC image: the float route
    mixed = ResNetBackbone(a, ResNetExtractor((1,), (8,), 8, compute_dtype='bf16', avgpool=True))
    assert mixed.nhwc is False and mixed.ingest.out == 'nchw_f32'


def test_fold_rounds_the_fp32_product_once():
    from svol_amd.modeling.resnet import _fold
    g = torch.Generator().manual_seed(0)
    conv = torch.nn.Conv2d(5, 7, 3, bias=False)
    bn = torch.nn.BatchNorm2d(7)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        bn.weight.copy_(1 + 0.3 * torch.randn(7, generator=g))
        bn.bias.copy_(torch.randn(7, generator=g))
        bn.running_mean.copy_(torch.randn(7, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(7, generator=g))
    w32, b32 = _fold(conv, bn, torch.float32)
    w16, b16 = _fold(conv, bn, torch.float16)
    assert w16.dtype == torch.float16 and w16.shape == (7, 64) and b16.dtype == torch.float32
    assert torch.equal(w16, w32.to(torch.float16)) and torch.equal(b16, b32)
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    ref = (conv.weight.detach() * scale[:, None, None, None]).permute(0, 2, 3, 1).reshape(7, 45)
    assert torch.equal(w32[:, :45], ref) and float(w32[:, 45:].abs().max()) == 0.0


def _planted(dtype):
    from svol_amd.modeling.resnet import ResNetExtractor
    torch.manual_seed(0)
    m = ResNetExtractor((1, 1), (8, 16), 8, compute_dtype=dtype)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape))          # weights ~ 1
        bn = getattr(m, '5')[0].bn2
        bn.weight[3] = 1e3                             # gamma / sqrt(var + eps) = 1e3 / sqrt(1e-8 + 1e-5) = 3.2e5 > 65504
        bn.running_var[3] = 1e-8
    return m.eval()


def test_refold_names_the_unit_whose_fp16_weights_overflow():
    with pytest.raises(ValueError, match=r'5\.0\.conv2') as e:
        _planted('fp16').refold()
    assert '5.0.conv1' not in str(e.value) and '65504' in str(e.value)
    f = _planted('bf16').refold()                      # bf16 has fp32's exponent range
    assert all(bool(torch.isfinite(w).all()) for _, _, (w, _), (w2, _), _ in f['blocks'])
    assert _planted('fp16')._folded is None
