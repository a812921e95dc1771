"""tests/resnet50_ref.py pinned to an independent implementation, and the CPU-side surface of --backbone resnet50.

a. the fp64 restatement against transformers.ResNetModel(layer_type='bottleneck', downsample_in_bottleneck=False) — a tiny config with
   random weights built offline — in fp64: features in eval and train mode, the updated running statistics, every parameter gradient,
   to 1e-10 relative.  The key map between the two layouts is keymap() below.
b. svol_amd.modeling.resnet.resnet50() constructs on the CPU with torchvision's shapes and loads the restatement's state dict.
c. the option surface: --backbone resnet50 parses and sets both input widths to 2048; --backbone resnet still builds 34 / 18 at 512.
"""
import pytest
import torch

from tests import resnet50_ref as R

STEM, PLANES, DEPTHS = 16, (8, 16), (1, 2)


def keymap(depths):
    """restatement (torchvision) key prefix -> transformers.ResNetModel key prefix, module by module"""
    m = {'0': 'embedder.embedder.convolution', '1': 'embedder.embedder.normalization'}
    for li, n in enumerate(depths):
        for bi in range(n):
            tv, hf = f'{4 + li}.{bi}', f'encoder.stages.{li}.layers.{bi}'
            for j in (1, 2, 3):
                m[f'{tv}.conv{j}'] = f'{hf}.layer.{j - 1}.convolution'
                m[f'{tv}.bn{j}'] = f'{hf}.layer.{j - 1}.normalization'
            m[f'{tv}.downsample.0'] = f'{hf}.shortcut.convolution'
            m[f'{tv}.downsample.1'] = f'{hf}.shortcut.normalization'
    return m


def to_hf(sd, depths):
    km = keymap(depths)
    return {km[k.rsplit('.', 1)[0]] + '.' + k.rsplit('.', 1)[1]: v for k, v in sd.items()}


def hf_model(depths, planes, stem):
    from transformers import ResNetConfig, ResNetModel
    cfg = ResNetConfig(num_channels=3, embedding_size=stem, hidden_sizes=[4 * p for p in planes], depths=list(depths), layer_type='bottleneck',
                       hidden_act='relu', downsample_in_first_stage=False, downsample_in_bottleneck=False)
    return ResNetModel(cfg).double()


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
def test_restatement_agrees_with_transformers_resnet_bottleneck(train):
    net, sd = R.build(DEPTHS, PLANES, STEM, seed=3)
    hf = hf_model(DEPTHS, PLANES, STEM)
    missing = hf.load_state_dict({k: v.double() for k, v in to_hf(sd, DEPTHS).items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    net.train(train)
    hf.train(train)
    x = R.synth_pixels(3, 32, seed=4).double()
    f = net(x)
    o = hf(x)
    assert f.shape == o.last_hidden_state.shape == (3, 4 * PLANES[-1], 4, 4)
    assert rel(f, o.last_hidden_state) <= 1e-10
    assert rel(f.mean((2, 3)), o.pooler_output.flatten(1)) <= 1e-10
    probe = torch.randn(f.shape, generator=torch.Generator().manual_seed(5)).double()
    (f * probe).sum().backward()
    (o.last_hidden_state * probe).sum().backward()
    km = keymap(DEPTHS)
    hp, hb = dict(hf.named_parameters()), dict(hf.named_buffers())
    n = 0
    for k, p in net.named_parameters():
        mod, leaf = k.rsplit('.', 1)
        assert rel(p.grad, hp[f'{km[mod]}.{leaf}'].grad) <= 1e-10, k
        n += 1
    assert n == len(hp)
    for k, b in net.named_buffers():   # running statistics: updated in train mode, untouched in eval mode
        mod, leaf = k.rsplit('.', 1)
        assert rel(b, hb[f'{km[mod]}.{leaf}']) <= 1e-10, k
        if leaf == 'num_batches_tracked':
            assert int(b) == (1 if train else 0)


def test_average_pool_and_token_order():
    net, sd = R.build(DEPTHS, PLANES, STEM, seed=3)
    pooled = R.RefBottleneckNet(DEPTHS, PLANES, STEM, avgpool=True)
    pooled.load_state_dict(sd)
    net.eval()
    pooled.eval()
    x = R.synth_pixels(2, 64, seed=6)
    f = net(x)
    assert f.shape == (2, 64, 8, 8) and pooled(x).shape == (2, 64)
    assert rel(pooled(x), f.mean((2, 3))) <= 1e-14
    t = R.tokens(f)
    assert t.shape == (2, 64, 64) and torch.equal(t[1, 8 * 2 + 3], f[1, :, 2, 3])


def test_resnet50_constructs_with_torchvisions_layout():
    from svol_amd.modeling.resnet import ResNetExtractor, resnet50
    m = resnet50()
    assert sum(p.numel() for p in m.parameters()) == 23_508_032
    assert m.out_channels == 2048
    sd = m.state_dict()
    for k, shape in (('0.weight', (64, 3, 7, 7)), ('4.0.conv1.weight', (64, 64, 1, 1)), ('4.0.conv3.weight', (256, 64, 1, 1)),
                     ('4.0.downsample.0.weight', (256, 64, 1, 1)), ('5.0.conv2.weight', (128, 128, 3, 3)), ('7.2.conv3.weight', (2048, 512, 1, 1))):
        assert tuple(sd[k].shape) == shape, k
    blk = getattr(m, '5')[0]
    assert blk.conv2.stride == (2, 2) and blk.conv1.stride == (1, 1) and blk.downsample[0].stride == (2, 2)
    assert getattr(m, '4')[0].downsample is not None and getattr(m, '4')[0].conv2.stride == (1, 1)
    assert getattr(m, '4')[1].downsample is None
    assert [len(getattr(m, str(i))) for i in (4, 5, 6, 7)] == [3, 4, 6, 3]
    assert not any(p.requires_grad for p in m.parameters())
    assert all(p.requires_grad for p in resnet50(trainable=True).parameters())
    ref = R.RefBottleneckNet()
    assert sum(p.numel() for p in ref.parameters()) == 23_508_032
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    tiny = ResNetExtractor((1, 2), (8, 16), 16, block='bottleneck')
    tiny.load_state_dict({k: v.float() for k, v in R.build((1, 2), (8, 16), 16, seed=1)[1].items()}, strict=True)
    with pytest.raises(RuntimeError, match='no CPU path'):
        m(torch.zeros(1, 3, 32, 32))


def test_backbone_resnet50_parses_and_sets_both_widths_to_2048():
    from svol_amd import configs
    from svol_amd.modeling.model import build_backbone
    from svol_amd.modeling.resnet import ResNetBackbone
    args = configs.parse_args(['--backbone', 'resnet50'])
    assert args.backbone == 'resnet50'
    bb = build_backbone(args)
    assert isinstance(bb, ResNetBackbone)
    assert args.input_vid_dim == 2048 and args.input_skch_dim == 2048
    assert bb.video_backbone.block == 'bottleneck' and bb.sketch_backbone.block == 'bottleneck'
    assert bb.video_backbone.out_channels == 2048 and bb.sketch_backbone.out_channels == 2048
    assert not bb.video_backbone.avgpool and bb.sketch_backbone.avgpool
    assert bb.video_backbone.trainable and bb.sketch_backbone.trainable          # the reference trains its backbone
    frozen = build_backbone(configs.parse_args(['--backbone', 'resnet50', '--freeze_backbone', '--compute_dtype', 'fp16']))
    assert not frozen.video_backbone.trainable and frozen.video_backbone.compute_dtype == torch.float16
    assert build_backbone(configs.parse_args(['--backbone', 'resnet50', '--train_backbone', '0', '--sync_bn'])).video_backbone.sync_bn


def test_backbone_resnet_still_builds_34_and_18_at_512():
    from svol_amd import configs
    from svol_amd.modeling.model import build_backbone
    args = configs.parse_args(['--backbone', 'resnet'])
    bb = build_backbone(args)
    assert args.input_vid_dim == 512 and args.input_skch_dim == 512
    assert bb.video_backbone.block == 'basic' and bb.sketch_backbone.block == 'basic'
    assert [len(getattr(bb.video_backbone, str(i))) for i in (4, 5, 6, 7)] == [3, 4, 6, 3]
    assert [len(getattr(bb.sketch_backbone, str(i))) for i in (4, 5, 6, 7)] == [2, 2, 2, 2]
    assert bb.video_backbone.out_channels == 512 and bb.sketch_backbone.out_channels == 512
