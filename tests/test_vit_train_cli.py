"""Trainable ViT-B/16 extractor, host side and static (no GPU): the reference-style command line builds the extractors the
reference trains (train.py:72 optimises every parameter of build_model(args); preprocess/sketch_vit_finetune.py:43-69 the last K
layers + the final LayerNorm), and the short-sequence attention kernels of csrc/vit.hip — the new backward included — compile for
gfx950 without register spills or scratch."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ['--backbone', 'vit', '--num_layers', '1', '--num_queries', '10', '--matcher', 'video_matcher']
N_VIT = 4 + 12 * 16 + 2   # embeddings (cls, pos, patch W / b), 12 layers x 16, final LayerNorm


def _finetune_names(k):
    names = {'layernorm.weight', 'layernorm.bias'}
    for i in range(12 - k, 12):
        for m in ('attention.q_proj', 'attention.k_proj', 'attention.v_proj', 'attention.o_proj', 'layernorm_before',
                  'layernorm_after', 'mlp.fc1', 'mlp.fc2'):
            names |= {f'layers.{i}.{m}.weight', f'layers.{i}.{m}.bias'}
    return names


@pytest.mark.parametrize('extra,want', [([], None), (['--train_backbone', '1'], 'all'),
                                        (['--train_backbone', '1', '--finetune_layers', '2'], 2),
                                        (['--train_backbone', '0'], None), (['--freeze_backbone'], None)])
def test_vit_cli_builds_the_requested_extractors(extra, want):
    from svol_amd import configs
    from svol_amd.modeling.model import build_model
    args = configs.parse_args(BASE + extra)
    model = build_model(args)
    bb = list(model.backbone.parameters())
    assert len(bb) == 2 * N_VIT
    n_train = sum(1 for p in bb if p.requires_grad)
    for ext in (model.backbone.video_backbone, model.backbone.sketch_backbone):
        names = {n for n, p in ext.named_parameters() if p.requires_grad}
        if want is None:
            assert not names and not ext.trainable
        elif want == 'all':
            assert len(names) == N_VIT and ext.trainable and ext.train_layers is None
        else:
            assert names == _finetune_names(want) and ext.train_layers == want
    assert n_train == {None: 0, 'all': 2 * N_VIT, 2: 2 * 34}[want]
    n_opt = sum(1 for p in model.parameters() if p.requires_grad)   # train.py:72's list
    assert n_opt == sum(1 for p in model.head.parameters() if p.requires_grad) + n_train


def test_finetune_layers_is_a_build_extra():
    """--finetune_layers is additive: the reference's option surface (tests/golden/configs_defaults.json) is unchanged."""
    from svol_amd import configs
    assert 'finetune_layers' not in configs.reference_defaults()
    assert configs.parse_args([]).finetune_layers is None


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


def test_vit_kernels_compile_without_spills_or_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.fail('hipcc not found: the gfx950 build needs it')
    out = tmp_path / 'vit.s'
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-S',
                           os.path.join(REPO, 'svol_amd', 'csrc', 'vit.hip'), '-o', str(out)], cwd=REPO)
    asm = out.read_text()
    kernels = re.findall(r'\.amdhsa_kernel (\S+)', asm)
    assert any('attn_small_bwd_kernel' in k for k in kernels), kernels
    assert sum('attn_small_bwd_kernel' in k for k in kernels) == 2   # dh = 32 and 64
    for k in kernels:
        i = asm.index('.amdhsa_kernel ' + k)
        block = asm[i:asm.index('.end_amdhsa_kernel', i)]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', block).group(1)) == 0, k
    # the code-object metadata: one .vgpr_spill_count per kernel, all zero
    assert len(re.findall(r'\.vgpr_spill_count:\s+\d+', asm)) == len(kernels)
    assert len(re.findall(r'\.vgpr_spill_count:\s+0', asm)) == len(kernels)
