"""Host side of the device-side dropout step counter (no GPU): the four ``*_sd`` entry points are declared, bound and exported with
their namesake's arguments plus the counter, ``transformer._drop`` hands a counter on without refusing, and the Transformer's
dropout state folds an installed counter in (``dropout_state``) and zeroes it (``load_dropout_state``)."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [('svol_dropout_sd', 'svol_dropout'), ('svol_dropout_add_sd', 'svol_dropout_add'),
         ('svol_attn_fwd_dropout_sd', 'svol_attn_fwd_dropout'), ('svol_attn_bwd_dropout_sd', 'svol_attn_bwd_dropout')]


def _declared_args():
    """{entry: [parameter declarations]} of include/svol_hip.h"""
    txt = open(os.path.join(REPO, 'include', 'svol_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'\b(svol_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', txt)}


@pytest.mark.parametrize('sd,base', PAIRS)
def test_seed_step_entries_are_declared_bound_and_exported(sd, base):
    from svol_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    decl = _declared_args()
    assert sd in decl, f'{sd} is not in include/svol_hip.h'
    assert len(decl[sd]) == len(decl[base]) + 1
    i = next(j for j, a in enumerate(decl[base]) if re.search(r'\bseed$', a))
    assert decl[sd][:i + 1] == decl[base][:i + 1] and decl[sd][i + 2:] == decl[base][i + 1:]
    assert re.fullmatch(r'const\s+int64_t\s*\*\s*seed_step_dev', decl[sd][i + 1]), decl[sd][i + 1]
    assert sd in _lib.SIGNATURES and len(_lib.SIGNATURES[sd]) == len(_lib.SIGNATURES[base]) + 1 == len(decl[sd])
    assert hasattr(_lib.lib(), sd), f'{sd} is not exported by the library'


def test_abi_version_stays_7():
    from svol_amd import _lib
    assert _lib.lib().svol_abi_version() == 7


def test_drop_hands_the_counter_on():
    from svol_amd.modeling import transformer as T
    layer = T.TransformerEncoderLayer(32, 4, 64, dropout=0.1).train()
    layer.layer_id = 3
    t = torch.zeros((1,), dtype=torch.int64)
    seed = (1 << 44) + (5 << 12)
    d = T._drop(layer, seed, 0, 1, seed_dev=t)
    assert isinstance(d, tuple) and len(d) == 4 and d[3] is t
    assert d[:3] == (0.1, seed + (3 << 4), seed + (3 << 4) + 1)   # the host seeds of the call without a counter
    layer.eval()
    assert T._drop(layer, seed, 0, 1, seed_dev=t) is None


def test_dropout_state_folds_the_counter_in_and_load_zeroes_it():
    from svol_amd.modeling.transformer import Transformer
    tr = Transformer(d_model=32, nhead=4, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=64, dropout=0.1)
    assert tr.step_dev is None
    tr.load_dropout_state({'drop_base_seed': 7, 'drop_step': 1234})
    assert tr.dropout_state() == {'drop_base_seed': 7, 'drop_step': 1234}          # no counter: as before
    tr.step_dev = torch.tensor([5], dtype=torch.int64)
    assert tr.dropout_state() == {'drop_base_seed': 7, 'drop_step': 1239}
    assert tr._drop_step == 1234
    tr.load_dropout_state({'drop_base_seed': 9, 'drop_step': 40})
    assert int(tr.step_dev[0]) == 0 and tr._drop_step == 40 and tr.drop_base_seed == 9
    assert tr.dropout_state() == {'drop_base_seed': 9, 'drop_step': 40}


def test_variant_heads_take_a_counter_and_keep_no_dropout_state():
    from svol_amd import synthetic as syn
    from svol_amd.modeling.sketch_detr import build_sketchdetr
    from svol_amd.modeling.svanet_variants import build_svanet
    for head in (build_svanet(syn.encdec_args()), build_sketchdetr(syn.encdec_args(sketch_head='sketch_detr'))):
        assert head.step_dev is None and not hasattr(head, 'dropout_state')
        assert [n for n, m in head.named_modules() if hasattr(m, 'dropout_state')] == ['transformer']
