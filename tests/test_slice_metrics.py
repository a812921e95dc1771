"""The slice metric (tests/slice_metrics.py) is sensitive enough for the bars tests/test_gpu_layer_blocks.py uses: a reference with
16-bit-sized noise passes at the largest 16-bit bar, and a further 5 % error confined to one head, one 128-row tile, the tail tile,
one video or one parameter block fails it and is named — where a norm-wise bar over the whole tensor would not notice."""
import pytest
import torch

from tests import slice_metrics as S
from tests.test_gpu_layer_blocks import BARS, COMP_BARS, NOISE_16

# the 16-bit bars that claim 5 % sensitivity (the 'zero' and single-layer 'gate' groups do not: see BARS)
BAR = max([BARS[dt][k] for dt in (torch.bfloat16, torch.float16) for k in ('fwd', 'act', 'param')] +
          [COMP_BARS[k] for k in ('fwd', 'act', 'param', 'gate')])
H = 8


def _noisy(ref, seed):
    """ref with independent relative noise per element, sized so that the WORST slice lands near NOISE_16, the worst slice error the
    16-bit kernels show on the device (a typical slice sits below its tensor's worst one)."""
    g = torch.Generator().manual_seed(seed)
    return ref * (1 + NOISE_16 / 1.5 * torch.randn(ref.shape, generator=g, dtype=torch.float64))


def _ref(shape, seed):
    g = torch.Generator().manual_seed(seed)
    # uneven magnitudes: rows and columns of different scale, as real activations and gradients have
    r = torch.randn(shape, generator=g, dtype=torch.float64)
    r = r * torch.exp(0.5 * torch.randn(shape[:-1] + (1,), generator=g, dtype=torch.float64))
    return r * torch.exp(0.3 * torch.randn(shape[-1:], generator=g, dtype=torch.float64))


# (tensor kind, shape, the slice as an index, the name the metric must report)
ACT = (3, 1000, 256)                # [B, L, D], D / H = 32 columns per head, tail tile rows 896:1000
CASES = [
    ('one head', 'act', ACT, (1, slice(None), slice(96, 128)), 'b=1, head=3'),
    ('one 128-row tile', 'act', ACT, (2, slice(256, 384), slice(None)), 'rows 256:384'),
    ('the tail tile', 'act', ACT, (0, slice(896, 1000), slice(None)), 'rows 896:1000'),
    ('one video', 'act', ACT, (2, slice(None), slice(None)), 'b=2'),
    ('one head of dskch', 'bd', (8, 256), (5, slice(64, 96)), 'b=5, head=2'),
    ('K rows of one head', 'in_proj_weight', (768, 256), (slice(256 + 5 * 32, 256 + 6 * 32), slice(None)), 'k, head=5'),
    ('V bias of one head', 'in_proj_bias', (768,), (slice(512, 544),), 'v, head=0'),
    ('one head of out_proj', 'out_proj_weight', (256, 256), (slice(None), slice(224, 256)), 'head=7 columns'),
    ('one fc1 row block', 'row_blocks', (2048, 256), (slice(1920, 2048), slice(None)), 'rows 1920:2048'),
    ('one fc1 bias block', 'row_blocks', (2048,), (slice(128, 256),), 'rows 128:256'),
    ('one fc2 column block', 'col_blocks', (256, 2048), (slice(None), slice(384, 512)), 'columns 384:512'),
    ('one LayerNorm chunk', 'vector', (256,), (slice(32, 64),), '[32:64]'),
]


def test_bars_stay_below_a_single_slice_5_percent_error():
    """every 16-bit bar leaves room for the noise the kernels show and is below what a 5 % slice error produces"""
    assert NOISE_16 < BAR < 0.05


@pytest.mark.parametrize('what,kind,shape,idx,name', CASES, ids=[c[0] for c in CASES])
def test_5_percent_in_one_slice_fails_and_is_named(what, kind, shape, idx, name):
    ref = _ref(shape, 1)
    got = _noisy(ref, 2)
    clean = S.compare('t', got, ref, kind, H)
    assert clean.finite and 0.6 * NOISE_16 <= clean.err <= BAR, f'{what}: noise alone fails (or is not 16-bit sized): {clean}'
    bad = got.clone()
    bad[idx] = bad[idx] + 0.05 * ref[idx]
    r = S.compare('t', bad, ref, kind, H)
    assert r.err > BAR, f'{what}: a 5 % error in one slice passes: {r}'
    assert name in r.where, f'{what}: the worst slice is {r.where}, expected {name}'
    if kind in ('act', 'in_proj_weight', 'out_proj_weight') and what != 'one video':
        # the whole-tensor norm-wise error of the same result: what a per-parameter L2 bar (bench-shaped bf16: 3e-2) sees
        whole = float((bad - ref).norm() / ref.norm())
        assert whole < 0.03, whole


def test_non_finite_and_exact_results():
    ref = _ref(ACT, 3)
    assert S.compare('t', ref.clone(), ref, 'act', H).err == 0.0
    bad = ref.clone()
    bad[1, 999, 3] = float('nan')
    r = S.compare('t', bad, ref, 'act', H)
    assert not r.finite and r.err == float('inf')
    # a slice whose reference is zero is measured against the floor, not divided by zero
    z = ref.clone()
    z[0, :128] = 0
    got = z.clone()
    got[0, :128] = 1e-3 * float(z.norm()) / z.numel() ** 0.5
    assert S.compare('t', got, z, 'act', H).err < 2.0


def test_element_bar():
    ref = _ref((256, 256), 4)
    got = ref.clone()
    got[17, 3] += 0.5 * float(ref.abs().max())
    assert abs(S.compare('t', got, ref, 'out_proj_weight', H).elem - 0.5) < 1e-12


@pytest.mark.parametrize('name,kind', [('layers.0.content_self_attn.in_proj_weight', 'in_proj_weight'),
                                       ('token_self_attn.in_proj_bias', 'in_proj_bias'),
                                       ('content_token_cross_attn.out_proj.weight', 'out_proj_weight'),
                                       ('content_token_cross_attn.out_proj.bias', 'vector'), ('mlp1.fc1.weight', 'row_blocks'),
                                       ('mlp2.fc1.bias', 'row_blocks'), ('mlp1.fc2.weight', 'col_blocks'), ('mlp2.fc2.bias', 'vector'),
                                       ('norm3.weight', 'vector'), ('norm6.bias', 'vector')])
def test_param_kind(name, kind):
    assert S.param_kind(name) == kind
