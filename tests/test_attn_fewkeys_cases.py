"""tests/attn_fewkeys_cases.py on the CPU: the point table covers what it says, the chunk rule is the library's, the emulation of the
kernels' rounding sites meets every figure, and its worst slice error per operand type is the constant tests/test_gpu_attn_fewkeys.py
derives its bar from (3 x, the project's factor)."""
from __future__ import annotations

import math

import pytest
import torch

from tests import attn_fewkeys_cases as A


def test_points_cover_every_edge():
    pts = A.points()
    assert 36 <= len(pts) <= 44 and len(set(pts)) == len(pts)
    for Lk in A.LKS:
        assert {p[4] for p in pts if p[3] == Lk} == set(A.DHS), Lk
    assert {p[2] for p in pts} >= set(A.LQS) | {2049}
    assert {p[1] for p in pts} == {1, 3} and {p[0] for p in pts} == {1, 2}
    assert {p[5] for p in pts} == set(A.FAMILIES) and {p[6] for p in pts} == set(A.MASKS)
    assert any(p[7] for p in pts)
    # the chunk edges: one chunk exactly, two chunks with a one-row tail, two tiles per chunk with a one-row last chunk
    assert A.chunk_rows(256) == 256 and A.chunk_rows(257) == 256 and -(-257 // 256) == 2
    assert A.chunk_rows(2049) == 512 and 2049 % 512 == 1
    for p in pts:     # masks differ per batch row and never mask a whole row
        kb = A.key_bias(p[0], p[3], p[6])
        if kb is not None:
            assert not torch.equal(kb[0], kb[1]) and bool((kb == 0).any(1).all())


def test_chunk_rule_is_the_librarys():
    from svol_amd import ops
    for Lq in (1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 6272, 1 << 20):
        assert ops.attn_fewkeys_chunk(Lq) == A.chunk_rows(Lq), Lq
        assert -(-Lq // A.chunk_rows(Lq)) <= 8
    assert ops.attn_fewkeys_ws_bytes(8, 8, 6272, 49, 32) == 8 * 8 * 7 * 2 * 64 * 32 * 4
    assert ops.attn_fewkeys_ok(torch.bfloat16, 49, 32) and ops.attn_fewkeys_ok(torch.float16, 256, 64)
    assert not ops.attn_fewkeys_ok(torch.float32, 49, 32) and not ops.attn_fewkeys_ok(torch.bfloat16, 257, 32)
    assert not ops.attn_fewkeys_ok(torch.bfloat16, 49, 40) and not ops.attn_fewkeys_ok(torch.bfloat16, 0, 32)
    # the dispatch rule: the measured shapes (profiles/sketch_tokens.md) and nothing beyond them at dh = 32
    assert ops.attn_fewkeys_faster(49, 32) and ops.attn_fewkeys_faster(197, 32) and ops.attn_fewkeys_faster(98, 64)
    assert not ops.attn_fewkeys_faster(198, 32) and not ops.attn_fewkeys_faster(256, 32) and ops.attn_fewkeys_faster(256, 64)


def test_masked_and_canary_rows_are_hostile():
    c = A.make_case(2, 3, 257, 49, 32, 'normal', 'edges', True, A.BF16)
    B, H, Lq, Lk, dh = c['dims']
    assert bool(torch.isnan(c['k'][0]).all()) and bool(torch.isnan(c['v'][2 * Lk - 1]).all())
    assert bool(torch.isnan(c['v'][B * Lk:]).all()) and bool(torch.isnan(c['q'][B * Lq:]).all())
    assert float(c['k'][B * Lk:].abs().min()) == A.CANARY_MAG
    ref = A.reference(2, 3, 257, 49, 32, 'normal', 'edges', True, A.BF16)
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    assert float(ref[3][0].abs().max()) == 0.0 and float(ref[4][2 * Lk - 1].abs().max()) == 0.0


def test_reference_is_torchs_attention():
    """the fp64 reference against torch's scaled_dot_product_attention and autograd at a masked point"""
    p = (2, 3, 33, 49, 32, 'normal', 'edges', False, A.FP16)
    c = A.make_case(*p)
    B, H, Lq, Lk, dh = c['dims']
    q, k, v, do = (torch.nan_to_num(t.double(), nan=0.0) for t in A.real(c))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    h4 = lambda t, L: t.view(B, L, H, dh).transpose(1, 2)   # noqa: E731
    o = torch.nn.functional.scaled_dot_product_attention(h4(q, Lq), h4(k, Lk), h4(v, Lk), attn_mask=c['kbias'].double()[:, None, None, :])
    o = o.transpose(1, 2).reshape(B * Lq, H * dh)
    o.backward(do)
    o_r, _, dq_r, dk_r, dv_r = A.reference(*p)
    for a, b in ((o, o_r), (q.grad, dq_r), (k.grad, dk_r), (v.grad, dv_r)):
        assert float((a.detach() - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('dt', A.DTYPES, ids=['bf16', 'fp16'])
def test_emulation_meets_every_figure_and_sets_the_bar(dt):
    from tests import test_gpu_attn_fewkeys as G
    worst, where = 0.0, None
    for p in A.points():
        c = A.make_case(*p, dt)
        fig = A.figures(c, A.emulation(*p, dt), A.reference(*p, dt), math.inf)
        assert not A.failing(fig), (A.point_id(*p), A.failing(fig))
        w = A.worst_slice(fig)
        if w > worst:
            worst, where = w, p
    quoted, at = G.EMULATED[dt]
    print(f'{dt}: emulation worst slice {worst:.3e} at {A.point_id(*where)}')
    assert at == where
    assert abs(worst - quoted) <= 0.005 * quoted
    assert G.BARS[dt] == 3.0 * quoted
