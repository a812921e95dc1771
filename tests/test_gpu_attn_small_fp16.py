"""The short-sequence (ViT) attention kernels of csrc/vit.hip with fp16 operands (their _Float16 instances, v_mfma_f32_32x32x16_f16)
through the ``_h16`` entry points, on the cases of tests/attn_small_cases.py converted to fp16 (tests/attn_h16_cases.py), against fp64
computed from the converted tensors.  a - e mirror tests/test_gpu_attn_small.py:

  a. parity: every (L, dh, family) point through ops.attn_small_fwd(want_lse=True) and ops.attn_small_bwd on fp16 tensors (which take
     svol_attn_small_fwd_lse_h16 / svol_attn_small_bwd_h16), packed as there.  Slice errors on (image, head, 32-row block) slices;
     element errors at gpu_checks.TOL[fp16] = 1.5e-3 for o and twice that for the gradients; lse2 at 2e-5 max(1, max |ref|); every
     value finite; L = 1 identities exact; 'deep' heads' dk / dv finite and within the element bar.
  b. the plain forward and the lse forward give the same o bits at every point.
  c. every point's forward and backward twice: bit-identical.
  d. through the C ABI with o, dq, dk, dv column slices of wider sentinel-filled buffers with sentinel rows behind n L, and lse2 a
     prefix of a longer sentinel-filled vector: the results are those of (a), the sentinels are intact (L = 33 and 225, both widths).
  e. the three ``_h16`` entry points' return codes for what they refuse; nothing is launched.
  f. the ``_h16`` entry points with SVOL_BF16 return the bits of the entries without the suffix (L = 97 and 225, both widths).

Slice bar (BARS): 3 x the worst slice error, over every point, of attn_dropout_ref.emulate with fp16 roundings (P, dS and the outputs);
tests/test_attn_h16_cases.py re-derives the worst point and holds EMULATED to it.  The factor is the project's
(tests/test_gpu_attn_small.py).  A device figure above a bar the emulation meets is a kernel finding, not a bar to move.

    emulation (worst point)                                    bar
    8.71e-4   L = 225, dh = 64, planted (dk rows 224:225)      2.61e-3
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from tests import attn_h16_cases as Hc
from tests import attn_small_cases as A

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F16 = Hc.F16
# worst slice error of the fp16 emulation, where (L, dh, family) and the slice's rows
EMULATED = (8.71e-4, (225, 64, 'planted'), 'rows 224:225')
BARS = 3.0 * EMULATED[0]
POINTS = A.points()
IDS = [A.point_id(*p) for p in POINTS]
SENTINEL = 7.0


def _packed(c):
    """-> (the packed [n L + 32, 3 d] q | k | v buffer, dO [n L + 32, d]) on the device"""
    return torch.cat([c['q'], c['k'], c['v']], 1).to(DEV), c['do'].to(DEV)


def run(c, lse=True):
    """forward and backward of one case -> (o, lse2, dq, dk, dv) on the device (o alone without lse).  Every operand the kernels read
    is the first n L rows of an allocation 32 rows longer."""
    from svol_amd import ops
    n, H, L, dh = c['dims']
    d, M = H * dh, n * L
    qkv, do = _packed(c)
    assert qkv.dtype == c['q'].dtype
    g = qkv[:M]
    o, lse2 = ops.attn_small_fwd(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], n, H, L, dh, want_lse=lse)
    if not lse:
        torch.cuda.synchronize()
        return o
    o_buf = torch.zeros((M + A.CANARY_ROWS, d), dtype=qkv.dtype, device=DEV)
    o_buf[:M] = o
    lse_buf = torch.zeros(n * H * L + A.CANARY_ROWS, dtype=torch.float32, device=DEV)
    lse_buf[:n * H * L] = lse2.reshape(-1)
    out = torch.empty((M, 3 * d), dtype=qkv.dtype, device=DEV)
    ops.attn_small_bwd(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], o_buf[:M], do[:M], lse_buf[:n * H * L].view(n, H, L), n, H, L, dh,
                       out[:, :d], out[:, d:2 * d], out[:, 2 * d:])
    torch.cuda.synchronize()
    return o, lse2, out[:, :d], out[:, d:2 * d], out[:, 2 * d:]


@functools.lru_cache(maxsize=None)
def first_run(L, dh, family):
    """one point's device result, computed once and shared (never modified)"""
    return run(Hc.small_case(L, dh, family))


def check(fig, what):
    bad = []
    for label, (val, bar) in fig.items():
        ok = val <= bar
        print(f'{what} {label}: {val:.3e} (<= {bar:.3e}){"" if ok else "   <-- FAILS"}')
        if not ok:
            bad.append(f'{label}: {val:.3e} vs {bar:.3e}')
    assert not bad, f'{what}: ' + '; '.join(bad)


def test_bars_are_the_projects():
    from tests import gpu_checks as G
    assert Hc.TOL == G.TOL[F16]


# ---- a. parity
@pytest.mark.parametrize('L,dh,family', POINTS, ids=IDS)
def test_parity_with_fp64_by_32_row_slice(L, dh, family):
    c = Hc.small_case(L, dh, family)
    got = first_run(L, dh, family)
    assert all(t.dtype == F16 for t in (got[0],) + got[2:])
    fig = Hc.small_figures(c, got, Hc.small_reference(L, dh, family), BARS)
    print(f'{A.point_id(L, dh, family)} worst slice {A.worst_slice(fig):.3e}')
    check(fig, A.point_id(L, dh, family))


# ---- b. the two forwards agree
@pytest.mark.parametrize('L,dh,family', POINTS, ids=IDS)
def test_plain_forward_gives_the_lse_forwards_bits(L, dh, family):
    o_plain = run(Hc.small_case(L, dh, family), lse=False)
    assert torch.equal(o_plain, first_run(L, dh, family)[0])


# ---- c. repeatability
@pytest.mark.parametrize('L,dh,family', POINTS, ids=IDS)
def test_forward_and_backward_are_bit_reproducible(L, dh, family):
    again = run(Hc.small_case(L, dh, family))
    for tag, a, b in zip(('o', 'lse2', 'dq', 'dk', 'dv'), first_run(L, dh, family), again):
        assert torch.equal(a, b), tag


# ---- d. nothing else written
@pytest.mark.parametrize('L,dh', [(33, 32), (33, 64), (225, 32), (225, 64)])
def test_nothing_is_written_outside_the_outputs(L, dh):
    from svol_amd import _lib
    from svol_amd.ops import _dt, _ptr, _stream
    c = Hc.small_case(L, dh, 'benign')
    n, H, _, _ = c['dims']
    d, M, pad = H * dh, n * L, 8
    qkv, do = _packed(c)
    g = qkv[:M]
    nl = n * H * L
    scale = 1.0 / math.sqrt(dh)
    lib = _lib.lib()
    qkv_args = (_ptr(g[:, :d]), 3 * d, _ptr(g[:, d:2 * d]), 3 * d, _ptr(g[:, 2 * d:]), 3 * d)
    o_ref, lse_ref, dq_ref, dk_ref, dv_ref = first_run(L, dh, 'benign')
    for with_lse in (False, True):
        buf = torch.full((M + 5, d + 2 * pad), SENTINEL, dtype=F16, device=DEV)
        o = buf[:M, pad:pad + d]
        lse_buf = torch.full((nl + 64,), SENTINEL, dtype=torch.float32, device=DEV)
        tail = (n, H, L, dh, scale, _dt(g), _stream())
        if with_lse:
            rc = lib.svol_attn_small_fwd_lse_h16(*qkv_args, _ptr(o), o.stride(0), _ptr(lse_buf), *tail)
        else:
            rc = lib.svol_attn_small_fwd_h16(*qkv_args, _ptr(o), o.stride(0), *tail)
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(o, o_ref)
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:M, pad:pad + d] = False
        assert bool((buf[mask] == SENTINEL).all()), 'the forward wrote outside its o slice'
        if with_lse:
            assert torch.equal(lse_buf[:nl], lse_ref.reshape(-1))
            assert bool((lse_buf[nl:] == SENTINEL).all()), 'the forward wrote behind lse2'
        else:
            assert bool((lse_buf == SENTINEL).all())
    # the backward: dq | dk | dv with sentinel columns between and around them and sentinel rows behind n L
    gb = torch.full((M + 5, 3 * (d + pad) + pad), SENTINEL, dtype=F16, device=DEV)
    sl = [gb[:M, pad + j * (d + pad):pad + j * (d + pad) + d] for j in range(3)]
    o_in = o_ref.contiguous()
    rc = lib.svol_attn_small_bwd_h16(*qkv_args, _ptr(o_in), d, _ptr(do), d, _ptr(lse_ref), _ptr(sl[0]), gb.stride(0), _ptr(sl[1]),
                                     gb.stride(0), _ptr(sl[2]), gb.stride(0), n, H, L, dh, scale, _dt(g), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    mask = torch.ones_like(gb, dtype=torch.bool)
    for j, ref in enumerate((dq_ref, dk_ref, dv_ref)):
        assert torch.equal(sl[j], ref), ('dq', 'dk', 'dv')[j]
        mask[:M, pad + j * (d + pad):pad + j * (d + pad) + d] = False
    assert bool((gb[mask] == SENTINEL).all()), 'the backward wrote outside its gradient slices'


# ---- e. refusals
def test_h16_entry_points_refuse_without_launching():
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    from tests.test_gpu_attn_small import _codes
    K = _codes()
    n, H, L, dh = 2, 3, 33, 32
    d, M = H * dh, n * L
    qkv = torch.zeros((M, 3 * d), dtype=F16, device=DEV)
    do = torch.zeros((M, d), dtype=F16, device=DEV)
    o = torch.full((M, d), SENTINEL, dtype=F16, device=DEV)
    lse2 = torch.full((n, H, L), SENTINEL, dtype=torch.float32, device=DEV)
    grads = torch.full((M, 3 * d), SENTINEL, dtype=F16, device=DEV)
    lib = _lib.lib()

    def call(entry, n=n, L=L, dh=dh, dtype=K['SVOL_F16'], ldq=3 * d, q_off=0, lse=True):
        q, k, v = _ptr(qkv) + q_off, _ptr(qkv[:, d:2 * d]), _ptr(qkv[:, 2 * d:])
        scale, lp = 1.0 / math.sqrt(dh), (_ptr(lse2) if lse else None)
        if entry == 'fwd':
            return lib.svol_attn_small_fwd_h16(q, ldq, k, 3 * d, v, 3 * d, _ptr(o), d, n, H, L, dh, scale, dtype, _stream())
        if entry == 'fwd_lse':
            return lib.svol_attn_small_fwd_lse_h16(q, ldq, k, 3 * d, v, 3 * d, _ptr(o), d, lp, n, H, L, dh, scale, dtype, _stream())
        return lib.svol_attn_small_bwd_h16(q, ldq, k, 3 * d, v, 3 * d, _ptr(o), d, _ptr(do), d, lp, _ptr(grads), 3 * d,
                                           _ptr(grads[:, d:2 * d]), 3 * d, _ptr(grads[:, 2 * d:]), 3 * d, n, H, L, dh, scale, dtype,
                                           _stream())

    unsupported = [dict(L=257), dict(dh=16), dict(dh=128), dict(dtype=K['SVOL_F32']), dict(dtype=7), dict(ldq=3 * d + 4), dict(q_off=2),
                   dict(n=65536)]
    for entry in ('fwd', 'fwd_lse', 'bwd'):
        for dt in (K['SVOL_F16'], K['SVOL_BF16']):
            for kw in unsupported:
                assert call(entry, **dict(dict(dtype=dt), **kw)) == K['SVOL_E_UNSUPPORTED'], (entry, dt, kw)
            assert call(entry, dtype=dt, L=0) == K['SVOL_E_INVALID'], entry
    assert call('fwd_lse', lse=False) == K['SVOL_E_INVALID']
    assert call('bwd', lse=False) == K['SVOL_E_INVALID']
    torch.cuda.synchronize()
    for t in (o, lse2, grads):
        assert bool((t == SENTINEL).all())


# ---- f. bf16 through the new entries
@pytest.mark.parametrize('L,dh', [(97, 32), (97, 64), (225, 32), (225, 64)])
def test_h16_entries_with_bf16_give_the_old_entries_bits(L, dh):
    from svol_amd import _lib
    from svol_amd.ops import _dt, _ptr, _stream
    c = A.make_case(L, dh, 'planted')
    n, H, _, _ = c['dims']
    d, M = H * dh, n * L
    qkv, do = _packed(c)
    assert qkv.dtype == torch.bfloat16
    g = qkv[:M]
    lib = _lib.lib()
    scale = 1.0 / math.sqrt(dh)
    qkv_args = (_ptr(g[:, :d]), 3 * d, _ptr(g[:, d:2 * d]), 3 * d, _ptr(g[:, 2 * d:]), 3 * d)
    tail = (n, H, L, dh, scale, _dt(g), _stream())
    res = {}
    for sfx in ('', '_h16'):
        o_plain = torch.zeros((M, d), dtype=g.dtype, device=DEV)
        o = torch.zeros((M, d), dtype=g.dtype, device=DEV)
        lse2 = torch.zeros((n, H, L), dtype=torch.float32, device=DEV)
        out = torch.zeros((M, 3 * d), dtype=g.dtype, device=DEV)
        assert getattr(lib, 'svol_attn_small_fwd' + sfx)(*qkv_args, _ptr(o_plain), d, *tail) == 0
        assert getattr(lib, 'svol_attn_small_fwd_lse' + sfx)(*qkv_args, _ptr(o), d, _ptr(lse2), *tail) == 0
        assert getattr(lib, 'svol_attn_small_bwd' + sfx)(*qkv_args, _ptr(o), d, _ptr(do), d, _ptr(lse2), _ptr(out), 3 * d,
                                                        _ptr(out[:, d:2 * d]), 3 * d, _ptr(out[:, 2 * d:]), 3 * d, *tail) == 0
        torch.cuda.synchronize()
        res[sfx] = (o_plain, o, lse2, out)
    for tag, a, b in zip(('o plain', 'o', 'lse2', 'dq | dk | dv'), res[''], res['_h16']):
        assert torch.equal(a, b), tag
    assert bool(res[''][3].float().abs().sum() > 0)
