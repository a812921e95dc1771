"""The one-query ([CLS]) attention kernels of csrc/sketch_cls.hip with fp16 operands through the ``_h16`` entry points, on the cases of
tests/attn_cls_cases.py converted to fp16 (tests/attn_h16_cases.py), against fp64 computed from the converted tensors.  a - d mirror
tests/test_gpu_attn_cls.py:

  a. parity: every (n, H, L, dh, family) point through ops.attn_cls_fwd and ops.attn_cls_bwd on fp16 tensors (which take
     svol_attn_cls_fwd_h16 / svol_attn_cls_bwd_h16), packed as there.  Slice errors of o / dq per (image, head) and of dk / dv per
     (image, head, 64-key block); element errors at gpu_checks.TOL[fp16] = 1.5e-3 for o and twice that for the gradients; lse2 within
     2e-5 max(1, max |ref|); every value finite; L = 1: dq = dk = 0 and dv = dout exactly.
  b. every point's forward and backward twice: bit-identical.
  c. through the C ABI with o / dq / dk / dv as column slices of sentinel-filled buffers with sentinel rows behind them and lse2 a
     prefix of a longer sentinel-filled vector: the results are those of (a) and the sentinels are intact.
  d. the two ``_h16`` entry points' return codes for what they refuse; nothing is launched.
  e. the ``_h16`` entry points with SVOL_BF16 return the bits of the entries without the suffix (L = 97 and 225, both widths).

Slice bar (BARS): 3 x the worst slice error, over every point, of attn_h16_cases.cls_emulation (fp64 arithmetic, o / dq / dk / dv
rounded to fp16); tests/test_attn_h16_cases.py re-derives it and holds EMULATED to it.

    emulation (worst point)                                  bar
    4.49e-4   n2 H3 L = 65, dh = 64, deep (dk rows 64:65)    1.35e-3
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from tests import attn_cls_cases as A
from tests import attn_h16_cases as Hc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F16 = Hc.F16
# worst slice error of the fp16 emulation, where (n, H, L, dh, family) and the slice's rows
EMULATED = (4.49e-4, (2, 3, 65, 64, 'deep'), 'rows 64:65')
BARS = 3.0 * EMULATED[0]
POINTS = A.points()
IDS = [A.point_id(*p) for p in POINTS]
SENTINEL = 7.0


def _operands(c):
    """-> (q [n, d], the packed k | v buffer [n L + 32, 2 d], dout [n + 32, d]) on the device"""
    return c['q'].to(DEV), torch.cat([c['k'], c['v']], 1).to(DEV), c['do'].to(DEV)


def run(c):
    """forward and backward of one case -> (o, lse2, dq, dk, dv) on the device"""
    from svol_amd import ops
    n, H, L, dh = c['dims']
    d, M = H * dh, n * L
    q, kv, do = _operands(c)
    g = kv[:M]
    o, lse2 = ops.attn_cls_fwd(q, g[:, :d], g[:, d:], n, H, L, dh)
    dq = torch.empty((n, d), dtype=q.dtype, device=DEV)
    out = torch.empty((M, 2 * d), dtype=q.dtype, device=DEV)
    ops.attn_cls_bwd(q, g[:, :d], g[:, d:], o, do[:n], lse2, n, H, L, dh, dq, out[:, :d], out[:, d:])
    torch.cuda.synchronize()
    return o, lse2, dq, out[:, :d], out[:, d:]


@functools.lru_cache(maxsize=None)
def first_run(*p):
    """one point's device result, computed once and shared (never modified)"""
    return run(Hc.cls_case(*p))


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


@pytest.mark.parametrize('p', POINTS, ids=IDS)
def test_parity_with_fp64_by_slice(p):
    c = Hc.cls_case(*p)
    got = first_run(*p)
    assert all(t.dtype == F16 for t in (got[0],) + got[2:])
    fig = Hc.cls_figures(c, got, Hc.cls_reference(*p), BARS)
    print(f'{A.point_id(*p)} worst slice {A.worst_slice(fig):.3e}')
    check(fig, A.point_id(*p))


@pytest.mark.parametrize('p', POINTS, ids=IDS)
def test_forward_and_backward_are_bit_reproducible(p):
    again = run(Hc.cls_case(*p))
    for tag, a, b in zip(('o', 'lse2', 'dq', 'dk', 'dv'), first_run(*p), again):
        assert torch.equal(a, b), tag


@pytest.mark.parametrize('p', [(2, 3, 65, 32, 'benign'), (2, 3, 65, 64, 'benign'), (2, 3, 197, 32, 'benign'), (5, 1, 197, 64, 'benign')],
                         ids=lambda p: A.point_id(*p))
def test_nothing_is_written_outside_the_outputs(p):
    from svol_amd import _lib
    from svol_amd.ops import _dt, _ptr, _stream
    c = Hc.cls_case(*p)
    n, H, L, dh = c['dims']
    d, M, pad = H * dh, n * L, 8
    q, kv, do = _operands(c)
    g = kv[:M]
    small = torch.full((n + 5, 2 * (d + pad) + pad), SENTINEL, dtype=F16, device=DEV)     # | pad | o | pad | dq | pad |
    o, dq = small[:n, pad:pad + d], small[:n, 2 * pad + d:2 * pad + 2 * d]
    big = torch.full((M + 5, 2 * (d + pad) + pad), SENTINEL, dtype=F16, device=DEV)       # | pad | dk | pad | dv | pad |
    dk, dv = big[:M, pad:pad + d], big[:M, 2 * pad + d:2 * pad + 2 * d]
    lse_buf = torch.full((n * H + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    scale = 1.0 / math.sqrt(dh)
    lib = _lib.lib()
    rc = lib.svol_attn_cls_fwd_h16(_ptr(q), d, _ptr(g[:, :d]), 2 * d, _ptr(g[:, d:]), 2 * d, _ptr(o), o.stride(0), _ptr(lse_buf), n, H, L,
                                   dh, scale, _dt(q), _stream())
    assert rc == 0
    rc = lib.svol_attn_cls_bwd_h16(_ptr(q), d, _ptr(g[:, :d]), 2 * d, _ptr(g[:, d:]), 2 * d, _ptr(o), o.stride(0), _ptr(do), d,
                                   _ptr(lse_buf), _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), n, H, L, dh, scale,
                                   _dt(q), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    o_r, lse_r, dq_r, dk_r, dv_r = first_run(*p)
    for tag, a, b in (('o', o, o_r), ('dq', dq, dq_r), ('dk', dk, dk_r), ('dv', dv, dv_r), ('lse2', lse_buf[:n * H], lse_r.reshape(-1))):
        assert torch.equal(a, b), tag
    for buf, rows in ((small, n), (big, M)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:rows, pad:pad + d] = False
        mask[:rows, 2 * pad + d:2 * pad + 2 * d] = False
        assert bool((buf[mask] == SENTINEL).all()), 'a kernel wrote outside its output slices'
    assert bool((lse_buf[n * H:] == SENTINEL).all()), 'the forward wrote behind lse2'


def test_h16_entry_points_refuse_without_launching():
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    from tests.test_gpu_attn_cls import _codes
    K = _codes()
    n, H, L, dh = 2, 3, 33, 32
    d, M = H * dh, n * L
    q = torch.zeros((n, d + 8), dtype=F16, device=DEV)
    kv = torch.zeros((M, 2 * d), dtype=F16, device=DEV)
    do = torch.zeros((n, d), dtype=F16, device=DEV)
    o = torch.full((n, d), SENTINEL, dtype=F16, device=DEV)
    lse2 = torch.full((n, H), SENTINEL, dtype=torch.float32, device=DEV)
    dq = torch.full((n, d), SENTINEL, dtype=F16, device=DEV)
    grads = torch.full((M, 2 * d), SENTINEL, dtype=F16, device=DEV)
    lib = _lib.lib()

    def call(entry, n=n, L=L, dh=dh, dtype=K['SVOL_F16'], ldq=d + 8, ldk=2 * d, q_off=0, dk_off=0, lse=True, k=True):
        qp, kp, vp = _ptr(q) + q_off, (_ptr(kv) if k else None), _ptr(kv[:, d:])
        scale, lp = 1.0 / math.sqrt(dh), (_ptr(lse2) if lse else None)
        if entry == 'fwd':
            return lib.svol_attn_cls_fwd_h16(qp, ldq, kp, ldk, vp, 2 * d, _ptr(o), d, lp, n, H, L, dh, scale, dtype, _stream())
        return lib.svol_attn_cls_bwd_h16(qp, ldq, kp, ldk, vp, 2 * d, _ptr(o), d, _ptr(do), d, lp, _ptr(dq), d, _ptr(grads) + dk_off, 2 * d,
                                         _ptr(grads[:, d:]), 2 * d, n, H, L, dh, scale, dtype, _stream())

    unsupported = [dict(L=257), dict(dh=16), dict(dh=128), dict(dtype=K['SVOL_F32']), dict(dtype=7), dict(ldq=d + 4), dict(ldk=2 * d + 4),
                   dict(q_off=2), dict(q_off=8)]
    for entry in ('fwd', 'bwd'):
        for dt in (K['SVOL_F16'], K['SVOL_BF16']):
            for kw in unsupported:
                assert call(entry, **dict(dict(dtype=dt), **kw)) == K['SVOL_E_UNSUPPORTED'], (entry, dt, kw)
            for kw in (dict(L=0), dict(n=0), dict(lse=False), dict(k=False)):
                assert call(entry, dtype=dt, **kw) == K['SVOL_E_INVALID'], (entry, dt, kw)
    assert call('bwd', dk_off=4) == K['SVOL_E_UNSUPPORTED']
    torch.cuda.synchronize()
    for t in (o, lse2, dq, grads):
        assert bool((t == SENTINEL).all())


@pytest.mark.parametrize('L,dh', [(97, 32), (97, 64), (225, 32), (225, 64)])
def test_h16_entries_with_bf16_give_the_old_entries_bits(L, dh):
    """bf16 operands at L = 97 and 225 (no point of attn_cls_cases: randn * 1.2 drawn here), both head widths, n = 2, H = 3"""
    from svol_amd import _lib
    from svol_amd.ops import _dt, _ptr, _stream
    n, H = 2, 3
    d, M = H * dh, n * L
    gen = torch.Generator().manual_seed(L + dh)
    q = (torch.randn(n, d, generator=gen) * 1.2).bfloat16().to(DEV)
    kv = (torch.randn(M, 2 * d, generator=gen) * 1.2).bfloat16().to(DEV)
    do = torch.randn(n, d, generator=gen).bfloat16().to(DEV)
    lib = _lib.lib()
    scale = 1.0 / math.sqrt(dh)
    res = {}
    for sfx in ('', '_h16'):
        o = torch.zeros((n, d), dtype=q.dtype, device=DEV)
        lse2 = torch.zeros((n, H), dtype=torch.float32, device=DEV)
        dq = torch.zeros((n, d), dtype=q.dtype, device=DEV)
        out = torch.zeros((M, 2 * d), dtype=q.dtype, device=DEV)
        assert getattr(lib, 'svol_attn_cls_fwd' + sfx)(_ptr(q), d, _ptr(kv), 2 * d, _ptr(kv[:, d:]), 2 * d, _ptr(o), d, _ptr(lse2), n, H, L, dh,
                                                       scale, _dt(q), _stream()) == 0
        assert getattr(lib, 'svol_attn_cls_bwd' + sfx)(_ptr(q), d, _ptr(kv), 2 * d, _ptr(kv[:, d:]), 2 * d, _ptr(o), d, _ptr(do), d, _ptr(lse2),
                                                       _ptr(dq), d, _ptr(out), 2 * d, _ptr(out[:, d:]), 2 * d, n, H, L, dh, scale, _dt(q),
                                                       _stream()) == 0
        torch.cuda.synchronize()
        res[sfx] = (o, lse2, dq, out)
    for tag, a, b in zip(('o', 'lse2', 'dq', 'dk | dv'), res[''], res['_h16']):
        assert torch.equal(a, b), tag
    assert bool(res[''][3].float().abs().sum() > 0)
