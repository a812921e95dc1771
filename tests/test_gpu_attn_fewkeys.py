"""The many-queries / few-keys attention kernels of csrc/attn_fewkeys.hip on the device (tests/attn_fewkeys_cases.py: the points, the
planted families, the masks, the canary rows, the figures), against fp64, in bf16 and fp16.

  a. parity: every point through ops.attn_fewkeys_fwd and ops.attn_fewkeys_bwd, k / v as column slices of a packed [B Lk + 32, 2 d]
     buffer of which the kernels see the first B Lk rows, q / dout the first B Lq rows of [B Lq + 32, d]; the rows behind are canaries
     (keys that would win, NaN values) and the K / V rows of masked keys are NaN.  Figures: slice errors of o / dq per (batch, head) and
     of dk / dv per (batch, head, 64-key block) <= the derived bar; element errors on the same slices against the slice's largest
     reference entry (gpu_checks.TOL[dtype] for o, twice that for the gradients); lse2 within 2e-5 max(1, max |ref|); every value
     finite; dk / dv rows of masked keys exactly 0.
  b. every point's forward and backward twice: bit-identical (no atomics, the chunk partials are added in chunk order).
  c. through the C ABI with o / dq / dk / dv as column slices of sentinel-filled buffers with sentinel rows behind them and lse2 a prefix
     of a longer sentinel-filled vector: the results are those of (a) and the sentinels are intact.
  d. the entry points' return codes for what they refuse; nothing is launched, sentinel-filled outputs stay untouched.
  e. at three points svol_attn_fwd / svol_attn_bwd on the same operands (their masked keys' rows zeroed: that family does not promise to
     ignore them) meet the same bars against fp64: the two families are interchangeable, each held to fp64 and not to the other's bits.

Slice bar (BARS): 3 x the worst slice error, over every point, of attn_fewkeys_cases.emulation (fp64 arithmetic with P, dS, o, dq, dk, dv
rounded to the operand type); tests/test_attn_fewkeys_cases.py re-derives it and holds EMULATED to it.  The factor covers accumulation
order and the hardware exp2 / log2, and is the project's (tests/test_gpu_attn_cls.py, tests/test_gpu_attn_small.py).

    type   emulation (worst point)                                         bar       device's worst slice
    bf16   4.49e-3   B2 H1 Lq256 Lk197 dh64 first edges (dk rows 192:197)    1.35e-2   4.487e-3 (the same point)
    fp16   5.72e-4   B2 H3 Lq257 Lk197 dh32 first one_live (dk rows 192:197) 1.72e-3   5.723e-4 (the same point)

The device's worst slice errors equal the emulation's to three digits; the other points stand at 1.9e-3 .. 3.8e-3 (bf16) and
1.7e-4 .. 4.7e-4 (fp16).  All 169 tests passed on the first device run; every point's two runs were bit-identical.
"""
from __future__ import annotations

import functools
import math
import os
import re

import pytest
import torch

from tests import attn_fewkeys_cases as A

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# worst slice error of the emulation per operand type and where
EMULATED = {A.BF16: (4.49e-3, (2, 1, 256, 197, 64, 'first', 'edges', False)),
            A.FP16: (5.72e-4, (2, 3, 257, 197, 32, 'first', 'one_live', False))}
BARS = {dt: 3.0 * e for dt, (e, _) in EMULATED.items()}
POINTS = [p + (dt,) for dt in A.DTYPES for p in A.points()]
IDS = [A.point_id(*p[:-1]) + ('-bf16' if p[-1] == A.BF16 else '-fp16') for p in POINTS]
SENTINEL = 7.0


def _operands(c):
    """-> (q [B Lq + 32, d], the packed k | v buffer [B Lk + 32, 2 d], dout [B Lq + 32, d], kbias or None) on the device"""
    kb = c['kbias'].to(DEV) if c['kbias'] is not None else None
    return c['q'].to(DEV), torch.cat([c['k'], c['v']], 1).to(DEV), c['do'].to(DEV), kb


def run(c, generic=False):
    """forward and backward of one case -> (o, lse2, dq, dk, dv) on the device; generic: through ops.attn_fwd / attn_bwd"""
    from svol_amd import ops
    B, H, Lq, Lk, dh = c['dims']
    d, Mq, Mk = H * dh, B * Lq, B * Lk
    q, kv, do, kb = _operands(c)
    if generic:
        kv = torch.nan_to_num(kv, nan=0.0)
    g = kv[:Mk]
    dq = torch.empty((Mq, d), dtype=c['dtype'], device=DEV)
    out = torch.empty((Mk, 2 * d), dtype=c['dtype'], device=DEV)
    fwd, bwd = (ops.attn_fwd, ops.attn_bwd) if generic else (ops.attn_fewkeys_fwd, ops.attn_fewkeys_bwd)
    o, lse2 = fwd(q[:Mq], g[:, :d], g[:, d:], B, H, Lq, Lk, dh, kb, c['premul'])
    bwd(q[:Mq], g[:, :d], g[:, d:], o, do[:Mq], lse2, B, H, Lq, Lk, dh, dq, out[:, :d], out[:, d:], kb, c['premul'])
    torch.cuda.synchronize()
    return o, lse2, dq, out[:, :d], out[:, d:]


@functools.lru_cache(maxsize=None)
def first_run(*p):
    """one point's device result, computed once and shared (never modified)"""
    return run(A.make_case(*p))


def check(fig, what):
    bad = []
    for label, (val, bar) in fig.items():
        ok = val <= bar
        print(f'{what} {label}: {val:.3e} (<= {bar:.3e}){"" if ok else "   <-- FAILS"}')
        if not ok:
            bad.append(f'{label}: {val:.3e} vs {bar:.3e}')
    assert not bad, f'{what}: ' + '; '.join(bad)


def test_bars_and_chunk_rule_are_the_projects():
    from svol_amd import ops
    from tests import gpu_checks as G
    for dt in A.DTYPES:
        assert A.TOL[dt] == G.TOL[dt]
    for Lq in (1, 255, 256, 257, 2048, 2049, 6272, 100000):
        assert ops.attn_fewkeys_chunk(Lq) == A.chunk_rows(Lq)


@pytest.mark.parametrize('p', POINTS, ids=IDS)
def test_parity_with_fp64_by_slice(p):
    c = A.make_case(*p)
    fig = A.figures(c, first_run(*p), A.reference(*p), BARS[p[-1]])
    print(f'{A.point_id(*p[:-1])} {p[-1]} worst slice {A.worst_slice(fig):.3e}')
    check(fig, A.point_id(*p[:-1]))


@pytest.mark.parametrize('p', POINTS, ids=IDS)
def test_forward_and_backward_are_bit_reproducible(p):
    again = run(A.make_case(*p))
    for tag, a, b in zip(('o', 'lse2', 'dq', 'dk', 'dv'), first_run(*p), again):
        assert torch.equal(a, b), tag


ABI_POINTS = [(2, 3, 257, 49, 32, 'normal', 'edges', True, A.BF16), (1, 1, 2049, 49, 32, 'normal', 'none', False, A.FP16),
              (1, 3, 160, 197, 64, 'normal', 'none', True, A.BF16), (2, 1, 2049, 33, 64, 'normal', 'edges', True, A.FP16)]


@pytest.mark.parametrize('p', ABI_POINTS, ids=lambda p: A.point_id(*p[:-1]))
def test_nothing_is_written_outside_the_outputs(p):
    from svol_amd import _lib, ops
    from svol_amd.ops import _dt, _ptr, _stream
    c = A.make_case(*p)
    B, H, Lq, Lk, dh = c['dims']
    d, Mq, Mk, pad = H * dh, B * Lq, B * Lk, 8
    q, kv, do, kb = _operands(c)
    g = kv[:Mk]
    wide = 2 * (d + pad) + pad
    small = torch.full((Mq + 5, wide), SENTINEL, dtype=c['dtype'], device=DEV)     # | pad | o | pad | dq | pad |
    o, dq = small[:Mq, pad:pad + d], small[:Mq, 2 * pad + d:2 * pad + 2 * d]
    big = torch.full((Mk + 5, wide), SENTINEL, dtype=c['dtype'], device=DEV)       # | pad | dk | pad | dv | pad |
    dk, dv = big[:Mk, pad:pad + d], big[:Mk, 2 * pad + d:2 * pad + 2 * d]
    lse_buf = torch.full((B * H * Lq + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    nws = ops.attn_fewkeys_ws_bytes(B, H, Lq, Lk, dh)
    ws = torch.full((nws // 4 + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    scale = 1.0 / math.sqrt(dh)
    lib = _lib.lib()
    rc = lib.svol_attn_fewkeys_fwd(_ptr(q), d, _ptr(g[:, :d]), 2 * d, _ptr(g[:, d:]), 2 * d, _ptr(o), o.stride(0), _ptr(lse_buf), _ptr(kb),
                                   B, H, Lq, Lk, dh, scale, c['premul'], _dt(q), _stream())
    assert rc == 0
    rc = lib.svol_attn_fewkeys_bwd(_ptr(q), d, _ptr(g[:, :d]), 2 * d, _ptr(g[:, d:]), 2 * d, _ptr(o), o.stride(0), _ptr(do), d, _ptr(lse_buf),
                                   _ptr(kb), _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), B, H, Lq, Lk, dh, scale,
                                   c['premul'], _ptr(ws), nws, _dt(q), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    o_r, lse_r, dq_r, dk_r, dv_r = first_run(*p)
    for tag, a, b in (('o', o, o_r), ('dq', dq, dq_r), ('dk', dk, dk_r), ('dv', dv, dv_r), ('lse2', lse_buf[:B * H * Lq], lse_r.reshape(-1))):
        assert torch.equal(a, b), tag
    for buf, rows in ((small, Mq), (big, Mk)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:rows, pad:pad + d] = False
        mask[:rows, 2 * pad + d:2 * pad + 2 * d] = False
        assert bool((buf[mask] == SENTINEL).all()), 'a kernel wrote outside its output slices'
    assert bool((lse_buf[B * H * Lq:] == SENTINEL).all()), 'the forward wrote behind lse2'
    assert bool((ws[nws // 4:] == SENTINEL).all()), 'the backward wrote behind its scratch'


def _codes():
    """the SVOL_* constants of include/svol_hip.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'svol_hip.h')
    with open(path) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(SVOL_\w+)\s+\(?(-?\d+)\)?', f.read())}


def test_entry_points_refuse_without_launching():
    from svol_amd import _lib, ops
    from svol_amd.ops import _ptr, _stream
    K = _codes()
    B, H, Lq, Lk, dh = 2, 3, 40, 33, 32
    d, Mq, Mk = H * dh, B * Lq, B * Lk
    q = torch.zeros((Mq, d + 8), dtype=A.BF16, device=DEV)
    kv = torch.zeros((8 * Mk, 2 * d), dtype=A.BF16, device=DEV)
    do = torch.zeros((Mq, d), dtype=A.BF16, device=DEV)
    o = torch.full((Mq, d), SENTINEL, dtype=A.BF16, device=DEV)
    lse2 = torch.full((B, H, Lq), SENTINEL, dtype=torch.float32, device=DEV)
    dq = torch.full((Mq, d), SENTINEL, dtype=A.BF16, device=DEV)
    grads = torch.full((8 * Mk, 2 * d), SENTINEL, dtype=A.BF16, device=DEV)
    nws = ops.attn_fewkeys_ws_bytes(B, H, Lq, Lk, dh)
    assert nws == B * H * 1 * 2 * 64 * dh * 4
    assert ops.attn_fewkeys_ws_bytes(B, H, Lq, 257, dh) == 0 and ops.attn_fewkeys_ws_bytes(B, H, Lq, Lk, 40) == 0
    ws = torch.full((nws // 4,), SENTINEL, dtype=torch.float32, device=DEV)
    lib = _lib.lib()

    def call(entry, Lk=Lk, dh=dh, dtype=K['SVOL_BF16'], ldq=d + 8, ldk=2 * d, q_off=0, dk_off=0, lse=True, k=True, ws_bytes=nws, wsp=True):
        qp, kp, vp = _ptr(q) + q_off, (_ptr(kv) if k else None), _ptr(kv[:, d:])
        scale, lp = 1.0 / math.sqrt(dh), (_ptr(lse2) if lse else None)
        if entry == 'fwd':
            return lib.svol_attn_fewkeys_fwd(qp, ldq, kp, ldk, vp, 2 * d, _ptr(o), d, lp, None, B, H, Lq, Lk, dh, scale, 0.0, dtype, _stream())
        return lib.svol_attn_fewkeys_bwd(qp, ldq, kp, ldk, vp, 2 * d, _ptr(o), d, _ptr(do), d, lp, None, _ptr(dq), d, _ptr(grads) + dk_off, 2 * d,
                                         _ptr(grads[:, d:]), 2 * d, B, H, Lq, Lk, dh, scale, 0.0, (_ptr(ws) if wsp else None), ws_bytes,
                                         dtype, _stream())

    unsupported = [dict(dtype=K['SVOL_F32']), dict(dh=40), dict(dh=16), dict(Lk=0), dict(Lk=257), dict(ldq=d + 4), dict(ldk=2 * d + 4),
                   dict(q_off=2), dict(q_off=8)]
    for entry in ('fwd', 'bwd'):
        for kw in unsupported:
            assert call(entry, **kw) == K['SVOL_E_UNSUPPORTED'], (entry, kw)
        for kw in (dict(lse=False), dict(k=False)):
            assert call(entry, **kw) == K['SVOL_E_INVALID'], (entry, kw)
    assert call('bwd', dk_off=4) == K['SVOL_E_UNSUPPORTED']
    for kw in (dict(ws_bytes=nws - 4), dict(ws_bytes=0), dict(wsp=False)):     # an undersized or missing scratch
        assert call('bwd', **kw) == K['SVOL_E_INVALID'], kw
    torch.cuda.synchronize()
    for t in (o, lse2, dq, grads, ws):
        assert bool((t == SENTINEL).all())


GENERIC_POINTS = [(2, 3, 257, 49, 32, 'normal', 'edges', True, A.BF16), (1, 3, 160, 197, 64, 'normal', 'none', True, A.FP16),
                  (1, 1, 2049, 49, 32, 'normal', 'none', False, A.BF16)]


@pytest.mark.parametrize('p', GENERIC_POINTS, ids=lambda p: A.point_id(*p[:-1]))
def test_generic_kernels_meet_the_same_bars(p):
    c = A.make_case(*p)
    for name, got in (('fewkeys', first_run(*p)), ('generic', run(c, generic=True))):
        check(A.figures(c, got, A.reference(*p), BARS[p[-1]]), f'{name} {A.point_id(*p[:-1])}')
