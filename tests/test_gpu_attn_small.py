"""The short-sequence (ViT) attention kernels of csrc/vit.hip on the device at every length where a loop bound changes, at benign and
at planted inputs (tests/attn_small_cases.py: the cases, the layouts, the canary rows, the figures), against fp64.

  a. parity: every (L, dh, family) point through ops.attn_small_fwd(want_lse=True) and ops.attn_small_bwd, q / k / v as column slices
     of a packed [n L + 32, 3 d] buffer (the kernels see its first n L rows; the 32 behind them are the canary rows), gradients into a
     packed buffer.  Figures: slice errors on (image, head, 32-row block) slices; element errors per (image, head) separately over
     planted and other rows (o, dq) / keys (dk, dv) against the largest reference entry of the (image, head); lse2 over each row set;
     every value finite; L = 1: dq = dk = 0 and dv = dO exactly; 'deep' heads (lse2 <= -128: the padded key lanes of the backward's
     key-stationary phase hold inf): dk / dv of the real keys finite and within the element bar.
  b. the plain forward and the lse forward give the same o bits at every point.
  c. every point's forward and backward twice: bit-identical (neither kernel has atomics).
  d. the forward through the C ABI with o a column slice of a wider sentinel-filled buffer with sentinel rows behind n L, and lse2 a
     prefix of a longer sentinel-filled vector: the sentinels are intact (L = 33 and 225, both head widths).
  e. the three entry points' return codes for what they refuse; nothing is launched, sentinel-filled outputs stay untouched.

Slice bar (BARS): 3 x the worst slice error, over every point, of attn_dropout_ref.emulate (bf16 roundings at the kernels' rounding
sites) without bias or dropout; tests/test_attn_small_cases.py re-derives the worst point and holds EMULATED to it.  The factor covers
accumulation order and the hardware exp2 / log2, and is the project's existing one (tests/test_gpu_attn_range.py).

    emulation (worst point)                      bar       device's worst slice
    6.66e-3   L = 97, dh = 64, benign (dq)       2.00e-2   6.66e-3 (L = 97, dh = 64, benign, dq rows 96:97)

The device's slice errors equal the emulation's to three digits at every point.  Element bars are the project's: gpu_checks.TOL[bf16]
for o, twice that for the gradients; the device's worst element figure is 0.34 of its bar (dq of the benign rows of a 'deep' head,
L = 256, dh = 32), its worst 'deep' head figure 5.5e-3 (dv, L = 224, dh = 32) against 2.4e-2.  lse2: 2e-5 max(1, max |ref|), the bar
test_hand_placed_forward_at_small_tile_counts uses for an fp32 lse2; the device's worst is 2.4e-7 (planted rows, L = 128, dh = 32),
the fp32 evaluation of m c + log2 l on the host 5.3e-7 (tests/test_attn_small_cases.py).

Found on the device: at L = 1 dq and dk were not exactly 0 (max |dq| 2.1e-7 to 6.1e-7, max |dk| 1.9e-7 to 2.2e-5; dv = dO held).
dS = P (dP - delta) took dP = dO . v from the MFMA and delta = rowsum(dO * o) from an fma chain over 8-element chunks and a shuffle
tree; o = v bit for bit at L = 1, and the two sums of the same 32 / 64 products differed in the last fp32 bits (q0 = 256 of a planted
row multiplies that into dk).  attn_small_bwd_kernel now takes delta from the diagonal of dO O^T, formed by the same MFMA chain as
dP: the identities hold exactly, in both phases.
"""
from __future__ import annotations

import functools
import math
import os
import re

import pytest
import torch

from tests import attn_small_cases as A

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16 = A.BF16
# worst slice error of the emulation and where (L, dh, family)
EMULATED = (6.66e-3, (97, 64, 'benign'))
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
    g = qkv[:M]
    o, lse2 = ops.attn_small_fwd(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], n, H, L, dh, want_lse=lse)
    if not lse:
        torch.cuda.synchronize()
        return o
    o_buf = torch.zeros((M + A.CANARY_ROWS, d), dtype=BF16, device=DEV)
    o_buf[:M] = o
    lse_buf = torch.zeros(n * H * L + A.CANARY_ROWS, dtype=torch.float32, device=DEV)
    lse_buf[:n * H * L] = lse2.reshape(-1)
    out = torch.empty((M, 3 * d), dtype=BF16, device=DEV)
    ops.attn_small_bwd(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], o_buf[:M], do[:M], lse_buf[:n * H * L].view(n, H, L), n, H, L, dh,
                       out[:, :d], out[:, d:2 * d], out[:, 2 * d:])
    torch.cuda.synchronize()
    return o, lse2, out[:, :d], out[:, d:2 * d], out[:, 2 * d:]


@functools.lru_cache(maxsize=None)
def first_run(L, dh, family):
    """one point's device result, computed once and shared (never modified)"""
    return run(A.make_case(L, dh, family))


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
    assert A.TOL == G.TOL[BF16]


# ----------------------------------------------------------------------------------------------------------------------
# a. parity
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,dh,family', POINTS, ids=IDS)
def test_parity_with_fp64_by_32_row_slice(L, dh, family):
    c = A.make_case(L, dh, family)
    fig = A.figures(c, first_run(L, dh, family), A.reference(L, dh, family), BARS)
    print(f'{A.point_id(L, dh, family)} worst slice {A.worst_slice(fig):.3e}')
    check(fig, A.point_id(L, dh, family))


# ----------------------------------------------------------------------------------------------------------------------
# b. the two forwards agree
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,dh,family', POINTS, ids=IDS)
def test_plain_forward_gives_the_lse_forwards_bits(L, dh, family):
    o_plain = run(A.make_case(L, dh, family), lse=False)
    assert torch.equal(o_plain, first_run(L, dh, family)[0])


# ----------------------------------------------------------------------------------------------------------------------
# c. repeatability
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,dh,family', POINTS, ids=IDS)
def test_forward_and_backward_are_bit_reproducible(L, dh, family):
    again = run(A.make_case(L, dh, family))
    for tag, a, b in zip(('o', 'lse2', 'dq', 'dk', 'dv'), first_run(L, dh, family), again):
        assert torch.equal(a, b), tag


# ----------------------------------------------------------------------------------------------------------------------
# d. nothing else written
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_lse', [False, True], ids=['plain', 'lse'])
@pytest.mark.parametrize('L,dh', [(33, 32), (33, 64), (225, 32), (225, 64)])
def test_forward_writes_nothing_outside_its_output(L, dh, with_lse):
    from svol_amd import _lib
    from svol_amd.ops import _dt, _ptr, _stream
    c = A.make_case(L, dh, 'benign')
    n, H, _, _ = c['dims']
    d, M, pad = H * dh, n * L, 8
    qkv, _ = _packed(c)
    g = qkv[:M]
    buf = torch.full((M + 5, d + 2 * pad), SENTINEL, dtype=BF16, device=DEV)
    o = buf[:M, pad:pad + d]
    nl = n * H * L
    lse_buf = torch.full((nl + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    args = (_ptr(g[:, :d]), 3 * d, _ptr(g[:, d:2 * d]), 3 * d, _ptr(g[:, 2 * d:]), 3 * d, _ptr(o), o.stride(0))
    tail = (n, H, L, dh, 1.0 / math.sqrt(dh), _dt(g), _stream())
    if with_lse:
        rc = _lib.lib().svol_attn_small_fwd_lse(*args, _ptr(lse_buf), *tail)
    else:
        rc = _lib.lib().svol_attn_small_fwd(*args, *tail)
    torch.cuda.synchronize()
    assert rc == 0
    o_ref, lse_ref = first_run(L, dh, 'benign')[:2]
    assert torch.equal(o, o_ref)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:M, pad:pad + d] = False
    assert bool((buf[mask] == SENTINEL).all()), 'the forward wrote outside its o slice'
    if with_lse:
        assert torch.equal(lse_buf[:nl], lse_ref.reshape(-1))
        assert bool((lse_buf[nl:] == SENTINEL).all()), 'the forward wrote behind lse2'
    else:
        assert bool((lse_buf == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# e. refusals
# ----------------------------------------------------------------------------------------------------------------------
def _codes():
    """the SVOL_* constants of include/svol_hip.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'svol_hip.h')
    with open(path) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(SVOL_\w+)\s+\(?(-?\d+)\)?', f.read())}


def test_entry_points_refuse_without_launching():
    from svol_amd import _lib, ops
    from svol_amd.ops import _ptr, _stream
    K = _codes()
    assert (K['SVOL_F32'], K['SVOL_BF16'], K['SVOL_F16']) == tuple(ops._DT[t] for t in (torch.float32, BF16, torch.float16))
    n, H, L, dh = 2, 3, 33, 32
    d, M = H * dh, n * L
    qkv = torch.zeros((M, 3 * d), dtype=BF16, device=DEV)
    do = torch.zeros((M, d), dtype=BF16, device=DEV)
    o = torch.full((M, d), SENTINEL, dtype=BF16, device=DEV)
    lse2 = torch.full((n, H, L), SENTINEL, dtype=torch.float32, device=DEV)
    grads = torch.full((M, 3 * d), SENTINEL, dtype=BF16, device=DEV)
    lib = _lib.lib()

    def call(entry, n=n, L=L, dh=dh, dtype=K['SVOL_BF16'], ldq=3 * d, q_off=0, lse=True):
        q, k, v = _ptr(qkv) + q_off, _ptr(qkv[:, d:2 * d]), _ptr(qkv[:, 2 * d:])
        scale, lp = 1.0 / math.sqrt(dh), (_ptr(lse2) if lse else None)
        if entry == 'fwd':
            return lib.svol_attn_small_fwd(q, ldq, k, 3 * d, v, 3 * d, _ptr(o), d, n, H, L, dh, scale, dtype, _stream())
        if entry == 'fwd_lse':
            return lib.svol_attn_small_fwd_lse(q, ldq, k, 3 * d, v, 3 * d, _ptr(o), d, lp, n, H, L, dh, scale, dtype, _stream())
        return lib.svol_attn_small_bwd(q, ldq, k, 3 * d, v, 3 * d, _ptr(o), d, _ptr(do), d, lp, _ptr(grads), 3 * d,
                                       _ptr(grads[:, d:2 * d]), 3 * d, _ptr(grads[:, 2 * d:]), 3 * d, n, H, L, dh, scale, dtype,
                                       _stream())

    unsupported = [dict(L=257), dict(dh=16), dict(dh=128), dict(dtype=K['SVOL_F32']), dict(dtype=K['SVOL_F16']), dict(ldq=3 * d + 4),
                   dict(q_off=2), dict(n=65536)]
    for entry in ('fwd', 'fwd_lse', 'bwd'):
        for kw in unsupported:
            assert call(entry, **kw) == K['SVOL_E_UNSUPPORTED'], (entry, kw)
        assert call(entry, L=0) == K['SVOL_E_INVALID'], entry
    assert call('fwd_lse', lse=False) == K['SVOL_E_INVALID']
    assert call('bwd', lse=False) == K['SVOL_E_INVALID']
    torch.cuda.synchronize()
    for t in (o, lse2, grads):
        assert bool((t == SENTINEL).all())
