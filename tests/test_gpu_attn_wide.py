"""The generic attention template of csrc/attention.hip through ops.attn_fwd / ops.attn_bwd, i.e. svol_attn_fwd_dropout /
svol_attn_bwd_dropout: head widths 32 < dh <= 64 (two d-tiles, f32 / bf16 / fp16) and, in fp32, dh <= 32 (one d-tile).

Inputs, reference and bars are those of tests/gpu_checks.py::check_attention: _rnd with seeds 30-33 (q and k scaled by 1.5), fp64 by
autograd, whole-tensor rel_err at TOL[dtype] for o, 2 TOL[dtype] for dq / dk / dv, 1e-5 (fp32) / 3e-3 (16-bit) for lse2; each case with
plain q and with q pre-multiplied by log2(e) / sqrt(dh) (reference: the unscaled q the kernel effectively sees).  Dropout: the fp64
reference of tests/attn_dropout_ref.py under the numpy twin's keep mask, same bars.

Each case is the smallest shape that reaches a distinct way to go wrong (B, H, Lq, Lk, dh, masked):
  (2,4,70,150,64,T)   ragged query and key tiles, a mask          (1,2,129,64,64,F)   a second query tile holding one row, exactly one key tile
  (2,2,7,333,64,T)    few queries, many key tiles                 (1,4,200,256,64,F)  full key tiles
  (1,2,100,128,48,F)  zero-padded second d-tile                   (2,3,33,97,40,T)    zero-padded second d-tile, masked
  (1,1,1,1,64,F)      degenerate 1 x 1
NARROW holds the one-tile instance <float, 1> to the same assertions and bars, fp32 only (16-bit operands at dh <= 32 take
csrc/attention_bf16.hip): widths below one tile (8, 24), a ragged last query block, a ragged last key tile, dead keys and 1 x 1 — where a
wrong chunk map or store guard in the template's traits would show.
The 16-bit rounding model (attn_dropout_ref.emulate with rounder(dtype) against ::reference) stays within 0.42 of its bar at every one
of them, both premuls, without dropout and with dropout 0.1 / 0.25 under the twin's mask (worst: bf16 o of the 7 x 333 case).  Measured
on the device: 0.43 of the bar at the worst (the same tensor), fp32 below 0.06 (profiles/attn_wide.md).

The 1 x 1 case's dq and dk have an identically zero reference (one key: P = 1, dS = 0), where rel_err has nothing to divide by; they
are held, at the same 2 TOL, against the size of the term that cancels (_cancel_scales).
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from tests import attn_dropout_ref as R
from tests.dropout_twin import dropout_keep_numpy

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [FP32, BF16, FP16]
LSE_BAR = {FP32: 1e-5, BF16: 3e-3, FP16: 3e-3}
CASES = [(2, 4, 70, 150, 64, True), (1, 2, 129, 64, 64, False), (2, 2, 7, 333, 64, True), (1, 4, 200, 256, 64, False),
         (1, 2, 100, 128, 48, False), (2, 3, 33, 97, 40, True), (1, 1, 1, 1, 64, False)]
DROP_CASES = CASES[:-1]   # (the 1 x 1 case's reference gradients vanish)
# one d-tile, fp32 only (16-bit operands at dh <= 32 take csrc/attention_bf16.hip, which has other bars and uses atomics)
NARROW = [(2, 4, 70, 150, 32, True), (1, 2, 129, 64, 24, False), (2, 3, 33, 97, 8, True), (1, 1, 1, 1, 16, False)]
POINTS = [(c, d) for c in CASES for d in DTYPES] + [(c, FP32) for c in NARROW]
DROP_POINTS = [(c, d) for c in DROP_CASES for d in DTYPES] + [(c, FP32) for c in NARROW[:-1]]
ZONE_POINTS = [(c, d) for c in (CASES[0], CASES[5]) for d in DTYPES] + [(NARROW[1], FP32)]
DROP_SEED = (7 << 44) + (3 << 12) + 1   # the model's form (base << 44) + (step << 12) + site
NEG0 = -2147483648   # 0x80000000 as int32: fp32 -0.0 (tests/test_gpu_guards.py)
SVOL_E_UNSUPPORTED = -2   # include/svol_hip.h
_cid = lambda c: 'B{}H{}q{}k{}d{}{}'.format(*c[:5], 'm' if c[5] else '')
_did = lambda d: R.DT_NAME[d]
_pids = lambda points: [f'{_cid(c)}-{_did(d)}' for c, d in points]


def _kbias(case):
    B, H, Lq, Lk, dh, masked = case
    if not masked:
        return None
    kb = torch.zeros(B, Lk)
    kb[:, Lk - Lk // 4:] = float('-inf')
    kb[0, 3] = float('-inf')
    return kb


@functools.lru_cache(maxsize=None)
def point(case, dtype, premul_on, p):
    """inputs and the fp64 reference of one parity point, computed once and shared (never modified).  p = 0: check_attention's reference
    (_attn_ref + autograd); p > 0: attn_dropout_ref.reference under the twin's mask."""
    from tests.gpu_checks import _attn_ref, _rnd
    B, H, Lq, Lk, dh, masked = case
    d = H * dh
    q, k, v = _rnd((B * Lq, d), dtype, 30, 1.5), _rnd((B * Lk, d), dtype, 31, 1.5), _rnd((B * Lk, d), dtype, 32)
    do = _rnd((B * Lq, d), dtype, 33)
    kb = _kbias(case)
    pm = 1.4426950408889634 / math.sqrt(dh) if premul_on else 0.0
    if premul_on:
        q = (q.double() * pm).to(dtype)
        qref = q.double() / pm   # the unscaled q the kernel effectively sees
    else:
        qref = q.double()
    if p == 0.0:
        q64, k64, v64 = qref.clone().requires_grad_(True), k.double().requires_grad_(True), v.double().requires_grad_(True)
        o_ref, lse_ref = _attn_ref(q64, k64, v64, B, H, Lq, Lk, dh, kb)
        (o_ref * do.double()).sum().backward()
        ref = (o_ref.detach(), lse_ref.detach(), q64.grad, k64.grad, v64.grad)
    else:
        keep = torch.from_numpy(dropout_keep_numpy((B, H, Lq, Lk), p, DROP_SEED))
        ref = R.reference(qref, k, v, do, kb, keep, p, (B, H, Lq, Lk, dh))
    return dict(q=q, k=k, v=v, do=do, kb=kb, pm=pm, ref=ref, cancel=_cancel_scales(qref, k, v, do, kb, ref, (B, H, Lq, Lk, dh)))


def _cancel_scales(qref, k, v, do, kb, ref, dims):
    """{tag: scale} for the gradients whose reference is IDENTICALLY zero (one valid key: P = 1 and dS = P (dP - delta) = 0, the 1 x 1
    case's dq and dk).  rel_err divides by max|ref|, which is 0 there, and the device's dP (an MFMA sum over d) and delta (a sum over d
    of dO O in another order) agree to fp32 rounding, not bit for bit.  Such a tensor is held, at the same bar, against the size of the
    term that cancels: dq = scale (P dP) k - scale (P delta) k, scale = max|scale (P dP) k| in fp64 (dk: with q for k)."""
    B, H, Lq, Lk, dh = dims
    out = {}
    if float(ref[2].abs().max()) != 0.0 and float(ref[3].abs().max()) != 0.0:
        return out
    q4, k4, v4, do4 = (R._heads(t.double(), B, L, H, dh) for t, L in ((qref, Lq), (k, Lk), (v, Lk), (do, Lq)))
    s = q4 @ k4.transpose(-1, -2) / math.sqrt(dh)
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    PdP = torch.softmax(s, -1) * (do4 @ v4.transpose(-1, -2)) / math.sqrt(dh)
    if float(ref[2].abs().max()) == 0.0:
        out['dq'] = float((PdP @ k4).abs().max())
    if float(ref[3].abs().max()) == 0.0:
        out['dk'] = float((PdP.transpose(-1, -2) @ q4).abs().max())
    return out


def launch(case, c, p=0.0, drop_entry=None):
    """forward + backward on the device -> o, lse2, dq, dk, dv.  drop_entry: go through drop=(p, seed) even at p = 0"""
    from svol_amd import ops
    B, H, Lq, Lk, dh, _ = case
    qd, kd, vd, dod = (c[n].to(DEV) for n in ('q', 'k', 'v', 'do'))
    kbd = None if c['kb'] is None else c['kb'].to(DEV)
    drop = (p, DROP_SEED) if (p > 0.0 or drop_entry) else None
    o, lse2 = ops.attn_fwd(qd, kd, vd, B, H, Lq, Lk, dh, kbd, c['pm'], drop=drop)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    ops.attn_bwd(qd, kd, vd, o, dod, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbd, c['pm'], drop=drop)
    torch.cuda.synchronize()
    return o, lse2, dq, dk, dv


def hold(case, dtype, c, got, what):
    """check_attention's whole-tensor bars; masked keys' gradient rows exactly 0; everything finite"""
    from tests.gpu_checks import TOL, rel_err
    B, H, Lq, Lk, dh, _ = case
    bars = (TOL[dtype], LSE_BAR[dtype], 2 * TOL[dtype], 2 * TOL[dtype], 2 * TOL[dtype])
    bad = []
    for tag, g, r, bar in zip(('o', 'lse2', 'dq', 'dk', 'dv'), got, c['ref'], bars):
        assert bool(torch.isfinite(g.float()).all()), f'{what}: {tag} is not finite'
        e = rel_err(g, r.reshape(g.shape))
        if tag in c['cancel']:   # an identically zero reference: against the term that cancels (_cancel_scales)
            e = float(g.double().abs().max()) / c['cancel'][tag]
        print(f'{what} {tag}: {e:.3e} (<= {bar:.3e}){"" if e <= bar else "   <-- FAILS"}')
        if not e <= bar:
            bad.append(f'{tag}: {e:.3e} vs {bar:.3e}')
    if c['kb'] is not None:
        gone = (c['kb'] != 0).reshape(B * Lk).to(DEV)
        for tag, g in (('dk', got[3]), ('dv', got[4])):
            z = float(g[gone].double().abs().max())
            print(f'{what} masked keys {tag}: {z:.3e} (== 0)')
            if z != 0.0:
                bad.append(f'masked keys {tag}: {z:.3e}')
    assert not bad, f'{what}: ' + '; '.join(bad)


@pytest.mark.parametrize('premul_on', [False, True], ids=['plain', 'premul'])
@pytest.mark.parametrize('case,dtype', POINTS, ids=_pids(POINTS))
def test_forward_and_backward_against_fp64(case, dtype, premul_on):
    c = point(case, dtype, premul_on, 0.0)
    a = launch(case, c)
    hold(case, dtype, c, a, f'{_cid(case)} {_did(dtype)} premul={premul_on}')
    # no atomics, no workspace: a second run gives the same bits; the dropout entries at p = 0 are the plain entries
    b = launch(case, c)
    z = launch(case, c, 0.0, drop_entry=True)
    for tag, x, y, w in zip(('o', 'lse2', 'dq', 'dk', 'dv'), a, b, z):
        assert torch.equal(x, y), f'{tag}: two runs differ'
        assert torch.equal(x, w), f'{tag}: the dropout entry at p = 0 differs from the plain entry'


@pytest.mark.parametrize('p', [0.1, 0.25], ids=lambda p: f'p{p}')
@pytest.mark.parametrize('premul_on', [False, True], ids=['plain', 'premul'])
@pytest.mark.parametrize('case,dtype', DROP_POINTS, ids=_pids(DROP_POINTS))
def test_dropout_against_fp64_under_the_twins_mask(case, dtype, premul_on, p):
    c = point(case, dtype, premul_on, p)
    a = launch(case, c, p)
    hold(case, dtype, c, a, f'{_cid(case)} {_did(dtype)} premul={premul_on} p={p}')
    b = launch(case, c, p)
    for tag, x, y in zip(('o', 'lse2', 'dq', 'dk', 'dv'), a, b):
        assert torch.equal(x, y), f'{tag}: two runs differ'


@pytest.mark.parametrize('dtype', DTYPES, ids=_did)
def test_column_slices_of_a_packed_buffer(dtype):
    """self-attention over a packed [B L, 3 d] buffer, q / k / v as column slices; dq / dk / dv into the slices of a packed gradient"""
    from svol_amd import ops
    from tests.gpu_checks import TOL, _attn_ref, _rnd, rel_err
    B, H, L, dh = 2, 2, 96, 64
    d = H * dh
    qkv = _rnd((B * L, 3 * d), dtype, 34)
    do = _rnd((B * L, d), dtype, 33)
    qkvd = qkv.to(DEV)
    o, lse2 = ops.attn_fwd(qkvd[:, :d], qkvd[:, d:2 * d], qkvd[:, 2 * d:], B, H, L, L, dh)
    dqkv = torch.empty_like(qkvd)
    ops.attn_bwd(qkvd[:, :d], qkvd[:, d:2 * d], qkvd[:, 2 * d:], o, do.to(DEV), lse2, B, H, L, L, dh, dqkv[:, :d], dqkv[:, d:2 * d],
                 dqkv[:, 2 * d:])
    torch.cuda.synchronize()
    x64 = qkv.double().requires_grad_(True)
    o_ref, lse_ref = _attn_ref(x64[:, :d], x64[:, d:2 * d], x64[:, 2 * d:], B, H, L, L, dh, None)
    (o_ref * do.double()).sum().backward()
    fig = {'o': (rel_err(o, o_ref), TOL[dtype]), 'lse2': (rel_err(lse2, lse_ref), LSE_BAR[dtype])}
    for j, tag in enumerate(('dq', 'dk', 'dv')):
        fig[tag] = (rel_err(dqkv[:, j * d:(j + 1) * d], x64.grad[:, j * d:(j + 1) * d]), 2 * TOL[dtype])
    for tag, (e, bar) in fig.items():
        print(f'packed {_did(dtype)} {tag}: {e:.3e} (<= {bar:.3e})')
    assert all(e <= bar for e, bar in fig.values()), fig


class RedZone:
    """an interior block [rows, cols] of a larger buffer filled with fp32 -0.0 words: sentinel rows above and below, sentinel columns
    left and right (ld > cols)"""

    def __init__(self, rows, cols, dtype, pad_rows=9, pad_cols=8):
        esz = torch.empty((), dtype=dtype).element_size()
        self.pad_rows, self.pad_cols, self.ld = pad_rows, pad_cols, cols + 3 * pad_cols
        assert self.ld * esz % 4 == 0
        self.words = torch.full(((rows + 2 * pad_rows) * self.ld * esz // 4,), NEG0, dtype=torch.int32, device=DEV)
        self.full = self.words.view(dtype).view(rows + 2 * pad_rows, self.ld)
        self.view = self.full[pad_rows:pad_rows + rows, pad_cols:pad_cols + cols]

    def check(self, what):
        assert bool(torch.isfinite(self.view.float()).all()), f'{what}: not (fully) written'
        n = self.changed(self.view.shape[1])
        assert n == 0, f'{what}: {n} sentinel words changed'

    def changed(self, cols):
        """sentinel words that changed outside the first `cols` columns of the block's rows"""
        per = 4 // self.full.element_size()   # elements per 32-bit word
        rest = self.words.clone().view(self.full.shape[0], self.ld // per)
        rest[self.pad_rows:self.pad_rows + self.view.shape[0], self.pad_cols // per:(self.pad_cols + cols) // per] = NEG0
        return int((rest != NEG0).sum())


@pytest.mark.parametrize('case,dtype', ZONE_POINTS, ids=_pids(ZONE_POINTS))
def test_outputs_stay_inside_their_buffers(case, dtype):
    """o, dq, dk, dv as interior row / column ranges of sentinel-filled buffers (ld > H dh), lse2 and delta as interior ranges too"""
    from svol_amd import _lib, ops
    B, H, Lq, Lk, dh, _ = case
    d = H * dh
    c = point(case, dtype, True, 0.0)
    q, k, v, do = (c[n].to(DEV) for n in ('q', 'k', 'v', 'do'))
    kb = None if c['kb'] is None else c['kb'].to(DEV)
    zo, zq, zk, zv = RedZone(B * Lq, d, dtype), RedZone(B * Lq, d, dtype), RedZone(B * Lk, d, dtype), RedZone(B * Lk, d, dtype)
    zl, zd = RedZone(1, B * H * Lq, FP32, pad_cols=64), RedZone(1, 3 * B * H * Lq, FP32, pad_cols=64)
    lse2, delta = zl.view[0], zd.view[0]
    lib, P = _lib.lib(), ops._ptr
    sc = 1.0 / math.sqrt(dh)
    for p, seed in ((0.0, 0), (0.1, DROP_SEED)):
        _lib.check(lib.svol_attn_fwd_dropout(P(q), q.stride(0), P(k), k.stride(0), P(v), v.stride(0), P(zo.view), zo.ld, P(lse2), P(kb), B, H,
                                             Lq, Lk, dh, sc, c['pm'], None, 0, p, seed, ops._dt(q), ops._stream()), 'svol_attn_fwd_dropout')
        _lib.check(lib.svol_attn_bwd_dropout(P(q), q.stride(0), P(k), k.stride(0), P(v), v.stride(0), P(zo.view), zo.ld, P(do), do.stride(0),
                                             P(lse2), P(delta), P(kb), P(zq.view), zq.ld, P(zk.view), zk.ld, P(zv.view), zv.ld, B, H, Lq, Lk,
                                             dh, sc, c['pm'], None, 0, p, seed, ops._dt(q), ops._stream()), 'svol_attn_bwd_dropout')
        torch.cuda.synchronize()
        for tag, z in (('o', zo), ('dq', zq), ('dk', zk), ('dv', zv), ('lse2', zl)):
            z.check(f'{_cid(case)} {_did(dtype)} p={p} {tag}')
        # delta: the first B H Lq floats of the caller's 3 B H Lq, the rest of it and its surroundings untouched
        assert zd.changed(B * H * Lq) == 0, 'delta: written past its first B H Lq floats'


def test_return_codes_and_scratch_queries():
    from svol_amd import _lib, ops
    lib, P = _lib.lib(), ops._ptr
    assert lib.svol_abi_version() == 7
    assert int(lib.svol_attn_ws_bytes(2, 4, 70, 150, 64)) == 0
    for dtype in DTYPES:
        assert int(lib.svol_attn_bwd_sp_image_bytes(2, 4, 1536, 1536, 64, 1 << 30, ops._DT[dtype])) == 0
        for dh, want in ((72, SVOL_E_UNSUPPORTED), (128, SVOL_E_UNSUPPORTED), (36, SVOL_E_UNSUPPORTED), (64, 0), (40, 0)):
            B, H, L = 1, 2, 16
            d = H * dh
            q = torch.zeros((B * L, d), dtype=dtype, device=DEV)
            o = torch.full_like(q, 7.0)
            lse2 = torch.zeros((B, H, L), dtype=torch.float32, device=DEV)
            rc = lib.svol_attn_fwd(P(q), d, P(q), d, P(q), d, P(o), d, P(lse2), None, B, H, L, L, dh, 1.0 / math.sqrt(dh), 0.0, None, 0,
                                   ops._DT[dtype], ops._stream())
            assert rc == want, (dh, dtype, rc)
            dq, dk, dv = (torch.full_like(q, 7.0) for _ in range(3))
            delta = torch.zeros((3, B, H, L), dtype=torch.float32, device=DEV)
            rc = lib.svol_attn_bwd(P(q), d, P(q), d, P(q), d, P(o), d, P(q), d, P(lse2), P(delta), None, P(dq), d, P(dk), d, P(dv), d, B, H,
                                   L, L, dh, 1.0 / math.sqrt(dh), 0.0, None, 0, ops._DT[dtype], ops._stream())
            assert rc == want, (dh, dtype, rc)
            torch.cuda.synchronize()
            if want:   # a refused call writes nothing
                assert all(bool((t == 7.0).all()) for t in (o, dq, dk, dv))
        ws = torch.zeros((64,), dtype=torch.float32, device=DEV)
        assert lib.svol_attn_bwd_zero_ws(P(ws), 256, 1, 2, 16, 16, 64, ops._DT[dtype], ops._stream()) == SVOL_E_UNSUPPORTED
