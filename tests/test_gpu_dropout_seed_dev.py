"""The device-side dropout step counter of the ``*_sd`` entry points (svol_dropout_sd, svol_dropout_add_sd, svol_attn_fwd_dropout_sd,
svol_attn_bwd_dropout_sd): the mask of (seed, counter k) IS the numpy twin's (tests/dropout_twin.py) at seed + (k << 12) -- never a
mask the device drew --, a NULL pointer or a counter of 0 is bit for bit the entry without the suffix, and neighbouring counters give
independent masks."""
from __future__ import annotations

import pytest
import torch

from tests import attn_dropout_ref as R
from tests.dropout_twin import dropout_keep_numpy

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
STRIDE = 12      # the counter enters as k << 12 (Transformer.forward's host stride)


def _counter(k):
    return torch.tensor([k], dtype=torch.int64, device=DEV)


# ----------------------------------------------------------------------------------------------------------------------
# svol_dropout_sd / svol_dropout_add_sd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [0, 1, 5])
@pytest.mark.parametrize('seed', R.SEEDS, ids=['seed_small', 'seed_model'])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('dtype', [FP32, BF16, FP16], ids=lambda d: R.DT_NAME[d])
def test_dropout_sd_is_the_twin_at_the_composed_seed(dtype, p, seed, k):
    from svol_amd import ops
    shape = (37, 100)
    want = torch.from_numpy(dropout_keep_numpy(shape, p, seed + (k << STRIDE))).float() / (1.0 - p)
    x = torch.ones(shape, dtype=dtype, device=DEV)
    y = ops.dropout(x, p, seed, seed_dev=_counter(k))
    assert torch.equal(y.cpu(), want.to(dtype)), 'svol_dropout_sd'
    if dtype == FP32:   # (svol_dropout_add is fp32 only) res + ones * keep, res = 2: exact in fp32
        t = torch.ones(shape, dtype=FP32, device=DEV)
        res = torch.full(shape, 2.0, dtype=FP32, device=DEV)
        out = ops.dropout_add(t, res, p, seed, _counter(k))
        assert torch.equal(out.cpu(), 2.0 + want), 'svol_dropout_add_sd'


@pytest.mark.parametrize('dtype', [FP32, BF16, FP16], ids=lambda d: R.DT_NAME[d])
def test_dropout_null_and_zero_counter_are_the_existing_entry(dtype):
    from svol_amd import _lib, ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn((37, 100), generator=g).to(dtype).to(DEV)
    p, seed = 0.1, R.SEEDS[1]
    old = torch.empty_like(x)
    _lib.check(_lib.lib().svol_dropout(ops._ptr(x), ops._ptr(old), x.numel(), 100, p, seed, ops._dt(x), ops._stream()), 'svol_dropout')
    null = torch.empty_like(x)
    _lib.check(_lib.lib().svol_dropout_sd(ops._ptr(x), ops._ptr(null), x.numel(), 100, p, seed, None, ops._dt(x), ops._stream()), 'svol_dropout_sd')
    assert torch.equal(null, old) and torch.equal(ops.dropout(x, p, seed), old) and torch.equal(ops.dropout(x, p, seed, seed_dev=_counter(0)), old)
    if dtype == FP32:
        res = torch.randn((37, 100), generator=g).to(DEV)
        olda = torch.empty_like(x)
        _lib.check(_lib.lib().svol_dropout_add(ops._ptr(x), ops._ptr(res), ops._ptr(olda), x.numel(), 100, p, seed, ops._stream()),
                   'svol_dropout_add')
        nulla = torch.empty_like(x)
        _lib.check(_lib.lib().svol_dropout_add_sd(ops._ptr(x), ops._ptr(res), ops._ptr(nulla), x.numel(), 100, p, seed, None, ops._stream()),
                   'svol_dropout_add_sd')
        assert torch.equal(nulla, olda) and torch.equal(ops.dropout_add(x.clone(), res, p, seed), olda)
        assert torch.equal(ops.dropout_add(x.clone(), res, p, seed, _counter(0)), olda)


def test_neighbouring_counters_give_independent_masks():
    """p = 0.5: two independent masks differ in an element with probability 2 p (1 - p) = 0.5; over 10^4 elements sigma is 0.005, the
    band [0.45, 0.55] is 10 sigma wide on either side"""
    from svol_amd import ops
    x = torch.ones((100, 100), dtype=FP32, device=DEV)
    seed = R.SEEDS[1]
    for k in (0, 1, 5):
        a, b = ops.dropout(x, 0.5, seed, seed_dev=_counter(k)), ops.dropout(x, 0.5, seed, seed_dev=_counter(k + 1))
        share = float(((a != 0) != (b != 0)).float().mean())
        print(f'counters {k} / {k + 1}: masks differ in {share:.4f} of {x.numel()} elements')
        assert 0.45 <= share <= 0.55, share


# ----------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------
PROBE_K = 3
PROBE_SEED = R.SEEDS[1]
W64 = (2, 4, 130, 256, 64, 'none')   # U1's size class at head width 64: csrc/attention.hip at two d-tiles
PROBES = [('U1', BF16), ('S2', BF16), ('M1', FP32), ('W64', BF16)]


def _launch(name, q, k, v, do, kb, p, seed, seed_dev, entry='sd'):
    """one forward + backward -> o, lse2, dq, dk, dv.  entry 'sd': ops.attn_fwd / attn_bwd with the counter tensor `seed_dev` (the *_sd
    entries); 'null': the *_sd entries called directly with a NULL pointer; 'old': the entries without the suffix, called directly"""
    from svol_amd import _lib, ops
    B, H, Lq, Lk, dh, _ = R.CASES[name]
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, do))
    kbd = None if kb is None else kb.to(DEV)
    dq = torch.empty((B * Lq, H * dh), dtype=qd.dtype, device=DEV)
    dk, dv = (torch.empty((B * Lk, H * dh), dtype=qd.dtype, device=DEV) for _ in range(2))
    if entry == 'sd':
        o, lse2 = ops.attn_fwd(qd, kd, vd, B, H, Lq, Lk, dh, kbd, 0.0, drop=(p, seed, seed_dev))
        ops.attn_bwd(qd, kd, vd, o, dod, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbd, 0.0, drop=(p, seed, seed_dev))
    else:
        L, P = _lib.lib(), ops._ptr
        o = torch.empty((B * Lq, H * dh), dtype=qd.dtype, device=DEV)
        lse2 = torch.empty((B, H, Lq), dtype=FP32, device=DEV)
        delta = torch.empty((3, B, H, Lq), dtype=FP32, device=DEV)
        ws, ws2 = ops._attn_ws(qd, B, H, Lq, Lk, dh), ops._attn_ws(qd, B, H, Lq, Lk, dh)
        nb = lambda w: w.numel() * 4 if w is not None else 0
        sc = 1.0 / dh ** 0.5
        fwd, bwd, extra = ((L.svol_attn_fwd_dropout, L.svol_attn_bwd_dropout, ()) if entry == 'old' else
                           (L.svol_attn_fwd_dropout_sd, L.svol_attn_bwd_dropout_sd, (None,)))
        _lib.check(fwd(P(qd), qd.stride(0), P(kd), kd.stride(0), P(vd), vd.stride(0), P(o), o.stride(0), P(lse2), P(kbd), B, H, Lq, Lk, dh, sc,
                       0.0, P(ws), nb(ws), p, seed, *extra, ops._dt(qd), ops._stream()), 'attention forward, ' + entry)
        _lib.check(bwd(P(qd), qd.stride(0), P(kd), kd.stride(0), P(vd), vd.stride(0), P(o), o.stride(0), P(dod), dod.stride(0), P(lse2),
                       P(delta), P(kbd), P(dq), dq.stride(0), P(dk), dk.stride(0), P(dv), dv.stride(0), B, H, Lq, Lk, dh, sc, 0.0, P(ws2),
                       nb(ws2), p, seed, *extra, ops._dt(qd), ops._stream()), 'attention backward, ' + entry)
    torch.cuda.synchronize()
    return o, lse2, dq, dk, dv


@pytest.fixture
def cases(monkeypatch):
    monkeypatch.setitem(R.CASES, 'W64', W64)   # (the probes look their geometry up by name; gone again after the test)
    return R.CASES


@pytest.mark.parametrize('kind', ['fwd', 'dv', 'dq', 'dk'])
@pytest.mark.parametrize('name,dtype', PROBES, ids=[f'{n}-{R.DT_NAME[d]}' for n, d in PROBES])
def test_attention_mask_probe_reads_the_twin_at_the_composed_seed(cases, name, dtype, kind):
    """the mask probes of tests/attn_dropout_ref.py through the *_sd entries at (seed, counter 3): every valid (row, key) bit is the
    twin's at seed + (3 << 12), as the forward, the dK/dV kernel's two products and the dQ kernel applied it.  U1: no key split, S2: key
    split + combine + dq finish, M1: fp32 kernels, ragged and masked, W64: the wide kernels."""
    sdev = _counter(PROBE_K)

    def run(q, k, v, do, kb):
        o, _, dq, dk, dv = _launch(name, q, k, v, do, kb, R.PROBE_P, PROBE_SEED, sdev)
        return o, dq, dk, dv
    rec = R.probe(kind, name, run, dtype)
    want = R.keep_mask(name, R.PROBE_P, PROBE_SEED + (PROBE_K << STRIDE))
    wrong, missed = rec.mismatches(want, R.expected_seen(name))
    host_seed_wrong, _ = rec.mismatches(R.keep_mask(name, R.PROBE_P, PROBE_SEED), R.expected_seen(name))
    print(f'{name} {R.DT_NAME[dtype]} {kind}: {int(rec.seen.sum())} bits read, {wrong} wrong, {missed} left out; '
          f'{host_seed_wrong} differ from the mask of the host seed alone')
    assert wrong == 0 and missed == 0, f'{kind} probe on {name}: {wrong} wrong bits, {missed} elements left out'
    assert host_seed_wrong > 0.4 * int(rec.seen.sum()), 'the counter did not enter the seed'


@pytest.mark.parametrize('name,dtype', PROBES, ids=[f'{n}-{R.DT_NAME[d]}' for n, d in PROBES])
def test_attention_null_and_zero_counter_are_the_existing_entry(cases, name, dtype):
    """o and lse2 of a NULL pointer, of a counter at 0 and of the entry without the suffix: the same bits (the forward of these plans
    takes no atomics); so are the gradients where the backward takes none (the key-split plans accumulate dQ with fp32 atomics)."""
    B, H, Lq, Lk, dh, _ = R.CASES[name]
    d = H * dh
    q, k, v, do = (R._rnd((B * L, d), dtype, 30 + i, s) for i, (L, s) in enumerate(((Lq, 1.5), (Lk, 1.5), (Lk, 1.0), (Lq, 1.0))))
    kb = R.key_bias(name)
    p, seed = 0.1, PROBE_SEED
    old = _launch(name, q, k, v, do, kb, p, seed, None, entry='old')
    null = _launch(name, q, k, v, do, kb, p, seed, None, entry='null')
    zero = _launch(name, q, k, v, do, kb, p, seed, _counter(0))
    moved = _launch(name, q, k, v, do, kb, p, seed, _counter(1))
    for tag, a, b, c in zip(('o', 'lse2'), old, null, zero):
        assert torch.equal(a, b) and torch.equal(a, c), tag
    if name != 'S2':
        for tag, a, b, c in zip(('dq', 'dk', 'dv'), old[2:], null[2:], zero[2:]):
            assert torch.equal(a, b) and torch.equal(a, c), tag
    assert not torch.equal(old[0], moved[0]) and torch.equal(old[1], moved[1])   # another mask, the same (undropped) lse2
