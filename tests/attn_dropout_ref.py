"""Reference side of the attention-dropout tests (plain torch on the CPU, no GPU import): the launch cases, the fp64 reference under
the twin's keep mask, its emulation with the operand dtype's roundings at the kernels' rounding sites (the slice bars come from it),
and the mask probes -- inputs that make an output read the keep mask bit by bit.

A *runner* is any callable ``run(q, k, v, do, kbias) -> (o, dq, dk, dv)`` over 2-D ``[B * L, H * dh]`` tensors: the device launch in
tests/test_gpu_attn_dropout.py, the fp64 reference (with the twin's mask or a deliberately faulty one) in
tests/test_attn_dropout_probe.py.  The probes only ever see the runner.

    python -m tests.attn_dropout_ref        prints the emulation's worst slice error per dtype and case (the bar table)
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import slice_metrics as S
from tests.dropout_twin import dropout_keep_numpy

LOG2E = 1.4426950408889634
# name: B, H, Lq, Lk, dh, mask ('none' | 'quarter': last quarter of the keys and kb[0, 3] | 'last1': the last key of video 0)
CASES = {
    'U1': (2, 4, 130, 256, 32, 'none'),      # <false> kernels, no split, 2-row last query tile
    'M1': (2, 4, 101, 333, 8, 'quarter'),    # <true>, odd Lq, odd Lk, ragged key tile
    'T1': (1, 2, 300, 400, 16, 'none'),      # ragged: several query tiles x several key tiles, no split
    'S1': (1, 8, 70, 2048, 32, 'none'),      # unmasked key split + attn_combine + attn_dq_finish
    'S2': (2, 4, 100, 1500, 32, 'quarter'),  # key split with fully masked trailing splits
    'S3': (2, 8, 7, 1153, 32, 'none'),       # key split, odd Lk, one partial query tile
    'E1': (2, 8, 256, 257, 32, 'last1'),     # encoder self-attention with the appended sketch token, in small
    'P1': (2, 4, 96, 96, 8, 'none'),         # self-attention over a packed [M, 3 d] buffer: the column-slice test's shape
}
FP32_CASES = ('U1', 'M1', 'T1', 'S2', 'P1')
PROBE_CASES = ('U1', 'M1', 'S2', 'S3')
PS = (0.1, 0.5)
SEEDS = (5, (7 << 44) + (3 << 12) + 1)      # a small one; the model's form (base << 44) + (step << 12) + site
DT_NAME = {torch.bfloat16: 'bf16', torch.float16: 'fp16', torch.float32: 'fp32'}


def premuls(dh):
    return (0.0, LOG2E / math.sqrt(dh))


def key_bias(name):
    B, H, Lq, Lk, dh, mask = CASES[name]
    if mask == 'none':
        return None
    kb = torch.zeros(B, Lk)
    if mask == 'quarter':       # check_attention's mask
        kb[:, Lk - Lk // 4:] = float('-inf')
        kb[0, 3] = float('-inf')
    else:
        kb[0, Lk - 1] = float('-inf')
    return kb


def keep_mask(name, p, seed):
    B, H, Lq, Lk, dh, _ = CASES[name]
    return torch.from_numpy(dropout_keep_numpy((B, H, Lq, Lk), p, seed))


def _rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def make_inputs(name, dtype, premul=0.0):
    """check_attention's inputs.  -> q (what the kernel is given: pre-multiplied and rounded when premul != 0), qref (fp64, the
    unscaled q the kernel effectively sees: gradients are taken w.r.t. it), k, v, do."""
    B, H, Lq, Lk, dh, _ = CASES[name]
    d = H * dh
    q, k, v = _rnd((B * Lq, d), dtype, 30, 1.5), _rnd((B * Lk, d), dtype, 31, 1.5), _rnd((B * Lk, d), dtype, 32)
    do = _rnd((B * Lq, d), dtype, 33)
    if premul != 0.0:
        q = (q.double() * premul).to(dtype)
        return q, q.double() / premul, k, v, do
    return q, q.double(), k, v, do


def _heads(t, B, L, H, dh):
    return t.view(B, L, H, dh).transpose(1, 2)


def _flat(t, B, L, H, dh):
    return t.transpose(1, 2).reshape(B * L, H * dh)


def reference(q, k, v, do, kbias, keep, p, dims):
    """THE reference: P = softmax(q k^T scale + kbias), P~ = P * keep / (1 - p), O = P~ v in fp64, gradients by autograd.
    keep None: no dropout.  -> o, lse2 [B, H, Lq] (of the undropped softmax), dq, dk, dv"""
    B, H, Lq, Lk, dh = dims
    q64, k64, v64 = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    s = _heads(q64, B, Lq, H, dh) @ _heads(k64, B, Lk, H, dh).transpose(-1, -2) / math.sqrt(dh)
    if kbias is not None:
        s = s + kbias.double()[:, None, None, :]
    P = torch.softmax(s, -1)
    if keep is not None:
        P = P * (keep.double() / (1.0 - p))
    o = _flat(P @ _heads(v64, B, Lk, H, dh), B, Lq, H, dh)
    (o * do.double()).sum().backward()
    lse2 = torch.logsumexp(s.detach(), -1) / math.log(2.0)
    return o.detach(), lse2, q64.grad, k64.grad, v64.grad


def emulate(q, k, v, do, kbias, keep, p, dims, rnd=None, work=torch.float64):
    """The same formula written out, backward included, with ``rnd`` applied where the 16-bit kernels round (csrc/attention_bf16.hip):
    the masked softmax numerators before P~ V (mma_second's operand; the row sum and lse stay fp32 and undropped), the output, P~ before
    dO^T P~, dS = P (dP~ - delta) before its two products, and the three gradients; delta is taken from the ROUNDED output, as the
    device's backward reads it.  rnd None and work fp64: the reference itself (the CPU test holds it to autograd); work fp32, rnd
    None: the formula in fp32 arithmetic, the fp32 kernels' yardstick.  -> o, dq, dk, dv"""
    B, H, Lq, Lk, dh = dims
    r = (lambda t: t) if rnd is None else rnd
    scale = 1.0 / math.sqrt(dh)
    q4, k4, v4, do4 = (_heads(t.to(work), B, L, H, dh) for t, L in ((q, Lq), (k, Lk), (v, Lk), (do, Lq)))
    s = q4 @ k4.transpose(-1, -2) * scale
    if kbias is not None:
        s = s + kbias.to(work)[:, None, None, :]
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    ms = torch.ones((), dtype=work) if keep is None else keep.to(work) / (1.0 - p)
    o4 = r(r(e * ms) @ v4 / l)
    P = e / l
    delta = (o4 * do4).sum(-1, keepdim=True)
    dv4 = r(r(P * ms).transpose(-1, -2) @ do4)
    dS = r(P * ((do4 @ v4.transpose(-1, -2)) * ms - delta))
    dq4 = r(dS @ k4 * scale)
    dk4 = r(dS.transpose(-1, -2) @ q4 * scale)
    return _flat(o4, B, Lq, H, dh), _flat(dq4, B, Lq, H, dh), _flat(dk4, B, Lk, H, dh), _flat(dv4, B, Lk, H, dh)


def rounder(dtype):
    return lambda t: t.to(dtype).to(t.dtype)


def slice_errors(name, got, ref):
    """{tensor: SliceResult} of (o, dq, dk, dv) on the (batch, 128-row tile, head) slices: query tiles for o / dq, key tiles for dk / dv."""
    return slice_errors_dims(CASES[name][:5], got, ref)


def slice_errors_dims(dims, got, ref):
    """slice_errors for a launch given by its (B, H, Lq, Lk, dh)"""
    B, H, Lq, Lk, dh = dims
    out = {}
    for tag, g, r, L in zip(('o', 'dq', 'dk', 'dv'), got, ref, (Lq, Lq, Lk, Lk)):
        out[tag] = S.compare(tag, g.reshape(B, L, H * dh), r.reshape(B, L, H * dh), 'act', heads=H)
    return out


def emulation_error(name, dtype, premul, p, seed):
    """worst slice error of the emulation in ``dtype`` against the fp64 reference at one parameter point"""
    B, H, Lq, Lk, dh, _ = CASES[name]
    dims = (B, H, Lq, Lk, dh)
    q, qref, k, v, do = make_inputs(name, dtype, premul)
    kb, keep = key_bias(name), keep_mask(name, p, seed)
    o, _, dq, dk, dv = reference(qref, k, v, do, kb, keep, p, dims)
    if dtype == torch.float32:
        emu = emulate(qref.float(), k, v, do, kb, keep, p, dims, None, torch.float32)
    else:
        emu = emulate(qref, k, v, do, kb, keep, p, dims, rounder(dtype), torch.float64)
    return max(r.err for r in slice_errors(name, emu, (o, dq, dk, dv)).values())


def points(name, dtype):
    dh = CASES[name][4]
    return [(pm, p, seed) for pm in premuls(dh) for p in PS for seed in SEEDS]


def cases_of(dtype):
    return FP32_CASES if dtype == torch.float32 else tuple(CASES)


# ----------------------------------------------------------------------------------------------------------------------
# mask probes
# ----------------------------------------------------------------------------------------------------------------------
PROBE_P = 0.5


def valid_keys(name):
    """[B, Lk] bool: keys the bias leaves in"""
    B, H, Lq, Lk, dh, _ = CASES[name]
    kb = key_bias(name)
    return torch.ones(B, Lk, dtype=torch.bool) if kb is None else kb == 0


def windows(L, dh, starts=None):
    """windows of dh rows: the tiling 0, dh, 2 dh, ... (the last one ragged) -- every row of [0, L) lies in one -- or the given starts"""
    return [(s, min(s + dh, L)) for s in (range(0, L, dh) if starts is None else starts)]


def sampled_key_windows(name, tiles_per_split=2, n_random=6, seed=0):
    """starts of the key windows a sampled probe run takes on the long cases: those that straddle each 128-key boundary (which
    includes every key-split boundary: a split is ``tiles_per_split`` 128-key tiles), the window at each side of it, the first and
    the ragged last one, and a fixed random sample of the rest."""
    B, H, Lq, Lk, dh, _ = CASES[name]
    starts = {0, (Lk - 1) // dh * dh}
    for b in range(128, Lk, 128):
        starts.update(s for s in (b - dh, b - dh // 2, b) if 0 <= s < Lk)
    rest = sorted(set(range(0, Lk, dh)) - starts)
    g = torch.Generator().manual_seed(seed)
    starts.update(rest[i] for i in torch.randperm(len(rest), generator=g)[:n_random].tolist())
    return sorted(starts)


def _onehot_rows(B, L, H, dh, w, dtype):
    """[B * L, H * dh]: row w0 + j of every (batch, head) is the unit vector e_j"""
    t = torch.zeros(B, L, H, dh, dtype=dtype)
    for j in range(w[1] - w[0]):
        t[:, w[0] + j, :, j] = 1
    return t.view(B * L, H * dh)


def _e0_rows(B, L, H, dh, dtype):
    t = torch.zeros(B, L, H, dh, dtype=dtype)
    t[..., 0] = 1
    return t.view(B * L, H * dh)


def _zeros(B, L, H, dh, dtype):
    return torch.zeros(B * L, H * dh, dtype=dtype)


class Recovered:
    """the keep bits a probe run read back: ``bits`` [B, H, Lq, Lk] and ``seen`` (which elements a probe covered)"""

    def __init__(self, dims):
        B, H, Lq, Lk, dh = dims
        self.bits = torch.zeros(B, H, Lq, Lk, dtype=torch.bool)
        self.seen = torch.zeros(B, H, Lq, Lk, dtype=torch.bool)

    def mismatches(self, keep, expect_seen):
        """(wrong bits among the probed elements, elements that should have been probed and were not)"""
        return int(((self.bits != keep) & self.seen).sum()), int((expect_seen & ~self.seen).sum())


def probe(kind, name, run, dtype, key_starts=None, p=PROBE_P):
    """Run one probe family through ``run`` and decode the keep bits each launch's output carries.  Every score is 0 (q = 0 or k = 0),
    so P is uniform at 1 / n over the n valid keys of the video and:

      'fwd'  q = 0, v one-hot over a key window:                          O[q, j]  = keep[q, k0 + j] / ((1 - p) n)
      'dv'   q = 0, dO one-hot over a query window:                       dV[k, j] = keep[q0 + j, k] / ((1 - p) n)
      'dq'   q = 0, k one-hot over a key window, v = e_0, dO = e_0:       dQ[q, j] = scale (keep[q, k0 + j] / (1 - p) - delta_q) / n
      'dk'   k = 0, q one-hot over a query window, v = e_0, dO = e_0:     dK[k, j] = scale (keep[q0 + j, k] / (1 - p) - delta_{q0 + j}) / n

    delta_q = O[q, 0], the kept share of row q (about 1): read from the run's own forward output.  The bit is the value against the
    midpoint of its two levels.  Masked keys carry no mask information and are left out.  -> Recovered"""
    B, H, Lq, Lk, dh, _ = CASES[name]
    dims = (B, H, Lq, Lk, dh)
    kb, vk = key_bias(name), valid_keys(name)
    n = vk.sum(1).double()                                # [B] valid keys
    scale = 1.0 / math.sqrt(dh)
    rec = Recovered(dims)
    unit = (1.0 / ((1.0 - p) * n))[:, None, None, None]   # the kept level of 'fwd' / 'dv', per video
    z = lambda L: _zeros(B, L, H, dh, dtype)
    over_keys = kind in ('fwd', 'dq')
    for w in windows(Lk if over_keys else Lq, dh, key_starts if over_keys else None):
        wn = w[1] - w[0]
        if kind == 'fwd':
            q, k, v, do = z(Lq), z(Lk), _onehot_rows(B, Lk, H, dh, w, dtype), z(Lq)
        elif kind == 'dv':
            q, k, v, do = z(Lq), z(Lk), z(Lk), _onehot_rows(B, Lq, H, dh, w, dtype)
        elif kind == 'dq':
            q, k, v, do = z(Lq), _onehot_rows(B, Lk, H, dh, w, dtype), _e0_rows(B, Lk, H, dh, dtype), _e0_rows(B, Lq, H, dh, dtype)
        else:
            q, k, v, do = _onehot_rows(B, Lq, H, dh, w, dtype), z(Lk), _e0_rows(B, Lk, H, dh, dtype), _e0_rows(B, Lq, H, dh, dtype)
        o, dq, dk, dv = (t.detach().double().cpu() for t in run(q, k, v, do, kb))
        o4 = _heads(o.reshape(B * Lq, H * dh), B, Lq, H, dh)            # [B, H, Lq, dh]
        if kind == 'fwd':
            bits = o4[..., :wn] > 0.5 * unit                             # [B, H, Lq, wn]
            rec.bits[..., w[0]:w[1]] = bits
            rec.seen[..., w[0]:w[1]] = vk[:, None, None, w[0]:w[1]]
        elif kind == 'dv':
            dv4 = _heads(dv.reshape(B * Lk, H * dh), B, Lk, H, dh)      # [B, H, Lk, dh]
            rec.bits[:, :, w[0]:w[1], :] = (dv4[..., :wn] > 0.5 * unit).transpose(-1, -2)
            rec.seen[:, :, w[0]:w[1], :] = vk[:, None, None, :]
        elif kind == 'dq':
            dq4 = _heads(dq.reshape(B * Lq, H * dh), B, Lq, H, dh)
            mid = scale * (1.0 - o4[..., :1]) / n[:, None, None, None]  # [B, H, Lq, 1]
            rec.bits[..., w[0]:w[1]] = dq4[..., :wn] > mid
            rec.seen[..., w[0]:w[1]] = vk[:, None, None, w[0]:w[1]]
        else:
            dk4 = _heads(dk.reshape(B * Lk, H * dh), B, Lk, H, dh)      # [B, H, Lk, dh]
            mid = scale * (1.0 - o4[:, :, w[0]:w[1], 0]) / n[:, None, None]   # [B, H, wn]: delta of row q0 + j
            rec.bits[:, :, w[0]:w[1], :] = (dk4[..., :wn] > mid[:, :, None, :]).transpose(-1, -2)
            rec.seen[:, :, w[0]:w[1], :] = vk[:, None, None, :]
    return rec


def expected_seen(name, key_starts=None, over_keys=True):
    """the elements a probe family must have covered: every valid key of every row (of the sampled key windows, when given)"""
    B, H, Lq, Lk, dh, _ = CASES[name]
    vk = valid_keys(name)[:, None, None, :].expand(B, H, Lq, Lk).clone()
    if over_keys and key_starts is not None:
        inwin = torch.zeros(Lk, dtype=torch.bool)
        for w in windows(Lk, dh, key_starts):
            inwin[w[0]:w[1]] = True
        vk &= inwin
    return vk


def reference_runner(name, keep, p=PROBE_P):
    """the fp64 reference under the mask ``keep`` (the twin's, or a faulty one) as a runner"""
    B, H, Lq, Lk, dh, _ = CASES[name]

    def run(q, k, v, do, kb):
        o, _, dq, dk, dv = reference(q, k, v, do, kb, keep, p, (B, H, Lq, Lk, dh))
        return o, dq, dk, dv
    return run


# ----------------------------------------------------------------------------------------------------------------------
# the faults a kernel's mask generation could plausibly have, as masks
# ----------------------------------------------------------------------------------------------------------------------
def fault_fields_swapped_in_odd_keys(name, p, seed):
    """an odd key reads the even key's 16-bit field of the pair's word"""
    keep = keep_mask(name, p, seed).clone()
    Lk = keep.shape[-1]
    odd = torch.arange(1, Lk, 2)
    keep[..., odd] = keep_mask(name, p, seed)[..., odd - 1]
    return keep


def fault_rows_swapped_in_odd_lanes(name, p, seed):
    """the odd lane (odd key) of a row pair (q0, q0 + 1) keeps its own word instead of its neighbour's: rows swapped in odd keys"""
    good = keep_mask(name, p, seed)
    keep = good.clone()
    Lq, Lk = keep.shape[-2:]
    swapped = (torch.arange(Lq) ^ 1).clamp_max(Lq - 1)
    keep[..., 1::2] = good[:, :, swapped, 1::2]
    return keep


def fault_last_row_unclamped(name, p, seed):
    """the last row of an odd Lq drawn from row Lq (the next head's first row) instead of row Lq - 1"""
    B, H, Lq, Lk, dh, _ = CASES[name]
    assert Lq % 2 == 1
    flat = torch.from_numpy(dropout_keep_numpy((B * H * Lq + 1, Lk), p, seed))
    keep = flat[:-1].view(B, H, Lq, Lk).clone()
    nxt = flat[torch.arange(1, B * H + 1) * Lq].view(B, H, Lk)
    keep[:, :, Lq - 1, :] = nxt
    return keep


def fault_tile_row_base(name, p, seed, b=0, h=1, qt=0, kt=0):
    """one 128 x 128 tile of one (batch, head) drawn with the next head's row base"""
    good = keep_mask(name, p, seed)
    keep = good.clone()
    H = keep.shape[1]
    qs, ks = slice(qt * 128, (qt + 1) * 128), slice(kt * 128, (kt + 1) * 128)
    keep[b, h, qs, ks] = good[b, (h + 1) % H, qs, ks]
    return keep


FAULTS = {'fields_swapped_in_odd_keys': fault_fields_swapped_in_odd_keys, 'rows_swapped_in_odd_lanes': fault_rows_swapped_in_odd_lanes,
          'last_row_unclamped': fault_last_row_unclamped, 'tile_row_base': fault_tile_row_base}


if __name__ == '__main__':
    torch.set_num_threads(8)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        worst = (0.0, None)
        for name in cases_of(dt):
            e = max((emulation_error(name, dt, *pt), pt) for pt in points(name, dt))
            print(f'{DT_NAME[dt]} {name}: {e[0]:.3e} at premul={e[1][0]:.4f} p={e[1][1]} seed={e[1][2]}', flush=True)
            worst = max(worst, (e[0], (name,) + e[1]))
        print(f'{DT_NAME[dt]} worst {worst[0]:.3e} at {worst[1]}  -> bar {3 * worst[0]:.3e}', flush=True)
