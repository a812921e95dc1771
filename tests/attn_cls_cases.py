"""One-query ([CLS]) attention, csrc/sketch_cls.hip attn_cls_fwd_kernel / attn_cls_bwd_kernel: the cases, the inputs, the fp64 reference,
the bf16 emulation and the figures (plain torch on the CPU, importable without the device library).  tests/test_attn_cls_cases.py holds
this file's emulation to the constants the device test quotes, tests/test_gpu_attn_cls.py runs the cases on the device.

1. Cases (n, H, L, dh).  n = 2 images, H = 3 heads: 6 (image, head) pairs, so the second four-wave workgroup has a ragged tail.  L in
   LENGTHS: 1 (P = 1, dS = 0); 2 (at dh = 32 the two half-waves of phase 2 get one key each); 63 / 64 / 65, 128 / 129, 192 / 193 and
   255 / 256: a lane holds keys lane + 64 i, so a fourth, a half, ... of the per-lane key slots fill up there; 197: the ViT's length.
   Both head widths at every L.  One more point (5, 1, 197, dh): five pairs, H = 1.
2. Families.  'benign': randn * 1.2.  'first' / 'last': channel 0 of every head is reserved; q0 = +-A = 256 (+ in even images) with the
   row's other channels scaled by 0.25, k0 = 0 except at key 0 / key L - 1, where it is +-KD (2.25 at dh = 32, 3.125 at dh = 64): that
   key outscores every other by about 145 log2 units (one unit of q0 k0 is log2 e / sqrt(dh) units: 65.3 / 46.2), so the others
   underflow and P is one-hot.  'deep': every key at k0 = -+KD: every score is about -145 units, lse2 <= -128 at every L.
   Every planted value is exact in bf16.
3. Canary rows.  k and v are allocated with CANARY_ROWS = 32 rows behind n L, dout with 32 rows behind n; the kernels get views of the
   leading rows.  The canary keys are 64 sign(q of the last image): read as a key of that image one scores 64 sum |q| (hundreds of
   units above any real key); canary v and dout entries have magnitude 64.
4. `figures`: slice errors (tests/slice_metrics.py) of o and dq on (image, head) slices and of dk / dv on (image, head, 64-key block)
   slices; element errors per (image, head) against the largest reference entry of that (image, head); lse2; finiteness; at L = 1
   dq = dk = 0 and dv = dout exactly.  A reference that is identically zero (dq, dk at L = 1 and under a one-hot P) is measured on
   dv's scale.
"""
from __future__ import annotations

import functools
import math

import torch

from tests import slice_metrics as S

LOG2E = 1.4426950408889634
BF16 = torch.bfloat16
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 192, 193, 197, 255, 256)
DHS = (32, 64)
FAMILIES = ('benign', 'first', 'last', 'deep')
KEY_BLOCK = 64            # keys of one pass of the lane = key phases
CANARY_ROWS = 32
CANARY_MAG = 64.0
A = 256.0
KD = {32: 2.25, 64: 3.125}
TOL = 1.2e-2              # tests/gpu_checks.py TOL[bf16]: o; the gradients take twice that
LSE_BAR = 2e-5            # of max(1, max |lse2|)
TINY = 2.0 ** -126        # fp32's smallest normal: a reference below it (dS under a one-hot P: ~2^-145) counts as zero


def points():
    """[(n, H, L, dh, family)]"""
    pts = [(2, 3, L, dh, fam) for L in LENGTHS for dh in DHS for fam in FAMILIES]
    return pts + [(5, 1, 197, dh, 'benign') for dh in DHS]


def point_id(n, H, L, dh, fam):
    return f'n{n}-H{H}-L{L}-dh{dh}-{fam}'


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


@functools.lru_cache(maxsize=None)
def make_case(n, H, L, dh, family):
    """-> dict: q [n, d], k / v [n L + 32, d], do [n + 32, d] (bf16, canary rows included), dims.  Shared between tests: never modified."""
    d, M = H * dh, n * L
    q = _rnd((n, d), 50 + L, 1.2)
    k, v = _rnd((M + CANARY_ROWS, d), 51 + L, 1.2), _rnd((M + CANARY_ROWS, d), 52 + L, 1.2)
    do = _rnd((n + CANARY_ROWS, d), 53 + L)
    if family != 'benign':
        q3, k4 = q.view(n, H, dh), k[:M].view(n, L, H, dh)
        q3[..., 1:] = (q3[..., 1:].double() * 0.25).to(BF16)
        k4[..., 0] = 0
        for b in range(n):
            s = 1.0 if b % 2 == 0 else -1.0
            q3[b, :, 0] = s * A
            if family == 'first':
                k4[b, 0, :, 0] = s * KD[dh]
            elif family == 'last':
                k4[b, L - 1, :, 0] = s * KD[dh]
            else:
                k4[b, :, :, 0] = -s * KD[dh]
    sgn = lambda t: torch.where(t.double() < 0, -CANARY_MAG, CANARY_MAG).to(BF16)   # noqa: E731
    k[M:] = sgn(q[n - 1]).expand(CANARY_ROWS, d)
    v[M:] = sgn(v[M:])
    do[n:] = sgn(do[n:])
    return dict(dims=(n, H, L, dh), family=family, q=q, k=k, v=v, do=do)


def real(c):
    """the rows the kernels are handed: (q [n, d], k, v [n L, d], do [n, d])"""
    n, H, L, dh = c['dims']
    return c['q'], c['k'][:n * L], c['v'][:n * L], c['do'][:n]


def _math(q, k, v, do, dims):
    """fp64 one-query attention and its gradients -> (o [n, d], lse2 [n, H], dq [n, d], dk, dv [n L, d])"""
    n, H, L, dh = dims
    q3, do3 = q.double().view(n, H, dh), do.double().view(n, H, dh)
    k4, v4 = (t.double().view(n, L, H, dh).transpose(1, 2) for t in (k, v))            # [n, H, L, dh]
    scale = 1.0 / math.sqrt(dh)
    s = torch.einsum('bhjc,bhc->bhj', k4, q3) * scale
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = torch.einsum('bhj,bhjc->bhc', P, v4)
    delta = (do3 * o).sum(-1)
    dS = P * (torch.einsum('bhjc,bhc->bhj', v4, do3) - delta[..., None])
    dq = scale * torch.einsum('bhj,bhjc->bhc', dS, k4)
    dk = scale * dS[..., None] * q3[:, :, None, :]
    dv = P[..., None] * do3[:, :, None, :]
    flat = lambda t: t.transpose(1, 2).reshape(n * L, H * dh)                          # noqa: E731
    return o.reshape(n, H * dh), lse / math.log(2.0), dq.reshape(n, H * dh), flat(dk), flat(dv)


@functools.lru_cache(maxsize=None)
def reference(n, H, L, dh, family):
    """fp64 -> (o, lse2, dq, dk, dv) (shared, never modified)"""
    c = make_case(n, H, L, dh, family)
    return _math(*real(c), c['dims'])


def emulation(n, H, L, dh, family):
    """the kernels' rounding sites in fp64 arithmetic: o, dq, dk, dv are stored as bf16; P and dS are never rounded, and delta is
    formed from P and dout . v_j, not from the stored o -> (o, lse2, dq, dk, dv)"""
    c = make_case(n, H, L, dh, family)
    o, lse2, dq, dk, dv = _math(*real(c), c['dims'])
    r = lambda t: t.to(BF16).double()   # noqa: E731
    return r(o), lse2, r(dq), r(dk), r(dv)


def _head_max(t, H, dh):
    """[R, H dh] with R = n or n L -> max |t| per (image, head) [n, H]"""
    return t.abs().view(t.shape[0], H, dh).amax(-1)


def figures(c, got, ref, slice_bar):
    """every figure of one point as {label: (value, bar)}; a figure holds when value <= bar.  got / ref: (o, lse2, dq, dk, dv)."""
    n, H, L, dh = c['dims']
    o, lse2, dq, dk, dv = (t.detach().double().cpu() for t in got)
    o_r, lse_r, dq_r, dk_r, dv_r = ref
    fig = {}
    finite = all(bool(torch.isfinite(t).all()) for t in (o, lse2, dq, dk, dv))
    fig['not finite'] = (0.0 if finite else math.inf, 0.0)
    dvn = float(dv_r.norm())
    dv_head = _head_max(dv_r, H, dh).view(n, L, H).amax(1)                            # [n, H]
    for tag, g, r, rows in (('o', o, o_r, 1), ('dq', dq, dq_r, 1), ('dk', dk, dk_r, L), ('dv', dv, dv_r, L)):
        zero = float(r.abs().max()) < TINY
        if zero:
            r = torch.zeros_like(r)
        if rows == 1:
            res = S.compare(tag, g, r, 'bd', heads=H, ref_norm=dvn if zero else None)
        else:
            res = S.compare(tag, g.reshape(n, L, H * dh), r.reshape(n, L, H * dh), 'act', heads=H, ref_norm=dvn if zero else None,
                            row_block=KEY_BLOCK)
        fig[f'slice/{res.where}'] = (res.err if res.finite else math.inf, slice_bar)
        diff = torch.nan_to_num((g - r).abs(), nan=math.inf)
        num = _head_max(diff, H, dh).view(n, rows, H).amax(1)
        den = _head_max(r, H, dh).view(n, rows, H).amax(1)
        den = torch.where(den < TINY, dv_head, den).clamp_min(1e-300)
        e = num / den
        i = int(e.argmax())
        fig[f'elem/{tag} [b={i // H}, head={i % H}]'] = (float(e.view(-1)[i]), TOL if tag == 'o' else 2 * TOL)
    err = torch.nan_to_num((lse2 - lse_r).abs(), nan=math.inf)
    fig['lse2'] = (float(err.max()), LSE_BAR * max(1.0, float(lse_r.abs().max())))
    if L == 1:      # one key: P = 1, dS = 0
        do = real(c)[3].double()
        for tag, t in (('dq = 0', dq), ('dk = 0', dk), ('dv = dO', dv - do)):
            fig[f'L1/{tag}'] = (float(torch.nan_to_num(t, nan=math.inf).abs().max()), 0.0)
    return fig


def failing(fig):
    return [label for label, (val, bar) in fig.items() if not val <= bar]


def worst_slice(fig):
    return max(v for label, (v, _) in fig.items() if label.startswith('slice/'))
