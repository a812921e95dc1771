"""Short-sequence (ViT) attention, csrc/vit.hip attn_small_kernel / attn_small_bwd_kernel, at every length where a loop bound
changes and at planted scores: the cases, the inputs, the figures and the fault runners (plain torch on the CPU, importable without
the device library).  tests/test_attn_small_cases.py holds this file to fp64 on the CPU, tests/test_gpu_attn_small.py runs the cases
on the device.

1. Cases (n, H, L, dh): L in LENGTHS (1; 31 / 32 / 33: one ragged block, one exact block, a second block of one row; 97: dh = 32 at a
   ragged multi-block L; 128 / 129: the forward's four waves start a second trip at block 4; 224 / 225: the backward's eighth wave
   gets work; 255 / 256), both head widths at every L (the LDS swizzle differs: row >> 2 at dh = 32), n = 2 images, H = 3 heads up to
   L = 129 and 5 above (odd: a head-offset slip cannot cancel).
2. Input families.  'benign': randn * 1.2, the inputs of tests/test_gpu_vit.py.  'planted': the same draw with channel 0 of every
   head reserved, as attn_range_cases.make_case does: k[:, 0] = 0 except at planted keys, q[:, 0] = 0 except at planted rows, where
   it is +-A = 256 and the row's other channels are scaled by 0.25.  Every planted value is exact in bf16.  One unit of q0 * k0 is
   log2 e / sqrt(dh) log2 units of score: 65.3 units per unit of k0 at dh = 32, 46.2 at dh = 64.  A is large so that every planted
   k0 stays within three sigma of the benign keys: dq[:, 0] = scale sum_j dS_j k0_j cancels exactly where many keys share one k0,
   and a large k0 multiplies the bf16 rounding of dS into it (A = 32 with k0 = 18 on every key put the benign rows of such a head at
   twice their element bar in the bf16 emulation).  The heads of the two images take the layouts in turn
   (slot = (h + b (6 - H)) % 6, which keeps 'first' in image 0):

     'first'  the top key is key 0, at k0 = KD (2.25 at dh = 32, 3.125 at dh = 64): about 145 log2 units above every other key,
              which underflow -- and, being key 0, in the first half-wave (bit 2 of the in-block key index, 4h, clear)
     'last'   the top key is key L - 1, the last valid key of the ragged block, at k0 = BETA = 0.75 (49 / 35 units)
     'pair'   two top keys one unit apart (BETA and beta2, the other channels shared), the upper one in the middle of the last 32-key block, the lower one in
              the first block (both in the one block of L <= 32), with different 4h bits; they carry opposite v (v_low = -v_top / 2: with -v_top the o of a planted row, v_top / 3, left the emulation
              at 0.38 of its element bar), and the planted rows'
              dO lies along the upper one's sign pattern, scaled by DO_SCALE: dS stays large against the rounding of delta
     'deep'   every key at k0 = -KD: every score of a planted row is about -145 units, lse2 <= -128 at every L.  (Scores of -130
              would leave lse2 = -130 + log2 L above -128 from L = 4 on.)  exp2(0 - lse2) of a padded key lane of the backward's
              key-stationary phase is then inf
     'high'   the mirror image: every key at +KD, lse2 >= +128
     'none'   nothing planted

   Planted rows: 0 and 5 in the first 32-row block, L - 1 and L - 5 in the last (5 and L - 5 where they fall into that block); the
   two of a block differ in bit 2 of the in-block index, the half-wave a query lands in in the key-stationary phase.  'pair' rows
   stay out of a last block of fewer than 8 rows: the o of such a row is (p1 - p2) v with p1 - p2 = 1/3, three times the relative
   rounding of a benign row, and a slice of one such row has nothing to average it with.
   In image 1 every planted sign is flipped (q0 = -A, k0 negated): the layouts are unchanged, and a key planted for image 0's rows
   scores at the far negative end for image 1's.
3. Canary rows.  Every operand is allocated with CANARY_ROWS = 32 rows more than n L and the kernels get the first n L rows as a
   view: an over-read of up to 32 rows stays inside the allocation.  The extra rows hold keys at k0 = -KC (3 / 4: 196 / 185 units
   against a planted row of the last image, image 1 with q0 = -A; at least 20 above its highest real key) and v / dO / q entries of
   magnitude 64.  Where L is ragged the leading keys of image 1 play the same part for image 0: k0 = +KC in every head, real keys of
   image 1 that score -196 / -185 units against its own planted rows and are ordinary keys for its benign rows.  They are the
   32 ceil(L / 32) - L rows image 0's last block reaches, but no more than L / 4 of them (neighbour_canaries): with 31 of its 33 keys
   taken, a planted row of image 1 is a softmax over two keys, and its one-row dq slice doubled the emulation's worst slice error.
4. `figures`: slice errors of o / dq / dk / dv on (image, head, 32-row block) slices; element errors per (image, head) separately
   over planted rows / keys and the others, against the largest reference entry of that (image, head); lse2 over each row set;
   finiteness; at L = 1 dq = dk = 0 and dv = dO exactly; on 'deep' heads dk / dv of the real keys finite and within the element bar.
   A reference that is identically zero (dq and dk at L = 1) is measured on dv's scale in the slice and element figures.
5. Fault runners: the fp64 reference with one deliberate defect each.
"""
from __future__ import annotations

import functools
import math

import torch

from tests import attn_dropout_ref as R
from tests import slice_metrics as S

LOG2E = R.LOG2E
BF16 = torch.bfloat16
LENGTHS = (1, 31, 32, 33, 97, 128, 129, 224, 225, 255, 256)
DHS = (32, 64)
FAMILIES = ('benign', 'planted')
N_IMAGES = 2
BLOCK = 32                # rows of a query / key block of both kernels
CANARY_ROWS = 32
LAYOUTS = ('first', 'last', 'pair', 'deep', 'high', 'none')
A = 256.0                 # |q0| of a planted row
BETA = 0.75               # k0 of the 'last' key and of the upper 'pair' key
KD = {32: 2.25, 64: 3.125}    # |k0| of the 'first' key and of 'deep' / 'high' keys
KC = {32: 3.0, 64: 4.0}       # k0 of a canary key
DO_SCALE = 1.0 / 128
CANARY_MAG = 64.0
TOL = 1.2e-2              # tests/gpu_checks.py TOL[bf16]: o; the gradients take twice that
LSE_BAR = 2e-5            # of max(1, max |lse2|): tests/test_gpu_attn_range.py's fp32 lse2 bar


def heads_of(L):
    return 3 if L <= 129 else 5


def dims_of(L, dh):
    return N_IMAGES, heads_of(L), L, dh


def points():
    """[(L, dh, family)]"""
    return [(L, dh, fam) for L in LENGTHS for dh in DHS for fam in FAMILIES]


def point_id(L, dh, fam):
    return f'L{L}-dh{dh}-{fam}'


def layout_of(b, h, H):
    return LAYOUTS[(h + b * (6 - H)) % 6]


def sign_of(b):
    return 1.0 if b % 2 == 0 else -1.0


def beta2(dh):
    """k0 of the lower 'pair' key: one log2 unit under BETA for a planted row, cut to 8 significant bits"""
    x = BETA - 1.0 / (A * LOG2E / math.sqrt(dh))
    return math.floor(x * 256) / 256


def nblocks(L):
    return -(-L // BLOCK)


def neighbour_canaries(L):
    """the number of leading keys of image b + 1 that are canaries for image b: the rows behind a ragged L up to the end of its
    block, but at most a quarter of the image (its own planted rows keep three quarters of their keys)"""
    return min(nblocks(L) * BLOCK - L, L // 4)


def planted_row_numbers(L, layout):
    last0 = (nblocks(L) - 1) * BLOCK
    rows = {0, L - 1}
    if 5 < min(L, BLOCK):
        rows.add(5)
    if L - 5 >= last0:
        rows.add(L - 5)
    if layout == 'pair' and 0 < last0 and L - last0 < 8:
        rows = {r for r in rows if r < last0}
    return sorted(rows)


def pair_keys(L, b=0):
    """(upper, lower) key of a 'pair' head of image b; L = 1: the one key.  The lower key sits in the first block, or in the second
    where image b's leading keys are the canaries of image b - 1."""
    if L == 1:
        return 0, None
    if L <= BLOCK:
        return 20, 10
    last0 = (nblocks(L) - 1) * BLOCK
    top = last0 + (L - 1 - last0) // 2
    first = BLOCK if b > 0 and neighbour_canaries(L) > 10 and L > 3 * BLOCK else 0
    return top, first + (10 if top & 4 else 14)


@functools.lru_cache(maxsize=None)
def make_case(L, dh, family):
    """-> dict: q, k, v, do (bf16 [n L + 32, H dh]: what the device test packs, canary rows included), dims (n, H, L, dh), prow /
    pkey [n, H, L] bool (planted rows / keys), layouts {(b, h): name}, rows {(b, h): [planted row]}.  Shared between tests: never
    modified."""
    n, H, _, _ = dims = dims_of(L, dh)
    d, M = H * dh, n * L
    rows = M + CANARY_ROWS
    q, k, v = R._rnd((rows, d), BF16, 40 + L, 1.2), R._rnd((rows, d), BF16, 41 + L, 1.2), R._rnd((rows, d), BF16, 42 + L, 1.2)
    do = R._rnd((rows, d), BF16, 43 + L)
    prow, pkey = torch.zeros(n, H, L, dtype=torch.bool), torch.zeros(n, H, L, dtype=torch.bool)
    layouts, prows = {}, {}
    # canary rows: entries of magnitude 64 with the draw's signs, keys that outscore every real key of a planted row of the last image
    sgn = lambda t: torch.where(t.double() < 0, -CANARY_MAG, CANARY_MAG).to(BF16)   # noqa: E731
    for t in (q, v, do):
        t[M:] = sgn(t[M:])
    k.view(rows, H, dh)[M:, :, 0] = sign_of(n - 1) * KC[dh]
    if family == 'planted':
        q4, k4, v4, do4 = (t[:M].view(n, L, H, dh) for t in (q, k, v, do))
        q4[..., 0] = 0
        k4[..., 0] = 0
        for b in range(n):
            s = sign_of(b)
            for h in range(H):
                lay = layouts[(b, h)] = layout_of(b, h, H)
                top = None
                if lay == 'first':
                    k4[b, 0, h, 0] = s * KD[dh]
                elif lay == 'last':
                    k4[b, L - 1, h, 0] = s * BETA
                elif lay == 'pair':
                    top, low = pair_keys(L, b)
                    k4[b, top, h, 0] = s * BETA
                    if low is not None:
                        k4[b, low, h, :] = k4[b, top, h, :]
                        k4[b, low, h, 0] = s * beta2(dh)
                        v4[b, low, h, :] = (-0.5 * v4[b, top, h, :].double()).to(BF16)
                elif lay in ('deep', 'high'):
                    k4[b, :, h, 0] = s * KD[dh] * (-1.0 if lay == 'deep' else 1.0)
                prows[(b, h)] = [] if lay == 'none' else planted_row_numbers(L, lay)
                for r in prows[(b, h)]:
                    q4[b, r, h, 1:] = (q4[b, r, h, 1:].double() * 0.25).to(BF16)
                    q4[b, r, h, 0] = s * A
                    prow[b, h, r] = True
                    if top is not None:
                        vsign = torch.where(v4[b, top, h, :] < 0, -1.0, 1.0).double()
                        do4[b, r, h, :] = (do4[b, r, h, :].double().abs() * vsign * DO_SCALE).to(BF16)
            # the keys image b - 1 would read past its ragged end
            if b > 0:
                k4[b, :neighbour_canaries(L), :, 0] = sign_of(b - 1) * KC[dh]
        pkey = k4[..., 0].transpose(1, 2) != 0
    return dict(L=L, dh=dh, family=family, dims=dims, q=q, k=k, v=v, do=do, prow=prow, pkey=pkey.clone(), layouts=layouts, rows=prows)


def real(c, t):
    """the first n L rows of an operand: what the kernels are handed"""
    n, H, L, dh = c['dims']
    return t[:n * L]


def scores2(c):
    """fp64 scores in log2 units [n, H, L, L + 32]: every row of an image against its own keys and the 32 rows behind them (the keys an
    over-read of image b reaches: the next image's first rows, or the canary rows)"""
    n, H, L, dh = c['dims']
    q4 = real(c, c['q']).double().view(n, L, H, dh).transpose(1, 2)
    k_all = c['k'].double().view(-1, H, dh)
    out = []
    for b in range(n):
        kb = k_all[b * L:b * L + L + CANARY_ROWS].transpose(0, 1)        # [H, L + 32, dh]
        out.append(q4[b] @ kb.transpose(-1, -2))
    return torch.stack(out) * (LOG2E / math.sqrt(dh))


# ----------------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------------
def _dims5(c):
    n, H, L, dh = c['dims']
    return n, H, L, L, dh


@functools.lru_cache(maxsize=None)
def reference(L, dh, family):
    """attn_dropout_ref.reference without bias or dropout -> o, lse2 [n, H, L], dq, dk, dv (fp64; shared, never modified)"""
    c = make_case(L, dh, family)
    return R.reference(*(real(c, c[t]) for t in ('q', 'k', 'v', 'do')), None, None, 0.0, _dims5(c))


def emulation(L, dh, family):
    """attn_dropout_ref.emulate with bf16 roundings at the kernels' rounding sites -> o, dq, dk, dv"""
    c = make_case(L, dh, family)
    return R.emulate(*(real(c, c[t]) for t in ('q', 'k', 'v', 'do')), None, None, 0.0, _dims5(c), R.rounder(BF16), torch.float64)


def lse2_fp32(c):
    """the kernel's formula for lse2 in fp32 arithmetic: m c + log2(sum exp2(s c - m c)) -> [n, H, L] fp32"""
    n, H, L, dh = c['dims']
    q4, k4 = (real(c, c[t]).float().view(n, L, H, dh).transpose(1, 2) for t in ('q', 'k'))
    s = q4 @ k4.transpose(-1, -2)
    cc = torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    mc = -s.max(-1, keepdim=True).values * cc
    l = torch.exp2(s * cc + mc).sum(-1)
    return -mc[..., 0] + torch.log2(l)


# ----------------------------------------------------------------------------------------------------------------------
# figures
# ----------------------------------------------------------------------------------------------------------------------
def _head_max(ref, n, L, H, dh):
    """[n L, H dh] -> max |ref| per (image, head) [n, H]"""
    return ref.abs().view(n, L, H, dh).amax(-1).permute(0, 2, 1).amax(-1)


def _set_elem(got, ref, sets, n, L, H, dh, zero_scale):
    """got / ref [n L, H dh] fp64; sets {tag: [n, H, L] bool} -> {tag: (worst over (image, head) of max |got - ref| over the set's rows
    / max |ref| over the (image, head), where)}; an empty set gives no entry.  zero_scale [n, H]: the scale of an (image, head) whose
    reference is identically zero (dq and dk at L = 1: dv's)"""
    diff = torch.nan_to_num((got - ref).abs(), nan=math.inf).view(n, L, H, dh).amax(-1).permute(0, 2, 1)      # [n, H, L]
    scale = _head_max(ref, n, L, H, dh)
    scale = torch.where(scale == 0, zero_scale, scale).clamp_min(1e-300)
    out = {}
    for tag, s in sets.items():
        if not bool(s.any()):
            continue
        e = torch.where(s, diff, torch.zeros((), dtype=diff.dtype)).amax(-1) / scale
        i = int(e.argmax())
        out[tag] = (float(e.view(-1)[i]), f'b={i // H}, head={i % H}')
    return out


def figures(c, got, ref, slice_bar, lse=True):
    """every figure of one point as {label: (value, bar)}; a figure holds when value <= bar.  got / ref: (o, lse2, dq, dk, dv), the
    tensors [n L, H dh], lse2 [n, H, L]."""
    n, H, L, dh = c['dims']
    o, lse2, dq, dk, dv = (t.detach().double().cpu() for t in got)
    o_r, lse_r, dq_r, dk_r, dv_r = ref
    fig = {}
    finite = all(bool(torch.isfinite(t).all()) for t in (o, lse2, dq, dk, dv))
    fig['not finite'] = (0.0 if finite else math.inf, 0.0)
    for tag, g, r in (('o', o, o_r), ('dq', dq, dq_r), ('dk', dk, dk_r), ('dv', dv, dv_r)):
        # a reference that is identically zero (dq and dk at L = 1) is measured on dv's scale
        zero = float(r.abs().max()) == 0.0
        res = S.compare(tag, g.reshape(n, L, H * dh), r.reshape(n, L, H * dh), 'act', heads=H, ref_norm=float(dv_r.norm()) if zero else None,
                        row_block=BLOCK)
        fig[f'slice/{res.where}'] = (res.err if res.finite else math.inf, slice_bar)
    prow, pkey = c['prow'], c['pkey']
    zs = _head_max(dv_r, n, L, H, dh)
    for tag, g, r, pl, bar in (('o', o, o_r, prow, TOL), ('dq', dq, dq_r, prow, 2 * TOL), ('dk', dk, dk_r, pkey, 2 * TOL),
                               ('dv', dv, dv_r, pkey, 2 * TOL)):
        for st, (val, where) in _set_elem(g, r, {'planted': pl, 'other': ~pl}, n, L, H, dh, zs).items():
            fig[f'elem/{tag} {st} [{where}]'] = (val, bar)
    if lse:
        err = torch.nan_to_num((lse2 - lse_r).abs(), nan=math.inf)
        for st, s in (('planted', prow), ('other', ~prow)):
            if bool(s.any()):
                num = torch.where(s, err, torch.zeros((), dtype=err.dtype)).amax(-1)
                den = torch.where(s, lse_r.abs(), torch.zeros((), dtype=err.dtype)).amax(-1).clamp_min(1.0)
                fig[f'lse2 {st}'] = (float((num / den).max()), LSE_BAR)
    if L == 1:      # one key: P = 1, dS = 0
        do = real(c, c['do']).double()
        for tag, t in (('dq = 0', dq), ('dk = 0', dk), ('dv = dO', dv - do)):
            fig[f'L1/{tag}'] = (float(torch.nan_to_num(t, nan=math.inf).abs().max()), 0.0)
    deep = torch.zeros(n, H, L, dtype=torch.bool)
    for (b, h), lay in c['layouts'].items():
        deep[b, h] = lay == 'deep'
    if bool(deep.any()):
        for tag, g, r in (('dk', dk, dk_r), ('dv', dv, dv_r)):
            val, where = _set_elem(g, r, {'deep': deep}, n, L, H, dh, zs)['deep']
            fig[f'deep/{tag} [{where}]'] = (val, 2 * TOL)
    return fig


def failing(fig):
    return [label for label, (val, bar) in fig.items() if not val <= bar]


def worst_slice(fig):
    return max(v for label, (v, _) in fig.items() if label.startswith('slice/'))


# ----------------------------------------------------------------------------------------------------------------------
# fault runners: the fp64 reference with one deliberate defect -> (o, lse2, dq, dk, dv)
# ----------------------------------------------------------------------------------------------------------------------
def key_mask_off_by_one(q, k, v, do, n, H, L, dh, images=None):
    """the reference with the key mask key > L on operands of at least n L + 1 rows: image b (every image, or those of ``images``)
    takes the row behind it as a key, in the forward and in both phases of the backward; that key's dk / dv row is not stored"""
    outs = []
    for b in range(n):
        extra = 1 if images is None or b in images else 0
        rq, rk = slice(b * L, (b + 1) * L), slice(b * L, (b + 1) * L + extra)
        o, lse2, dq, dk, dv = R.reference(q[rq], k[rk], v[rk], do[rq], None, None, 0.0, (1, H, L, L + extra, dh))
        outs.append((o, lse2, dq, dk[:L], dv[:L]))
    return tuple(torch.cat(t, 0) for t in zip(*outs))


def fault_key_mask_off_by_one(c):
    """1. the key mask is key > L: the row behind image b is image b + 1's first row, or the first canary row"""
    return key_mask_off_by_one(c['q'], c['k'], c['v'], c['do'], *c['dims'])


def fault_max_of_one_half_wave(c):
    """2. the forward's row maximum is not exchanged between the half-waves: it is taken over the keys with 4h = 4 (bit 2 of the key
    index set) only, in fp32 as the kernel computes it.  A row whose top key sits in the other half-wave, 128 units or more above,
    overflows."""
    n, H, L, dh = c['dims']
    o_r, lse_r, dq, dk, dv = reference(c['L'], c['dh'], c['family'])
    q4, k4, v4 = (real(c, c[t]).float().view(n, L, H, dh).transpose(1, 2) for t in ('q', 'k', 'v'))
    s = (q4 @ k4.transpose(-1, -2)) * (LOG2E / math.sqrt(dh))
    half = (torch.arange(L) & 4) != 0
    if not bool(half.any()):
        half[:] = True
    m = s[..., half].max(-1, keepdim=True).values
    e = torch.exp2(s - m)
    l = e.sum(-1, keepdim=True)
    o = (e @ v4) / l
    lse2 = (m + torch.log2(l))[..., 0]
    return R._flat(o, n, L, H, dh).double(), lse2.double(), dq, dk, dv


def fault_padded_lanes_summed(c):
    """3. the key-stationary phase adds its padded key lanes into the last real key: a padded lane holds P = exp2(0 - lse2) (fp32: inf
    at lse2 <= -128) and dS = P (0 - delta)"""
    n, H, L, dh = c['dims']
    o, lse2, dq, dk, dv = reference(c['L'], c['dh'], c['family'])
    npad = nblocks(L) * BLOCK - L
    if npad == 0:
        return o, lse2, dq, dk, dv
    q4, do4 = (real(c, c[t]).float().view(n, L, H, dh).transpose(1, 2) for t in ('q', 'do'))      # [n, H, L, dh]
    o4 = R._heads(o, n, L, H, dh).to(BF16).float()
    delta = (o4 * do4).sum(-1)
    P = torch.exp2(-lse2.float())                                                                  # [n, H, L]
    dS = P * (0.0 - delta)
    add_dv = npad * (P[..., None] * do4).sum(2)                                                    # [n, H, dh]
    add_dk = npad * (dS[..., None] * q4).sum(2) / math.sqrt(dh)
    dk4, dv4 = dk.clone().view(n, L, H, dh), dv.clone().view(n, L, H, dh)
    dk4[:, L - 1] += add_dk.double()
    dv4[:, L - 1] += add_dv.double()
    return o, lse2, dq, dk4.view(n * L, H * dh), dv4.view(n * L, H * dh)


def fault_second_trip_lse(c):
    """4. the forward's second trip (blocks 4 and above) writes the lse2 of the block four earlier"""
    o, lse2, dq, dk, dv = reference(c['L'], c['dh'], c['family'])
    L = c['L']
    assert L > 4 * BLOCK
    lse2 = lse2.clone()
    lse2[..., 4 * BLOCK:] = lse2[..., :L - 4 * BLOCK]
    return o, lse2, dq, dk, dv


def fault_dk_heads_exchanged(c):
    """5. the column groups of heads 0 and 1 are exchanged in dk"""
    n, H, L, dh = c['dims']
    o, lse2, dq, dk, dv = reference(c['L'], c['dh'], c['family'])
    dk = dk.clone()
    dk[:, :dh], dk[:, dh:2 * dh] = dk[:, dh:2 * dh].clone(), dk[:, :dh].clone()
    return o, lse2, dq, dk, dv


def fault_dq_last_block_left_out(c):
    """6. with eight blocks the eighth wave never runs the query-stationary phase: dq of rows 224 and above is not computed"""
    n, H, L, dh = c['dims']
    assert nblocks(L) == 8
    o, lse2, dq, dk, dv = reference(c['L'], c['dh'], c['family'])
    dq4 = dq.clone().view(n, L, H * dh)
    dq4[:, 7 * BLOCK:] = 0
    return o, lse2, dq4.view(n * L, H * dh), dk, dv
