"""Slice-wise comparison of a device result with a high-precision reference (plain torch, runs on any device).

A whole-tensor error bar averages a wrong head, tile or video away: 5 % wrong on one head of eight moves the norm-wise error of an
[in_proj] gradient by ~0.05 * sqrt(1/24).  Here every tensor is cut into a fixed partition and each slice s is held to its own
relative error

    err_s = ||T_s - R_s|| / max(||R_s||, floor_s),    floor_s = 1e-3 * ||R|| * sqrt(n_s / n)

(the floor keeps slices whose reference is ~0 from dividing noise by noise).  The partitions follow the way the kernels tile the
work:

    activations [B, L, D] / [B, N, D] and their gradients   (video, 128-row tile, head's column group)
    [B, D] vectors (the sketch token's gradient)             (video, head's column group)
    in_proj_weight / in_proj_bias gradients                  (q / k / v, head) row blocks
    out_proj.weight gradient                                 head column groups
    fc1 / fc2 gradients                                      128-row / 128-column blocks
    LayerNorm gamma / beta and other [D] vectors             the whole vector, plus 32-wide chunks

Beside the slices: the worst element against the tensor's largest reference entry, and that every value is finite.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

FLOOR = 1e-3
TILE = 128      # rows of an activation tile; rows / columns of an fc1 / fc2 block
CHUNK = 32      # width of a [D]-vector chunk


@dataclass
class SliceResult:
    err: float          # worst slice error
    where: str          # that slice, e.g. 'dK[b=5, head=3, rows 768:896]'
    elem: float         # worst |T - R| over max |R|
    finite: bool

    def __str__(self):
        return f'{self.where}: slice {self.err:.2e}, element {self.elem:.2e}' + ('' if self.finite else ', NOT FINITE')


def _block_sq(x, rb, cb):
    """x [B, R, C] -> per-block sums of squares [B, ceil(R / rb), ceil(C / cb)] (tail blocks padded with zeros)."""
    B, R, C = x.shape
    nr, nc = -(-R // rb), -(-C // cb)
    if nr * rb != R or nc * cb != C:
        x = torch.nn.functional.pad(x, (0, nc * cb - C, 0, nr * rb - R))
    return x.pow(2).view(B, nr, rb, nc, cb).sum(dim=(2, 4))


def _block_counts(B, R, C, rb, cb):
    r = torch.tensor([min(rb, R - i * rb) for i in range(-(-R // rb))], dtype=torch.float64)
    c = torch.tensor([min(cb, C - j * cb) for j in range(-(-C // cb))], dtype=torch.float64)
    return (r[:, None] * c[None, :]).expand(B, -1, -1)


def _worst(diff, ref, rb, cb, name_of, ref_norm):
    """diff / ref as [B, R, C] float64 -> (worst error, its name) over the (rb x cb) blocks."""
    B, R, C = ref.shape
    dn = _block_sq(diff, rb, cb).sqrt().cpu()
    rn = _block_sq(ref, rb, cb).sqrt().cpu()
    n = _block_counts(B, R, C, rb, cb)
    floor = FLOOR * ref_norm * (n / (B * R * C)).sqrt()
    err = dn / torch.maximum(rn, floor).clamp_min(1e-300)
    i = int(err.argmax())
    b, rem = divmod(i, err.shape[1] * err.shape[2])
    r, c = divmod(rem, err.shape[2])
    return float(err.view(-1)[i]), name_of(b, r, c)


def _span(i, blk, n):
    return f'{i * blk}:{min((i + 1) * blk, n)}'


def _partitions(kind, shape, heads, row_block=TILE):
    """-> [(view shape [B, R, C], row block, column block, namer(b, r, c))] for one tensor kind."""
    if kind == 'act':                      # [B, L, D]
        B, L, D = shape
        dh = D // heads
        return [((B, L, D), row_block, dh, lambda b, r, c: f'b={b}, head={c}, rows {_span(r, row_block, L)}')]
    if kind == 'bd':                       # [B, D]
        B, D = shape
        dh = D // heads
        return [((B, 1, D), 1, dh, lambda b, r, c: f'b={b}, head={c}')]
    if kind in ('in_proj_weight', 'in_proj_bias'):   # [3D, D] / [3D]
        D3 = shape[0]
        C = shape[1] if len(shape) == 2 else 1
        dh = D3 // 3 // heads
        return [((1, D3, C), dh, C, lambda b, r, c: f'{"qkv"[r // heads]}, head={r % heads}')]
    if kind == 'out_proj_weight':          # [D, D]: input columns = heads
        D = shape[0]
        dh = shape[1] // heads
        return [((1, D, shape[1]), D, dh, lambda b, r, c: f'head={c} columns')]
    if kind == 'row_blocks':               # fc1.weight [F, D] / fc1.bias [F]
        F = shape[0]
        C = shape[1] if len(shape) == 2 else 1
        return [((1, F, C), TILE, C, lambda b, r, c: f'rows {_span(r, TILE, F)}')]
    if kind == 'col_blocks':               # fc2.weight [D, F]
        D, F = shape
        return [((1, D, F), D, TILE, lambda b, r, c: f'columns {_span(c, TILE, F)}')]
    if kind == 'vector':                   # [D]: whole + 32-wide chunks
        D = shape[0]
        return [((1, 1, D), 1, D, lambda b, r, c: 'whole'),
                ((1, 1, D), 1, CHUNK, lambda b, r, c: f'[{_span(c, CHUNK, D)}]')]
    raise ValueError(kind)


def param_kind(name):
    """the partition of a parameter gradient, from its state-dict name."""
    if name.endswith(('in_proj_weight', 'in_proj_bias')):
        return name.rsplit('.', 1)[-1]
    if name.endswith('out_proj.weight'):
        return 'out_proj_weight'
    if name.endswith(('fc1.weight', 'fc1.bias')):
        return 'row_blocks'
    if name.endswith('fc2.weight'):
        return 'col_blocks'
    return 'vector'


def compare(label, got, ref, kind, heads, ref_norm=None, row_block=TILE):
    """SliceResult of ``got`` against ``ref`` on the partition ``kind`` ('act', 'bd', a param_kind).  ``ref_norm`` replaces ||R|| in
    the floor where the reference is exactly zero (the norm of a related gradient sets the scale).  ``row_block``: the rows of an
    'act' tile (the short-sequence attention kernels work in 32-row blocks)."""
    ref = ref.detach().to(torch.float64)
    got = got.detach().to(device=ref.device, dtype=torch.float64)
    assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return SliceResult(math.inf, f'{label}[not finite]', math.inf, False)
    diff = got - ref
    ref_norm = float(ref.norm()) if ref_norm is None else ref_norm
    rmax = float(ref.abs().max())
    elem = float(diff.abs().max()) / max(rmax, 1e-300)
    worst, where = -1.0, ''
    for vshape, rb, cb, namer in _partitions(kind, tuple(ref.shape), heads, row_block):
        e, w = _worst(diff.reshape(vshape), ref.reshape(vshape), rb, cb, namer, ref_norm)
        if e > worst:
            worst, where = e, w
    return SliceResult(worst, f'{label}[{where}]', elem, True)
