"""Host-side operators of the SVOL hot path: thin tensor wrappers over the C-ABI
(libsvol_hip.so), no autograd.  The ``torch.autograd.Function`` s that compose them are in
``layers``, the weight cache and the gradient sinks in ``params``; both import this module,
which imports neither.

PyTorch here is plumbing only: device memory and the current HIP stream.  Every arithmetic
op on the hot path is a hand-written gfx950 kernel behind ``include/svol_hip.h``; there is
no CPU or eager fallback — a non-CUDA tensor or a missing library raises.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional

import torch

from . import _lib, wgrad

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID, ACT_RELU_RES, ACT_GELU_D = 0, 1, 2, 3, 4, 5
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}   # SVOL_F32 / SVOL_BF16 / SVOL_F16


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise _lib.SvolHipError(f'unsupported dtype {t.dtype}')


# the raw handle of torch's CURRENT stream.  torch.cuda.current_stream() costs 5-8 us of Python per call (device-index
# resolution through is_available / os.getenv) and every C-ABI call needs it: ~3 ms of host time per training step; the two
# private C entry points below are what it wraps (0.3 us).
_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_CUR_DEVICE = getattr(torch._C, '_cuda_getDevice', None)


def _stream() -> int:
    if _RAW_STREAM is not None and _CUR_DEVICE is not None:
        return _RAW_STREAM(_CUR_DEVICE())
    return torch.cuda.current_stream().cuda_stream


_STREAM_OBJS = {}


def _current_stream_obj():
    """torch.cuda.current_stream() through a cache keyed by the raw handle (same reason as _stream)."""
    if _RAW_STREAM is None or _CUR_DEVICE is None:
        return torch.cuda.current_stream()
    key = (_CUR_DEVICE(), _RAW_STREAM(_CUR_DEVICE()))
    obj = _STREAM_OBJS.get(key)
    if obj is None:
        obj = _STREAM_OBJS[key] = torch.cuda.current_stream()
    return obj


def _ptr(t: Optional[torch.Tensor]) -> int:
    if t is None:
        return 0
    if not t.is_cuda:
        raise _lib.SvolHipError('svol_amd ops need device tensors (no CPU fallback)')
    return t.data_ptr()


class KernelTimer:
    """Optional per-kernel timing with HIP events recorded on the launch stream (the stream every
    C-ABI call is enqueued on = torch's current stream).  Disabled by default (zero overhead);
    bench.py enables it for the dominant kernels to report the live roofline numbers."""

    def __init__(self):
        self.enabled = False
        self.names = set()
        self.records = {}

    def enable(self, names):
        self.enabled, self.names, self.records = True, set(names), {}

    def disable(self):
        self.enabled = False

    def clear(self):
        self.records = {}

    def start(self, name, meta=None):
        if not self.enabled or name not in self.names:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return (name, meta, e0, e1)

    def stop(self, tok):
        if tok is None:
            return
        name, meta, e0, e1 = tok
        e1.record()
        self.records.setdefault((name, meta), []).append((e0, e1))

    def summary(self):
        """{(name, meta): (launches, mean_ms)} — call after torch.cuda.synchronize()."""
        out = {}
        for k, evs in self.records.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[k] = (len(ms), sum(ms) / len(ms))
        return out


timer = KernelTimer()


# ----------------------------------------------------------------------------
# raw wrappers (no autograd)
# ----------------------------------------------------------------------------
def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.check(_lib.lib().svol_cast(_ptr(x), _dt(x), _ptr(out), _DT[dtype], x.numel(), _stream()), 'svol_cast')
    return out


def cast_transpose(w: torch.Tensor, dtype: torch.dtype, want: bool = True, want_t: bool = True):
    """fp32 [R,C] -> (dtype [R,C] or None, dtype [C,R] or None)."""
    assert w.dtype == torch.float32 and w.dim() == 2
    w = w.contiguous()
    R, C = w.shape
    d = torch.empty((R, C), dtype=dtype, device=w.device) if want else None
    dT = torch.empty((C, R), dtype=dtype, device=w.device) if want_t else None
    _lib.check(_lib.lib().svol_cast_transpose(_ptr(w), _ptr(d), _ptr(dT), _DT[dtype], R, C, _stream()),
               'svol_cast_transpose')
    return d, dT


def gemm_nt(A, B, bias=None, act=ACT_NONE, residual=None, want_pre=False, out=None, out_f32=False, colscale=None, pre_out=None):
    """out[M,N] = act(A[M,K] @ B[N,K]^T + bias) + residual.  A/B/out/residual may be column slices
    of wider row-major buffers (stride(0) is the leading dimension).  out_f32: `out` and `residual`
    are fp32 (the fp32 residual stream) whatever the operand dtype."""
    assert A.dim() == 2 and B.dim() == 2 and A.stride(1) == 1 and B.stride(1) == 1
    M, K = A.shape
    N = B.shape[0]
    cdt = torch.float32 if out_f32 else A.dtype
    if out is None:
        out = torch.empty((M, N), dtype=cdt, device=A.device)
    assert out.dtype == cdt and (residual is None or residual.dtype == cdt)
    pre = (pre_out if pre_out is not None else torch.empty((M, N), dtype=A.dtype, device=A.device)) if want_pre else None
    rc = _lib.lib().svol_gemm_nt(_ptr(A), A.stride(0), 0, 0, _ptr(B), B.stride(0), _ptr(out), out.stride(0),
                                 _ptr(bias), _ptr(colscale), act, _ptr(pre), pre.stride(0) if pre is not None else 0,
                                 _ptr(residual),
                                 residual.stride(0) if residual is not None else 0, 1 if out_f32 else 0, M, N, K,
                                 _dt(A), _stream())
    _lib.check(rc, 'svol_gemm_nt')
    return (out, pre) if want_pre else out


def gemm_nt_split(A, W_hilo, bias=None, out=None):
    """out[M,N] (bf16) = A[M,K] @ (W_hi + W_lo)[N,K]^T + bias with W_hilo [N, 2K] = [hi | lo] (the weight cache's get_split): one
    K-concatenated product, [A | A] is never materialised."""
    assert A.dim() == 2 and W_hilo.dim() == 2 and A.stride(1) == 1 and W_hilo.stride(1) == 1 and A.dtype == torch.bfloat16
    M, K = A.shape
    N = W_hilo.shape[0]
    assert W_hilo.shape[1] == 2 * K
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    rc = _lib.lib().svol_gemm_nt_split(_ptr(A), A.stride(0), _ptr(W_hilo), W_hilo.stride(0), _ptr(out), out.stride(0), _ptr(bias),
                                       M, N, K, _stream())
    _lib.check(rc, 'svol_gemm_nt_split')
    return out


def gemm_tn(A, B, out=None, colsum=None, stream=None):
    """out[N,K] (fp32) += A[Mc,N]^T @ B[Mc,K]; a fresh zeroed `out` is allocated when not given.
    colsum (fp32 [N], zeroed by the caller) += column sums of A (bias gradient, fused).  stream: raw handle (default: current)."""
    assert A.dim() == 2 and B.dim() == 2 and A.shape[0] == B.shape[0]
    assert A.stride(1) == 1 and B.stride(1) == 1
    Mc, N = A.shape
    K = B.shape[1]
    if out is None:
        out = torch.zeros((N, K), dtype=torch.float32, device=A.device)
    rc = _lib.lib().svol_gemm_tn(_ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), out.stride(0), _ptr(colsum),
                                 Mc, N, K, _dt(A), _stream() if stream is None else stream)
    _lib.check(rc, 'svol_gemm_tn')
    return out


def gemm_tn_grouped(problems, stream=None):
    """several gemm_tn problems of one element type in one launch: problems = [(A, B, out, colsum | None), ...], out / colsum fp32,
    accumulated into (svol_gemm_tn_grouped)."""
    n = len(problems)
    arr = (_lib.TnProblem * n)()
    dt = None
    for i, (A, B, out, cs) in enumerate(problems):
        assert A.dim() == 2 and B.dim() == 2 and A.shape[0] == B.shape[0] and A.stride(1) == 1 and B.stride(1) == 1 and A.dtype == B.dtype
        assert dt is None or dt == A.dtype
        dt = A.dtype
        arr[i] = _lib.TnProblem(_ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), out.stride(0), _ptr(cs), A.shape[0], A.shape[1],
                                B.shape[1])
    rc = _lib.lib().svol_gemm_tn_grouped(ctypes.cast(arr, ctypes.c_void_p), n, _DT[dt], _stream() if stream is None else stream)
    _lib.check(rc, 'svol_gemm_tn_grouped')


def gemm_tn_sink(A, B, out, colsum=None):
    """gemm_tn into a persistent gradient bucket view, off the critical path (svol_amd.wgrad).  `out` / `colsum` must be sink
    views: nothing on the current stream may read them before BucketedGradAllReduce.finish()."""
    if not wgrad.issue(lambda ws: gemm_tn(A, B, out=out, colsum=colsum, stream=ws.cuda_stream), (A, B), _current_stream_obj()):
        gemm_tn(A, B, out=out, colsum=colsum)
    return out


def gemm_nt_dact(A, B, aux, act, want_colsum=True, colsum_out=None):
    """(A @ B^T) * act'(aux), and its column sums (fp32, accumulated into colsum_out when given) — fused MLP
    backward step.  act = ACT_GELU (aux = saved pre-activation) or ACT_RELU (aux = saved post-activation)."""
    M, K = A.shape
    N = B.shape[0]
    out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    cs = colsum_out
    if cs is None and want_colsum:
        cs = torch.zeros((N,), dtype=torch.float32, device=A.device)
    rc = _lib.lib().svol_gemm_nt_dact(_ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), out.stride(0), _ptr(aux),
                                      aux.stride(0), act, _ptr(cs), M, N, K, _dt(A), _stream())
    _lib.check(rc, 'svol_gemm_nt_dact')
    return out, cs


def gemm_nt_dgelu(A, B, pre, want_colsum=True, colsum_out=None):
    return gemm_nt_dact(A, B, pre, ACT_GELU, want_colsum, colsum_out)


def colsum(X, out=None):
    assert X.dim() == 2 and X.stride(1) == 1
    M, N = X.shape
    if out is None:
        out = torch.zeros((N,), dtype=torch.float32, device=X.device)
    _lib.check(_lib.lib().svol_colsum(_ptr(X), X.stride(0), _ptr(out), M, N, _dt(X), _stream()), 'svol_colsum')
    return out


def act_bwd(dy, aux, act):
    dy = dy.contiguous()
    aux = aux.contiguous()
    out = torch.empty_like(dy)
    _lib.check(_lib.lib().svol_act_bwd(_ptr(dy), _ptr(aux), _ptr(out), act, dy.numel(), _dt(dy), _stream()),
               'svol_act_bwd')
    return out


def layernorm_fwd(x, gamma, beta, dtype, pos=None, p=0.0, seed=0, want32=False, want_t=True, seed_dev=None):
    """x [M,D] (fp32 residual stream or `dtype`) -> (y32 | None, y | None, ypos | None, mean, rstd)."""
    x = x.contiguous()
    M, D = x.shape
    x_f32 = 1 if (x.dtype == torch.float32 and dtype != torch.float32) else 0
    assert x.dtype in (dtype, torch.float32)
    y32 = torch.empty((M, D), dtype=torch.float32, device=x.device) if want32 else None
    y = torch.empty((M, D), dtype=dtype, device=x.device) if want_t else None
    ypos = torch.empty((M, D), dtype=dtype, device=x.device) if pos is not None else None
    mean = torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device)
    if pos is not None:
        pos = pos.contiguous()
        assert pos.dtype == dtype and pos.shape[-1] == D
    rc = _lib.lib().svol_layernorm_fwd(_ptr(x), x_f32, _ptr(gamma), _ptr(beta), _ptr(y32), _ptr(y), _ptr(ypos),
                                       _ptr(pos), pos.numel() // D if pos is not None else 0, _ptr(mean), _ptr(rstd),
                                       M, D, float(p), int(seed), _ptr(seed_dev), _DT[dtype], _stream())
    _lib.check(rc, 'svol_layernorm_fwd')
    return y32, y, ypos, mean, rstd


def layernorm_bwd(dy32, dy, dy2, x, gamma, mean, rstd, dtype, p=0.0, seed=0, want32=False, want_t=True,
                  want_colsum=False, seed_dev=None, dg_out=None, db_out=None, cs_out=None):
    """LN backward; any of dy32 (fp32) / dy / dy2 (`dtype`) may be None.  Returns (dx32|None, dx|None, dg, db)
    (+ the column sums of dx when want_colsum: the bias gradient of the Linear feeding this LN)."""
    M, D = x.shape
    x_f32 = 1 if (x.dtype == torch.float32 and dtype != torch.float32) else 0
    cont = lambda t: None if t is None else t.reshape(M, D).contiguous()
    dy32, dy, dy2 = cont(dy32), cont(dy), cont(dy2)
    assert dy32 is None or dy32.dtype == torch.float32
    assert (dy is None or dy.dtype == dtype) and (dy2 is None or dy2.dtype == dtype)
    dx32 = torch.empty((M, D), dtype=torch.float32, device=x.device) if want32 else None
    dx = torch.empty((M, D), dtype=dtype, device=x.device) if want_t else None
    dg, db, cs = dg_out, db_out, (cs_out if want_colsum else None)  # accumulated into (gradient sinks) when given
    if dg is None or db is None or (want_colsum and cs is None):
        red = torch.zeros((3, D), dtype=torch.float32, device=x.device)  # one memset for dgamma | dbeta | colsum(dx)
        dg = red[0] if dg is None else dg
        db = red[1] if db is None else db
        cs = (red[2] if cs is None else cs) if want_colsum else None
    rc = _lib.lib().svol_layernorm_bwd(_ptr(dy32), _ptr(dy), _ptr(dy2), _ptr(x), x_f32, _ptr(gamma), _ptr(mean),
                                       _ptr(rstd), _ptr(dx32), _ptr(dx), _ptr(dg), _ptr(db), _ptr(cs), M, D, float(p),
                                       int(seed), _ptr(seed_dev), _DT[dtype], _stream())
    _lib.check(rc, 'svol_layernorm_bwd')
    if want_colsum:
        return dx32, dx, dg, db, cs
    return dx32, dx, dg, db


def posenc_sine(mask_f32: torch.Tensor, D: int, dtype: torch.dtype) -> torch.Tensor:
    mask_f32 = mask_f32.contiguous()
    B, L = mask_f32.shape
    pos = torch.empty((B, L, D), dtype=dtype, device=mask_f32.device)
    _lib.check(_lib.lib().svol_posenc_sine(_ptr(mask_f32), _ptr(pos), B, L, D, _DT[dtype], _stream()),
               'svol_posenc_sine')
    return pos


def attn_ws_bytes(dtype, B, H, Lq, Lk, dh):
    """bytes of scratch the attention launches need: partial results of the key-split (few queries, many keys), the key-tile classes
    of the masked fast kernels, or the per-workgroup redo flags of the fast unmasked forward; 0 when the library needs none."""
    return max(int(_lib.lib().svol_attn_ws_bytes(B, H, Lq, Lk, dh)), 0) if dtype != torch.float32 else 0


def _attn_ws(q, B, H, Lq, Lk, dh):
    n = attn_ws_bytes(q.dtype, B, H, Lq, Lk, dh)
    return torch.empty((n // 4,), dtype=torch.float32, device=q.device) if n else None


def dropout(x, p, seed, out=None, seed_dev=None):
    """x * keep(seed, row, column) (0 or 1/(1-p)) over x viewed as [-1, x.shape[-1]]; out may be x (in place).  x contiguous.
    seed_dev: device int64 step counter or None — the mask is that of seed + (seed_dev[0] << 12) (svol_dropout_sd)."""
    assert x.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    args = (_ptr(x), _ptr(out), x.numel(), max(1, x.shape[-1] if x.dim() else 1), float(p), int(seed))
    if seed_dev is None:   # (the entry it always was: the launch sequence of a host-seeded step stays what it was)
        _lib.check(_lib.lib().svol_dropout(*args, _dt(x), _stream()), 'svol_dropout')
    else:
        _lib.check(_lib.lib().svol_dropout_sd(*args, _ptr(seed_dev), _dt(x), _stream()), 'svol_dropout_sd')
    return out


def dropout_add(t32, res32, p, seed, seed_dev=None):
    """res32 + dropout(t32), fp32, written over t32 (rows = t32.shape[-1] wide).  seed_dev: as in dropout."""
    assert t32.is_contiguous() and res32.is_contiguous() and t32.dtype == torch.float32 and res32.dtype == torch.float32
    args = (_ptr(t32), _ptr(res32), _ptr(t32), t32.numel(), max(1, t32.shape[-1]), float(p), int(seed))
    if seed_dev is None:
        _lib.check(_lib.lib().svol_dropout_add(*args, _stream()), 'svol_dropout_add')
    else:
        _lib.check(_lib.lib().svol_dropout_add_sd(*args, _ptr(seed_dev), _stream()), 'svol_dropout_add_sd')
    return t32


def _attn_drop(drop):
    """drop = None | (p, seed) | (p, seed, seed_dev) -> (p, seed, seed_dev) of the launch; p <= 0: no dropout"""
    if drop is None or drop[0] <= 0.0:
        return 0.0, 0, None
    return float(drop[0]), int(drop[1]), (drop[2] if len(drop) > 2 else None)


def attn_fwd(q, k, v, B, H, Lq, Lk, dh, kbias=None, premul=0.0, drop=None):
    """q/k/v: 2-D [B*L, >=H*dh] views (column slices allowed). Returns o [B*Lq, H*dh], lse2 [B,H,Lq].
    drop = (p, seed) or (p, seed, seed_dev): attention-probability dropout (None or p <= 0: none); seed_dev: device int64 step counter,
    the masks are those of seed + (seed_dev[0] << 12)."""
    o = torch.empty((B * Lq, H * dh), dtype=q.dtype, device=q.device)
    lse2 = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    ws = _attn_ws(q, B, H, Lq, Lk, dh)
    p, seed, seed_dev = _attn_drop(drop)
    wgrad.attn_forward(B * H * Lq * Lk)
    tok = timer.start('attn_fwd', (B, H, Lq, Lk, dh))
    args = (_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0), _ptr(lse2), _ptr(kbias), B, H, Lq, Lk,
            dh, 1.0 / math.sqrt(dh), float(premul), _ptr(ws), ws.numel() * 4 if ws is not None else 0, p, seed)
    if seed_dev is None:
        rc = _lib.lib().svol_attn_fwd_dropout(*args, _dt(q), _stream())
    else:
        rc = _lib.lib().svol_attn_fwd_dropout_sd(*args, _ptr(seed_dev), _dt(q), _stream())
    timer.stop(tok)
    _lib.check(rc, 'svol_attn_fwd')
    return o, lse2


def attn_bwd(q, k, v, o, do, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbias=None, premul=0.0, drop=None):
    """Writes dq/dk/dv (2-D views, column slices allowed)."""
    do = do if do.stride(1) == 1 else do.contiguous()
    wgrad.attn_backward(B * H * Lq * Lk)   # the queued weight-gradient GEMMs run beside this launch
    delta = torch.empty((3, B, H, Lq), dtype=torch.float32, device=q.device)  # delta | -lse2 pairs | -delta pairs (svol_hip.h)
    ws = _attn_ws(q, B, H, Lq, Lk, dh)
    p, seed, seed_dev = _attn_drop(drop)
    tok = timer.start('attn_bwd', (B, H, Lq, Lk, dh))
    args = (_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0), _ptr(do), do.stride(0), _ptr(lse2),
            _ptr(delta), _ptr(kbias), _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), B, H, Lq, Lk, dh,
            1.0 / math.sqrt(dh), float(premul), _ptr(ws), ws.numel() * 4 if ws is not None else 0, p, seed)
    if seed_dev is None:
        rc = _lib.lib().svol_attn_bwd_dropout(*args, _dt(q), _stream())
    else:
        rc = _lib.lib().svol_attn_bwd_dropout_sd(*args, _ptr(seed_dev), _dt(q), _stream())
    timer.stop(tok)
    _lib.check(rc, 'svol_attn_bwd')


def _h16_entry(name, t):
    """the entry point of a short-sequence / one-query attention call: fp16 tensors go through the ``_h16`` twin (the entries without
    the suffix refuse SVOL_F16), bf16 tensors keep the entry they always had"""
    name = name + '_h16' if t.dtype == torch.float16 else name
    return getattr(_lib.lib(), name), name


def attn_small_fwd(q, k, v, n, H, L, dh, want_lse=False):
    """short-sequence attention (L <= 256, bf16 or fp16): q/k/v 2-D [n*L, >= H*dh] views (column slices allowed).
    -> (o [n*L, H*dh], lse2 [n, H, L] fp32 with want_lse, else None)."""
    o = torch.empty((n * L, H * dh), dtype=q.dtype, device=q.device)
    args = (_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0))
    tail = (n, H, L, dh, 1.0 / math.sqrt(dh), _dt(q), _stream())
    if want_lse:
        lse2 = torch.empty((n, H, L), dtype=torch.float32, device=q.device)
        fn, name = _h16_entry('svol_attn_small_fwd_lse', q)
        _lib.check(fn(*args, _ptr(lse2), *tail), name)
        return o, lse2
    fn, name = _h16_entry('svol_attn_small_fwd', q)
    _lib.check(fn(*args, *tail), name)
    return o, None


def attn_small_bwd(q, k, v, o, do, lse2, n, H, L, dh, dq, dk, dv):
    """gradients of attn_small_fwd into dq / dk / dv (2-D views of q's dtype, column slices allowed)."""
    fn, name = _h16_entry('svol_attn_small_bwd', q)
    _lib.check(fn(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0), _ptr(do), do.stride(0), _ptr(lse2),
                  _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), n, H, L, dh, 1.0 / math.sqrt(dh), _dt(q), _stream()),
               name)


def attn_cls_fwd(q, k, v, n, H, L, dh):
    """one query row per image against all L <= 256 keys (bf16 or fp16 operands, fp32 arithmetic): q [n, H*dh], k / v 2-D [n*L, >= H*dh]
    views (column slices allowed) -> (o [n, H*dh] of q's dtype, lse2 [n, H] fp32, log2 units)."""
    o = torch.empty((n, H * dh), dtype=q.dtype, device=q.device)
    lse2 = torch.empty((n, H), dtype=torch.float32, device=q.device)
    fn, name = _h16_entry('svol_attn_cls_fwd', q)
    _lib.check(fn(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0), _ptr(lse2), n, H, L, dh,
                  1.0 / math.sqrt(dh), _dt(q), _stream()), name)
    return o, lse2


def attn_cls_bwd(q, k, v, o, do, lse2, n, H, L, dh, dq, dk, dv):
    """gradients of attn_cls_fwd into dq [n, H*dh] and dk / dv [n*L, H*dh] (2-D views of q's dtype, column slices allowed)."""
    fn, name = _h16_entry('svol_attn_cls_bwd', q)
    _lib.check(fn(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0), _ptr(do), do.stride(0), _ptr(lse2),
                  _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), n, H, L, dh, 1.0 / math.sqrt(dh), _dt(q), _stream()),
               name)


FEWKEYS_LMAX = 256   # keys of the many-queries / few-keys attention kernels (csrc/attn_fewkeys.hip)


def attn_fewkeys_ok(dtype, Lk, dh) -> bool:
    """whether svol_attn_fewkeys_fwd / _bwd take the shape: bf16 or fp16 operands, dh in {32, 64}, 1 <= Lk <= 256 (any Lq)"""
    return dtype in (torch.bfloat16, torch.float16) and dh in (32, 64) and 1 <= Lk <= FEWKEYS_LMAX


FEWKEYS_FASTER_LK32 = 197   # dh = 32: the largest key count at which the few-keys pair was measured faster than attn_fwd / attn_bwd


def attn_fewkeys_faster(Lk, dh) -> bool:
    """where the few-keys kernels were measured faster than the generic ones by more than the run-to-run spread
    (profiles/sketch_tokens.md: B = 8, H = 8, bf16 and fp16).  dh = 32: Lk = 49 (2.1 x backward, 1.6 x forward) and 197 (1.14 x /
    1.15 x), the margin shrinking with Lk, so key counts above 197 — not measured; at 256 the tuned 128-key kernels serve the generic
    path — stay on the generic kernels.  dh = 64: Lk = 98, 5 x backward and 1.3 x forward against the two-pass kernels that serve
    every key count at that width, so every Lk <= 256."""
    return dh == 64 or Lk <= FEWKEYS_FASTER_LK32


def attn_fewkeys_chunk(Lq: int) -> int:
    """queries a workgroup of the few-keys kernels walks: a function of Lq alone (256 * ceil(Lq / 2048): at most 8 chunks per
    (batch, head)); the backward's dK / dV partials are per chunk and are added in chunk order"""
    return int(_lib.lib().svol_attn_fewkeys_chunk_rows(int(Lq)))


def attn_fewkeys_ws_bytes(B, H, Lq, Lk, dh) -> int:
    return int(_lib.lib().svol_attn_fewkeys_ws_bytes(B, H, Lq, Lk, dh))


def attn_fewkeys_fwd(q, k, v, B, H, Lq, Lk, dh, kbias=None, premul=0.0):
    """attn_fwd's contract on the few-keys kernels (Lk <= 256, many queries): q/k/v 2-D [B*L, >= H*dh] views (column slices allowed)
    -> (o [B*Lq, H*dh], lse2 [B, H, Lq] fp32, log2 domain).  A shape outside attn_fewkeys_ok raises: the caller chooses the family."""
    o = torch.empty((B * Lq, H * dh), dtype=q.dtype, device=q.device)
    lse2 = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    wgrad.attn_forward(B * H * Lq * Lk)
    tok = timer.start('attn_fewkeys_fwd', (B, H, Lq, Lk, dh))
    rc = _lib.lib().svol_attn_fewkeys_fwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0), _ptr(lse2),
                                          _ptr(kbias), B, H, Lq, Lk, dh, 1.0 / math.sqrt(dh), float(premul), _dt(q), _stream())
    timer.stop(tok)
    _lib.check(rc, 'svol_attn_fewkeys_fwd')
    return o, lse2


def attn_fewkeys_bwd(q, k, v, o, do, lse2, B, H, Lq, Lk, dh, dq, dk, dv, kbias=None, premul=0.0):
    """gradients of attn_fewkeys_fwd into dq / dk / dv (2-D views, column slices allowed).  The fp32 scratch of the per-chunk dK / dV
    partials is a torch allocation; the sums have a fixed order (same bits every run)."""
    do = do if do.stride(1) == 1 else do.contiguous()
    wgrad.attn_backward(B * H * Lq * Lk)
    n = attn_fewkeys_ws_bytes(B, H, Lq, Lk, dh)
    ws = torch.empty((max(n, 4) // 4,), dtype=torch.float32, device=q.device)
    tok = timer.start('attn_fewkeys_bwd', (B, H, Lq, Lk, dh))
    rc = _lib.lib().svol_attn_fewkeys_bwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0), _ptr(do),
                                          do.stride(0), _ptr(lse2), _ptr(kbias), _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv),
                                          dv.stride(0), B, H, Lq, Lk, dh, 1.0 / math.sqrt(dh), float(premul), _ptr(ws), n, _dt(q), _stream())
    timer.stop(tok)
    _lib.check(rc, 'svol_attn_fewkeys_bwd')


def softmax_xent(logits, targets):
    """nn.CrossEntropyLoss() of fp32 logits [n, C] (a row-strided view is fine) and int64 targets [n] -> (loss [1] fp32 = the mean over
    rows, dlogits [n, C] = (softmax - onehot) / n, correct [1] int32 = top-1 hits).  C <= 1024."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32 and targets.dtype == torch.int64
    n, C = logits.shape
    targets = targets.contiguous()
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    correct = torch.empty((1,), dtype=torch.int32, device=logits.device)
    dlogits = torch.empty((n, C), dtype=torch.float32, device=logits.device)
    _lib.check(_lib.lib().svol_softmax_xent(_ptr(logits), logits.stride(0), _ptr(targets), _ptr(loss), _ptr(dlogits), dlogits.stride(0),
                                            _ptr(correct), n, C, _stream()), 'svol_softmax_xent')
    return loss, dlogits, correct


def im2col(x, N, H, W, C, kh, kw, stride, pad, dtype, strides=None, ldcols=None):
    """x: image batch addressed by element `strides` (sn, sh, sw, sc) — default NHWC contiguous — -> (cols [N*Ho*Wo, ldcols]
    in `dtype`, Ho, Wo); column order (ky, kx, c), zero padding outside the image and in columns >= kh*kw*C."""
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    K = kh * kw * C
    ldcols = K if ldcols is None else ldcols
    sn, sh, sw, sc = strides if strides is not None else (H * W * C, W * C, C, 1)
    cols = torch.empty((N * Ho * Wo, ldcols), dtype=dtype, device=x.device)
    rc = _lib.lib().svol_im2col(_ptr(x), sn, sh, sw, sc, _dt(x), _ptr(cols), ldcols, N, H, W, C, kh, kw, stride, pad, _DT[dtype],
                                _stream())
    _lib.check(rc, 'svol_im2col')
    return cols, Ho, Wo


def ingest_resize(src, xtab, kx, ytab, ky, lut, flip, out, out_strides, OH, OW):
    """Pillow-exact bilinear resize + table look-up of uint8 frames src [n,H,W,3] (any strides, channel stride 1) into `out`,
    addressed by the ELEMENT strides out_strides = (image, channel, row, column); xtab / ytab int32 [OW, 2+kx] / [OH, 2+ky]
    (svol_amd.ingest.resample_tables), lut fp32 [3,256], flip uint8 [n] or None.  See svol_ingest_resize in include/svol_hip.h."""
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or (src.shape[0] and src.stride(3) != 1):
        raise _lib.SvolHipError(f'ingest_resize takes uint8 [n,H,W,3] with channel stride 1, got {src.dtype} {tuple(src.shape)}')
    n, H, W = src.shape[:3]
    if n == 0:   # (an empty tensor has no data pointer to pass)
        return out
    o_n, o_c, o_h, o_w = out_strides
    rc = _lib.lib().svol_ingest_resize(_ptr(src), n, H, W, src.stride(0), src.stride(1), src.stride(2), _ptr(xtab), kx, _ptr(ytab), ky,
                                       _ptr(lut), _ptr(flip), _ptr(out), o_n, o_c, o_h, o_w, OH, OW, _dt(out), _stream())
    _lib.check(rc, 'svol_ingest_resize')
    return out


def ingest_resample(src, xtab, kx, ytab, ky, lut, flip, out, out_strides, OH, OW, invert=False):
    """ingest_resize generalised: any of Pillow's filters (signed taps: svol_amd.ingest.resample_tables(in, out, filter)), grey
    sources, and an inversion of the source bytes before the taps.  src is uint8 [n,H,W,3] (channel stride 1) or a grey [n,H,W]
    (any strides); the three output channels of a grey source are lut[c][u].  See svol_ingest_resample in include/svol_hip.h."""
    grey = src.dim() == 3
    if src.dtype != torch.uint8 or not (grey or (src.dim() == 4 and src.shape[3] == 3 and (not src.shape[0] or src.stride(3) == 1))):
        raise _lib.SvolHipError(f'ingest_resample takes uint8 [n,H,W,3] with channel stride 1 or uint8 [n,H,W], got {src.dtype} {tuple(src.shape)}')
    n, H, W = src.shape[:3]
    if n == 0:   # (an empty tensor has no data pointer to pass)
        return out
    o_n, o_c, o_h, o_w = out_strides
    rc = _lib.lib().svol_ingest_resample(_ptr(src), n, H, W, src.stride(0), src.stride(1), src.stride(2), 1 if grey else 3, int(bool(invert)),
                                         _ptr(xtab), kx, _ptr(ytab), ky, _ptr(lut), _ptr(flip), _ptr(out), o_n, o_c, o_h, o_w, OH, OW,
                                         _dt(out), _stream())
    _lib.check(rc, 'svol_ingest_resample')
    return out


def conv_nhwc(x, w, bias, act, N, H, W, C, kh, kw, stride, pad, residual=None):
    """convolution of an NHWC activation [N*H*W, C] with folded weights w [Cout, kh*kw*C (+pad)] -> (y [N*Ho*Wo, Cout], Ho, Wo).
    The implicit-GEMM kernel when the shape fits it (bf16 or fp16, C % 32 == 0), else im2col + gemm_nt."""
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    Cout = w.shape[0]
    if x.dtype in (torch.bfloat16, torch.float16) and C % 32 == 0 and _CONV_IMPLICIT:
        y = torch.empty((N * Ho * Wo, Cout), dtype=x.dtype, device=x.device)
        rc = _lib.lib().svol_conv_nhwc(_ptr(x), _ptr(w), w.stride(0), _ptr(y), _ptr(bias), act, _ptr(residual), N, H, W, C, Cout, kh,
                                       kw, stride, pad, _dt(x), _stream())
        if rc == 0:
            return y, Ho, Wo
        if rc != -2:  # SVOL_E_UNSUPPORTED falls through to the explicit path
            _lib.check(rc, 'svol_conv_nhwc')
    cols, Ho, Wo = im2col(x, N, H, W, C, kh, kw, stride, pad, x.dtype, ldcols=w.shape[1])
    return gemm_nt(cols, w, bias, act, residual=residual), Ho, Wo


_CONV_IMPLICIT = os.environ.get('SVOL_CONV_IM2COL') is None


def maxpool_nhwc(x, N, H, W, C, k, stride, pad):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.empty((N * Ho * Wo, C), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().svol_maxpool_nhwc(_ptr(x), _ptr(y), N, H, W, C, k, stride, pad, _dt(x), _stream()), 'svol_maxpool_nhwc')
    return y, Ho, Wo


def avgpool_nhwc(x, N, HW, C):
    y = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().svol_avgpool_nhwc(_ptr(x), _ptr(y), N, HW, C, _dt(x), _stream()), 'svol_avgpool_nhwc')
    return y


# ---- the backbone in training mode (csrc/resnet_train.hip) --------------------------------------------------------------
BN_STATS_TWO_PASS = os.environ.get('SVOL_BN_TWO_PASS') is not None   # batch mean first, then the moment about it (tests: torch's own order)


def _bn_sync_world(sync):
    """ranks whose batch statistics are shared (apex convert_syncbn_model, train.py:65-68): the default process group, > 1 only."""
    if not sync:
        return 1
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def bn_train_stats(z, gamma, beta, running_mean, running_var, momentum, eps, sync=False):
    """train-mode nn.BatchNorm2d statistics of an NHWC activation z [M, C] (16-bit) in ONE pass over z: sums of (z - s) and (z - s)^2
    about a per-channel pivot s = the first row of z (a sample of the channel: the variance's subtraction loses a few bits, not the
    variance — a plain sum z^2 would at |mean| >> std; measured against fp64: mean 1e-7 of a standard deviation, rstd 1e-6), then
    everything [C]-sized at once (svol_bn_finalize): -> fp32 [C] rows (mean, rstd, scale = gamma * rstd, shift = beta - mean * scale);
    running_mean / running_var (may be None) are updated in place.  BN_STATS_TWO_PASS (SVOL_BN_TWO_PASS=1): the batch mean first, then
    the second moment about it — one more pass over z, statistics equal to torch's to the last bits (the end-to-end gradient test
    compares with a torch network whose ReLU masks flip with the 7th digit of a statistic).
    sync (``--sync_bn`` with more than one rank: apex SyncBatchNorm, train.py:65-68): the statistics are those of the GLOBAL batch —
    every rank sums about rank 0's pivot (one [C] broadcast), the [2, C] sums are all-reduced and divided by the global row count
    (every rank holds the same number of rows: the per-GPU batch of svol_dataloader.py:70)."""
    M, C = z.shape
    buf = torch.zeros((7, C), dtype=torch.float32, device=z.device)
    L_ = _lib.lib()
    dt, s = _dt(z), _stream()
    world = _bn_sync_world(sync)
    if world > 1:
        import torch.distributed as dist
    if BN_STATS_TWO_PASS:
        _lib.check(L_.svol_bn_colstats(_ptr(z), None, 0.0, _ptr(buf[0]), _ptr(buf[6]), M, C, dt, s), 'svol_bn_colstats')
        buf[6].zero_()
        if world > 1:
            dist.all_reduce(buf[0])
        _lib.check(L_.svol_bn_colstats(_ptr(z), _ptr(buf[0]), 1.0 / (M * world), _ptr(buf[6]), _ptr(buf[1]), M, C, dt, s), 'svol_bn_colstats')
        if world > 1:
            dist.all_reduce(buf[1])
        pivot = None
    else:
        buf[6].copy_(z[0])
        if world > 1:
            dist.broadcast(buf[6], src=0)
        _lib.check(L_.svol_bn_colstats(_ptr(z), _ptr(buf[6]), 1.0, _ptr(buf[0]), _ptr(buf[1]), M, C, dt, s), 'svol_bn_colstats')
        if world > 1:
            dist.all_reduce(buf[0:2])
        pivot = buf[6]
    _lib.check(L_.svol_bn_finalize(_ptr(buf[0]), _ptr(buf[1]), _ptr(pivot), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                   float(momentum), float(eps), M * world, C, _ptr(buf[2]), _ptr(buf[3]), _ptr(buf[4]), _ptr(buf[5]), s),
               'svol_bn_finalize')
    return buf[2], buf[3], buf[4], buf[5]


def conv_weight_pack(w, dtype, flip=False):
    """nn.Conv2d weight fp32 [Cout, Cin, kh, kw] -> the GEMMs' layout in `dtype`: [Cout, pad32(kh*kw*Cin)] in (ky, kx, c) order, or with
    flip the stride-1 data gradient's [Cin, pad32(kh*kw*Cout)] (taps reversed, channels swapped)."""
    Cout, Cin, kh, kw = w.shape
    rows, K = (Cin, kh * kw * Cout) if flip else (Cout, kh * kw * Cin)
    Kp = (K + 31) // 32 * 32
    out = torch.empty((rows, Kp), dtype=dtype, device=w.device)
    wc = w.detach()
    wc = wc if wc.is_contiguous() else wc.contiguous()
    _lib.check(_lib.lib().svol_conv_weight_pack(_ptr(wc), _ptr(out), Cout, Cin, kh, kw, Kp, 1 if flip else 0, _DT[dtype], _stream()),
               'svol_conv_weight_pack')
    return out


def conv_wgrad_nhwc(dz, x, N, H, W, C, kh, kw, stride, pad, Kp):
    """[Cout, Kp] fp32 = dz^T im2col(x) without the im2col matrix (svol_conv_wgrad_nhwc); None when the kernel does not take the shape."""
    Cout = dz.shape[1]
    dwp = torch.zeros((Cout, Kp), dtype=torch.float32, device=dz.device)
    rc = _lib.lib().svol_conv_wgrad_nhwc(_ptr(dz), _ptr(x), _ptr(dwp), N, H, W, C, Cout, kh, kw, stride, pad, Kp, _dt(dz), _stream())
    if rc == -2:
        return None
    _lib.check(rc, 'svol_conv_wgrad_nhwc')
    return dwp


def conv_weight_unpack_add(dwp, grad):
    """grad [Cout, Cin, kh, kw] (fp32, contiguous) += dwp [Cout, Kp] (fp32, (ky, kx, c) order)"""
    Cout, Cin, kh, kw = grad.shape
    assert grad.is_contiguous() and dwp.is_contiguous() and dwp.dtype == torch.float32 and grad.dtype == torch.float32
    _lib.check(_lib.lib().svol_conv_weight_unpack_add(_ptr(dwp), _ptr(grad), Cout, Cin, kh, kw, dwp.shape[1], _stream()),
               'svol_conv_weight_unpack_add')


def bn_apply(z, scale, shift, residual=None, relu=False):
    M, C = z.shape
    y = torch.empty_like(z)
    _lib.check(_lib.lib().svol_bn_apply(_ptr(z), _ptr(scale), _ptr(shift), _ptr(residual), 1 if relu else 0, _ptr(y), M, C, _dt(z),
                                        _stream()), 'svol_bn_apply')
    return y


def bn_bwd(dy, y, z, mean, rstd, gamma, want_dres, sync=False):
    """(dz, dres | None, dgamma, dbeta) of y = relu?(BN_train(z) + res): y = the saved output when a ReLU follows, else None.
    sync: the statistics were the global batch's (bn_train_stats(sync=True)) — dz needs the GLOBAL means of g and g * xhat (one
    [2, C] all-reduce); dgamma / dbeta stay this rank's sums, the gradient exchange averages them like every other parameter's."""
    M, C = z.shape
    sums = torch.zeros((2, C), dtype=torch.float32, device=z.device)
    L_ = _lib.lib()
    _lib.check(L_.svol_bn_bwd_reduce(_ptr(dy), _ptr(y), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(sums[0]), _ptr(sums[1]), M, C, _dt(z),
                                     _stream()), 'svol_bn_bwd_reduce')
    world = _bn_sync_world(sync)
    if world > 1:
        import torch.distributed as dist
        local = sums.clone()
        dist.all_reduce(sums)
        sums.mul_(1.0 / world)   # svol_bn_bwd_apply divides by ITS row count M: (sum over ranks / world) / M = global sum / (M * world)
        dz = torch.empty_like(z)
        dres = torch.empty_like(z) if want_dres else None
        _lib.check(L_.svol_bn_bwd_apply(_ptr(dy), _ptr(y), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(sums[0]), _ptr(sums[1]), _ptr(dz),
                                        _ptr(dres), M, C, _dt(z), _stream()), 'svol_bn_bwd_apply')
        return dz, dres, local[1], local[0]
    dz = torch.empty_like(z)
    dres = torch.empty_like(z) if want_dres else None
    _lib.check(L_.svol_bn_bwd_apply(_ptr(dy), _ptr(y), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(sums[0]), _ptr(sums[1]), _ptr(dz),
                                    _ptr(dres), M, C, _dt(z), _stream()), 'svol_bn_bwd_apply')
    return dz, dres, sums[1], sums[0]


def col2im_nhwc(dcols, N, H, W, C, kh, kw, stride, pad):
    dx = torch.empty((N * H * W, C), dtype=dcols.dtype, device=dcols.device)
    _lib.check(_lib.lib().svol_col2im_nhwc(_ptr(dcols), dcols.stride(0), _ptr(dx), N, H, W, C, kh, kw, stride, pad, _dt(dcols), _stream()),
               'svol_col2im_nhwc')
    return dx


def maxpool_idx_nhwc(x, N, H, W, C, k, stride, pad):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.empty((N * Ho * Wo, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((N * Ho * Wo, C), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().svol_maxpool_idx_nhwc(_ptr(x), _ptr(y), _ptr(idx), N, H, W, C, k, stride, pad, _dt(x), _stream()),
               'svol_maxpool_idx_nhwc')
    return y, idx, Ho, Wo


def maxpool_bwd_nhwc(dy, idx, N, H, W, C, k, stride, pad):
    dx = torch.empty((N * H * W, C), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.lib().svol_maxpool_bwd_nhwc(_ptr(dy), _ptr(idx), _ptr(dx), N, H, W, C, k, stride, pad, _dt(dy), _stream()),
               'svol_maxpool_bwd_nhwc')
    return dx


def attn_weights_mean(q, k, lse2, B, H, Lq, Lk, dh, kbias=None, premul=0.0):
    """head-averaged softmax probabilities [B,Lq,Lk] fp32 (nn.MultiheadAttention's second return value), recomputed
    from q, k and the lse2 of attn_fwd."""
    att = torch.empty((B, Lq, Lk), dtype=torch.float32, device=q.device)
    rc = _lib.lib().svol_attn_weights_mean(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(lse2), _ptr(kbias), _ptr(att),
                                           B, H, Lq, Lk, dh, 1.0 / math.sqrt(dh), float(premul), _dt(q), _stream())
    _lib.check(rc, 'svol_attn_weights_mean')
    return att
