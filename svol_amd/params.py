"""Everything the hot path keeps per PARAMETER: the compute-dtype copies of the fp32 master weights (``weights``), the gradient
sinks a reducer hands out (``GradSink`` / ``claim``), and the one rule for where a parameter's gradient is written and what the
producing ``torch.autograd.Function`` returns for it (``GradGroup``).
"""
from __future__ import annotations

import math
import os
import struct
import weakref

import torch

from . import _lib, ops, wgrad

# bf16 mode: the VALUE projections of every attention block multiply by split weights W_hi + W_lo (two bf16 operands = 16
# mantissa bits of the fp32 master weight, one K-concatenated GEMM).  Rounding W_v to bf16 shifts every token's value the same way,
# which attention over thousands of keys and LayerNorm do not average out: at the benchmark depth (6 layers, L = 6272) the V weights
# of the query -> video attention (4.3e-3 rms) and of the video self-attention (2.7e-3) were 95 % of the 6.8e-3 rms logit error, the
# q / k / MLP weights together 1.1e-3 (profiles/round3_bf16_output_error.md).  Forward only: gradients take the plain bf16 copy.
# SVOL_NO_SPLIT_V=1 restores single-bf16 V weights (A/B; changes results).
SPLIT_V = os.environ.get('SVOL_NO_SPLIT_V') is None


# ----------------------------------------------------------------------------
# parameter cache: fp32 master weights -> compute-dtype copies (W and W^T), refreshed when the
# optimizer bumps the tensor version.  One cast per weight per step.
# ----------------------------------------------------------------------------
PLAIN, SPLIT = 'plain', 'split'


class _Entry:
    """one cached copy.  kind PLAIN: out = (W, W^T) in the compute dtype of the whole weight; kind SPLIT: out = [hi | lo] bf16 of a
    row range.  ptr: address of the first source row; key: where the entry sits in the parameter's ``_svol_cache``."""
    __slots__ = ('kind', 'out', 'key', 'ptr', 'shape', 'epoch', 'version')


class _WeightCache:
    """fp32 master weight -> compute-dtype copies (W and W^T) in persistent buffers.

    Every weight is (re)cast once per EPOCH — the model advances the epoch at the start of every forward —
    because tensor version counters cannot be trusted to see optimizer updates (``torch.optim.AdamW(fused=True)``
    rewrites parameters without bumping ``_version`` on ROCm).  The first time a weight is seen it is cast on the
    spot and registered; from then on ``new_epoch()`` refreshes ALL registered weights of a (device, dtype) with
    ONE ``svol_cast_transpose_multi`` launch driven by a device-side descriptor table (64 launches -> 1 per step
    at the benchmark size).  With ``static=True`` (frozen weights, e.g. serving) nothing is refreshed."""

    def __init__(self):
        self.epoch = 0
        self.static = False
        self._sets = {}  # (device, dtype) -> {'items': [(weakref(param), entry)], 'table': tensor|None, 'tiles': int}

    def new_epoch(self):
        wgrad.forward_starts()
        if self.static:
            return
        self.epoch += 1
        for key, st in self._sets.items():
            self._refresh(key, st)

    def _refresh(self, key, st):
        dev, dtype = key
        if dtype not in ops._DT:
            return
        def alive(r, e):
            w = r()
            return w is not None and getattr(w, '_svol_cache', {}).get(e.key) is e and (e.kind == SPLIT or w.data_ptr() == e.ptr)
        live = [(r, e) for (r, e) in st['items'] if alive(r, e)]
        if len(live) != len(st['items']) or st['table'] is None:
            st['items'] = live
            st['table'] = None
            if not live:
                return
            recs = []
            t0 = 0
            for r, e in live:
                R, C = e.shape
                tc = (C + 31) // 32
                # src, dst, dstT, dstS (8 bytes each) ; R, C, tiles_c, tile_begin (int32)
                if e.kind == SPLIT:   # split copy of a row range of the weight (get_split): its own record
                    recs.append((e.ptr, 0, 0, e.out.data_ptr(), R, C, tc, t0))
                else:
                    recs.append((e.ptr, 0 if dtype == torch.float32 else e.out[0].data_ptr(), e.out[1].data_ptr(), 0, R, C, tc, t0))
                t0 += ((R + 31) // 32) * tc
            blob = b''.join(struct.pack('<QQQQiiii', *rec) for rec in recs)
            st['table'] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
            st['tiles'] = t0
            st['gen'] = st.get('gen', 0) + 1
        _lib.check(_lib.lib().svol_cast_transpose_multi(ops._ptr(st['table']), len(st['items']), st['tiles'], ops._DT[dtype],
                                                        ops._stream()), 'svol_cast_transpose_multi')
        # The copies were allocated on the stream of their first use (the query half's weights: the side stream) and are
        # rewritten HERE, on the caller's stream.  Tell the allocator, or a copy whose owner dies (a model dropped between two
        # tests, a re-built module) goes back to its own stream's pool while this launch is still queued and the refresh lands
        # in whoever got the block next (seen as a 1-in-15 garbage forward in the test suite, never with one long-lived model)
        if dev.type == 'cuda':
            cur = ops._current_stream_obj()
            done = st.setdefault('recorded', set())
            key_ = (cur.cuda_stream, st.get('gen', 0))
            if key_ not in done:
                done.clear()
                done.add(key_)
                for r, e in st['items']:
                    if e.kind == SPLIT:
                        e.out.record_stream(cur)
                        continue
                    wc, wt = e.out
                    if wc.dtype != torch.float32:
                        wc.record_stream(cur)
                    wt.record_stream(cur)
        for r, e in st['items']:
            e.epoch = self.epoch
            e.version = r()._version

    def _entry(self, w, kind, key, dtype, ptr):
        """the one lookup -> validate -> (re)cast -> register path of both kinds of copy; an entry that is only stale (version or
        epoch) is re-cast INTO its buffers."""
        cache = getattr(w, '_svol_cache', None)
        if cache is None:
            cache = {}
            try:
                w._svol_cache = cache
            except Exception:  # pragma: no cover  (non-leaf views etc.: just do not cache)
                pass
        e = cache.get(key)
        if e is not None and e.ptr == ptr and e.version == w._version and (self.static or e.epoch == self.epoch):
            return e.out
        wd = w.detach()
        assert wd.dtype == torch.float32 and wd.dim() == 2 and wd.is_contiguous()
        R, C = tuple(w.shape) if kind == PLAIN else (key[1], w.shape[1])
        fresh = e is None or e.ptr != ptr or (R, C) != e.shape
        if fresh:
            e = _Entry()
            e.kind, e.key, e.ptr, e.shape = kind, key, ptr, (R, C)
            if kind == SPLIT:
                e.out = torch.empty((R, 2 * C), dtype=torch.bfloat16, device=w.device)
            else:
                e.out = (wd if dtype == torch.float32 else torch.empty((R, C), dtype=dtype, device=w.device),
                         torch.empty((C, R), dtype=dtype, device=w.device))
        if kind == SPLIT:
            _lib.check(_lib.lib().svol_cast_split(ptr, C, ops._ptr(e.out), R, C, ops._stream()), 'svol_cast_split')
        else:
            _lib.check(_lib.lib().svol_cast_transpose(ops._ptr(wd), 0 if dtype == torch.float32 else ops._ptr(e.out[0]), ops._ptr(e.out[1]),
                                                      ops._DT[dtype], R, C, ops._stream()), 'svol_cast_transpose')
        e.epoch, e.version = self.epoch, w._version
        if fresh:
            cache[key] = e
            st = self._sets.setdefault((w.device, dtype), {'items': [], 'table': None, 'tiles': 0})
            try:
                st['items'].append((weakref.ref(w), e))
                st['table'] = None
            except TypeError:  # pragma: no cover
                pass
        return e.out

    def get(self, w: torch.Tensor, dtype: torch.dtype):
        """(W, W^T) of the fp32 master weight `w` in `dtype`: the same tuple object for as long as the buffers are the same."""
        return self._entry(w, PLAIN, dtype, dtype, w.data_ptr())

    def get_split(self, w: torch.Tensor, row0: int, rows: int):
        """bf16 split copy [rows, 2C] = [hi | lo] of rows [row0, row0 + rows) of the fp32 master weight `w` (svol_cast_split):
        the operand of gemm_nt_split.  Refreshed once per epoch by the same multi-weight launch as the plain copies."""
        return self._entry(w, SPLIT, (row0, rows), torch.bfloat16, w.data_ptr() + row0 * w.shape[1] * 4)


weights = _WeightCache()


# ----------------------------------------------------------------------------
# gradient sinks: when svol_amd.parallel.BucketedGradAllReduce owns the gradients (param.grad is a view into
# a flat fp32 bucket that is zeroed once per step), the weight-/bias-/LayerNorm-gradient kernels accumulate
# STRAIGHT into that view and the Function returns None for the parameter — no per-parameter memset, no
# AccumulateGrad add.  The parameter's post-accumulate-grad hook (the reducer's bucket countdown) still fires:
# autograd runs the AccumulateGrad node with an undefined gradient after the producing Function has finished.
# ----------------------------------------------------------------------------
class GradSink:
    """view: the parameter's slice of a flat gradient bucket.  owner / bucket: who to tell that the gradient is complete when the
    producing Function keeps the parameter OUT of the autograd graph (svol_amd.blocks: no AccumulateGrad node, no hook) —
    ``owner.params_done(bucket, n)``."""
    __slots__ = ('view', 'owner', 'bucket')

    def __init__(self, view, owner=None, bucket=-1):
        self.view, self.owner, self.bucket = view, owner, bucket


def claim(p, needed=True):
    """forward: the sink of parameter `p` if its gradient can be written in place, else None."""
    s = getattr(p, '_svol_sink', None) if (needed and p is not None) else None
    g = p.grad if s is not None else None
    if g is None or g.data_ptr() != s.view.data_ptr():
        return None
    return s


# ----------------------------------------------------------------------------
# gradient targets.  THE RULE: gradients that GEMMs produce go straight to the sinks (gemm_tn_sink: off the critical path) only
# when EVERY member of their group has one; otherwise the whole group is written into one fresh zeroed buffer (one memset), added
# to whichever sinks exist, and the rest is returned to autograd.  Element-wise producers choose tensor by tensor.
# ----------------------------------------------------------------------------
def sink_view(s):
    """per tensor, for a producer that allocates its own zeroed output when given none: the sink's view or None"""
    return s.view if s is not None else None


def unless_sunk(s, g):
    """... and what the Function returns for that parameter"""
    return None if s is not None else g


class GradGroup:
    """The gradient targets of one group of parameters, by the rule above.
    targets: (sink | None, shape) per member; a third item False marks a member nobody wants a gradient of (it keeps its place in
    the buffer and does not stop the group from being direct).  ``out[i]`` is the fp32 tensor to accumulate member i into: the sinks'
    views when the group is direct, else views of ONE zeroed buffer.  each=True is the per-tensor variant for element-wise
    producers: every member with a sink is written there, the others share the zeroed buffer."""
    __slots__ = ('sinks', 'wanted', 'direct', 'each', 'out', 'buf')

    def __init__(self, targets, device, each=False):
        self.sinks = sinks = [t[0] for t in targets]
        self.wanted = wanted = [len(t) < 3 or t[2] for t in targets]
        self.each, self.buf = each, None
        self.direct = direct = not any(s is None and w for s, w in zip(sinks, wanted))
        if direct:   # (the common case with a reducer: no allocation, no arithmetic on shapes)
            self.out = [None if s is None else (s.view if s.view.dim() == len(t[1]) else s.view.view(t[1])) for s, t in zip(sinks, targets)]
            return
        sizes = [math.prod(t[1]) for t in targets]
        self.buf = buf = torch.zeros((sum(sizes),), dtype=torch.float32, device=device)   # one memset for the whole group
        self.out, o = [], 0   # (the members lie in the buffer back to back: a caller may cover several with one launch)
        for s, n, t in zip(sinks, sizes, targets):
            shape = t[1]
            if s is not None and each:
                self.out.append(s.view)
            else:
                v = buf[o:o + n]
                self.out.append(v.view(shape) if len(shape) > 1 else v)
            o += n

    def tn(self, A, B, w, b=None, rows=None):
        """member w (rows `rows` of it) += A^T B, member b += column sums of A: on the weight-gradient stream when direct"""
        out = self.out[w] if rows is None else self.out[w][rows]
        cs = None if b is None else (self.out[b] if rows is None else self.out[b][rows])
        if self.direct:
            ops.gemm_tn_sink(A, B, out=out, colsum=cs)
        else:
            ops.gemm_tn(A, B, out=out, colsum=cs)

    def finish(self):
        """the buffer's members are added to whichever sinks exist -> per member what the Function returns to autograd: None where
        a sink has the gradient"""
        if self.direct:
            return (None,) * len(self.sinks)
        res = []
        for s, w, g in zip(self.sinks, self.wanted, self.out):
            if s is not None and not self.each:
                v = s.view
                v.add_(g if g.dim() == v.dim() else g.view(v.shape))
            res.append(g if (s is None and w) else None)
        return tuple(res)

