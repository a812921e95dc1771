"""Data-parallel gradient exchange for the SVOL training step: one process per GPU, bucketed
all-reduce over RCCL / xGMI (``torch.distributed`` backend "nccl" IS RCCL on ROCm), overlapped with
the backward pass.

The reference wraps the model in apex ``DistributedDataParallel(delay_allreduce=True)`` (train.py:124):
ONE flattened all-reduce of every gradient after backward has finished, no overlap.  Semantics kept:
the result is the MEAN over ranks of the per-rank gradients (each rank's loss is a mean over its LOCAL
batch / matched pairs, i.e. mean-of-means — SURVEY.md §8e), parameters that receive no gradient
(``sketch_video_cross_attn.out_proj.*``, ``class_head.*``) are skipped on every rank.

MI355X-first differences:
* gradients live in a few large flat fp32 buckets (``param.grad`` is a VIEW into its bucket), so a
  bucket is reduced in place with no gather/scatter copies;
* buckets are filled in the order backward PRODUCES gradients (``arrival_order``: box / class heads, then
  the transformer layers last to first, then the query embedding and the input projections, whose
  gradients only exist at the very end of backward) and each bucket's all-reduce is issued on a side
  stream the moment its last gradient has been accumulated, so the exchange of layer k overlaps the
  backward kernels of layers < k and only the last, small bucket is exposed;
* xGMI is point-to-point (7 links x ~153 GB/s per GPU): the 74.4 MiB fp32 gradient of the benchmark
  head is cut into ~16 MiB buckets — large enough that each ring step is bandwidth- not latency-bound
  (per-link ring time ~ 2*(7/8)*16 MiB / 153 GB/s ~ 0.19 ms), small enough that the last bucket exposes
  little un-overlapped time.
"""
from __future__ import annotations

import contextlib
from typing import Iterable, List, Optional

import torch
import torch.distributed as dist

from . import _lib, wgrad   # (none loads the kernel library at import)
from .ops import _ptr, _stream
from .params import GradSink

_LATE = ('query_embed', 'input_', 'backbone', 'pos_embed', 'position_embedding')   # first used in forward = last in backward
_GATE = ('sketch_video_cross_attn',)   # the gate-vector algebra of every layer runs ahead of the layer loop (cross_modal_transformer.py):
                                       # its backward is the last thing the transformer does, just before the input projections'
_EARLY = ('bbox_embed', 'class_embed')                                            # the heads: last in forward


def arrival_order(model: torch.nn.Module) -> List[torch.nn.Parameter]:
    """The trainable parameters of ``model`` in the order backward is expected to produce their gradients:
    reverse registration order (layers L-1 .. 0, inside a layer the last sub-block first), except that the heads
    (registered before the transformer in SVANet, svanet.py:42-44, but applied last) come first and what the forward
    touches first although it is registered last (input projections svanet.py:49-60, query embedding, backbones) comes
    last.  A wrong guess costs overlap, never correctness."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]

    def rank(name):
        if any(t in name for t in _EARLY):
            return 0
        if any(t in name for t in _LATE):
            return 3
        if any(t in name for t in _GATE):
            return 2
        return 1
    idx = sorted(range(len(named)), key=lambda i: (rank(named[i][0]), -i))
    return [named[i][1] for i in idx]


class BucketedGradAllReduce:
    """``params`` is taken in the order given — pass ``arrival_order(model)`` (a plain ``model.parameters()`` list is
    re-ordered by ``reversed`` as a fallback guess when ``ordered=False``)."""

    def __init__(self, params: Iterable[torch.nn.Parameter], bucket_bytes: int = 16 << 20,
                 skip: Optional[Iterable[torch.nn.Parameter]] = None, process_group=None, ordered: bool = False,
                 tail_bytes: int = 2 << 20):
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        skip_ids = {id(p) for p in (skip or [])}
        plist = [p for p in params if p.requires_grad and id(p) not in skip_ids]
        if not plist:
            raise ValueError('no parameters to reduce')
        self.device = plist[0].device
        self.on_gpu = self.device.type == 'cuda'
        order = plist if ordered else list(reversed(plist))
        self.buckets: List[dict] = []
        groups, cur, cur_bytes = [], [], 0
        for p in order:
            nbytes = p.numel() * 4
            if cur and cur_bytes + nbytes > bucket_bytes:
                groups.append(cur)
                cur, cur_bytes = [], 0
            cur.append(p)
            cur_bytes += nbytes
        if cur:
            groups.append(cur)
        # The LAST bucket's all-reduce cannot overlap with anything: its last gradient is the last thing backward produces.
        # Keep that exposed exchange small: the final `tail_bytes` of the arrival order (the input projections, the query
        # embedding, the end of layer 0) get a bucket of their own, the rest of the old last bucket reduces under layer 0's backward.
        if tail_bytes and groups:
            last, tail, tb = groups[-1], [], 0
            while len(last) > 1 and tb + last[-1].numel() * 4 <= tail_bytes:
                tb += last[-1].numel() * 4
                tail.insert(0, last.pop())
            if tail:
                groups.append(tail)
        for g in groups:
            self._make_bucket(g)
        self._handles = []
        self._hooks = []
        # SVOL_FORCE_ALLREDUCE=1: run the collective path at world size 1 too (a 1-rank RCCL communicator is a real communicator: the
        # all-reduce is enqueued on the communication stream behind the same producer-stream waits, finish() joins it) — how the
        # stream choreography is exercised against RCCL on a one-GPU box (tests/test_gpu_parallel.py)
        import os
        self.force = self.world == 1 and dist.is_initialized() and os.environ.get('SVOL_FORCE_ALLREDUCE') == '1'
        self.spans = []            # per launched bucket: (bucket index, start event, end event) on the communication stream (GPU only)
        self.exposed = None        # (event, event) around finish()'s wait for the communication stream: the exchange backward did not hide
        self.record_spans = self.force or os.environ.get('SVOL_DP_SPANS') == '1'
        # SVOL_ALLREDUCE_SPIN=ring|direct (with SVOL_FORCE_ALLREDUCE=1 only): a one-rank communicator's all-reduce is a copy — to
        # rehearse a collective that COSTS TIME on one GPU, a spin kernel of the exchange's modelled duration over xGMI at 8 ranks
        # follows every bucket's collective on the communication stream (7 links x ~153 GB/s per GPU,
        # point to point): ring 2 (7/8) bytes / 153 GB/s (per-link bound), direct reduce-scatter + all-gather 2 (bytes / 8) / 153 GB/s
        # + 20 us.  The spin holds one CU and moves no bytes: it tests the ORDER and EXPOSURE of the exchange (which buckets hide
        # behind backward, what finish() waits for), not the bandwidth RCCL's copies take from the weight-gradient stream.
        self.spin = os.environ.get('SVOL_ALLREDUCE_SPIN') if self.force else None
        if self.spin not in (None, 'ring', 'direct'):
            raise ValueError('SVOL_ALLREDUCE_SPIN must be ring or direct')
        self._spin_cycles_per_ms = None
        self.pending_scale = 1.0   # see finish(mean=False)
        self.on_bucket_reduced = None   # FlatAdamW(step_in_backward=True): callable(bucket index, stream handle), see _launch
        self._early_any = False
        self.fire_order: List[int] = []   # diagnostics: bucket index of every hook of the current step, in firing order
        self.comm_stream = torch.cuda.Stream(device=self.device) if self.on_gpu else None
        # the stream the caller computes on (the video half of the model, the criterion, the optimizer); re-read
        # at every zero_grad() on the caller's thread — hooks run on the autograd thread under the NODE's stream
        self.main_stream = torch.cuda.current_stream(self.device) if self.on_gpu else None
        for bi, b in enumerate(self.buckets):
            for p in b['params']:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(bi)))
                # the svol kernels accumulate weight / bias / LayerNorm gradients straight into the bucket view
                # (svol_amd.params "gradient sinks"); the hook above still fires for them
                p._svol_sink = GradSink(p.grad, self, bi)

    def _make_bucket(self, params):
        # every tensor starts on a 16-byte boundary (the kernels take 16-byte vector accesses on gradients and — FlatAdamW —
        # on the parameters that share this layout); the few padding floats stay zero
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        flat = torch.zeros(n, dtype=torch.float32, device=params[0].device)
        for p, off in zip(params, offs):
            assert p.dtype == torch.float32, 'master parameters are fp32'
            p.grad = flat[off:off + p.numel()].view_as(p)  # autograd accumulates in place into the view
        self.buckets.append({'index': len(self.buckets), 'params': params, 'offsets': offs, 'flat': flat, 'pending': len(params),
                             'n': len(params)})

    def _make_hook(self, bi):
        def hook(_p):
            b = self.buckets[bi]
            self.fire_order.append(bi)
            b['pending'] -= 1
            if b['pending'] == 0:
                self._launch(b)
        return hook

    def params_done(self, bi, n=1):
        """`n` parameters of bucket `bi` have their complete gradient enqueued (or queued for the weight-gradient stream): what the
        per-parameter hooks do, for producers that write into the bucket without an autograd edge to the parameter (svol_amd.blocks)."""
        b = self.buckets[bi]
        self.fire_order.extend([bi] * n)
        b['pending'] -= n
        if b['pending'] < 0:
            # a second backward() without zero_grad() in between (gradient accumulation): the bucket was already handed to the
            # exchange once — reducing it again would double-count
            raise RuntimeError('BucketedGradAllReduce: more gradients arrived for a bucket than it has parameters — call zero_grad() '
                               'before every backward() (gradient accumulation over several backward passes is not supported by the '
                               'block programs\' gradient sinks)')
        if b['pending'] == 0:
            self._launch(b)

    def _producer_streams(self):
        """every stream a gradient of a bucket can have been written on: the caller's compute stream (video half,
        heads, input projections), the model's side stream (query half: gradient-sink kernels and AccumulateGrad nodes
        created under ``torch.cuda.stream(side)``), and the stream of the node whose hook is running."""
        from .modeling import cross_modal_transformer as cmt
        ss = ([self.main_stream, torch.cuda.current_stream(self.device)] + list(cmt.side_streams(self.device)) +
              list(wgrad.streams(self.device)))   # weight-gradient GEMMs run on a stream of their own
        out = []
        for s in ss:
            if s is not None and all(s != t for t in out):
                out.append(s)
        return out

    def _launch(self, b):
        collective = not (self.world == 1 and not self.force)
        early = self.on_bucket_reduced is not None and self.on_gpu
        if not collective:
            if early:
                self._early_step_local(b)
            return
        if self.on_gpu:
            # The hook runs on the autograd thread under the stream guard of the LAST-arriving parameter's node.  That
            # can be the side stream (query half), which runs far ahead of the main stream: waiting only on it would
            # start the all-reduce before the main stream has written the video-half gradients of the same bucket.
            # By the time the last hook of a bucket fires every producing kernel of the bucket has been ENQUEUED on
            # its stream (autograd issues nodes in order on the host), so waiting on all producer streams here is
            # sufficient.
            wgrad.flush()   # weight-gradient GEMMs still queued on the host may belong to this bucket
            for s in self._producer_streams():
                self.comm_stream.wait_stream(s)
            with torch.cuda.stream(self.comm_stream):
                if self.record_spans:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(self.comm_stream)
                h = dist.all_reduce(b['flat'], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                if self.spin is not None:
                    h.wait()
                    torch.cuda._sleep(int(self.modelled_exchange_ms(b['flat'].numel() * 4) * self._spin_rate()))
                if self.record_spans:
                    h.wait()       # (stream-side wait: orders the communication stream behind the collective, does not block the host)
                    e1.record(self.comm_stream)
                    self.spans.append((b['index'], e0, e1))
                if early:          # the bucket's optimizer update right behind its exchange, on the communication stream
                    h.wait()
                    self._early_any = True
                    self.on_bucket_reduced(b['index'], self.comm_stream.cuda_stream)
        else:
            h = dist.all_reduce(b['flat'], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._handles.append((h, b))

    def _early_step_local(self, b):
        """world size 1, FlatAdamW(step_in_backward=True): the bucket's update as soon as its gradients are final, on the communication
        stream behind every producer stream's work so far.  Weight-gradient launches still QUEUED on the host (wgrad: deferred to
        the next large attention backward) belong in front of it: the update joins that queue behind them, so the deferral keeps its
        schedule and the update lands beside the attention backward — an issue-bound launch that leaves the memory side idle."""
        def issue():
            for s in self._producer_streams():
                self.comm_stream.wait_stream(s)
            self._early_any = True
            self.on_bucket_reduced(b['index'], self.comm_stream.cuda_stream)

        wgrad.run_behind_pending(issue)

    def modelled_exchange_ms(self, nbytes: int, ranks: int = 8, link_gbs: float = 153.0) -> float:
        """duration of one bucket's all-reduce over xGMI in the SVOL_ALLREDUCE_SPIN model (see __init__)."""
        if self.spin == 'direct':
            return 2.0 * (nbytes / ranks) / (link_gbs * 1e9) * 1e3 + 0.02
        return 2.0 * (ranks - 1) / ranks * nbytes / (link_gbs * 1e9) * 1e3

    def _spin_rate(self) -> float:
        """torch.cuda._sleep cycles per millisecond on this device (calibrated once, synchronising; first use only)."""
        if self._spin_cycles_per_ms is None:
            s_ = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(s_):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(1_000_000)
                e0.record(s_)
                torch.cuda._sleep(20_000_000)
                e1.record(s_)
            e1.synchronize()
            self._spin_cycles_per_ms = 20_000_000 / max(e0.elapsed_time(e1), 1e-3)
        return self._spin_cycles_per_ms

    def zero_grad(self):
        """Zero the flat buckets (replaces optimizer.zero_grad(); keeps the grad views alive)."""
        if self.on_gpu:
            self.main_stream = torch.cuda.current_stream(self.device)
            wgrad.drop_pending()   # weight-gradient launches a failed backward left queued must not land in the zeroed buckets
        self.fire_order = []
        self.spans = []
        self._early_any = False
        for b in self.buckets:
            if b.pop('clean', False):
                pass   # FlatAdamW(zero_grads=True) zeroed the range behind its read of it (svol_adamw_flat_zero)
            else:
                b['flat'].zero_()
            b['pending'] = b['n']
            for p in b['params']:
                if p.grad is None or p.grad.data_ptr() < b['flat'].data_ptr() or \
                        p.grad.data_ptr() >= b['flat'].data_ptr() + b['flat'].numel() * 4:
                    raise RuntimeError('a parameter gradient was re-bound (zero_grad(set_to_none=True)?); use '
                                       'BucketedGradAllReduce.zero_grad() instead of optimizer.zero_grad()')

    def finish(self, mean: bool = True):
        """Wait for every in-flight bucket and turn sums into means.  Call after backward() — MANDATORY before anything reads
        ``param.grad`` (a gradient-norm log, clipping, a torch optimizer), also at world size 1: the block programs write the gradient
        buckets from the query-half and weight-gradient streams without autograd edges to the parameters, so ``backward()``
        returning does not order those streams against the caller's; this call does.  (For clipping and the norm with a flat
        optimizer use its ``max_grad_norm`` / ``grad_norm``: ``clip_grad_norm_`` over ``param.grad`` sees sums over ranks after
        ``mean=False`` and loss-scaled gradients under a loss scale.)
        mean=False: leave the SUMS in the buckets and remember the factor (``pending_scale`` = 1 / world) for ``FlatAdamW.step()``,
        which applies it inside its one pass over the gradients (no multiply launch per bucket)."""
        if self.on_gpu:
            # kernels that accumulate straight into the buckets (gradient sinks) may have run on the model's side
            # stream (query-stream / video-stream overlap): join it before anyone reads the buckets
            from .modeling import cross_modal_transformer as cmt
            wgrad.flush()
            for s in list(cmt.side_streams(self.device)) + list(wgrad.streams(self.device)):
                torch.cuda.current_stream().wait_stream(s)
        collective = self.world > 1 or self.force
        for b in self.buckets:
            if b['pending'] != 0 and collective:
                # a parameter of this bucket got no gradient this step (should not happen for a fixed
                # architecture); reduce what we have so that ranks stay in lock-step
                self._launch(b)
        for h, b in self._handles:
            h.wait()
        if self.on_gpu and self._early_any and not collective:
            torch.cuda.current_stream().wait_stream(self.comm_stream)   # bucket updates issued during backward (FlatAdamW(step_in_backward=True))
        if self.on_gpu and collective:
            cur = torch.cuda.current_stream()
            if self.record_spans:   # what the caller's stream waits here is the exchange that backward did not cover
                ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ea.record(cur)
            cur.wait_stream(self.comm_stream)
            if self.record_spans:
                eb.record(cur)
                self.exposed = (ea, eb)
        if self.world > 1:
            inv = 1.0 / self.world
            if mean:
                for b in self.buckets:
                    b['flat'].mul_(inv)
            else:
                self.pending_scale = inv
        self._handles.clear()

    def allreduce_report(self):
        """after a synchronised step with span recording on (SVOL_FORCE_ALLREDUCE / SVOL_DP_SPANS): per launched bucket (index, MiB, ms
        from the first recorded start, duration ms) on the communication stream, and the ms the caller's stream waited in finish()."""
        if not self.spans:
            return {'buckets': [], 'exposed_ms': 0.0}
        t0 = self.spans[0][1]
        out = [{'bucket': bi, 'mib': round(self.buckets[bi]['flat'].numel() * 4 / 2 ** 20, 2), 'start_ms': round(t0.elapsed_time(e0), 3),
                'ms': round(e0.elapsed_time(e1), 3)} for bi, e0, e1 in self.spans]
        exposed = self.exposed[0].elapsed_time(self.exposed[1]) if self.exposed else 0.0
        rep = {'buckets': out, 'exposed_ms': round(exposed, 4)}
        if self.spin is not None:
            rep['spin_model'] = self.spin
            rep['modelled_ms'] = [round(self.modelled_exchange_ms(self.buckets[bi]['flat'].numel() * 4), 3) for bi, _e0, _e1 in self.spans]
        return rep

    def bucket_fire_spans(self):
        """diagnostics after a backward: per bucket (first, last) position of its hooks in the step's firing order —
        with a good ``arrival_order`` the spans do not interleave and bucket k completes before bucket k+1 starts."""
        spans = {}
        for pos, bi in enumerate(self.fire_order):
            lo, _ = spans.get(bi, (pos, pos))
            spans[bi] = (lo, pos)
        return [spans.get(bi) for bi in range(len(self.buckets))]

    def remove(self):
        for h in self._hooks:
            h.remove()
        self._hooks.clear()
        for b in self.buckets:
            for p in b['params']:
                if hasattr(p, '_svol_sink'):
                    del p._svol_sink


class DynamicLossScaler:
    """apex-amp style dynamic loss scaling for fp16 operands (the reference's fp16 mode: configs.py:52-61, ``amp.scale_loss`` at
    train.py:231-232) kept entirely on the device: ``scale(loss)`` multiplies by the scale tensor, ``FlatAdamW.step()`` (FlatAdam, FlatSGD alike) checks the
    flat gradient buckets for inf / NaN, SKIPS the whole update when one is found (parameters, moments and the bias-correction step
    count keep their values), and halves / grows the scale — no host synchronisation, no ``.item()``.  ``state_dict()`` speaks the
    ``amp`` entry of the reference's checkpoints (``{'loss_scaler0': {'loss_scale', 'unskipped'}}``)."""

    def __init__(self, device, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0,
                 max_scale=2.0 ** 24):
        self.state = torch.tensor([float(init_scale), 0.0, 0.0, 0.0], dtype=torch.float32, device=device)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.min_scale, self.max_scale = float(min_scale), float(max_scale)

    def scale(self, loss):
        return loss * self.state[0]

    def state_dict(self):   # (a host read: checkpoint time only)
        st = self.state.tolist()
        return {'loss_scaler0': {'loss_scale': st[0], 'unskipped': int(st[2])}}

    def load_state_dict(self, sd):
        e = sd.get('loss_scaler0', sd)
        self.state[0] = float(e['loss_scale'])
        self.state[2] = float(e.get('unskipped', 0))


class _FlatOptimizer(torch.optim.Optimizer):
    """What FlatAdamW, FlatAdam and FlatSGD share: the parameters of every reducer bucket re-homed into one flat fp32 buffer
    (``param.data`` becomes a view, like ``param.grad`` already is) with flat state buffers beside it, one update kernel per bucket,
    the gradient mean's ``1 / world`` and the loss scale riding that kernel, ``zero_grads`` / ``step_in_backward``, the dynamic loss
    scaler, and checkpoints in the schema of the torch optimizer of the same name.  A subclass names its kernels (``_KERNEL``), its
    state buffers (``_STATE``), the hyper-parameters a checkpoint carries (``_HYPER``) and the ones its kernels take (``_hyper``)."""

    _KERNEL = ''       # the plain C entry; + '_zero' (zero_grads) / '_scaled' (state vector): the three share their leading arguments
    _STATE = ()        # (key in self.flat[i], key in torch's per-parameter state) per flat state buffer, in the entries' order
    _HYPER = ()        # hyper-parameter keys of the param group that load_state_dict() takes from a checkpoint
    _HAS_STEP = True   # torch's per-parameter state carries 'step', and the plain entries take a step count

    @staticmethod
    def _hyper(g) -> tuple:
        """the hyper-parameters of param group ``g`` in the order the C entries take them"""
        raise NotImplementedError

    @staticmethod
    def _hyper_row(g) -> tuple:
        """the first five floats of ``g``'s row of the grouped entries' hyper table: lr, beta1 | momentum, beta2, eps, weight_decay"""
        raise NotImplementedError

    def __init__(self, reducer: 'BucketedGradAllReduce', defaults: dict, params, zero_grads: bool, step_in_backward: bool,
                 max_grad_norm: Optional[float] = None, capturable: bool = False, ema_decay: Optional[float] = None,
                 ema_warmup: bool = True):
        owned = [p for b in reducer.buckets for p in b['params']]
        plist = list(params) if params is not None else owned
        self._params_given = params is not None
        as_dicts = bool(plist) and isinstance(plist[0], dict)
        if as_dicts:
            plist = [dict(g, params=list(g['params'])) for g in plist]
        in_groups = [p for g in plist for p in g['params']] if as_dicts else plist
        known = {id(p) for p in in_groups}
        missing = [p for p in owned if id(p) not in known]
        if missing:
            raise ValueError(f'{len(missing)} parameter(s) of the gradient buckets are not in `params`')
        if as_dicts and len(known) != len(in_groups):
            raise ValueError('a parameter appears twice in the groups of `params`')
        super().__init__(plist, defaults)   # (torch's list-of-dicts form too: a group's missing keys are filled from `defaults`)
        # The grouped path (_step_grouped): more than one param group, or a step that a graph capture may record.  The ..._grouped
        # entries read every hyper-parameter and the step count from device memory; one group and capturable=False is the plain path.
        self.capturable = bool(capturable)
        self._grouped = len(self.param_groups) > 1 or self.capturable
        if self._grouped and step_in_backward:
            raise ValueError('step_in_backward launches a bucket\'s update with a host step count: not with several param groups or '
                             'capturable=True')
        self.reducer = reducer
        self.t = 0
        # the loss was multiplied by this before backward (fp16 operands: gradients of ~1e-6 underflow otherwise); divided back out
        # inside the update kernel
        self.loss_scale = 1.0
        self._scaler: Optional[DynamicLossScaler] = None   # set for fp16 training: overflow check + skip + dynamic scale (see step())
        self.flat = []      # per bucket: flat parameters and flat state buffers
        self._slot = {}     # id(param) -> (bucket index, offset, numel)
        for bi, b in enumerate(reducer.buckets):
            flat_g = b['flat']
            flat_p = torch.zeros_like(flat_g)
            for p, off in zip(b['params'], b['offsets']):
                n = p.numel()
                flat_p[off:off + n].copy_(p.data.reshape(-1))
                p.data = flat_p[off:off + n].view_as(p)  # same layout as the gradient views of the bucket
                self._slot[id(p)] = (bi, off, n)
            st = {'p': flat_p}
            for k, _ in self._STATE:
                st[k] = torch.zeros_like(flat_p)
            self.flat.append(st)
        # The weight average (see FlatAdamW): a clone of every bucket's flat parameters, taken behind the re-homing copy.  A setting of
        # the object, like max_grad_norm: not a key of param_groups, not in state_dict().  None: no buffer, no launch.
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f'ema_decay must lie in [0, 1] or be None (off), got {ema_decay}')
        self._ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ema_swapped = False   # inside averaged_weights(): 'p' holds the average and 'ema' the weights
        if self._ema_decay is not None:
            for st in self.flat:
                st['ema'] = st['p'].clone()
        self.zero_grads = bool(zero_grads)
        self.step_in_backward = bool(step_in_backward)
        self._stepped = [False] * len(self.flat)
        if self.step_in_backward:
            reducer.on_bucket_reduced = self._step_bucket_early
        self._max_grad_norm: Optional[float] = None
        self._clip = None   # device buffers of the clipped step, made when clipping is first turned on (_clip_buffers)
        self.max_grad_norm = max_grad_norm
        if self._grouped:
            self._build_grouped()

    def _build_grouped(self):
        """The grouped path's tables, built once.  Per bucket the RUNS of its layout — maximal stretches of adjacent parameters of
        one group; the reducer laid the buckets out in arrival order before this optimizer existed, so groups alternate as they
        come — as (ends in units of four floats, group per run): ``seg_tables`` on the host, int32 tensors on the device.  One
        hyper table, a row of eight floats per group (``_hyper_row``), with a pinned host mirror that ``push_hyper`` uploads from;
        and the count of updates taken as one device float, which the kernels read unless a scaler owns the count."""
        dev = self.reducer.buckets[0]['flat'].device
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g['params']}
        self.seg_tables = []
        for b in self.reducer.buckets:
            ends, groups = [], []
            for p, off in zip(b['params'], b['offsets']):
                gi, end = group_of[id(p)], (off + (p.numel() + 3) // 4 * 4) // 4
                if groups and groups[-1] == gi:
                    ends[-1] = end
                else:
                    ends.append(end)
                    groups.append(gi)
            assert ends[-1] * 4 == b['flat'].numel()
            self.seg_tables.append((ends, groups))
        self._seg_dev = [(torch.tensor(e, dtype=torch.int32, device=dev), torch.tensor(g, dtype=torch.int32, device=dev))
                         for e, g in self.seg_tables]
        self._hyper_rows = self._rows()
        self._hyper_host = torch.tensor(self._hyper_rows, dtype=torch.float32)
        if dev.type == 'cuda':
            self._hyper_host = self._hyper_host.pin_memory()
        self._hyper_dev = self._hyper_host.to(dev)
        self._hyper_sent = None     # event behind the last upload: the mirror is not rewritten while a copy may still read it
        self._step_dev = torch.zeros(1, dtype=torch.float32, device=dev)

    def _rows(self):
        return [list(self._hyper_row(g)) + [0.0] * 3 for g in self.param_groups]

    def push_hyper(self):
        """Grouped path: re-read ``param_groups`` (what a scheduler edits) and, when a value changed, upload the hyper table — an
        asynchronous copy from the pinned mirror on the current stream, so kernels already enqueued keep the old values.  ``step()``
        calls it, except while its stream is capturing; around a captured step the caller does (``GraphedTrainStep`` before every
        replay).  A no-op on the plain path, whose launches take ``param_groups[0]`` as arguments."""
        if not self._grouped:
            return
        rows = self._rows()
        if rows == self._hyper_rows:
            return
        if self._hyper_sent is not None:
            self._hyper_sent.synchronize()
        self._hyper_host.copy_(torch.tensor(rows, dtype=torch.float32))
        self._hyper_dev.copy_(self._hyper_host, non_blocking=True)
        if self._hyper_dev.is_cuda:
            self._hyper_sent = torch.cuda.Event()
            self._hyper_sent.record()
        self._hyper_rows = rows

    def _sync_count(self):
        """push the host's count of updates (``self.t``, just loaded or taken over) to where the kernels read it"""
        if self._scaler is not None:
            self._scaler.state[3] = float(self.t)
        elif self._grouped:
            self._step_dev.fill_(float(self.t))

    # With a scaler attached the count of updates really taken lives on the DEVICE (scaler.state[3]: an overflow-skipped step does
    # not advance it, as apex + torch do not advance 'step'); it is the bias-correction step of the Adam family and what checkpoints
    # carry (a resume used to restart it at 1 under warm moments), so attaching a scaler or loading a state dict keeps
    # the two in step: whichever happens second pushes the loaded count to the device.
    @property
    def scaler(self) -> Optional['DynamicLossScaler']:
        return self._scaler

    @scaler.setter
    def scaler(self, sc: Optional['DynamicLossScaler']):
        # seed the new scaler's device count from the updates really TAKEN so far, read before the swap: with a scaler attached
        # self.t counts step() CALLS (overflow-skipped ones included), and replacing the scaler mid-run from it would inflate the
        # bias corrections
        taken = self.steps_taken()
        self._scaler = sc
        if sc is not None:
            sc.state[3] = float(taken)
        else:
            self.t = taken
            self._sync_count()

    # Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, 2-norm, between backward and step: DETR's --clip_max_norm) inside
    # step(): a setting of the LOOP, as torch's call is — it is not in param_groups and not in checkpoints.  clip_grad_norm_ itself over
    # the gradient views sees what the buckets HOLD: sums over ranks after finish(mean=False), gradients times the loss scale under
    # loss_scale / a DynamicLossScaler; the clipped step takes both factors out of the norm on the device.
    @property
    def max_grad_norm(self) -> Optional[float]:
        """None: no clipping.  May be set between steps; None or 0 turns clipping off, float('inf') measures the norm (``grad_norm``)
        without clipping, torch's idiom."""
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, v: Optional[float]):
        v = None if v is None or float(v) == 0.0 else float(v)
        if v is not None and not v > 0.0:
            raise ValueError(f'max_grad_norm must be positive, None or 0 (off), got {v}')
        self._max_grad_norm = v
        if v is not None and self._clip is None:
            self._clip = self._clip_buffers()

    def _clip_buffers(self):
        dev = self.reducer.buckets[0]['flat'].device
        ws = [torch.empty(int(_lib.lib().svol_grad_sqnorm_ws_bytes(b['flat'].numel())) // 4, dtype=torch.float32, device=dev)
              for b in self.reducer.buckets]
        return {'state': torch.zeros(8, dtype=torch.float32, device=dev),     # include/svol_hip.h, svol_grad_clip_state
                'sq': torch.zeros(len(ws), dtype=torch.float32, device=dev), 'ws': ws}

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """While clipping is on: a 0-dim fp32 DEVICE tensor (a view of the clip state, no host read) holding the last step's total
        2-norm of the TRUE gradient — mean over ranks, loss scale divided out, before clipping; inf / NaN on an overflowed step.
        None while clipping is off."""
        return self._clip['state'][4] if self._max_grad_norm is not None else None

    def steps_taken(self) -> int:
        """Updates really applied (what torch calls 'step'); a host read of the device count when a scaler is attached and on the
        grouped path."""
        if self._scaler is not None:
            return int(self._scaler.state[3].item())
        return int(self._step_dev.item()) if self._grouped else self.t

    # the hyper-parameters live in param_groups[0] (what torch's schedulers edit); attribute access kept for callers
    lr = property(lambda self: self.param_groups[0]['lr'], lambda self, v: self.param_groups[0].__setitem__('lr', float(v)))
    weight_decay = property(lambda self: self.param_groups[0]['weight_decay'])

    def _launch(self, bi, stream, gscale, t=None, state=None):
        """Bucket ``bi``'s update on ``stream``.  ``state`` None: the plain entry (the zeroing one under zero_grads) with step count
        ``t`` and gradient factor ``gscale``.  ``state`` a device vector of the scaler's layout (a DynamicLossScaler's, or the clip
        state): the _scaled entry, a no-op on an overflowed step, whose gradient factor is gscale / state[0]."""
        b, st = self.reducer.buckets[bi], self.flat[bi]
        zero = state is None and self.zero_grads
        name = self._KERNEL + ('_scaled' if state is not None else '_zero' if zero else '')
        tail = (gscale, _ptr(state)) if state is not None else ((t,) if self._HAS_STEP else ()) + (gscale,)
        rc = getattr(_lib.lib(), name)(_ptr(st['p']), _ptr(b['flat']), *(_ptr(st[k]) for k, _ in self._STATE), st['p'].numel(),
                                       *self._hyper(self.param_groups[0]), *tail, stream)
        _lib.check(rc, name)
        if zero:
            b['clean'] = True
        self._ema(bi, stream, t=t if state is None else 0, state=state)

    def _ema(self, bi, stream, t=0, state=None, count=None):
        """Bucket ``bi``'s weight average on ``stream``, directly behind its update launch and driven by what drove that update:
        the same ``state`` vector (nothing is averaged on an overflowed step) and the same source of the count of updates taken
        (``count``, a raw device pointer, on the grouped path; else ``state[3]``; else the host's ``t``), which is the warm-up's
        index.  Nothing at all with ``ema_decay=None``."""
        if self._ema_decay is None:
            return
        st = self.flat[bi]
        rc = _lib.lib().svol_ema_flat(_ptr(st['ema']), _ptr(st['p']), st['p'].numel(), self._ema_decay, int(self.ema_warmup), int(t),
                                      _ptr(state), count, stream)
        _lib.check(rc, 'svol_ema_flat')

    def _clip_state(self, gmul, stream):
        """max_grad_norm set: one sum-of-squares launch per bucket, then one launch that turns the sums into a state vector of the
        scaler's layout ([0] = scale / coef) for the *_scaled update kernels.  Under a loss scaler the sums double as the overflow
        check (a non-finite norm)."""
        L, sc, c = _lib.lib(), self._scaler, self._clip
        for bi, b in enumerate(self.reducer.buckets):
            _lib.check(L.svol_grad_sqnorm(_ptr(b['flat']), b['flat'].numel(), _ptr(c['ws'][bi]), c['sq'].data_ptr() + 4 * bi, stream),
                       'svol_grad_sqnorm')
        _lib.check(L.svol_grad_clip_state(_ptr(c['sq']), len(self.flat), gmul, self._max_grad_norm, float(self.loss_scale), self.t - 1,
                                          _ptr(sc.state) if sc is not None else None, _ptr(c['state']), stream), 'svol_grad_clip_state')
        return c['state']

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._ema_swapped:
            raise RuntimeError('step() inside averaged_weights(): the parameters hold the average')
        if self._grouped:
            self._step_grouped()
            return loss
        L, sc, stream, buckets = _lib.lib(), self._scaler, _stream(), range(len(self.flat))
        gmul = float(self.reducer.pending_scale)
        self.reducer.pending_scale = 1.0
        self.t += 1    # (host-side count of step() calls; under a scaler the DEVICE counts the steps really taken)
        if self._max_grad_norm is None and sc is None:
            gscale = gmul / float(self.loss_scale)
            for bi in buckets:
                if self._stepped[bi]:      # updated during backward (_step_bucket_early), with this step's count
                    self._stepped[bi] = False
                else:
                    self._launch(bi, stream, gscale, t=self.t)
            return loss
        if self._max_grad_norm is not None:
            state = self._clip_state(gmul, stream)
        else:
            # dynamic loss scaling (a static scale with no overflow check lets one inf gradient poison the parameters and the
            # optimizer state for good): the buckets are checked first, every update kernel is a no-op on an overflowed step, then the
            # scale moves
            for b in self.reducer.buckets:
                _lib.check(L.svol_grad_finite(_ptr(b['flat']), b['flat'].numel(), _ptr(sc.state), stream), 'svol_grad_finite')
            state = sc.state
        for bi in buckets:
            self._launch(bi, stream, gmul, state=state)
        if sc is not None:
            _lib.check(L.svol_loss_scaler_update(_ptr(sc.state), sc.growth_factor, sc.backoff_factor, sc.growth_interval, sc.min_scale,
                                                 sc.max_scale, stream), 'svol_loss_scaler_update')
        return loss

    def _step_grouped(self):
        """step() with several param groups or capturable=True: one ..._grouped launch per bucket, which reads its hyper-parameters per
        run from the device table and Adam's step from the device count, then the count moves (the scaler's update, or
        svol_flat_step_advance).  Nothing of the launches depends on a host value that changes from step to step, so a captured
        step replays right: the count advances on the device, and an ``lr`` a scheduler edits arrives through ``push_hyper``."""
        L, sc, stream = _lib.lib(), self._scaler, _stream()
        gmul = float(self.reducer.pending_scale)
        self.reducer.pending_scale = 1.0
        self.t += 1
        if not (self._hyper_dev.is_cuda and torch.cuda.is_current_stream_capturing()):
            self.push_hyper()
        state = None
        if self._max_grad_norm is not None:
            state = self._clip_state(gmul, stream)     # ([3], a host value, is not read by the grouped kernels)
        elif sc is not None:
            for b in self.reducer.buckets:
                _lib.check(L.svol_grad_finite(_ptr(b['flat']), b['flat'].numel(), _ptr(sc.state), stream), 'svol_grad_finite')
            state = sc.state
        else:
            gmul /= float(self.loss_scale)
        count = sc.state.data_ptr() + 12 if sc is not None else _ptr(self._step_dev)
        zero = state is None and self.zero_grads   # (a skipped step zeroes nothing: under a state vector the reducer's own fill runs)
        name = self._KERNEL + '_grouped'
        for bi, (b, st, (ends, groups)) in enumerate(zip(self.reducer.buckets, self.flat, self._seg_dev)):
            rc = getattr(L, name)(_ptr(st['p']), _ptr(b['flat']), *(_ptr(st[k]) for k, _ in self._STATE), st['p'].numel(), _ptr(ends),
                                  _ptr(groups), ends.numel(), _ptr(self._hyper_dev), len(self.param_groups),
                                  _ptr(state), *((count,) if self._HAS_STEP else ()), gmul, int(zero), stream)
            _lib.check(rc, name)
            if zero:
                b['clean'] = True
            self._ema(bi, stream, state=state, count=count)   # in front of the count's advance: the flag and the count the update saw
        if sc is not None:
            _lib.check(L.svol_loss_scaler_update(_ptr(sc.state), sc.growth_factor, sc.backoff_factor, sc.growth_interval, sc.min_scale,
                                                 sc.max_scale, stream), 'svol_loss_scaler_update')
        else:
            _lib.check(L.svol_flat_step_advance(_ptr(self._step_dev), _ptr(state), stream), 'svol_flat_step_advance')

    @torch.no_grad()
    def _step_bucket_early(self, bi, stream):
        """reducer callback (step_in_backward): bucket ``bi``'s gradients are final and ``stream`` is ordered behind every kernel
        that wrote them or read its parameters in this step."""
        if self._scaler is not None or self._max_grad_norm is not None or self._stepped[bi]:
            return   # (the overflow check and the gradient norm span all buckets)
        if self._ema_swapped:
            raise RuntimeError('a backward with step_in_backward inside averaged_weights(): the parameters hold the average')
        world = self.reducer.world
        self._launch(bi, stream, (1.0 / world if world > 1 else 1.0) / float(self.loss_scale), t=self.t + 1)
        self._stepped[bi] = True

    def zero_grad(self, set_to_none=False):
        self.reducer.zero_grad()

    def _views(self, p):
        bi, off, n = self._slot[id(p)]
        st = self.flat[bi]
        return tuple(st[k][off:off + n].view_as(p) for k, _ in self._STATE)

    # The weight average (ema_decay=...): readers, checkpoint state and the exchange for validation.  All of it is off the hot path.
    ema_decay = property(lambda self: self._ema_decay)

    def _need_ema(self, what):
        if self._ema_decay is None:
            raise RuntimeError(f'{what}: this optimizer was built with ema_decay=None')

    def ema_views(self, p):
        """The average of parameter ``p``: shaped like it, a view of the bucket's flat ``'ema'`` buffer (no copy).  Inside
        ``averaged_weights()`` the buffers are exchanged and this view holds the raw weights."""
        self._need_ema('ema_views')
        bi, off, n = self._slot[id(p)]
        return self.flat[bi]['ema'][off:off + n].view_as(p)

    def _averaged(self, p):
        """the average of ``p`` wherever it lives right now"""
        return p.detach() if self._ema_swapped else self.ema_views(p)

    @torch.no_grad()
    def ema_state_dict(self, model: torch.nn.Module):
        """``model.state_dict()`` with every parameter of a gradient bucket replaced by a clone of its average.  Buffers (BatchNorm
        statistics) and parameters outside the buckets (the reducer's skip list, frozen ones) keep their live values."""
        self._need_ema('ema_state_dict')
        sd = model.state_dict()
        for name, p in model.named_parameters(remove_duplicate=False):
            if id(p) in self._slot and name in sd:
                sd[name] = self._averaged(p).clone()
        return sd

    @torch.no_grad()
    def ema_extra_state(self):
        """What a checkpoint carries besides ``ema_state_dict``: ``{'decay', 'warmup', 'step', 'params'}``, ``params`` the averages
        without names, numbered by position in the groups' parameter lists as torch numbers ``state_dict()['state']``; ``step`` the
        updates taken (a host read), which the warm-up continues from under a rule whose own state carries no step (SGD)."""
        self._need_ema('ema_extra_state')
        out, i = {}, 0
        for g in self.param_groups:
            for j, p in enumerate(g['params']):
                if id(p) in self._slot:
                    out[i + j] = self._averaged(p).clone()
            i += len(g['params'])
        return {'decay': self._ema_decay, 'warmup': self.ema_warmup, 'step': self.steps_taken(), 'params': out}

    @torch.no_grad()
    def load_ema_extra_state(self, d):
        """Restore the averages from ``ema_extra_state()``'s dict, by position; ``None``: re-seed them from the current parameters
        (a checkpoint written without an average).  ``decay`` / ``warmup`` stay what this optimizer was built with: they are
        settings of the loop, as ``max_grad_norm`` is.  Call it after ``load_state_dict``."""
        self._need_ema('load_ema_extra_state')
        if self._ema_swapped:
            raise RuntimeError('load_ema_extra_state() inside averaged_weights()')
        if d is None:
            for st in self.flat:
                st['ema'].copy_(st['p'])
            return
        plist = [p for g in self.param_groups for p in g['params']]
        todo = []
        for pos, p in enumerate(plist):
            if id(p) not in self._slot:
                continue
            t = d['params'].get(pos)
            if t is None:
                raise ValueError(f'parameter {pos} has a gradient bucket here and no average in the loaded state')
            if t.numel() != p.numel():
                raise ValueError(f'parameter {pos}: an average of {t.numel()} elements for {p.numel()} weights')
            todo.append((p, t))
        for p, t in todo:
            self.ema_views(p).copy_(t.reshape(p.shape))
        if not self._HAS_STEP and 'step' in d:
            self.t = int(d['step'])
            self._sync_count()

    def _exchange(self):
        with torch.no_grad():
            for st in self.flat:
                tmp = st['p'].clone()
                st['p'].copy_(st['ema'])
                st['ema'].copy_(tmp)
            # caches keyed on a parameter's version (the extractors' frozen-path copies) must see the exchange; the head's and the
            # block plans' 16-bit copies are re-cast from the flat buffers at the next forward anyway (params._WeightCache.new_epoch)
            torch.autograd.graph.increment_version([p for g in self.param_groups for p in g['params'] if id(p) in self._slot])

    @contextlib.contextmanager
    def averaged_weights(self):
        """``with optimizer.averaged_weights(): validate(model)``: on entry the flat parameters and the averages are exchanged, bucket
        by bucket, with plain copies on the current stream (the parameters are views, so the model now IS the averaged model); on
        exit they are exchanged back, and parameters and averages are bit for bit what they were.  The model's 16-bit weight copies
        follow at its next forward.  No ``step()`` inside; raises when nested and inside a stream capture."""
        self._need_ema('averaged_weights')
        if self._ema_swapped:
            raise RuntimeError('averaged_weights() is already entered')
        if self.flat[0]['p'].is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('averaged_weights() inside a stream capture: the exchange is not part of a training step')
        self._exchange()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._exchange()
            self._ema_swapped = False

    def state_dict(self):
        """The schema of the torch optimizer of the same name.  A parameter has a state entry iff it has a slot in a gradient
        bucket and at least one step was taken (torch creates the entry at the first step of a parameter that has a gradient)."""
        state, groups, i = {}, [], 0
        taken = self.steps_taken()   # (not the count of step() calls: overflow-skipped steps are not steps)
        for g in self.param_groups:   # torch's numbering: positions in the groups' parameter lists, one after the other
            for j, p in enumerate(g['params']):
                if taken > 0 and id(p) in self._slot and self._group_keeps_state(g):
                    ent = {'step': torch.tensor(float(taken))} if self._HAS_STEP else {}
                    for (_, name), view in zip(self._STATE, self._views(p)):
                        ent[name] = view.clone()
                    state[i + j] = ent
            group = {k: v for k, v in g.items() if k != 'params'}
            group['params'] = list(range(i, i + len(g['params'])))
            groups.append(group)
            i += len(g['params'])
        return {'state': state, 'param_groups': groups}

    def _group_keeps_state(self, g) -> bool:
        """torch keeps per-parameter state for the parameters of a group with these hyper-parameters"""
        return True

    def _check_group(self, g0):
        """refuse a checkpoint written with options this optimizer does not implement"""
        if g0.get('amsgrad') or g0.get('maximize'):
            raise ValueError('amsgrad / maximize are not supported')

    def _entry_is_empty(self, ent) -> bool:
        """a per-parameter entry of a checkpoint that stands for "no state yet" and is passed over on load"""
        return False

    def load_state_dict(self, sd):
        name = type(self).__name__
        if not self._params_given:
            # torch's schema maps state to parameters BY POSITION in the optimizer's list (train.py:72: named_parameters() order);
            # this optimizer was built in bucket (arrival) order, so the state of the many equal-shaped d x d weights would be
            # silently permuted
            raise ValueError(f'{name}.load_state_dict: build the optimizer with params=<the parameter list in the order the checkpoint '
                             'was written with (the reference: every trainable parameter in named_parameters() order)>')
        groups = sd['param_groups']
        plist = [p for g in self.param_groups for p in g['params']]
        ids = [i for g in groups for i in g['params']]
        if len(ids) != len(plist):
            raise ValueError(f'loaded state dict holds {len(ids)} parameters, the optimizer {len(plist)}')
        if len(self.param_groups) == 1:
            # built with one group: loaded groups that agree are one group, groups that differ need an optimizer built with them
            g0 = groups[0]
            for g in groups[1:]:
                if any(g.get(k) != g0.get(k) for k in self._HYPER):
                    raise ValueError(f'{name} was built with one parameter group: the loaded groups differ in their hyper-parameters')
            loaded = [g0]
        else:   # torch's rule: the same number of groups, of the same sizes; each group's hyper-parameters come from the file
            if len(groups) != len(self.param_groups):
                raise ValueError(f'loaded state dict has {len(groups)} parameter groups, the optimizer {len(self.param_groups)}')
            if any(len(g['params']) != len(own['params']) for g, own in zip(groups, self.param_groups)):
                raise ValueError('loaded state dict has parameter groups of other sizes than the optimizer\'s')
            loaded = groups
        for g in loaded:
            self._check_group(g)
        steps = set()
        todo = []
        for pos, i in enumerate(ids):
            ent = sd['state'].get(i)
            p = plist[pos]
            if ent is None or self._entry_is_empty(ent):
                continue
            lacking = [k for _, k in self._STATE if ent.get(k) is None] + (['step'] if self._HAS_STEP and 'step' not in ent else [])
            if lacking:
                raise ValueError(f'parameter {pos}: the state entry lacks {lacking}')
            if id(p) not in self._slot:
                raise ValueError(f'parameter {pos} has optimizer state but no gradient bucket here')
            for _, k in self._STATE:
                if ent[k].numel() != p.numel():
                    raise ValueError(f'parameter {pos}: {k} of {ent[k].numel()} elements for {p.numel()} weights')
            if self._HAS_STEP:
                steps.add(int(float(ent['step'])))
            todo.append((p, ent))
        if len(steps) > 1:
            raise ValueError(f'per-parameter step counts differ ({sorted(steps)}); {name} keeps one')
        for st in self.flat:
            for k, _ in self._STATE:
                st[k].zero_()
        for p, ent in todo:
            for (_, k), view in zip(self._STATE, self._views(p)):
                view.copy_(ent[k].reshape(p.shape))
        # (a schema without 'step' does not say how many updates were taken; one is enough to know that state exists)
        self.t = (steps.pop() if steps else 0) if self._HAS_STEP else int(bool(todo))
        self._sync_count()
        for grp, g in zip(self.param_groups, loaded):
            for k in self._HYPER + ('initial_lr',):
                if k in g:
                    grp[k] = (float(g[k][0]), float(g[k][1])) if k == 'betas' else float(g[k])


class FlatAdamW(_FlatOptimizer):
    """torch.optim.AdamW (decoupled weight decay, amsgrad off; the reference's optimizer, train.py:98-99) over the reducer's
    flat buckets: the parameters of a bucket are re-homed into ONE flat fp32 buffer (``param.data`` becomes a view, like
    ``param.grad`` already is), the moments are flat too, and a step is one streaming kernel per bucket (``svol_adamw_flat``:
    28 bytes per parameter) instead of torch's multi-tensor launches over ~150 separate tensors (0.44 ms -> 0.15 ms at the
    benchmark size).  Parameters the reducer skips (they never receive a gradient) are not touched, as in torch.

    It IS a ``torch.optim.Optimizer``: one ``param_groups`` entry whose ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` the step
    reads (so ``StepLR`` / ``MultiStepLR`` of the reference loop, train.py:127-130, wrap it), and ``state_dict()`` /
    ``load_state_dict()`` speak torch AdamW's schema — ``{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups':
    [...]}`` with ``i`` indexing ``params`` — so a checkpoint written by the reference (train.py:267-284) resumes here and vice
    versa.  ``params``: the optimizer's parameter list in the REFERENCE's order (train.py:72: every trainable parameter in
    ``named_parameters()`` order, including the ones that never get a gradient and therefore have no state entry); defaults
    to the reducer's own parameters in bucket order."""

    _STATE = (('m', 'exp_avg'), ('v', 'exp_avg_sq'))
    _HYPER = ('lr', 'betas', 'eps', 'weight_decay')
    _KERNEL = 'svol_adamw_flat'

    def __init__(self, reducer: 'BucketedGradAllReduce', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 params: Optional[Iterable[torch.nn.Parameter]] = None, zero_grads: bool = False, step_in_backward: bool = False,
                 max_grad_norm: Optional[float] = None, capturable: bool = False, ema_decay: Optional[float] = None,
                 ema_warmup: bool = True):
        """zero_grads: the update kernel zeroes each gradient bucket behind its read (``svol_adamw_flat_zero``) and the reducer's next
        ``zero_grad()`` skips its fill — the reference loop's ``optimizer.zero_grad()`` (train.py:222) folded into ``step()``; for a
        loop that reads no ``param.grad`` between ``step()`` and ``zero_grad()``.
        step_in_backward: a bucket's update is issued as soon as its gradients are final (behind its all-reduce at world size > 1),
        on the reducer's communication stream, instead of all of them in ``step()`` behind the whole backward; ``step()`` then only
        updates what is left (the last bucket) and closes the step.  Same arithmetic on the same values: the reference's loop has no
        cross-bucket dependency between backward and the update (train.py:229-234).  NOT for a loop that may skip ``step()`` after
        ``backward()``; ignored while a loss scaler is attached (its overflow check spans all buckets) and while ``max_grad_norm``
        is set (so does the gradient norm).
        max_grad_norm: clip the global 2-norm of the gradient inside ``step()`` — ``torch.nn.utils.clip_grad_norm_(params, max_norm)``
        followed by the update, as a DETR-style loop does (``--clip_max_norm``) — on the norm of the TRUE gradient: the pending
        ``1 / world`` of ``finish(mean=False)`` and the loss scale are taken out on the device, which a ``clip_grad_norm_`` call over
        ``param.grad`` cannot do.  One streaming reduction per bucket and a one-thread kernel, no host synchronisation; under a
        loss scaler the reduction replaces the overflow check.  ``zero_grads`` then behaves as under a scaler: the reducer's own
        fill runs.  Without a scaler a non-finite norm skips nothing and behaves as in torch (``error_if_nonfinite=False``).  The
        norm of the last step is ``grad_norm`` (a device tensor).  See the ``max_grad_norm`` property; not part of ``state_dict()``.
        params as torch's list of dicts (``[{'params': [...], 'lr': ...}, {'params': [...]}]``; a missing key takes the constructor's
        value, every bucket parameter belongs to exactly one group): several ``param_groups``, each with hyper-parameters of its own —
        the backbone at a tenth of the head's ``lr`` (``reference_param_groups``), no weight decay on biases and norms — still one
        launch per bucket: the ``..._grouped`` kernels look the group up per run of the bucket's layout.  Schedulers edit every
        group; ``lr`` / ``weight_decay`` attribute access means group 0; checkpoints carry the groups in torch's schema and load
        under torch's rule (the same group count and sizes).  Not with ``step_in_backward``.
        capturable: the same device-side path with one group too, for a ``step()`` that a graph capture records
        (``graph.GraphedTrainStep``): the step count lives on the device, and hyper-parameters reach the kernels through
        ``push_hyper()``, which ``step()`` calls itself except while capturing.  (An attribute of this object, not of the param
        groups: their ``capturable`` key stays torch's default, so that a checkpoint written here loads into a CPU torch optimizer.)
        With one group and ``capturable=False`` the step is the plain path, launch for launch what it was.
        ema_decay: keep an exponential moving average of the weights on the device, ``ema += (1 - d) * (p - ema)`` after every update
        really taken: one more streaming launch per bucket (``svol_ema_flat``, 12 bytes per parameter) directly behind the
        bucket's update, on its stream, under the same overflow flag and the same count of updates — in ``step()`` on every path,
        in a captured step, and during backward under ``step_in_backward``.  A step the loss scaler skips moves neither the average
        nor its warm-up.  ``ema_warmup``: ``d = min(ema_decay, (1 + t) / (10 + t))`` at the t-th update, so that the average
        forgets the initial weights early on.  The average starts as a copy of the weights and lives in ``flat[i]['ema']``;
        ``ema_views(p)``, ``ema_state_dict(model)`` and ``averaged_weights()`` read it, ``ema_extra_state()`` /
        ``load_ema_extra_state()`` carry it through checkpoints (utils.checkpoint does both).  A setting of this object like
        ``max_grad_norm``: not in ``param_groups``, not in ``state_dict()``.  None (the default): no buffer and no launch."""
        super().__init__(reducer, self._defaults(lr, betas, eps, weight_decay), params, zero_grads, step_in_backward, max_grad_norm,
                         capturable, ema_decay, ema_warmup)

    @staticmethod
    def _defaults(lr, betas, eps, weight_decay):
        return dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                    weight_decay=float(weight_decay), amsgrad=False, maximize=False, foreach=None, capturable=False,
                    differentiable=False, fused=None)

    betas = property(lambda self: self.param_groups[0]['betas'])
    eps = property(lambda self: self.param_groups[0]['eps'])

    @staticmethod
    def _hyper(g):
        return float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay'])

    _hyper_row = _hyper   # (the table's row order is this family's argument order)

    def load_state_dict(self, sd):
        if 't' in sd and 'm' in sd:   # round-1 files of this build: flat moments per bucket, layout-dependent
            if len(sd['m']) != len(self.flat) or any(a.numel() != st['m'].numel() for a, st in zip(sd['m'], self.flat)):
                raise ValueError('flat optimizer state does not match this bucket layout')
            self.t, self.lr = int(sd['t']), float(sd['lr'])
            for st, m, v in zip(self.flat, sd['m'], sd['v']):
                st['m'].copy_(m)
                st['v'].copy_(v)
            self._sync_count()
            return
        super().load_state_dict(sd)


class FlatAdam(FlatAdamW):
    """torch.optim.Adam (``--optimizer adam``, train.py:96-97: weight decay as coupled L2 — ``wd * p`` joins the gradient before the
    moments —, amsgrad off) with everything FlatAdamW has: the same flat layout and constructor surface, one ``svol_adam_flat``
    kernel per bucket (28 bytes per parameter), and torch Adam's checkpoint schema ``{'step', 'exp_avg', 'exp_avg_sq'}``."""

    _KERNEL = 'svol_adam_flat'

    def __init__(self, reducer: 'BucketedGradAllReduce', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 params: Optional[Iterable[torch.nn.Parameter]] = None, zero_grads: bool = False, step_in_backward: bool = False,
                 max_grad_norm: Optional[float] = None, capturable: bool = False, ema_decay: Optional[float] = None,
                 ema_warmup: bool = True):
        super().__init__(reducer, lr, betas, eps, weight_decay, params, zero_grads, step_in_backward, max_grad_norm, capturable,
                         ema_decay, ema_warmup)

    @staticmethod
    def _defaults(lr, betas, eps, weight_decay):
        return dict(FlatAdamW._defaults(lr, betas, eps, weight_decay), decoupled_weight_decay=False)

    def _check_group(self, g0):
        super()._check_group(g0)
        if g0.get('decoupled_weight_decay'):
            raise ValueError('decoupled_weight_decay is AdamW: load this checkpoint into FlatAdamW')

    def load_state_dict(self, sd):
        _FlatOptimizer.load_state_dict(self, sd)   # (no round-1 flat format: that predates this class)


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD with momentum (``--optimizer sgd``, train.py:94-95: momentum 0.9, coupled weight decay, dampening 0, nesterov
    off) over the reducer's flat buckets, with the constructor surface and behaviour of FlatAdamW: one ``svol_sgd_flat`` kernel
    per bucket (20 bytes per parameter: p, g and the momentum buffer in, p and the buffer out).  The flat momentum buffer starts
    at zero, which makes the first update torch's ``buf = clone(d)``; ``momentum=0`` is plain SGD.  Checkpoints speak torch SGD's
    schema: ``{'momentum_buffer'}`` per parameter and no 'step', written once an update has been taken (never at momentum 0, where
    torch keeps no buffer either)."""

    _STATE = (('buf', 'momentum_buffer'),)
    _KERNEL = 'svol_sgd_flat'
    _HYPER = ('lr', 'momentum', 'weight_decay')
    _HAS_STEP = False

    def __init__(self, reducer: 'BucketedGradAllReduce', lr=1e-3, momentum=0.9, weight_decay=0.0,
                 params: Optional[Iterable[torch.nn.Parameter]] = None, zero_grads: bool = False, step_in_backward: bool = False,
                 max_grad_norm: Optional[float] = None, capturable: bool = False, ema_decay: Optional[float] = None,
                 ema_warmup: bool = True):
        """zero_grads, step_in_backward, max_grad_norm, capturable, ema_decay / ema_warmup and the list-of-dicts ``params``: see
        FlatAdamW."""
        defaults = dict(lr=float(lr), momentum=float(momentum), dampening=0, weight_decay=float(weight_decay), nesterov=False,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(reducer, defaults, params, zero_grads, step_in_backward, max_grad_norm, capturable, ema_decay, ema_warmup)

    momentum = property(lambda self: self.param_groups[0]['momentum'])

    @staticmethod
    def _hyper(g):
        return float(g['lr']), float(g['momentum']), float(g['weight_decay'])

    @staticmethod
    def _hyper_row(g):
        return float(g['lr']), float(g['momentum']), 0.0, 0.0, float(g['weight_decay'])

    def _group_keeps_state(self, g) -> bool:
        return g['momentum'] != 0

    def _entry_is_empty(self, ent) -> bool:
        return ent.get('momentum_buffer') is None   # (torch SGD keeps momentum_buffer None before a first update and at momentum 0)

    def _check_group(self, g0):
        if g0.get('nesterov') or g0.get('maximize') or g0.get('dampening', 0) != 0:
            raise ValueError('nesterov / dampening / maximize are not supported')


def reference_param_groups(model: torch.nn.Module, args) -> List[dict]:
    """The parameter groups of the recipe the reference carries commented out (train.py:76-90, 104-106): group 0 the trainable
    parameters whose name contains 'backbone' at ``args.lr_backbone`` (the recipe's ``lr * 0.1``; DETR's ``--lr_backbone``), group 1
    the other trainable parameters at ``args.lr``, each in ``named_parameters()`` order.  One group holding every trainable
    parameter (train.py:72) when ``lr_backbone`` is None or no backbone parameter is trainable."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    lr_backbone = getattr(args, 'lr_backbone', None)
    backbone = [p for n, p in named if 'backbone' in n]
    if lr_backbone is None or not backbone:
        return [{'params': [p for _, p in named]}]
    return [{'params': backbone, 'lr': float(lr_backbone)}, {'params': [p for n, p in named if 'backbone' not in n], 'lr': float(args.lr)}]


def build_optimizer(args, reducer: 'BucketedGradAllReduce', params: Optional[Iterable[torch.nn.Parameter]] = None, **kw):
    """The optimizer ``args.optimizer`` names, as the reference's train_setup builds it (train.py:94-99: SGD with momentum 0.9, Adam,
    AdamW, each with ``lr=args.lr, weight_decay=args.wd``), over ``reducer``'s flat buckets.  ``params``: the reference's parameter
    list or torch's list of group dicts, e.g. ``reference_param_groups(model, args)`` (see FlatAdamW); ``kw``: zero_grads /
    step_in_backward / max_grad_norm / capturable / ema_decay / ema_warmup.  ``args.clip_max_norm`` > 0 (DETR's option, configs.py)
    becomes ``max_grad_norm`` and ``args.model_ema_decay`` (not None) ``ema_decay``, each unless ``kw`` names one."""
    if 'ema_decay' not in kw and getattr(args, 'model_ema_decay', None) is not None:
        kw['ema_decay'] = float(args.model_ema_decay)
    if 'max_grad_norm' not in kw and (getattr(args, 'clip_max_norm', 0) or 0) > 0:
        kw['max_grad_norm'] = float(args.clip_max_norm)
    if args.optimizer == 'sgd':
        return FlatSGD(reducer, lr=args.lr, momentum=0.9, weight_decay=args.wd, params=params, **kw)
    if args.optimizer == 'adam':
        return FlatAdam(reducer, lr=args.lr, weight_decay=args.wd, params=params, **kw)
    if args.optimizer == 'adamw':
        return FlatAdamW(reducer, lr=args.lr, weight_decay=args.wd, params=params, **kw)
    raise ValueError(f"--optimizer {args.optimizer!r}: choose one of 'sgd', 'adam', 'adamw'")


class StepFence:
    """Bounds how far the host may run ahead of the GPU: ``tick()`` at the end of a training step records an event and waits (spinning,
    no interrupt) for the step ``max_inflight`` steps back.  With the block programs a step takes ~6 ms of host time against ~20 ms
    on the GPU, so an unfenced loop queues a dozen steps (>5000 packets over three streams) within a few iterations; at that depth
    the HIP runtime's own back-pressure (kernel-argument pool / signal recycling) takes over, and that wait was measured to stall
    host AND GPU for 0.1 - 1.7 s at a time (profiles/round3_summary.md, "host run-ahead").  Two steps in flight keep the queue full
    without ever reaching it.  The reference's loop is fenced the same way by its per-step ``loss.item()`` logging
    (lib/engine/train.py:233-240)."""

    def __init__(self, max_inflight: int = 2):
        from collections import deque
        self.max_inflight = max(1, int(max_inflight))
        self._q = deque()

    def tick(self) -> None:
        ev = torch.cuda.Event()
        ev.record()
        self._q.append(ev)
        while len(self._q) > self.max_inflight:
            self._q.popleft().synchronize()

    def drain(self) -> None:
        while self._q:
            self._q.popleft().synchronize()


def unused_parameters(model: torch.nn.Module):
    """Parameters that never receive a gradient (reference: grad None): the SVANet gate MHA's out_proj
    (only its attention WEIGHTS are used), the unused ``class_head``, and — svanet_variants — the input projections of
    the fusion modes the model was not built for."""
    mode = getattr(model, 'mode', None) or getattr(getattr(model, 'head', None), 'mode', None)
    dead = {'concat_to_seq': ('input_sketch_proj', 'input_video_proj', 'input_query_proj'),
            'append_to_seq': ('input_proj.', 'input_query_proj'),
            'concat_to_qry': ('input_proj.', 'input_sketch_proj')}.get(mode, ())
    # sketch_attn 'tokens' (video tokens attending to the sketch's tokens): that MHA's value and output projections are used and train
    tokens = any(getattr(m, 'sketch_attn', None) == 'tokens' for m in model.modules())
    out = []
    for name, p in model.named_parameters():
        if ('sketch_video_cross_attn.out_proj' in name and not tokens) or 'class_head' in name or any(d in name for d in dead):
            out.append(p)
    return out


def reduce_scalar_mean(t: torch.Tensor) -> torch.Tensor:
    """reduce_tensor of the reference (lib/utils/comm.py:21-25): mean of a logged scalar over ranks."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return t.clone()
    rt = t.detach().clone()
    dist.all_reduce(rt, op=dist.ReduceOp.SUM)
    rt /= dist.get_world_size()
    return rt
