"""Weight-gradient scheduling: where and when a dW = dY^T X launch group runs.  This module owns all of that state.

dW is needed by nobody until the optimizer step (or the bucket's all-reduce), while the dX chain behind it IS the critical path of
backward.  When the gradient lands in a reducer-owned bucket (a "sink": persistent memory, no autograd consumer), the launches are
issued on a dedicated stream that waits for the producing stream's work so far and is joined by BucketedGradAllReduce (before a
bucket's all-reduce and in finish()).  The split-M TN kernels are HBM / atomic bound, the attention-backward kernels they now run
beside are instruction-issue bound: the two overlap almost for free.

Deferral: the video attention backward — 1.3 ms per layer — is the part of the backward the weight-gradient GEMMs disturb least.  So a
launch group is only QUEUED (with an event that says "its operands exist") and the queue is flushed onto the weight-gradient stream
right before the next large attention backward is launched, before a bucket's all-reduce, and in BucketedGradAllReduce.finish()
(same-box A/B: -0.2 ms per step).  The autograd engine runs every backward node of a device on one thread, so the queue needs no lock.

Two variants were measured slower and are gone.  GATING the flushed launches behind an event recorded right before the attention
backward: round 3's two-pass backward (256 VGPRs, two workgroups per CU) gained from it, round 4's single-pass backward owns a CU's
whole register file (one 512-register wave per SIMD) and a gated GEMM only takes CUs away from it between its workgroup rounds —
19.72 ms/step gated (attention backward 1.31 ms in the step against 1.04 alone) against 19.45 ungated, +0.27 ms.  SPLITTING a video
half's weight gradients so that its MLP / out-projection part goes beside its OWN attention backward: +0.16 ms/step (more work beside
the attention backward than the shorter tail saves).
"""
from __future__ import annotations

import os

import torch

ASYNC = os.environ.get('SVOL_NO_WGRAD_STREAM') is None
DEFER = os.environ.get('SVOL_NO_WGRAD_DEFER') is None
IN_CAPTURE = False   # (svol_amd.graph: a captured step keeps everything on one stream unless told otherwise)
MIN_SCORES = 1 << 27   # B*H*Lq*Lk of an attention backward worth hiding weight gradients under (cfg2: 2.5e9)
INLINE, NOW, QUEUED = 'inline', 'now', 'queued'

_streams = {}
_pending = []
_armed = False
_big_attn = 0   # large attention forwards of this step whose backward has not run yet: nothing is deferred once it reaches 0
                # (after the first layer's attention backward there is nothing left to hide under)


def route(async_on, capture_ok, capturing, defer, outstanding):
    """INLINE on the current stream, NOW on the weight-gradient stream, or QUEUED until the next flush."""
    if not async_on or (not capture_ok and capturing):
        return INLINE
    if defer and outstanding > 0 and not capturing:
        return QUEUED
    return NOW


def streams(dev):
    """streams weight-gradient launches have been issued on for `dev` (svol_amd.parallel joins them)."""
    s = _streams.get(torch.device(dev) if not isinstance(dev, torch.device) else dev)
    return [s] if s is not None else []


def _stream(dev):
    ws = _streams.get(dev)
    if ws is None:
        ws = _streams[dev] = torch.cuda.Stream(device=dev)
    return ws


def issue(run, keep, cur, defer=True, capture_ok=None):
    """A weight-gradient launch group whose targets are all sinks: nothing on the current stream `cur` may read them before
    BucketedGradAllReduce.finish().  ``run(stream)`` launches it, `keep` are the tensors it reads.  Returns False, having done
    nothing, when it belongs in line on `cur` (the caller launches it there); else it runs, now or from the queue, on the
    weight-gradient stream behind an event recorded on `cur` here.  ``defer=False``: never queued; ``capture_ok=False``: in line
    under any stream capture."""
    capturing = torch.cuda.is_current_stream_capturing()
    r = route(ASYNC, IN_CAPTURE if capture_ok is None else capture_ok, capturing, DEFER and defer, _big_attn)
    if r is INLINE:
        return False
    ev = torch.cuda.Event()
    ev.record(cur)

    def later():
        ws = _stream(cur.device)
        ws.wait_event(ev)
        run(ws)   # (explicit stream: no current-stream switch on the host unless `run` makes one)
        for t in keep:
            t.record_stream(ws)

    if r is QUEUED:
        enqueue(later)
    else:
        later()
    return True


def enqueue(item):
    """queue a callable for the next flush, and make the autograd engine drain the queue before ``backward()`` returns, so a caller
    that never reaches ``BucketedGradAllReduce.finish()`` (an exception, a skipped batch) cannot leak a failed step's weight-gradient
    GEMMs into the next step's freshly zeroed buckets."""
    global _armed
    _pending.append(item)
    if _armed:
        return
    try:
        torch.autograd.Variable._execution_engine.queue_callback(_final_flush)
        _armed = True
    except RuntimeError:   # not inside a backward pass: finish() / the next flush point drains the queue
        pass


def run_behind_pending(item):
    """`item` now when nothing is queued, else from the queue behind what is (the deferral keeps its schedule)."""
    if _pending:
        enqueue(item)
    else:
        item()


def flush():
    """issue every queued item, first in first out (callables that put their launches on the weight-gradient stream behind the event
    recorded when they were queued); what an item queues stays for the next flush."""
    items = list(_pending)
    _pending.clear()
    for it in items:
        it()


def _final_flush():
    global _armed
    _armed = False
    flush()


def drop_pending():
    """a new step starts: whatever a FAILED backward left queued must not run into this step's buffers."""
    global _armed
    _pending.clear()
    _armed = False


def forward_starts():
    """a new forward starts: no large attention is outstanding, and nothing is queued (an armed flush belongs to a backward that is
    still running: leave it alone)."""
    global _big_attn
    _big_attn = 0
    if not torch.is_grad_enabled() or not _armed:
        drop_pending()


def attn_forward(scores):
    """the forward of an attention over `scores` = B*H*Lq*Lk scores is being launched -> whether it counts as large."""
    global _big_attn
    big = scores >= MIN_SCORES
    if big:
        _big_attn += 1
    return big


def attn_backward(scores):
    """the backward of that attention is about to be launched: the queued weight-gradient GEMMs run beside it (issue-bound; they are
    HBM / atomic bound)."""
    global _big_attn
    if scores >= MIN_SCORES:
        _big_attn -= 1
        flush()
