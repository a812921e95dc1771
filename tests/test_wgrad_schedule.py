"""svol_amd.wgrad without a device: the routing decision against a table written out from its two conditions, and the queue
(plain callables, CPU autograd): armed flush, failed backward, drop, first-in first-out, the large-attention counter."""
import itertools

import pytest
import torch

from svol_amd import wgrad

I, N, Q = wgrad.INLINE, wgrad.NOW, wgrad.QUEUED
# inline when not async or (not capture allowed and capturing); else queued when defer and outstanding > 0 and not capturing; else now
#  (async, capture allowed, capturing, defer): outstanding 0, 1, 2
ROUTES = {
    (0, 0, 0, 0): (I, I, I), (0, 0, 0, 1): (I, I, I), (0, 0, 1, 0): (I, I, I), (0, 0, 1, 1): (I, I, I),
    (0, 1, 0, 0): (I, I, I), (0, 1, 0, 1): (I, I, I), (0, 1, 1, 0): (I, I, I), (0, 1, 1, 1): (I, I, I),
    (1, 0, 0, 0): (N, N, N), (1, 0, 0, 1): (N, Q, Q), (1, 0, 1, 0): (I, I, I), (1, 0, 1, 1): (I, I, I),
    (1, 1, 0, 0): (N, N, N), (1, 1, 0, 1): (N, Q, Q), (1, 1, 1, 0): (N, N, N), (1, 1, 1, 1): (N, N, N),
}


def test_routing_table():
    seen = 0
    for a, c, cap, d in itertools.product((0, 1), repeat=4):
        for left in (0, 1, 2):
            assert wgrad.route(bool(a), bool(c), bool(cap), bool(d), left) is ROUTES[(a, c, cap, d)][left], (a, c, cap, d, left)
            seen += 1
    assert seen == 48 and len(ROUTES) == 16


@pytest.fixture(autouse=True)
def fresh():
    def reset():
        with torch.no_grad():
            wgrad.forward_starts()
        assert state() == (0, False, 0)
    reset()
    yield
    reset()


def state():
    return len(wgrad._pending), wgrad._armed, wgrad._big_attn


class _Queues(torch.autograd.Function):
    """identity whose backward queues `item`."""

    @staticmethod
    def forward(ctx, x, item):
        ctx.item = item
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        wgrad.enqueue(ctx.item)
        return g, None


class _Raises(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('this node fails')


def test_item_queued_in_a_backward_has_run_when_backward_returns():
    ran = []
    x = torch.ones(3, requires_grad=True)
    _Queues.apply(x, lambda: ran.append(state())).sum().backward()
    assert ran == [(0, False, 0)]   # (run by the engine's callback: the queue was already taken, the flush disarmed)
    assert state() == (0, False, 0)
    assert torch.equal(x.grad, torch.ones(3))


def test_queueing_outside_a_backward_does_not_arm():
    ran = []
    wgrad.enqueue(lambda: ran.append(1))
    assert ran == [] and state() == (1, False, 0)
    wgrad.drop_pending()
    assert ran == [] and state() == (0, False, 0)


def test_failed_backward_leaves_the_item_pending_and_armed_until_dropped():
    ran = []
    x = torch.ones(3, requires_grad=True)
    y = _Queues.apply(_Raises.apply(x), lambda: ran.append(1))   # backward: _Queues first, then the node that raises
    with pytest.raises(RuntimeError, match='this node fails'):
        y.sum().backward()
    assert ran == [] and state() == (1, True, 0)
    wgrad.forward_starts()                                       # gradients enabled, flush armed: not this call's to drop
    assert ran == [] and state() == (1, True, 0)
    wgrad.drop_pending()
    assert ran == [] and state() == (0, False, 0)


def test_forward_start_drops_what_is_not_armed_and_everything_without_grad():
    wgrad.enqueue(lambda: None)
    wgrad.forward_starts()
    assert state() == (0, False, 0)
    x = torch.ones(3, requires_grad=True)
    with pytest.raises(RuntimeError, match='this node fails'):
        _Queues.apply(_Raises.apply(x), lambda: None).sum().backward()
    assert state() == (1, True, 0)
    with torch.no_grad():
        wgrad.forward_starts()
    assert state() == (0, False, 0)


def test_flush_is_first_in_first_out_and_leaves_what_an_item_queues():
    ran = []
    wgrad.enqueue(lambda: ran.append('a'))
    wgrad.enqueue(lambda: (ran.append('b'), wgrad.enqueue(lambda: ran.append('d'))))
    wgrad.enqueue(lambda: ran.append('c'))
    wgrad.flush()
    assert ran == ['a', 'b', 'c'] and state() == (1, False, 0)
    wgrad.flush()
    assert ran == ['a', 'b', 'c', 'd'] and state() == (0, False, 0)
    wgrad.flush()
    assert ran == ['a', 'b', 'c', 'd']


def test_run_behind_pending():
    ran = []
    wgrad.run_behind_pending(lambda: ran.append('now'))
    assert ran == ['now'] and state() == (0, False, 0)
    wgrad.enqueue(lambda: ran.append('first'))
    wgrad.run_behind_pending(lambda: ran.append('behind'))
    assert ran == ['now'] and state() == (2, False, 0)
    wgrad.flush()
    assert ran == ['now', 'first', 'behind']


def test_run_behind_pending_arms_inside_a_backward():
    ran = []

    class _Behind(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            wgrad.run_behind_pending(lambda: ran.append('behind'))
            ran.append('node')
            return g

    x = torch.ones(3, requires_grad=True)
    _Queues.apply(_Behind.apply(x), lambda: ran.append('first')).sum().backward()   # backward: _Queues first, so something is pending
    assert ran == ['node', 'first', 'behind'] and state() == (0, False, 0)


def test_large_attention_counter():
    assert wgrad.MIN_SCORES == 1 << 27
    ran = []
    assert wgrad.attn_forward(wgrad.MIN_SCORES - 1) is False and state() == (0, False, 0)
    wgrad.enqueue(lambda: ran.append(wgrad._big_attn))
    wgrad.attn_backward(wgrad.MIN_SCORES - 1)          # below the threshold: no decrement, no flush
    assert ran == [] and state() == (1, False, 0)
    assert wgrad.attn_forward(wgrad.MIN_SCORES) is True and wgrad.attn_forward(8 * 8 * 6272 * 6272) is True
    assert state() == (1, False, 2)
    wgrad.attn_backward(8 * 8 * 6272 * 6272)           # decrement, THEN flush: the item sees 1
    assert ran == [1] and state() == (0, False, 1)
    wgrad.attn_backward(wgrad.MIN_SCORES)
    assert state() == (0, False, 0)
    wgrad.attn_forward(wgrad.MIN_SCORES)
    wgrad.forward_starts()
    assert state() == (0, False, 0)
