"""The fp64 twin of the weight average (tests/ema_ref.py) against what is known in closed form: it is the yardstick of
tests/test_gpu_flat_ema.py, so it is pinned first."""
import math

import numpy as np
import pytest
import torch

from tests import ema_ref


def test_schedule_first_values_and_where_it_reaches_the_decay():
    want = [2 / 11, 3 / 12, 4 / 13, 5 / 14, 6 / 15]
    for t, w in enumerate(want, 1):
        assert ema_ref.decay_at(0.999, True, t) == pytest.approx(w, rel=1e-15)
    # (1 + t) / (10 + t) >= decay  <=>  t >= (10 decay - 1) / (1 - decay): 8 at 0.5, 26 at 0.75 (both exact in fp32)
    for decay, first in ((0.5, 8), (0.75, 26)):
        ds = [ema_ref.decay_at(decay, True, t) for t in range(1, first + 5)]
        assert all(d < decay for d in ds[:first - 1]) and all(d == decay for d in ds[first - 1:]), (decay, ds)
        assert all(a < b for a, b in zip(ds[:first - 1], ds[1:first]))          # rising until then
    # the decay is an fp32 input: 0.99 means float32(0.99), and the schedule reaches THAT at t = 891, not at the real 890
    d32 = float(np.float32(0.99))
    assert ema_ref.decay_at(0.99, False, 1) == d32 == ema_ref.decay_at(0.99, True, 10 ** 6)
    first = math.ceil((10 * d32 - 1) / (1 - d32))
    assert first == 891 and ema_ref.decay_at(0.99, True, first - 1) < d32 == ema_ref.decay_at(0.99, True, first)
    assert ema_ref.decay_at(0.0, True, 5) == 0.0 and ema_ref.decay_at(1.0, True, 5) == 6 / 15


@pytest.mark.parametrize('decay,warmup', [(0.5, True), (0.99, True), (0.99, False), (0.0, False), (1.0, False)])
def test_recursion_against_the_closed_form_for_a_constant_p(decay, warmup):
    """ema_K = p + (ema_0 - p) * prod_i d_i"""
    g = torch.Generator().manual_seed(5)
    p, e0 = torch.randn(257, generator=g), torch.randn(257, generator=g)
    K = 40
    run = ema_ref.ema_run(e0, [p] * K, decay, warmup)
    assert len(run) == K and run[-1].dtype == torch.float64
    prod = 1.0
    for k in range(1, K + 1):
        prod *= ema_ref.decay_at(decay, warmup, k)
        want = p.double() + (e0.double() - p.double()) * prod
        # relative to the terms of the sum, not to a result that the two may cancel into (an element with p ~ -(ema_0 - p) prod)
        scale = p.double().abs() + (e0.double() - p.double()).abs() * prod
        assert float(((run[k - 1] - want).abs() / scale).max()) <= 1e-12, k
    if decay == 1.0:
        assert torch.equal(run[-1], e0.double())
    if decay == 0.0:
        assert torch.equal(run[-1], p.double())


def test_t0_continues_the_schedule_and_the_bar_is_zero_where_nothing_moves():
    g = torch.Generator().manual_seed(6)
    e0 = torch.randn(64, generator=g)
    ps = [torch.randn(64, generator=g) for _ in range(6)]
    whole = ema_ref.ema_run(e0, ps, 0.9, True)
    rest = ema_ref.ema_run(whole[2].float().double(), ps[3:], 0.9, True, t0=4)
    again = ema_ref.ema_run(whole[2], ps[3:], 0.9, True, t0=4)
    assert all(torch.equal(a, b) for a, b in zip(again, whole[3:]))
    assert not torch.equal(rest[-1], whole[-1])                 # (the fp32 round trip in between is visible in fp64)
    ref = ema_ref.ema_step(e0, e0, 0.3)
    assert torch.equal(ref, e0.double())
    assert torch.equal(ema_ref.bound(ref, e0, e0, 0.3), 2.0 ** -23 * e0.double().abs())
    ema_ref.check(e0, e0, e0, 0.3, 'p == ema')
    with pytest.raises(AssertionError):
        ema_ref.check(e0 * (1 + 2.0 ** -21), e0, e0, 0.3, 'four ulps off')
