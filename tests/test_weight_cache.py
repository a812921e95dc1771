"""params._WeightCache against the recording stand-in for the library (tests/test_perop_launches.py): which casts it launches and when,
what the descriptor table of the per-epoch multi-weight refresh holds, and what ``BlockPlan.fresh_copies`` makes of its answers."""
import ctypes
import gc
import struct

import torch

from svol_amd import blocks
from svol_amd import params as P
from tests.test_perop_launches import rec  # noqa: F401  (the fixture)

BF = torch.bfloat16
RECORD = '<QQQQiiii'   # src, dst, dstT, dstS ; R, C, tiles_c, tile_begin


def _table(call):
    """the records behind a svol_cast_transpose_multi call"""
    name, (ptr, n, tiles, dt, stream) = call
    assert name == 'cast_transpose_multi'
    return list(struct.iter_unpack(RECORD, ctypes.string_at(ptr, n * struct.calcsize(RECORD)))), tiles, dt


def _two():
    return torch.nn.Parameter(torch.randn(32, 16)), torch.nn.Parameter(torch.randn(32, 16))


def test_cache_call_sequence(rec):  # noqa: F811
    W = P._WeightCache()
    a, b = _two()
    wa, wb = W.get(a, BF), W.get(b, BF)
    assert rec.names() == ['cast_transpose', 'cast_transpose']     # first sight: cast on the spot
    again = W.get(a, BF)
    assert len(rec.calls) == 2 and all(x is y for x, y in zip(again, wa))   # same epoch: no call, the same tensors

    W.new_epoch()
    assert rec.names(2) == ['cast_transpose_multi']                # one launch for the whole (device, dtype) set
    recs, tiles, dt = _table(rec.calls[2])
    assert recs == [(a.data_ptr(), wa[0].data_ptr(), wa[1].data_ptr(), 0, 32, 16, 1, 0),
                    (b.data_ptr(), wb[0].data_ptr(), wb[1].data_ptr(), 0, 32, 16, 1, 1)]
    assert (tiles, dt) == (2, 1)
    assert all(x is y for x, y in zip(W.get(a, BF), wa)) and len(rec.calls) == 3   # refreshed: a hit

    hl = W.get_split(a, 16, 16)
    assert rec.names(3) == ['cast_split'] and tuple(hl.shape) == (16, 32) and hl.dtype == BF
    assert rec.calls[3][1][0] == a.data_ptr() + 16 * 16 * 4
    W.new_epoch()
    recs, tiles, _ = _table(rec.calls[4])
    assert len(recs) == 3 and recs[2] == (a.data_ptr() + 16 * 16 * 4, 0, 0, hl.data_ptr(), 16, 16, 1, 2) and tiles == 3

    del b
    gc.collect()
    W.new_epoch()
    recs, tiles, _ = _table(rec.calls[5])
    assert [r[0] for r in recs] == [a.data_ptr(), a.data_ptr() + 16 * 16 * 4] and [r[7] for r in recs] == [0, 1] and tiles == 2

    with torch.no_grad():
        a.add_(1.0)                                                  # a version bump: re-cast INTO the same buffers
    n = len(rec.calls)
    assert all(x is y for x, y in zip(W.get(a, BF), wa)) and W.get_split(a, 16, 16) is hl
    assert rec.names(n) == ['cast_transpose', 'cast_split']
    assert rec.calls[n][1][:3] == (a.data_ptr(), wa[0].data_ptr(), wa[1].data_ptr()) and rec.calls[n + 1][1][2] == hl.data_ptr()

    W.static = True
    n, epoch = len(rec.calls), W.epoch
    W.new_epoch()
    assert len(rec.calls) == n and W.epoch == epoch                # frozen weights: nothing is refreshed
    assert all(x is y for x, y in zip(W.get(a, BF), wa)) and len(rec.calls) == n


def test_fp32_copy_is_the_master_weight(rec):  # noqa: F811
    W = P._WeightCache()
    a, _ = _two()
    wc, wt = W.get(a, torch.float32)
    assert wc.data_ptr() == a.data_ptr() and tuple(wt.shape) == (16, 32)
    assert rec.calls[0][1][:3] == (a.data_ptr(), 0, wt.data_ptr())
    W.new_epoch()
    recs, _, dt = _table(rec.calls[1])
    assert recs == [(a.data_ptr(), 0, wt.data_ptr(), 0, 32, 16, 1, 0)] and dt == 0


def test_fresh_copies_follows_object_identity(rec):  # noqa: F811
    W = P._WeightCache()
    a, b = _two()
    plan = blocks.BlockPlan.__new__(blocks.BlockPlan)
    plan.casts = [(W.get, (a, BF), W.get(a, BF)), (W.get, (b, BF), W.get(b, BF)), (W.get_split, (a, 16, 16), W.get_split(a, 16, 16))]
    held = [t for c in plan.casts for t in (c[2] if isinstance(c[2], tuple) else (c[2],))]
    assert plan.fresh_copies()
    W.new_epoch()
    with torch.no_grad():
        b.mul_(2.0)
    n = len(rec.calls)
    assert plan.fresh_copies() and rec.names(n) == ['cast_transpose']   # stale: re-cast into its buffer, the plan stays valid
    now = list(W.get(a, BF)) + list(W.get(b, BF)) + [W.get_split(a, 16, 16)]
    assert all(x is y for x, y in zip(now, held))
    b.data = b.data.clone()                                             # the parameter moved: new buffers, the plan is void
    assert not plan.fresh_copies()
    assert W.get(b, BF)[1] is not held[3]
    plan.casts = plan.casts[:1] + plan.casts[2:]
    assert plan.fresh_copies()
    a.data = a.data.clone()
    plan.casts = plan.casts[1:]                                         # the split copy alone
    assert not plan.fresh_copies() and W.get_split(a, 16, 16) is not held[4]
