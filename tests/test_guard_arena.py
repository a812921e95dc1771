"""tests/guard_arena.py on the CPU: the fill words mean what their table says in all three operand types, and the arena plans,
builds, refills and checks dense and strided slots."""
import math

import pytest
import torch

from tests.guard_arena import FILLS, HUGE_WORD, NAN_WORD, NEG0, GuardArena


def _decode(word, dtype):
    w = word - (1 << 32) if word >= (1 << 31) else word
    return torch.tensor([w], dtype=torch.int32).view(dtype).double().tolist()


def test_fill_words_decode_to_their_table():
    assert _decode(NAN_WORD, torch.float32) != _decode(NAN_WORD, torch.float32)   # NaN != NaN
    for dt, n in ((torch.float32, 1), (torch.bfloat16, 2), (torch.float16, 2)):
        got = _decode(NAN_WORD, dt)
        assert len(got) == n and all(math.isnan(x) for x in got), (dt, got)
    f32, = _decode(HUGE_WORD, torch.float32)
    assert f32 == 2.0 ** 119 * (1 + 0x7B00 / 2.0 ** 23) and abs(f32 / 6.67e35 - 1) < 1e-3
    assert _decode(HUGE_WORD, torch.bfloat16) == [2.0 ** 119] * 2 and abs(2.0 ** 119 / 6.65e35 - 1) < 1e-3
    assert _decode(HUGE_WORD, torch.float16) == [57344.0] * 2
    neg0, = _decode(NEG0 & 0xFFFFFFFF, torch.float32)
    assert neg0 == 0.0 and math.copysign(1.0, neg0) == -1.0
    assert [n for n, _ in FILLS] == ['neg0', 'nan', 'huge'] and [w & 0xFFFFFFFF for _, w in FILLS] == [0x80000000, 0x7FC07FC0, 0x7B007B00]


def _arena(**kw):
    ar = GuardArena(device='cpu', **kw)
    ar.plan('a', (5, 7), torch.float32)
    ar.plan('packed_k', (9, 16), torch.bfloat16, ld=48, col=16)
    ar.plan('idx', (13,), torch.uint8)
    ar.plan('slice32', (4, 6), torch.float32, ld=10, col=3)
    ar.plan('h', (3, 10), torch.float16)
    return ar, ar.build()


def test_cpu_arena_plans_builds_refills_and_checks():
    ar, t = _arena()
    assert ar.guard == (1 << 18) // 4 and ar.fill == NEG0
    assert t['a'].shape == (5, 7) and t['a'].is_contiguous()
    assert t['packed_k'].shape == (9, 16) and t['packed_k'].stride() == (48, 1) and t['packed_k'].dtype == torch.bfloat16
    assert t['slice32'].stride() == (10, 1) and t['idx'].dtype == torch.uint8
    for v in t.values():
        assert v.data_ptr() % 4 == 0
        assert ar.buf.data_ptr() + ar.guard * 4 <= v.data_ptr() < ar.buf.data_ptr() + (ar.buf.numel() - ar.guard) * 4
    assert t['a'].data_ptr() % 256 == ar.buf.data_ptr() % 256          # 256-byte aligned starts relative to the allocation
    ar.check('fresh')
    for v in t.values():            # writing every element of every view touches no guard or gap
        v.fill_(1)
    ar.check('views written')
    for _, word in FILLS[1:]:
        ar.refill(word)
        ar.check('refilled')
        assert int((ar.buf == ar.fill).sum()) >= ar.buf.numel() - sum(v.numel() for v in t.values())
    # the guard in front of the first buffer and behind the last
    ar.buf[0] = 5
    with pytest.raises(AssertionError, match='guard word 0 changed'):
        ar.check('front')
    ar.buf[0] = ar.fill
    ar.buf[-1] = 5
    with pytest.raises(AssertionError, match='guard word'):
        ar.check('back')


def test_changed_gap_word_of_a_strided_slot_is_reported_by_name():
    ar, t = _arena(fill=NAN_WORD)
    o = ar.slots['packed_k'][0]
    rows = ar.buf[o:o + 9 * 24].view(9, 24)                     # 48 bf16 = 24 words per row; the view is words 8 .. 15
    for r, w in ((0, 7), (4, 16), (8, 23), (3, 0)):
        old = int(rows[r, w])
        rows[r, w] = 1
        with pytest.raises(AssertionError, match="strided slot 'packed_k'"):
            ar.check('gap')
        rows[r, w] = old
        ar.check('restored')
    rows[2, 8:16] = 3                                           # the view itself is free
    ar.check('view')
    o = ar.slots['slice32'][0]
    ar.buf[o + 10 + 2] = 9                                      # row 1, column 2: left of the view
    with pytest.raises(AssertionError, match="strided slot 'slice32'"):
        ar.check('gap32')


def test_refill_leaves_taken_ranges_bit_identical():
    ar, t = _arena()
    g = torch.Generator().manual_seed(1)
    for v in t.values():
        v.view(torch.uint8 if v.dtype == torch.uint8 else {2: torch.int16, 4: torch.int32}[v.element_size()]).copy_(
            torch.randint(-100, 100, v.shape, generator=g))
    before = {k: v.clone() for k, v in t.items()}
    raw = lambda x: x.contiguous().view(torch.uint8)
    for _, word in FILLS[::-1]:
        ar.refill(word)
        ar.check('refill')
        for k, v in t.items():
            assert torch.equal(raw(v), raw(before[k])), k


def test_plan_refuses_slots_that_are_not_whole_words():
    ar = GuardArena(device='cpu')
    with pytest.raises(ValueError):
        ar.plan('odd', (4, 5), torch.bfloat16, ld=16, col=0)
    with pytest.raises(ValueError):
        ar.plan('wide', (4, 8), torch.bfloat16, ld=12, col=6)
    with pytest.raises(ValueError):
        ar.plan('nold', (4, 8), torch.bfloat16, col=2)
