"""The test of tests/test_gpu_attn_dropout.py, on the fp64 reference alone (plain torch, CPU): the mask probes recover the twin's mask
bit for bit before any kernel is asked, every probe notices each fault a kernel's mask generation could plausibly have, the slice
bars catch a fault confined to one 128 x 128 tile, no reference slice is measured against slice_metrics' floor, and the bars are
what the emulation gives."""
import pytest
import torch

from tests import attn_dropout_ref as R
from tests import slice_metrics as S
from tests.test_gpu_attn_dropout import BARS, EMULATED

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
KINDS = ['fwd', 'dv', 'dq', 'dk']
SEED = R.SEEDS[1]
BAR16 = max(BARS[BF16], BARS[FP16])


def _dims(name):
    return R.CASES[name][:5]


def test_written_out_formula_is_the_autograd_reference():
    """the emulation without roundings is the reference: what the bars are derived from is the formula the device is held to"""
    for name in ('M1', 'S3'):
        q, qref, k, v, do = R.make_inputs(name, BF16, R.premuls(R.CASES[name][4])[1])
        kb, keep = R.key_bias(name), R.keep_mask(name, 0.1, SEED)
        o, _, dq, dk, dv = R.reference(qref, k, v, do, kb, keep, 0.1, _dims(name))
        for tag, a, b in zip(('o', 'dq', 'dk', 'dv'), R.emulate(qref, k, v, do, kb, keep, 0.1, _dims(name)), (o, dq, dk, dv)):
            assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), (name, tag)


@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=lambda d: R.DT_NAME[d])
def test_bars_are_three_times_the_emulation(dtype):
    """the recorded worst point of the emulation, re-derived (16-bit: fp64 arithmetic with exact roundings, reproducible to the last
    digits recorded; fp32: the summation order of the host's fp32 matrix product moves it, so to 30 %)"""
    emu, (name, premul_on, p, seed_i) = EMULATED[dtype]
    e = R.emulation_error(name, dtype, R.premuls(R.CASES[name][4])[1] if premul_on else 0.0, p, R.SEEDS[seed_i])
    assert abs(e - emu) <= (0.3 if dtype == FP32 else 0.01) * emu, (e, emu)
    assert BARS[dtype] == 3.0 * emu


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['U1', 'M1', 'S3'])
def test_probes_recover_the_twins_mask_from_the_reference(name, kind):
    keep = R.keep_mask(name, R.PROBE_P, SEED)
    rec = R.probe(kind, name, R.reference_runner(name, keep), torch.float64)
    wrong, missed = rec.mismatches(keep, R.expected_seen(name))
    assert wrong == 0 and missed == 0, (wrong, missed)
    assert int(rec.seen.sum()) == int(R.expected_seen(name).sum()) > 0


def test_sampled_key_windows_cover_the_boundaries():
    """the window sample for long cases: both sides of, and across, each 128-key boundary (a key split is a whole number of 128-key
    tiles), the first window and the ragged last one"""
    for name in ('S2', 'S3'):
        B, H, Lq, Lk, dh, _ = R.CASES[name]
        st = R.sampled_key_windows(name)
        assert 0 in st and (Lk - 1) // dh * dh in st and len(st) < len(range(0, Lk, dh)) + 2 * (Lk // 128)
        for b in range(128, Lk, 128):
            assert any(s < b < s + dh for s in st) and (b - dh) in st and b in st
        keep = R.keep_mask(name, R.PROBE_P, SEED)
        rec = R.probe('fwd', name, R.reference_runner(name, keep), torch.float64, key_starts=st)
        assert rec.mismatches(keep, R.expected_seen(name, st)) == (0, 0)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fault', list(R.FAULTS))
def test_every_probe_reports_each_fault(fault, kind):
    """M1 (odd Lq, odd Lk, 101 x 333): the reference run under a faulty mask stands in for a kernel with that fault"""
    name = 'M1'
    keep = R.keep_mask(name, R.PROBE_P, SEED)
    bad = R.FAULTS[fault](name, R.PROBE_P, SEED)
    differ = (bad != keep) & R.expected_seen(name)
    assert int(differ.sum()) > 0
    rec = R.probe(kind, name, R.reference_runner(name, bad), torch.float64)
    wrong, missed = rec.mismatches(keep, R.expected_seen(name))
    assert missed == 0 and wrong == int(differ.sum()), (fault, kind, wrong, int(differ.sum()))   # every faulty bit, and only those


@pytest.mark.parametrize('name,p', [('U1', 0.1), ('S2', 0.1), ('T1', 0.1), ('E1', 0.1), ('S2', 0.5)])
def test_tile_level_fault_exceeds_the_16_bit_slice_bars(name, p):
    """one 128 x 128 tile of one (batch, head) drawn with the wrong row base, at the model's p = 0.1 (the fewest flipped bits) and at
    the longest key axis (S2: the tile is 128 of 1125 valid keys): o, dq (the query tile's slice) and dk, dv (the key tile's) each
    exceed the larger 16-bit bar, and the slice named is the faulty one -- where check_attention's whole-tensor bar need not notice"""
    q, qref, k, v, do = R.make_inputs(name, BF16)
    kb = R.key_bias(name)
    good = R.reference(qref, k, v, do, kb, R.keep_mask(name, p, SEED), p, _dims(name))
    bad = R.reference(qref, k, v, do, kb, R.fault_tile_row_base(name, p, SEED, b=0, h=1, qt=0, kt=0), p, _dims(name))
    sl = R.slice_errors(name, (bad[0],) + bad[2:], (good[0],) + good[2:])
    for tag, r in sl.items():
        assert r.err > BAR16, f'{name} {tag}: the tile-level fault passes the slice bar: {r} vs {BAR16:.2e}'
        assert 'b=0, head=1, rows 0:' in r.where, r.where


def _slice_norms(ref3, heads):
    """per-slice reference norms and floors of an [B, L, D] tensor on the 'act' partition"""
    B, L, D = ref3.shape
    dh = D // heads
    rn = S._block_sq(ref3, S.TILE, dh).sqrt()
    n = S._block_counts(B, L, D, S.TILE, dh)
    return rn, S.FLOOR * float(ref3.norm()) * (n / (B * L * D)).sqrt()


@pytest.mark.parametrize('name', list(R.CASES))
def test_no_reference_slice_sits_at_the_floor(name):
    """every slice of the parity reference has a norm of its own, above twice slice_metrics' floor (so its error is a relative one;
    measured: >= 170 x the floor) -- except the key tiles whose keys are ALL masked: their dk / dv rows are exactly zero, which the
    device test asserts as zeros -- and except S3's tail tile, which is ONE key (1153 = 9 * 128 + 1) against 7 queries: its dk / dv
    row is a sum of 7 terms, each dropped with probability p, and comes out anywhere down to exactly 0 (all 7 dropped).  That slice
    is measured against the floor, i.e. absolutely; its mask bits are read one by one by the probes."""
    B, H, Lq, Lk, dh, _ = R.CASES[name]
    kb = R.key_bias(name)
    for premul in R.premuls(dh):
        q, qref, k, v, do = R.make_inputs(name, BF16, premul)
        for p in R.PS:
            o, _, dq, dk, dv = R.reference(qref, k, v, do, kb, R.keep_mask(name, p, SEED), p, _dims(name))
            for tag, t, L in (('o', o, Lq), ('dq', dq, Lq), ('dk', dk, Lk), ('dv', dv, Lk)):
                rn, floor = _slice_norms(t.reshape(B, L, H * dh), H)
                at_floor = rn <= 2 * floor
                if tag in ('dk', 'dv') and name == 'S3':
                    at_floor[:, -1, :] = False
                if tag in ('dk', 'dv') and kb is not None:
                    tiles = -(-Lk // S.TILE)
                    dead = torch.stack([torch.stack([(kb[b, i * S.TILE:(i + 1) * S.TILE] != 0).all() for i in range(tiles)]) for b in range(B)])
                    assert bool((rn[dead] == 0).all()), (name, tag)
                    gone = (kb != 0).reshape(B * Lk)
                    assert float(t[gone].abs().max()) == 0.0
                    at_floor = at_floor & ~dead[:, :, None]
                assert not bool(at_floor.any()), (name, tag, premul, p)
