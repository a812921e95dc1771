"""CPU-side checks of the generalised ingest (svol_ingest_resample; svol_amd.ingest.resample_tables(filter=)): the integer restatement
tests/ingest_filter_ref.py against the Pillow goldens of tests/golden/ingest_filter_cases.npz and against live Pillow, the properties
the kernel relies on (clamps reached, int32 enough, the window-growth bound, identity taps on an unchanged axis, inversion at the
source), and the C entry's argument validation without a device."""
import os

import numpy as np
import pytest

from svol_amd import ingest
from tests import ingest_filter_ref as ref
from tests import ingest_ref
from tests.test_ingest_tables import LIVE_SIZES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, 'tests', 'golden', 'ingest_filter_cases.npz'))
FILTERS = ref.FILTERS
BW_FILTERS = ('bicubic', 'lanczos')
WIDTH = {'box': 0.5, 'bilinear': 1.0, 'hamming': 1.0, 'bicubic': 2.0, 'lanczos': 3.0}    # Pillow's supports


def _taps(n_in, n_out, flt):
    return int(np.ceil(WIDTH[flt] * max(n_in / n_out, 1.0))) * 2 + 1


@pytest.mark.parametrize('flt', FILTERS)
@pytest.mark.parametrize('i', range(int(GOLDEN['n'])))
def test_restatement_equals_pillow_golden(i, flt):
    x = GOLDEN[f'c{i}/x']
    f = FILTERS.index(flt)
    for mode, src in (('grey', x[..., 1]), ('rgb', x)):
        y = GOLDEN[f'c{i}/{mode}'][f]
        got = ref.resize_u8(src, y.shape[:2], flt)
        assert got.dtype == np.uint8 and got.shape == y.shape and np.array_equal(got, y), (mode, x.shape, y.shape)


def test_case_table_is_the_one_the_fixture_was_asked_for():
    want = [((37, 53), (64, 64)), ((96, 128), (40, 56)), ((75, 77), (74, 78)), ((64, 64), (64, 64)), ((64, 40), (64, 56)), ((1, 1), (8, 8)),
            ((2, 200), (16, 24)), ((300, 7), (24, 16))]
    assert int(GOLDEN['n']) == len(want)
    for i, (src, dst) in enumerate(want):
        assert GOLDEN[f'c{i}/x'].shape == src + (3,)
        assert GOLDEN[f'c{i}/grey'].shape == (5,) + dst and GOLDEN[f'c{i}/rgb'].shape == (5,) + dst + (3,)
    assert ingest.resample_tables(200, 24, 'lanczos').shape[1] - 2 == 51        # case 7: taps clipped at both ends at k = 51
    # one combination lies beyond the entry's 64-tap limit (the sliver under lanczos, 300 -> 24: 77 taps): the restatement equals
    # its golden above, the device refuses it (tests/test_gpu_ingest_filters.py)
    over = [(i, flt) for i, (src, dst) in enumerate(want) for flt in FILTERS if max(_taps(src[0], dst[0], flt), _taps(src[1], dst[1], flt)) > ref.MAX_TAPS]
    assert over == [(7, 'lanczos')]
    assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', 'ingest_filter_cases.npz')) < 500_000


def test_quickdraw_line_and_the_order_of_the_inversion():
    """preprocess/quickdraw_array_to_pil.py:36: Image.fromarray(255 - bitmap).resize((224, 224), BICUBIC).  Inverting the RESULT of
    the resize of the raw bitmap is something else: the clamps sit at the other end."""
    x, y = GOLDEN['qd/x'], GOLDEN['qd/y']
    assert x.shape == (28, 28) and y.shape == (224, 224)
    assert np.array_equal(ref.resize_u8(x, (224, 224), 'bicubic', invert=True), y)
    after = 255 - ref.resize_u8(x, (224, 224), 'bicubic')
    assert int((after != y).sum()) > 0


@pytest.mark.parametrize('flt', BW_FILTERS)
@pytest.mark.parametrize('j', range(int(GOLDEN['n_bw'])))
def test_black_and_white_goldens_reach_both_clamps_in_both_passes(j, flt):
    """an accumulator below 0 and one above 255 * 2^22 (+ the rounding half) in the horizontal AND in the vertical pass: a kernel with
    unsigned accumulators, or one that clamps at one end only, cannot produce these bytes"""
    x, y = GOLDEN[f'bw{j}/x'], GOLDEN[f'bw{j}/y'][BW_FILTERS.index(flt)]
    assert set(np.unique(x)) == {0, 255}
    stats = []
    assert np.array_equal(ref.resize_u8(x, y.shape[:2], flt, stats=stats), y)
    assert len(stats) == 2
    for lo, hi in stats:
        assert lo < 0 and (hi >> 22) > 255, (stats, flt)


@pytest.mark.parametrize('flt', FILTERS)
def test_grey_equals_each_channel_of_the_replicated_rgb(flt):
    for i in (0, 1, 4, 6):
        g = np.ascontiguousarray(GOLDEN[f'c{i}/x'][..., 1])
        size = GOLDEN[f'c{i}/grey'].shape[1:]
        rgb = ref.resize_u8(np.repeat(g[..., None], 3, axis=2), size, flt)
        for c in range(3):
            assert np.array_equal(rgb[..., c], GOLDEN[f'c{i}/grey'][FILTERS.index(flt)])


# the sizes of tests/test_ingest_tables.py, leaving out those a filter's 64-tap limit excludes
LIVE = [(H, W, flt) for flt in FILTERS for H, W in LIVE_SIZES if max(_taps(H, 224, flt), _taps(W, 224, flt)) <= ref.MAX_TAPS]


@pytest.mark.parametrize('H,W,flt', LIVE)
def test_restatement_equals_live_pillow(H, W, flt):
    Image = pytest.importorskip('PIL.Image')
    pil = {'box': Image.BOX, 'bilinear': Image.BILINEAR, 'hamming': Image.HAMMING, 'bicubic': Image.BICUBIC, 'lanczos': Image.LANCZOS}[flt]
    x = ingest_ref.noise(H * 10007 + W, H, W)
    want = np.asarray(Image.fromarray(x, 'RGB').resize((224, 224), pil))
    assert np.array_equal(ref.resize_u8(x, (224, 224), flt), want)
    g = np.ascontiguousarray(x[..., 0])
    assert np.array_equal(ref.resize_u8(g, (224, 224), flt), np.asarray(Image.fromarray(g, 'L').resize((224, 224), pil)))


def test_default_filter_is_bilinear_and_unchanged():
    """resample_tables(a, b) is resample_tables(a, b, 'bilinear') and what it always returned (restated here as it was written)"""
    import math
    for a, b in [(224, 224), (3840, 224), (37, 64), (1, 8), (600, 24), (225, 224), (28, 224), (1111, 224)]:
        t = ingest.resample_tables(a, b)
        assert t.dtype == np.int32 and np.array_equal(t, ingest.resample_tables(a, b, 'bilinear'))
        scale = a / b
        support = max(scale, 1.0)
        ss = 1.0 / support
        assert t.shape == (b, 2 + int(math.ceil(support)) * 2 + 1)
        for xx in (0, b // 3, b - 1):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), a) - xmin
            w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            assert (t[xx, 0], t[xx, 1]) == (xmin, xmax)
            assert [int(v) for v in t[xx, 2:2 + xmax]] == [int(0.5 + v / ww * (1 << 22)) for v in w] and (t[xx, 2 + xmax:] == 0).all()
    assert np.array_equal(ingest_ref.resize_u8(GOLDEN['c0/x'], (64, 64)), ref.resize_u8(GOLDEN['c0/x'], (64, 64)))
    with pytest.raises(ValueError):
        ingest.resample_tables(8, 8, 'nearest')
    with pytest.raises(ValueError):
        ingest.FrameIngest(filter='nearest')


@pytest.mark.parametrize('flt', FILTERS)
def test_unchanged_axis_has_the_identity_taps(flt):
    """Pillow skips the pass of an axis whose size does not change; the kernel runs it with these taps, which select the byte"""
    for n in (1, 2, 3, 7, 28, 64, 224, 1111):
        t = ingest.resample_tables(n, n, flt)
        cnt = t[:, 1]
        j = np.arange(n) - t[:, 0]                        # where index i sits in its own window
        assert (j >= 0).all() and (j < cnt).all()
        taps = t[:, 2:].copy()
        assert (taps[np.arange(n), j] == 1 << 22).all()
        taps[np.arange(n), j] = 0
        assert (taps == 0).all()


@pytest.mark.parametrize('flt', FILTERS)
def test_window_growth_bound_the_kernel_tiles_by(flt):
    """include/svol_hip.h: t neighbouring outputs touch at most ceil((t-1) in/out) + k source indices, for any support"""
    for n_in, n_out in [(360, 224), (480, 224), (3840, 224), (37, 64), (1, 8), (600, 24), (7, 16), (9216, 512), (225, 224)]:
        tab = ingest.resample_tables(n_in, n_out, flt)
        k = tab.shape[1] - 2
        assert k == _taps(n_in, n_out, flt)
        lo, hi = tab[:, 0].astype(np.int64), (tab[:, 0] + tab[:, 1]).astype(np.int64)
        assert (np.diff(lo) >= 0).all() and (lo >= 0).all() and (hi <= n_in).all() and (tab[:, 1] >= 1).all() and (tab[:, 1] <= k).all()
        for t in (1, 2, 4, 16, 32, n_out):
            t = min(t, n_out)
            span = hi[t - 1:] - lo[:n_out - t + 1]
            assert span.max() <= min(-(-(t - 1) * n_in // n_out) + k, n_in), (n_in, n_out, t)


@pytest.mark.parametrize('flt', FILTERS)
def test_int32_is_enough_up_to_64_taps(flt):
    """255 * sum |taps| + 2^21 < 2^31 at every output index, from the identity to the largest downscale with k <= 64"""
    out = 16
    scales = [s for s in (1, 1.37, 2, 3.5, 5, 7.25, 10, 10.3, 15, 15.5, 20, 31, 40, 61.9) if int(np.ceil(WIDTH[flt] * s)) * 2 + 1 <= ref.MAX_TAPS]
    assert scales[-1] >= {'box': 61, 'bilinear': 31, 'hamming': 31, 'bicubic': 15, 'lanczos': 10}[flt]
    for s in scales:
        for n_in in (int(out * s), int(out * s) + 1):
            tab = ingest.resample_tables(n_in, out, flt)
            if tab.shape[1] - 2 > ref.MAX_TAPS:
                continue
            assert 255 * int(np.abs(tab[:, 2:].astype(np.int64)).sum(1).max()) + (1 << 21) < 2 ** 31, (n_in, flt)
    for n_in, n_out in [(28, 224), (37, 64), (1, 8), (3, 16)]:     # upscales
        tab = ingest.resample_tables(n_in, n_out, flt)
        assert 255 * int(np.abs(tab[:, 2:].astype(np.int64)).sum(1).max()) + (1 << 21) < 2 ** 31


def test_negative_taps_round_away_from_zero():
    """normalize_coeffs_8bpc: a negative tap is (int)(-0.5 + v * 2^22)"""
    t = ingest.resample_tables(28, 224, 'bicubic')
    assert t[:, 2:].min() < 0
    assert (t[:, 2:].astype(np.int64).sum(1) - (1 << 22)).__abs__().max() <= t.shape[1]      # rows sum to 1 up to the roundings
    for flt in ('box', 'bilinear', 'hamming'):
        assert ingest.resample_tables(300, 64, flt)[:, 2:].min() >= 0
    assert ingest.resample_tables(300, 64, 'lanczos')[:, 2:].min() < 0


def test_argument_validation_without_gpu():
    """Null pointers, src_channels other than 1 / 3, invert other than 0 / 1 and geometries beyond the documented limit are rejected
    before any launch; n == 0 launches nothing."""
    from svol_amd import _lib
    assert 'svol_ingest_resample' in _lib.SIGNATURES and len(_lib.SIGNATURES['svol_ingest_resample']) == len(_lib.SIGNATURES['svol_ingest_resize']) + 2
    fn = _lib.lib().svol_ingest_resample
    P = 4096   # never dereferenced on the host

    def call(src=P, n=1, H=8, W=8, sc=3, invert=0, xtab=P, kx=5, ytab=P, ky=5, lut=P, out=P, OH=8, OW=8, dt=0, s_w=None):
        s_w = sc if s_w is None else s_w
        return fn(src, n, H, W, H * W * sc, W * sc, s_w, sc, invert, xtab, kx, ytab, ky, lut, 0, out, 3 * OH * OW, OH * OW, OW, 1, OH, OW, dt, 0)
    for bad in (dict(src=0), dict(xtab=0), dict(ytab=0), dict(lut=0), dict(out=0), dict(n=-1), dict(H=0), dict(W=0), dict(OH=0),
                dict(OW=0), dict(kx=0), dict(ky=0), dict(dt=3), dict(s_w=-1), dict(sc=2), dict(sc=4), dict(sc=0), dict(invert=2),
                dict(invert=-1)):
        assert call(**bad) == -1, bad
    for sc in (1, 3):
        for invert in (0, 1):
            assert call(n=0, sc=sc, invert=invert) == 0
    assert call(n=0, sc=2) == -1 and call(n=0, invert=2) == -1
    # beyond the limit: more than 64 taps per axis, an output wider than 16384
    assert call(H=8960, ky=65) == -2 and call(W=8960, kx=65, sc=1) == -2
    assert call(OW=16385) == -2 and call(OH=16385, sc=1) == -2
    # a huge image count must not wrap the grid
    assert call(n=1 << 40) == -2 and call(n=1 << 40, sc=1, invert=1) == -2
    assert _lib.lib().svol_abi_version() == 7      # a new symbol only


def test_frame_ingest_options_without_a_device():
    import torch
    f = ingest.FrameIngest((224, 224), 'totensor', filter='bicubic', invert=True)
    assert f.filter == 'bicubic' and f.invert is True and len(list(f.parameters())) == 0
    d = ingest.FrameIngest()
    assert d.filter == 'bilinear' and d.invert is False
    with pytest.raises(RuntimeError):
        f(torch.zeros(1, 28, 28, dtype=torch.uint8))              # a CPU tensor: no host path
    g = torch.zeros(2, 1, 28, 28, dtype=torch.uint8)
    assert ingest.sketch_frames(g).shape == (2, 1, 28, 28, 1)
    rgb = torch.zeros(2, 1, 28, 28, 3, dtype=torch.uint8)
    assert ingest.sketch_frames(rgb) is rgb and ingest.sketch_frames([g]) == [g]


def test_backbones_take_the_sketch_options():
    """build_backbone reads args.sketch_filter / args.sketch_invert like pixel_preset; with both unset the sketch shares the frames'
    ingest"""
    from svol_amd import configs
    from svol_amd.modeling.model import build_backbone
    args = configs.parse_args(['--backbone', 'resnet', '--freeze_backbone'])
    assert not hasattr(args, 'sketch_filter') and not hasattr(args, 'sketch_invert')       # no command-line flag
    b = build_backbone(args)
    assert b.sketch_ingest is b.ingest
    args.sketch_filter, args.sketch_invert = 'bicubic', True
    b = build_backbone(args)
    assert b.sketch_ingest is not b.ingest and b.sketch_ingest.filter == 'bicubic' and b.sketch_ingest.invert
    assert b.ingest.filter == 'bilinear' and not b.ingest.invert and b.sketch_ingest.out == b.ingest.out
    assert b.sketch_ingest.preset == b.ingest.preset == 'totensor'
