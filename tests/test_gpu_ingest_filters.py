"""The generalised ingest on the MI355X (svol_ingest_resample in csrc/ingest.hip; FrameIngest(filter=, invert=), grey sources): every
comparison is EXACT.  The kernel's output must equal Pillow's bytes (tests/golden/ingest_filter_cases.npz) and the integer
restatement tests/ingest_filter_ref.py (pinned to Pillow on the CPU by tests/test_ingest_filter_tables.py) bit for bit.  This file
does not import PIL."""
import os

import numpy as np
import pytest
import torch

from tests.guard_arena import GuardArena, NEG0

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
FILTERS = ('box', 'bilinear', 'hamming', 'bicubic', 'lanczos')
_GOLDEN, _TABS = [], {}


def _golden():
    if not _GOLDEN:
        _GOLDEN.append(np.load(os.path.join(REPO, 'tests', 'golden', 'ingest_filter_cases.npz')))
    return _GOLDEN[0]


def _tab(n_in, n_out, flt):
    from svol_amd.ingest import resample_tables
    key = (n_in, n_out, flt)
    if key not in _TABS:
        t = resample_tables(n_in, n_out, flt)
        _TABS[key] = (torch.from_numpy(t).to(DEV), t.shape[1] - 2)
    return _TABS[key]


def _ident_lut():
    """channel c maps byte v to v + 256 c, which tells the channels apart (exact in fp32 only: the 16-bit outputs use _byte_lut)"""
    return (torch.arange(256, dtype=torch.float32)[None, :] + 256 * torch.arange(3, dtype=torch.float32)[:, None]).contiguous().to(DEV)


def _byte_lut():
    return torch.arange(256, dtype=torch.float32).expand(3, 256).contiguous().to(DEV)


def _resample(src, size, flt, invert=False, lut=None, flip=None, out=None, nhwc=False, dtype=torch.float32):
    """raw kernel call: src uint8 device [n,H,W,3] or grey [n,H,W] (any strides) -> out [n,3,OH,OW] (or NHWC) holding the BYTES"""
    from svol_amd import ops
    n, H, W = src.shape[:3]
    OH, OW = size
    (ytab, ky), (xtab, kx) = _tab(H, OH, flt), _tab(W, OW, flt)
    if out is None:
        out = torch.empty((n, OH, OW, 3) if nhwc else (n, 3, OH, OW), dtype=dtype, device=DEV)
    st = (out.stride(0), out.stride(3), out.stride(1), out.stride(2)) if nhwc else tuple(out.stride())
    return ops.ingest_resample(src, xtab, kx, ytab, ky, _byte_lut() if lut is None else lut, flip, out, st, OH, OW, invert=invert)


def _want_nchw(y):
    """numpy bytes [n,OH,OW] (grey: the three channels are the one) or [n,OH,OW,3] -> float32 torch [n,3,OH,OW]"""
    t = torch.from_numpy(np.ascontiguousarray(y))
    t = t[..., None].expand(*t.shape, 3) if t.dim() == 3 else t
    return t.permute(0, 3, 1, 2).float().contiguous()


def _ref(x, size, flt, invert=False):
    """numpy uint8 [n,H,W] / [n,H,W,3] -> float32 torch [n,3,OH,OW] through the restatement"""
    from tests import ingest_filter_ref as ref
    return _want_nchw(np.stack([ref.resize_u8(f, size, flt, invert=invert) for f in x]))


@pytest.mark.parametrize('flt', FILTERS)
def test_goldens_equal_pillow_bytes(flt):
    """every case, grey and RGB, in fp32 NCHW and in both 16-bit NHWC layouts (bytes are exact in bf16 and fp16); the fp32 run uses a
    table that tells the channels apart, so a grey source must reach all three"""
    from svol_amd._lib import SvolHipError
    z = _golden()
    f = FILTERS.index(flt)
    chan = 256 * torch.arange(3, dtype=torch.float32)[None, :, None, None]
    for i in range(int(z['n'])):
        x = z[f'c{i}/x']
        for mode, src in (('grey', np.ascontiguousarray(x[..., 1])), ('rgb', x)):
            y = z[f'c{i}/{mode}'][f]
            want = _want_nchw(y[None])
            xd = torch.from_numpy(src)[None].to(DEV)
            what = f'case {i} {mode} {flt}: {x.shape[:2]} -> {y.shape[:2]}'
            if max(_tab(x.shape[0], y.shape[0], flt)[1], _tab(x.shape[1], y.shape[1], flt)[1]) > 64:
                # the sliver under lanczos (300 -> 24: 77 taps) lies beyond the entry's 64-tap limit: it is refused, not computed (the
                # restatement equals this golden on the CPU)
                assert (i, flt) == (7, 'lanczos')
                with pytest.raises(SvolHipError, match='code -2'):
                    _resample(xd, y.shape[:2], flt)
                continue
            assert torch.equal(_resample(xd, y.shape[:2], flt, lut=_ident_lut()).cpu(), want + chan), what
            for dt in (torch.bfloat16, torch.float16):
                got = _resample(xd, y.shape[:2], flt, nhwc=True, dtype=dt)
                assert got.dtype == dt and torch.equal(got.cpu(), want.permute(0, 2, 3, 1).to(dt)), what


@pytest.mark.parametrize('flt', ['bicubic', 'lanczos'])
def test_black_and_white_goldens_reach_the_clamps(flt):
    """0 / 255 inputs whose accumulators leave [0, 255 * 2^22] at both ends in both passes (shown on the CPU by
    tests/test_ingest_filter_tables.py): unsigned accumulators or a one-sided clamp give other bytes"""
    z = _golden()
    for j in range(int(z['n_bw'])):
        x, y = z[f'bw{j}/x'], z[f'bw{j}/y'][('bicubic', 'lanczos').index(flt)]
        got = _resample(torch.from_numpy(x)[None].to(DEV), y.shape[:2], flt)
        assert torch.equal(got.cpu(), _want_nchw(y[None])), (j, flt)
        assert int((y == 0).sum()) and int((y == 255).sum())


@pytest.mark.parametrize('out', ['nchw_f32', 'nhwc_bf16'])
def test_quickdraw_line_through_frame_ingest(out):
    """preprocess/quickdraw_array_to_pil.py:36 on the raw bitmap: FrameIngest((224, 224), 'totensor', filter='bicubic', invert=True)
    equals table[Pillow's bytes]; inverting after the resize instead would not"""
    from svol_amd.ingest import FrameIngest, preset_table
    z = _golden()
    x, y = z['qd/x'], z['qd/y']
    m = FrameIngest((224, 224), 'totensor', filter='bicubic', invert=True, out=out)
    got = m(torch.from_numpy(x)[None].to(DEV)).cpu()
    table = preset_table('totensor')
    u = torch.from_numpy(y).long()
    want = torch.stack([table[c][u] for c in range(3)])              # [3, 224, 224]
    if out == 'nchw_f32':
        assert got.shape == (1, 3, 224, 224) and torch.equal(got[0], want)
    else:
        assert got.shape == (1, 224, 224, 3) and torch.equal(got[0], want.permute(1, 2, 0).bfloat16())
    plain = FrameIngest((224, 224), 'totensor', filter='bicubic', out='nchw_f32')(torch.from_numpy(x)[None].to(DEV)).cpu()
    assert not torch.equal(table[0][255 - (plain[0, 0] * 255).round().long()], want[0])


def test_grey_flip_leading_dimensions_and_lists():
    from svol_amd.ingest import FrameIngest
    from tests import ingest_filter_ref as ref
    # n = 3, the middle image mirrored, both layouts, an output width that is no multiple of 4
    x = np.stack([ref.noise(20 + i, 45, 61, 0) for i in range(3)])
    flip = torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    for flt in ('bilinear', 'bicubic'):
        want = _ref(x, (33, 50), flt)
        want[1] = want[1].flip(-1)
        assert torch.equal(_resample(xd, (33, 50), flt, flip=flip).cpu(), want)
        got = _resample(xd, (33, 50), flt, flip=flip, nhwc=True, dtype=torch.bfloat16)
        assert torch.equal(got.cpu(), want.permute(0, 2, 3, 1).bfloat16())
    # [B,T,H,W,1] keeps its leading dimensions; [n,H,W,1] and [n,H,W] are the same images; a list of mixed sizes, grey and RGB,
    # lands in one tensor, in order; n = 0 launches nothing
    m = FrameIngest((24, 32), 'totensor', filter='lanczos', invert=True)
    a, b = ref.noise(40, 30, 50, 0)[None], np.stack([ref.noise(41 + i, 64, 48, 0) for i in range(2)])
    c = ref.noise(44, 20, 36)[None]
    ad, bd, cd = (torch.from_numpy(v).to(DEV) for v in (a, b, c))
    want = torch.cat([_ref(a, (24, 32), 'lanczos', True), _ref(b, (24, 32), 'lanczos', True), _ref(c, (24, 32), 'lanczos', True)]) / 255
    got = m([ad, bd[..., None], cd])
    assert got.shape == (4, 3, 24, 32) and torch.equal(got.cpu(), want)
    got5 = m(bd[None, ..., None], flip=torch.tensor([1, 0], dtype=torch.uint8, device=DEV))
    assert got5.shape == (1, 2, 3, 24, 32) and torch.equal(got5[0, 0].cpu(), want[1].flip(-1)) and torch.equal(got5[0, 1].cpu(), want[2])
    assert torch.equal(m(bd).cpu(), want[1:3]) and torch.equal(m(bd[..., None]).cpu(), want[1:3])
    assert m(torch.empty((0, 30, 50), dtype=torch.uint8, device=DEV)).shape == (0, 3, 24, 32)
    with pytest.raises(TypeError):
        m(torch.zeros((1, 30, 50), device=DEV))
    with pytest.raises(ValueError):
        m(torch.zeros((1, 30, 50, 2), dtype=torch.uint8, device=DEV))


def test_strided_views():
    from tests import ingest_filter_ref as ref
    # a cropped grey view of a larger tensor: odd byte offset (3 * 67 + 4 = 205), row stride 67 (no multiple of 4)
    big = np.stack([ref.noise(30 + i, 50, 67, 0) for i in range(2)])
    view = torch.from_numpy(big).to(DEV)[:, 3:, 4:]
    assert view.data_ptr() % 2 == 1 and view.stride(1) % 4 != 0 and not view.is_contiguous()
    for flt in ('bilinear', 'bicubic', 'lanczos'):
        assert torch.equal(_resample(view, (40, 40), flt).cpu(), _ref(big[:, 3:, 4:], (40, 40), flt)), flt
    # the RGB channels of an RGBA tensor under bicubic (pixel stride 4), and ONE channel of it as a grey source (pixel stride 4)
    rgba = np.random.default_rng(5).integers(0, 256, size=(1, 21, 19, 4), dtype=np.uint8)
    rd = torch.from_numpy(rgba).to(DEV)
    assert torch.equal(_resample(rd[..., :3], (16, 24), 'bicubic').cpu(), _ref(rgba[..., :3], (16, 24), 'bicubic'))
    assert torch.equal(_resample(rd[..., 3], (16, 24), 'bicubic', invert=True).cpu(), _ref(rgba[..., 3], (16, 24), 'bicubic', True))
    # a cropped RGB view, inverted
    bigc = np.stack([ref.noise(35 + i, 50, 66) for i in range(2)])
    vc = torch.from_numpy(bigc).to(DEV)[:, 3:, 5:]
    assert vc.data_ptr() % 2 == 1
    assert torch.equal(_resample(vc, (40, 40), 'hamming', invert=True).cpu(), _ref(bigc[:, 3:, 5:], (40, 40), 'hamming', True))


def test_several_tiles_and_the_tap_limit():
    """sources large enough that an image takes several tiles in both directions, and the 64-tap limit itself under lanczos"""
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    from tests import ingest_filter_ref as ref
    g = ref.noise(7, 1111, 1111, 0)[None]                   # TU-Berlin's size: lanczos k = 31
    gd = torch.from_numpy(g).to(DEV)
    for flt in ('bilinear', 'lanczos'):
        assert torch.equal(_resample(gd, (224, 224), flt).cpu(), _ref(g, (224, 224), flt)), flt
    x = ref.noise(8, 360, 480)[None]
    assert torch.equal(_resample(torch.from_numpy(x).to(DEV), (224, 224), 'bicubic').cpu(), _ref(x, (224, 224), 'bicubic'))
    q = np.stack([ref.noise(50 + i, 28, 28, 0) for i in range(3)])      # 28 -> 224: eight outputs per source pixel
    assert torch.equal(_resample(torch.from_numpy(q).to(DEV), (224, 224), 'bicubic', invert=True).cpu(), _ref(q, (224, 224), 'bicubic', True))
    # the limit is taken: lanczos at a 10.3-fold downscale has 2 ceil(3 * 10.3125) + 1 = 63 taps
    assert _tab(165, 16, 'lanczos')[1] == 63
    t = ref.noise(9, 165, 8, 0)[None]
    assert torch.equal(_resample(torch.from_numpy(t).to(DEV), (16, 8), 'lanczos').cpu(), _ref(t, (16, 8), 'lanczos'))
    # beyond it: SVOL_E_UNSUPPORTED, nothing written
    H, W, OH, OW = 176, 8, 16, 8
    (ytab, ky), (xtab, kx) = _tab(H, OH, 'lanczos'), _tab(W, OW, 'lanczos')
    assert ky == 67
    src = torch.zeros((1, H, W), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, OH, OW), -7.0, device=DEV)
    rc = _lib.lib().svol_ingest_resample(_ptr(src), 1, H, W, H * W, W, 1, 1, 0, _ptr(xtab), kx, _ptr(ytab), ky, _ptr(_byte_lut()), 0,
                                         _ptr(out), 3 * OH * OW, OH * OW, OW, 1, OH, OW, 0, _stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((out == -7.0).all())


def test_rgb_bilinear_stays_on_the_old_entry(monkeypatch):
    """FrameIngest on RGB with the default filter and no inversion calls svol_ingest_resize and gives the bits that entry gives; the
    new entry computes the same bytes from the same tables"""
    from svol_amd import ops
    from svol_amd.ingest import FrameIngest, resample_tables
    from tests import ingest_filter_ref as ref
    x = np.stack([ref.noise(60 + i, 45, 61) for i in range(2)])
    xd = torch.from_numpy(x).to(DEV)
    m = FrameIngest((33, 50), 'imagenet')
    lut = m._lut_cpu.to(DEV)
    (ytab, ky), (xtab, kx) = _tab(45, 33, 'bilinear'), _tab(61, 50, 'bilinear')
    assert np.array_equal(resample_tables(45, 33), ytab.cpu().numpy())
    want = torch.empty((2, 3, 33, 50), device=DEV)
    ops.ingest_resize(xd, xtab, kx, ytab, ky, lut, None, want, tuple(want.stride()), 33, 50)
    new = _resample(xd, (33, 50), 'bilinear', lut=lut)
    assert torch.equal(new, want)

    def refuse(*a, **k):
        raise AssertionError('RGB + bilinear + no inversion must not reach svol_ingest_resample')
    monkeypatch.setattr(ops, 'ingest_resample', refuse)
    assert torch.equal(m(xd), want)
    monkeypatch.undo()
    calls = []
    real = ops.ingest_resample
    monkeypatch.setattr(ops, 'ingest_resample', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    FrameIngest((33, 50), 'imagenet', invert=True)(xd)
    FrameIngest((33, 50), 'imagenet', filter='box')(xd)
    FrameIngest((33, 50), 'imagenet')(xd[..., 0])
    assert len(calls) == 3


@pytest.mark.parametrize('flt', ['bicubic', 'lanczos'])
@pytest.mark.parametrize('grey', [True, False], ids=['grey', 'rgb'])
def test_red_zones(grey, flt):
    """outputs carved out of a -0.0 arena: guards intact and every element written (no table entry is -0.0).  The source is a strided
    view inside a larger allocation whose every other byte is hostile — 0xFF, then random bytes: the result is the same and equals the
    restatement, so nothing outside the addressed bytes is read into it"""
    from tests import ingest_filter_ref as ref
    OH, OW = 33, 50
    n, H, W = 2, 45, 61
    C = () if grey else (3,)
    x = np.stack([ref.noise(60 + i, H, W, 0 if grey else 3) for i in range(n)])
    want = _ref(x, (OH, OW), flt)
    plain = want.clone()
    want[0] = want[0].flip(-1)
    flip = torch.tensor([1, 0], dtype=torch.uint8, device=DEV)
    for fill in ('ff', 'random'):
        if fill == 'ff':
            store = torch.full((n + 2, H + 7, W + 9) + C, 255, dtype=torch.uint8, device=DEV)
        else:
            store = torch.from_numpy(np.random.default_rng(77).integers(0, 256, size=(n + 2, H + 7, W + 9) + C, dtype=np.uint8)).to(DEV)
        src = store[1:1 + n, 3:3 + H, 5:5 + W]
        src.copy_(torch.from_numpy(x))
        assert not src.is_contiguous()
        arena = GuardArena(guard_bytes=1 << 16)
        arena.plan('f32', (n, 3, OH, OW), torch.float32)
        arena.plan('bf16', (n, OH, OW, 3), torch.bfloat16)
        arena.plan('f16', (n, OH, OW, 3), torch.float16)
        t = arena.build()
        _resample(src, (OH, OW), flt, flip=flip, out=t['f32'])
        _resample(src, (OH, OW), flt, flip=flip, out=t['bf16'], nhwc=True)
        _resample(src, (OH, OW), flt, out=t['f16'], nhwc=True)
        torch.cuda.synchronize()
        arena.check(f'resample {flt} {"grey" if grey else "rgb"} {fill} {H}x{W} -> {OH}x{OW}')
        assert torch.equal(t['f32'].cpu(), want), fill
        assert torch.equal(t['bf16'].cpu(), want.permute(0, 2, 3, 1).bfloat16()), fill
        assert torch.equal(t['f16'].cpu(), plain.permute(0, 2, 3, 1).half()), fill
        assert bool((t['f32'].view(torch.int32) != NEG0).all())
        assert bool((t['bf16'].view(torch.int16) != -2 ** 15).all()) and bool((t['f16'].view(torch.int16) != -2 ** 15).all())


def test_graph_capture_and_replay():
    from svol_amd.ingest import FrameIngest
    from tests import ingest_filter_ref as ref
    m = FrameIngest((32, 48), 'imagenet', out='nhwc_bf16', filter='bicubic', invert=True)
    x = torch.from_numpy(np.stack([ref.noise(95 + i, 40, 72, 0) for i in range(2)])).to(DEV)
    eager = m(x).clone()
    static = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(static)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = m(static)
    static.copy_(x.flip(0))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager.flip(0))


def test_resnet_backbone_takes_grey_inverted_bicubic_sketches():
    """build_backbone with args.sketch_filter = 'bicubic', args.sketch_invert = True: raw grey 28 x 28 bitmaps [B,1,28,28] give the
    features, bit for bit, of the float pixels Pillow (the golden; the restatement for the second bitmap) plus the preset table make
    of them; the frames keep the bilinear ingest"""
    from svol_amd import configs
    from svol_amd.ingest import preset_table
    from svol_amd.modeling.model import build_backbone
    from tests import ingest_filter_ref as ref
    from tests import ingest_ref
    z = _golden()
    args = configs.parse_args(['--backbone', 'resnet', '--freeze_backbone'])
    args.sketch_filter, args.sketch_invert = 'bicubic', True
    torch.manual_seed(5)
    bb = build_backbone(args).to(DEV).eval()
    bitmaps = np.stack([z['qd/x'], np.ascontiguousarray(z['qd/x'][::-1, ::-1].T)])         # [2, 28, 28]
    bytes_ = np.stack([z['qd/y'], ref.resize_u8(bitmaps[1], (224, 224), 'bicubic', invert=True)])
    table = preset_table('totensor')
    u = torch.from_numpy(bytes_).long()
    sk_pix = torch.stack([table[c][u] for c in range(3)], 1)[:, None].to(DEV)            # [2, 1, 3, 224, 224]
    vid = np.stack([ingest_ref.noise(80 + i, 90, 120) for i in range(2)])[:, None]        # [2, 1, 90, 120, 3]
    vu = torch.from_numpy(np.stack([ingest_ref.resize_u8(f, (224, 224)) for f in vid[:, 0]])).long()
    vid_pix = torch.stack([table[c][vu[..., c]] for c in range(3)], 1)[:, None].to(DEV)
    with torch.no_grad():
        want_s, want_v = bb(sk_pix, vid_pix)
        got_s, got_v = bb(torch.from_numpy(bitmaps)[:, None].to(DEV), torch.from_numpy(vid).to(DEV))
        assert got_s.shape == want_s.shape == (2, 1, 512) and torch.equal(got_s, want_s) and torch.equal(got_v, want_v)
        assert bool(torch.isfinite(got_s).all())
        # [B,1,H,W,1] and a list of [1,H,W] bitmaps are the same call
        got5, _ = bb(torch.from_numpy(bitmaps)[:, None, :, :, None].to(DEV), torch.from_numpy(vid).to(DEV))
        gotl, _ = bb([torch.from_numpy(b)[None].to(DEV) for b in bitmaps], torch.from_numpy(vid).to(DEV))
        assert torch.equal(got5, want_s) and torch.equal(gotl, want_s)
