"""Frame ingest on the MI355X (csrc/ingest.hip, svol_amd/ingest.py): every comparison is EXACT — the resize is integer arithmetic
and the float stage a table, so the kernel's output must equal Pillow's bytes (tests/golden/ingest_cases.npz) and the integer
restatement tests/ingest_ref.py (pinned to Pillow on the CPU by tests/test_ingest_tables.py) bit for bit.  This file does not
import PIL."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
NEG0 = -2 ** 31          # the int32 pattern of -0.0


def _golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'ingest_cases.npz'))


_TABS = {}


def _tab(n_in, n_out):
    from svol_amd.ingest import resample_tables
    if (n_in, n_out) not in _TABS:
        t = resample_tables(n_in, n_out)
        _TABS[(n_in, n_out)] = (torch.from_numpy(t).to(DEV), t.shape[1] - 2)
    return _TABS[(n_in, n_out)]


def _ident_lut():
    return torch.arange(256, dtype=torch.float32).expand(3, 256).contiguous().to(DEV)


def _resize(src, size, lut=None, flip=None, out=None, nhwc=False, dtype=torch.float32):
    """raw kernel call: src uint8 device [n,H,W,3] (any strides) -> out [n,3,OH,OW] (or NHWC)"""
    from svol_amd import ops
    n, H, W = src.shape[:3]
    OH, OW = size
    (ytab, ky), (xtab, kx) = _tab(H, OH), _tab(W, OW)
    if out is None:
        out = torch.empty((n, OH, OW, 3) if nhwc else (n, 3, OH, OW), dtype=dtype, device=DEV)
    st = (out.stride(0), out.stride(3), out.stride(1), out.stride(2)) if nhwc else tuple(out.stride())
    return ops.ingest_resize(src, xtab, kx, ytab, ky, _ident_lut() if lut is None else lut, flip, out, st, OH, OW)


def _ref_nchw(x, size):
    """numpy uint8 [n,H,W,3] -> float32 torch [n,3,OH,OW] holding the resized BYTES"""
    from tests import ingest_ref
    return torch.from_numpy(np.stack([ingest_ref.resize_u8(f, size) for f in x])).permute(0, 3, 1, 2).float()


def test_goldens_equal_pillow_bytes():
    z = _golden()
    for i in range(int(z['n'])):
        x, y = z[f'c{i}/x'], z[f'c{i}/y']
        got = _resize(torch.from_numpy(x)[None].to(DEV), y.shape[:2])
        want = torch.from_numpy(y).permute(2, 0, 1)[None].float()
        assert torch.equal(got.cpu(), want), f'case {i}: {x.shape} -> {y.shape}'


@pytest.mark.parametrize('preset', ['totensor', 'vit', 'imagenet'])
@pytest.mark.parametrize('out', ['nchw_f32', 'nhwc_bf16', 'nhwc_f16'])
def test_presets_and_output_dtypes(preset, out):
    """each preset x layout equals table[channel][resized byte], cast once"""
    from svol_amd.ingest import FrameIngest
    z = _golden()
    x, y = z['c1/x'], z['c1/y']                      # 96 x 128 -> 40 x 56
    table = torch.from_numpy(z[f'lut/{preset}'])     # as torch / torchvision's constants / ViTImageProcessor produce it
    m = FrameIngest(y.shape[:2], preset, out=out)
    got = m(torch.from_numpy(x)[None].to(DEV)).cpu()
    u = torch.from_numpy(y).long()                   # [OH, OW, 3]
    want = torch.stack([table[c][u[..., c]] for c in range(3)], -1)    # [OH, OW, 3] fp32
    if out == 'nchw_f32':
        assert got.dtype == torch.float32 and torch.equal(got[0], want.permute(2, 0, 1))
    else:
        dt = torch.bfloat16 if out == 'nhwc_bf16' else torch.float16
        assert got.dtype == dt and got.shape == (1, 40, 56, 3) and torch.equal(got[0], want.to(dt))


def test_large_downscale_matches_the_restatement():
    from tests import ingest_ref
    x = ingest_ref.noise(7, 1080, 1920)[None]
    got = _resize(torch.from_numpy(x).to(DEV), (224, 224))
    assert torch.equal(got.cpu(), _ref_nchw(x, (224, 224)))


def test_flip_crop_list_and_empty():
    from svol_amd.ingest import FrameIngest
    from tests import ingest_ref
    # n = 3, the middle image mirrored, both layouts
    x = np.stack([ingest_ref.noise(20 + i, 45, 61) for i in range(3)])
    want = _ref_nchw(x, (33, 50))
    want[1] = want[1].flip(-1)
    flip = torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    assert torch.equal(_resize(xd, (33, 50), flip=flip).cpu(), want)
    got = _resize(xd, (33, 50), flip=flip, nhwc=True, dtype=torch.bfloat16)
    assert torch.equal(got.cpu(), want.permute(0, 2, 3, 1).bfloat16())        # bytes are exact in bf16
    # a cropped view of a larger tensor: odd byte offset (3 * (3 * 66 + 5) = 609), row stride 3 * 66 = 198 (no multiple of 4)
    big = np.stack([ingest_ref.noise(30 + i, 50, 66) for i in range(2)])
    view = torch.from_numpy(big).to(DEV)[:, 3:, 5:]
    assert view.data_ptr() % 2 == 1 and view.stride(1) % 4 != 0 and not view.is_contiguous()
    assert torch.equal(_resize(view, (40, 40)).cpu(), _ref_nchw(big[:, 3:, 5:], (40, 40)))
    # a pixel stride other than 3: the RGB channels of an RGBA tensor
    rgba = np.random.default_rng(5).integers(0, 256, size=(1, 21, 19, 4), dtype=np.uint8)
    assert torch.equal(_resize(torch.from_numpy(rgba).to(DEV)[..., :3], (16, 24)).cpu(), _ref_nchw(rgba[..., :3], (16, 24)))
    # a list with two sizes lands in one tensor, in order; [B,T,H,W,3] keeps its leading dimensions; n = 0 launches nothing
    m = FrameIngest((24, 32), 'totensor')
    a, b = ingest_ref.noise(40, 30, 50)[None], np.stack([ingest_ref.noise(41 + i, 64, 48) for i in range(2)])
    got = m([torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)])
    want = torch.cat([_ref_nchw(a, (24, 32)), _ref_nchw(b, (24, 32))]) / 255
    assert got.shape == (3, 3, 24, 32) and torch.equal(got.cpu(), want)
    got5 = m(torch.from_numpy(b).to(DEV)[None], flip=torch.tensor([1, 0], dtype=torch.uint8, device=DEV))
    assert got5.shape == (1, 2, 3, 24, 32) and torch.equal(got5[0, 0].cpu(), want[1].flip(-1)) and torch.equal(got5[0, 1].cpu(), want[2])
    assert m(torch.empty((0, 30, 50, 3), dtype=torch.uint8, device=DEV)).shape == (0, 3, 24, 32)
    with pytest.raises(TypeError):
        m(torch.zeros((1, 30, 50, 3), device=DEV))


class GuardArena:
    """One int32 allocation of -0.0 words; take() returns tensors of it separated by guard zones (also one in front of the first and
    one behind the last); check() verifies every word outside the taken ranges."""

    def __init__(self, guard_bytes=1 << 16):
        self.guard = guard_bytes // 4
        self.req = []

    def plan(self, name, shape, dtype):
        self.req.append((name, tuple(shape), dtype))

    @staticmethod
    def _numel(shape):
        n = 1
        for s in shape:
            n *= s
        return n

    def build(self):
        off = self.guard
        self.slots = {}
        for name, shape, dtype in self.req:
            words = (self._numel(shape) * torch.empty((), dtype=dtype).element_size() + 3) // 4
            words = (words + 63) // 64 * 64          # 256-byte aligned starts
            self.slots[name] = (off, words, shape, dtype)
            off += words + self.guard
        self.buf = torch.full((off,), NEG0, dtype=torch.int32, device='cuda')
        return {name: self.buf[o:o + w].view(dtype)[:self._numel(shape)].view(shape) for name, (o, w, shape, dtype) in self.slots.items()}

    def check(self, what):
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for name, (o, w, shape, dtype) in self.slots.items():
            used = (self._numel(shape) * torch.empty((), dtype=dtype).element_size() + 3) // 4
            keep[o:o + used] = False
        bad = (self.buf != NEG0) & keep
        if bool(bad.any()):
            idx = int(torch.nonzero(bad)[0])
            near = [nm for nm, (o, w, _, _) in self.slots.items() if o - self.guard <= idx < o + w + self.guard]
            raise AssertionError(f'{what}: guard word {idx} changed ({int(bad.sum())} words in all); nearest buffer(s): {near}')


@pytest.mark.parametrize('size', [(33, 50), (30, 64)])
def test_red_zones(size):
    """outputs carved out of a -0.0 arena: guards intact and every element written (no table entry is -0.0); the source ends exactly
    where its allocation ends and starts at an odd address, so the reads of its last rows have nothing behind them to borrow"""
    from tests import ingest_ref
    OH, OW = size
    n, H, W = 2, 45, 61
    x = np.stack([ingest_ref.noise(60 + i, H, W) for i in range(n)])
    store = torch.empty(1 + n * H * W * 3, dtype=torch.uint8, device=DEV)
    src = store[1:].view(n, H, W, 3)
    src.copy_(torch.from_numpy(x))
    arena = GuardArena()
    arena.plan('f32', (n, 3, OH, OW), torch.float32)
    arena.plan('bf16', (n, OH, OW, 3), torch.bfloat16)
    arena.plan('f16', (n, OH, OW, 3), torch.float16)
    t = arena.build()
    flip = torch.tensor([1, 0], dtype=torch.uint8, device=DEV)
    _resize(src, size, flip=flip, out=t['f32'])
    _resize(src, size, flip=flip, out=t['bf16'], nhwc=True)
    _resize(src, size, out=t['f16'], nhwc=True)
    torch.cuda.synchronize()
    arena.check(f'ingest {H}x{W} -> {OH}x{OW}')
    want = _ref_nchw(x, size)
    plain = want.clone()
    want[0] = want[0].flip(-1)
    assert torch.equal(t['f32'].cpu(), want)
    assert torch.equal(t['bf16'].cpu(), want.permute(0, 2, 3, 1).bfloat16())
    assert torch.equal(t['f16'].cpu(), plain.permute(0, 2, 3, 1).half())
    assert bool((t['f32'].view(torch.int32) != NEG0).all())
    assert bool((t['bf16'].view(torch.int16) != -2 ** 15).all()) and bool((t['f16'].view(torch.int16) != -2 ** 15).all())


def test_geometry_beyond_the_limit_is_refused_without_a_launch():
    """include/svol_hip.h: at most 64 taps per axis.  A 40-fold downscale (81 taps) returns SVOL_E_UNSUPPORTED and writes nothing."""
    from svol_amd import _lib
    from svol_amd.ops import _ptr, _stream
    H, W, OH, OW = 8960, 8, 224, 8
    src = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=DEV)
    (ytab, ky), (xtab, kx) = _tab(H, OH), _tab(W, OW)
    assert ky == 81
    out = torch.full((1, 3, OH, OW), -7.0, device=DEV)
    rc = _lib.lib().svol_ingest_resize(_ptr(src), 1, H, W, H * W * 3, W * 3, 3, _ptr(xtab), kx, _ptr(ytab), ky, _ptr(_ident_lut()), 0,
                                       _ptr(out), 3 * OH * OW, OH * OW, OW, 1, OH, OW, 0, _stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((out == -7.0).all())
    # the limit itself is taken: 64 taps = a 31-fold downscale (k = 2 * 31 + 1 = 63)
    Hk = 31 * 16
    x = np.random.default_rng(9).integers(0, 256, size=(1, Hk, 8, 3), dtype=np.uint8)
    assert _tab(Hk, 16)[1] == 63
    assert torch.equal(_resize(torch.from_numpy(x).to(DEV), (16, 8)).cpu(), _ref_nchw(x, (16, 8)))


def test_resnet_stem_consumes_the_nhwc_image():
    """tokens of the uint8 route (FrameIngest -> bf16 NHWC -> the stem's im2col through strides) equal the tokens of
    restatement -> fp32 NCHW -> today's route: the pixel is rounded to bf16 once either way"""
    from svol_amd.ingest import FrameIngest
    from svol_amd.modeling.resnet import ResNetExtractor
    from tests import ingest_ref
    torch.manual_seed(3)
    m = ResNetExtractor().to(DEV).eval()
    x = np.stack([ingest_ref.noise(70 + i, 50, 70) for i in range(2)])
    pix = FrameIngest((64, 64), 'totensor', out='nhwc_bf16')(torch.from_numpy(x).to(DEV))
    got = m(pix, nhwc=True)
    want = m((_ref_nchw(x, (64, 64)) / 255).to(DEV))
    assert got.shape == want.shape == (2, 4, 512) and torch.equal(got, want)


def _model(argv):
    from svol_amd import configs
    from svol_amd.modeling.model import build_model
    torch.manual_seed(11)
    return build_model(configs.parse_args(argv + ['--num_layers', '1', '--num_queries', '10', '--matcher', 'video_matcher'])).to(DEV).eval()


@pytest.mark.parametrize('backbone,T', [('resnet', 2), ('vit', 1)])
def test_model_takes_raw_frames(backbone, T):
    """build_model: uint8 frames 90 x 120 and a uint8 sketch 70 x 70 give the logits and boxes of the float-input call, bit for bit"""
    from svol_amd.ingest import preset_table
    from tests import ingest_ref
    model = _model(['--backbone', backbone] + (['--freeze_backbone'] if backbone == 'resnet' else []))
    vid = np.stack([ingest_ref.noise(80 + i, 90, 120) for i in range(T)])
    sk = ingest_ref.noise(90, 70, 70)[None]
    table = preset_table('totensor' if backbone == 'resnet' else 'vit')

    def pixels(x):   # the float input a caller builds on the host today
        u = _ref_nchw(x, (224, 224)).long()
        return torch.stack([table[c][u[:, c]] for c in range(3)], 1)[None].to(DEV)
    ms, mv = torch.ones(1, 1, device=DEV), torch.ones(1, T, device=DEV)
    want = model(pixels(sk), pixels(vid), ms, mv)
    got = model(torch.from_numpy(sk)[None].to(DEV), torch.from_numpy(vid)[None].to(DEV), ms, mv)
    assert torch.equal(got['pred_logits'], want['pred_logits']) and torch.equal(got['pred_boxes'], want['pred_boxes'])
    assert bool(torch.isfinite(got['pred_logits']).all())
    # a list of per-video tensors (sizes may differ between videos) is the same call
    got = model([torch.from_numpy(sk).to(DEV)], [torch.from_numpy(vid).to(DEV)], ms, mv)
    assert torch.equal(got['pred_logits'], want['pred_logits']) and torch.equal(got['pred_boxes'], want['pred_boxes'])


def test_graph_capture_and_replay():
    from svol_amd.ingest import FrameIngest
    from tests import ingest_ref
    m = FrameIngest((32, 48), 'imagenet', out='nhwc_bf16')
    x = torch.from_numpy(np.stack([ingest_ref.noise(95 + i, 40, 72) for i in range(2)])).to(DEV)
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
    # a size the module has not seen needs a host-to-device copy of its tables: refused before anything is captured
    g2 = torch.cuda.CUDAGraph()
    unseen = torch.zeros((1, 41, 73, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match='before capturing'):
        with torch.cuda.graph(g2):
            static.copy_(x)      # (the capture is not empty when it ends)
            m(unseen)
    m.prepare(41, 73)
    assert m(unseen).shape == (1, 32, 48, 3)
