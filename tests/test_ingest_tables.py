"""CPU-side checks of the frame ingest (svol_amd/ingest.py, csrc/ingest.hip): the integer restatement of Pillow's bilinear resample
(tests/ingest_ref.py over svol_amd.ingest.resample_tables) against the Pillow goldens of tests/golden/ingest_cases.npz and against
live Pillow, the preset tables against what torch / torchvision's constants / transformers' ViTImageProcessor produce, and the C
entry's argument validation without a device."""
import os

import numpy as np
import pytest
import torch

from svol_amd import ingest
from tests import ingest_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, 'tests', 'golden', 'ingest_cases.npz'))
# H x W sources resized to 224 x 224
LIVE_SIZES = [(224, 224), (375, 500), (37, 53), (1, 1), (480, 640), (640, 360), (223, 225), (1080, 1920), (2, 3000), (449, 447),
              (7, 224), (224, 7), (3584, 300)]


@pytest.mark.parametrize('i', range(int(GOLDEN['n'])))
def test_restatement_equals_pillow_golden(i):
    x, y = GOLDEN[f'c{i}/x'], GOLDEN[f'c{i}/y']
    got = ingest_ref.resize_u8(x, y.shape[:2])
    assert got.dtype == np.uint8 and np.array_equal(got, y)


@pytest.mark.parametrize('H,W', LIVE_SIZES)
def test_restatement_equals_live_pillow(H, W):
    Image = pytest.importorskip('PIL.Image')
    x = ingest_ref.noise(H * 10007 + W, H, W)
    want = np.asarray(Image.fromarray(x, 'RGB').resize((224, 224), Image.BILINEAR))
    assert np.array_equal(ingest_ref.resize_u8(x, (224, 224)), want)


def test_tables_shape_and_identity():
    t = ingest.resample_tables(224, 224)
    assert t.dtype == np.int32 and t.shape == (224, 2 + 3)
    assert (t[:, 0] == np.arange(224)).all() and (t[:-1, 1] == 2).all() and t[-1, 1] == 1
    assert (t[:, 2] == 1 << 22).all() and (t[:, 3:] == 0).all()          # the identity: no special case needed
    t = ingest.resample_tables(3840, 224)                                # scale 17.14: k = 2 * 18 + 1
    assert t.shape == (224, 2 + 37) and t[:, 2:].min() >= 0              # bilinear taps are never negative
    assert (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= 3840).all() and (t[:, 1] >= 1).all()
    assert 255 * int(t[:, 2:].sum(1).max()) + (1 << 21) < 2 ** 31         # int32 is enough
    with pytest.raises(ValueError):
        ingest.resample_tables(0, 224)


def test_window_growth_bound_the_kernel_tiles_by():
    """include/svol_hip.h: t neighbouring outputs touch at most ceil((t-1) in/out) + k source indices"""
    for n_in, n_out in [(360, 224), (480, 224), (3840, 224), (37, 64), (1, 8), (600, 24), (7, 16), (9216, 512), (225, 224)]:
        tab = ingest.resample_tables(n_in, n_out)
        k = tab.shape[1] - 2
        lo, hi = tab[:, 0].astype(np.int64), (tab[:, 0] + tab[:, 1]).astype(np.int64)
        assert (np.diff(lo) >= 0).all()
        for t in (1, 2, 4, 16, 32, n_out):
            t = min(t, n_out)
            span = hi[t - 1:] - lo[:n_out - t + 1]
            assert span.max() <= min(-(-(t - 1) * n_in // n_out) + k, n_in), (n_in, n_out, t)


@pytest.mark.parametrize('preset', ['totensor', 'vit', 'imagenet'])
def test_presets_equal_the_golden_tables(preset):
    got = ingest.preset_table(preset)
    assert got.dtype == torch.float32 and got.shape == (3, 256)
    assert np.array_equal(got.numpy().view(np.uint32), GOLDEN[f'lut/{preset}'].view(np.uint32))


def test_explicit_mean_std_override_the_preset():
    got = ingest.preset_table('totensor', mean=(0.5, 0.25, 0.0), std=(0.5, 0.5, 2.0))
    v = torch.arange(256, dtype=torch.uint8).float().div(255)
    assert torch.equal(got[1], (v - 0.25) / 0.5) and torch.equal(got[2], v / 2.0)
    with pytest.raises(ValueError):
        ingest.preset_table('bicubic')
    with pytest.raises(ValueError):
        ingest.FrameIngest(out='nchw_bf16')


def test_frame_ingest_and_feature_backbone_refuse_without_a_device_path():
    f = ingest.FrameIngest()
    assert len(list(f.parameters())) == 0
    with pytest.raises(RuntimeError):
        f(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))              # a CPU tensor: no host path
    from svol_amd.modeling.model import FeatureBackbone
    with pytest.raises(TypeError):
        FeatureBackbone()(torch.zeros(1, 1, 8), torch.zeros(1, 2, 4, 4, 3, dtype=torch.uint8))


def test_argument_validation_without_gpu():
    """Null pointers, bad sizes and geometries beyond the documented limit are rejected before any launch; n == 0 launches nothing."""
    from svol_amd import _lib
    fn = _lib.lib().svol_ingest_resize
    P = 4096   # never dereferenced on the host

    def call(src=P, n=1, H=8, W=8, xtab=P, kx=3, ytab=P, ky=3, lut=P, out=P, OH=8, OW=8, dt=0, s_w=3):
        return fn(src, n, H, W, H * W * 3, W * 3, s_w, xtab, kx, ytab, ky, lut, 0, out, 3 * OH * OW, OH * OW, OW, 1, OH, OW, dt, 0)
    for bad in (dict(src=0), dict(xtab=0), dict(ytab=0), dict(lut=0), dict(out=0), dict(n=-1), dict(H=0), dict(W=0), dict(OH=0),
                dict(OW=0), dict(kx=0), dict(ky=0), dict(dt=3), dict(s_w=-1)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0
    # beyond the limit: more than 64 taps per axis (a 40-fold downscale), an output wider than 16384
    assert call(H=8960, ky=81) == -2 and call(W=8960, kx=81) == -2
    assert call(OW=16385) == -2 and call(OH=16385) == -2
    # a huge image count must not wrap the grid
    assert call(n=1 << 40) == -2
