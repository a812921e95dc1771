"""Frame ingest on the device: raw uint8 frames and sketches -> the backbones' inputs (csrc/ingest.hip, svol_ingest_resize and
svol_ingest_resample).

The reference preprocesses on the model path: ``lib/modeling/backbone.py:31,49`` runs ``ViTFeatureExtractor(images=[frame])``
inside ``ViTBackbone.forward`` (PIL bilinear resize to 224 x 224, x 1/255, mean / std 0.5) and
``lib/dataset/svol_dataset.py:218-229`` runs ``Resize((224,224))`` + ``ToTensor()`` per frame for the ResNet path.  Here the
resize is Pillow's 8-bit bilinear resample restated in integers — the same fixed-point taps, the same uint8 rounding between the
horizontal and the vertical pass — so the resized bytes equal ``PIL.Image.resize(size, Image.BILINEAR)`` bit for bit, and the float
stage is a 256-entry table per channel built once on the host, so it equals what ``ToTensor`` / ``ViTImageProcessor`` compute bit
for bit as well (the in-kernel ``v * (2/255) - 1`` would be off by 1.2e-7).

The sketch, the other input of every model call, is made by ``preprocess/quickdraw_array_to_pil.py:36``
(``Image.fromarray(255 - bitmap.reshape(28, 28)).resize((224, 224), Image.BICUBIC)``) and opened with ``.convert('RGB')``
(``lib/dataset/svol_dataset.py:212-229``): a single-channel image, inverted, resampled with a filter that has negative lobes.
``FrameIngest(..., filter='bicubic', invert=True)`` on the raw 28 x 28 bitmaps is that line; grey files of any size and the other
Pillow filters go the same way (svol_ingest_resample: signed taps, one source channel through both passes).

    resample_tables(in_size, out_size, filter)   Pillow's precompute_coeffs + normalize_coeffs_8bpc: box, bilinear, hamming, bicubic, lanczos
    preset_table(preset, mean, std)              the [3, 256] fp32 table of 'totensor' / 'vit' / 'imagenet' or explicit mean / std
    FrameIngest                                  nn.Module without parameters: uint8 [n,H,W,3] / [B,T,H,W,3] / grey / a list -> one tensor
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from . import _lib, ops

PRECISION_BITS = 22
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # torchvision's constants
_OUT = {'nchw_f32': torch.float32, 'nhwc_bf16': torch.bfloat16, 'nhwc_f16': torch.float16}


def is_raw_frames(x) -> bool:
    """what the backbones send through a FrameIngest: a uint8 tensor, or a list of (uint8) frame tensors"""
    return isinstance(x, (list, tuple)) or (isinstance(x, torch.Tensor) and x.dtype == torch.uint8)


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    return max(0.0, 1.0 - abs(x))


_H54, _H46 = float(np.float32(0.54)), float(np.float32(0.46))   # Resample.c writes these two as float literals (0.54f, 0.46f)


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x *= math.pi
    return math.sin(x) / x * (_H54 + _H46 * math.cos(x))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x *= math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# Pillow's Resample.c: the kernel function and its support, per filter name
FILTERS = {'box': (_box, 0.5), 'bilinear': (_bilinear, 1.0), 'hamming': (_hamming, 1.0), 'bicubic': (_bicubic, 2.0), 'lanczos': (_lanczos, 3.0)}


def sketch_frames(x):
    """a raw sketch batch for FrameIngest: a 4-D uint8 tensor [B,1,H,W] is grey -> [B,1,H,W,1] (RGB sketches are [B,1,H,W,3]; as in
    FrameIngest a 4-D tensor whose last dimension is 3 keeps meaning RGB)"""
    return x.unsqueeze(-1) if isinstance(x, torch.Tensor) and x.dim() == 4 and x.shape[-1] != 3 else x


def resample_tables(in_size: int, out_size: int, filter: str = 'bilinear') -> np.ndarray:
    """int32 [out_size, 2 + k]: per output index the first source index, the tap count and k fixed-point taps (22 fraction
    bits) — Pillow's ``precompute_coeffs`` and ``normalize_coeffs_8bpc`` for ``filter`` (box, bilinear, hamming, bicubic with
    a = -0.5, lanczos), in Python floats (doubles).  Bicubic and lanczos taps may be negative (rounded away from zero, as Pillow
    rounds them).  An axis of unchanged size has the identity's taps under every filter, which is how Pillow's skipped pass
    is reproduced."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f'sizes must be positive, got {in_size} -> {out_size}')
    if filter not in FILTERS:
        raise ValueError(f"unknown filter '{filter}' ({', '.join(FILTERS)})")
    kernel, width = FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = width * fs
    k = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    tab = np.zeros((out_size, 2 + k), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [kernel((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        tab[xx, 0], tab[xx, 1] = xmin, xmax
        for x, v in enumerate(w):
            if ww != 0.0:
                v /= ww
            tab[xx, 2 + x] = int((-0.5 if v < 0 else 0.5) + v * (1 << PRECISION_BITS))
    return tab


def preset_table(preset: str = 'totensor', mean=None, std=None) -> torch.Tensor:
    """[3, 256] fp32 (CPU): the value a byte v becomes in channel c.
    'totensor'  v / 255 in IEEE fp32: torchvision's ToTensor (the dataset's transform)
    'vit'       ViTImageProcessor of google/vit-base-patch16-224-in21k: float32(float64(v) * (1/255)), then (x - 0.5) / 0.5 in fp32
    'imagenet'  (totensor - mean) / std in fp32 with torchvision's constants
    explicit mean= / std= (per channel or scalar) replace the preset's."""
    v = torch.arange(256, dtype=torch.uint8)
    if preset == 'vit':
        base = (v.double() * (1 / 255)).float()
        m, s = (0.5,) * 3, (0.5,) * 3
    elif preset in ('totensor', 'imagenet'):
        base = v.float().div(255)
        m, s = (IMAGENET_MEAN, IMAGENET_STD) if preset == 'imagenet' else (None, None)
    else:
        raise ValueError(f"unknown preset '{preset}' (totensor, vit, imagenet)")
    if mean is not None or std is not None:
        m = (0.0,) * 3 if mean is None else mean
        s = (1.0,) * 3 if std is None else std
    if m is None:
        return base.expand(3, 256).contiguous()
    m = torch.as_tensor(m, dtype=torch.float32).expand(3)
    s = torch.as_tensor(s, dtype=torch.float32).expand(3)
    return ((base[None, :] - m[:, None]) / s[:, None]).contiguous()


class FrameIngest(nn.Module):
    """uint8 frames -> backbone input, one svol_ingest_resize / svol_ingest_resample launch per distinct source size.

    filter  Pillow's resampling filter: 'box', 'bilinear' (the default), 'hamming', 'bicubic' or 'lanczos'
    invert  True: every source byte b enters the resize as 255 - b (QuickDraw's bitmaps are white on black)
    RGB sources with filter='bilinear' and invert=False go to svol_ingest_resize, as they always have; anything else goes to
    svol_ingest_resample.

    forward(frames, flip=None):
      frames  a uint8 device tensor [n,H,W,3] or [B,T,H,W,3] — any strides with channel stride 1, so a sliced or cropped view
              needs no copy — or a grey one, [n,H,W], [n,H,W,1] or [B,T,H,W,1] (any strides; what .convert('RGB') would replicate:
              one channel is resized and the three output channels are table[c][byte]), or a list of such tensors with different
              H x W; the results land in ONE output tensor, in order.  A 4-D tensor whose last dimension is 3 is RGB.
      flip    optional uint8 [n] (n = all frames, in order): nonzero mirrors that frame's output columns.  The reference flips each
              frame on its own and never flips the boxes: boxes are the caller's business.
      ->      out='nchw_f32': [n,3,OH,OW] fp32; 'nhwc_bf16' / 'nhwc_f16': [n,OH,OW,3] (5-D input: [B,T,...])

    The tap tables are cached per (device, in, out, filter) on the device; building one is a host-to-device copy, so a size must have
    been seen (or ``prepare``d) before a graph capture meets it — a capture on an unseen size raises before anything is captured.
    CPU tensors and other dtypes raise: like the rest of the product there is no host path."""

    def __init__(self, size=(224, 224), preset='totensor', mean=None, std=None, out='nchw_f32', filter='bilinear', invert=False):
        super().__init__()
        if out not in _OUT:
            raise ValueError(f"out must be one of {sorted(_OUT)}, got '{out}'")
        if filter not in FILTERS:
            raise ValueError(f"filter must be one of {sorted(FILTERS)}, got '{filter}'")
        self.filter, self.invert = filter, bool(invert)
        self.size = (int(size[0]), int(size[1]))
        self.preset, self.out = preset, out
        self._lut_cpu = preset_table(preset, mean, std)
        self._lut = {}      # device -> [3,256] fp32
        self._tabs = {}     # (device, in, out, filter) -> (int32 [out, 2+k], k)

    def _table(self, dev, n_in, n_out):
        key = (dev, n_in, n_out, self.filter)
        ent = self._tabs.get(key)
        if ent is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'FrameIngest: no tap table for {n_in} -> {n_out} yet and a graph is being captured (a table is a '
                                   'host-to-device copy): run this size once, or call prepare(H, W), before capturing')
            t = resample_tables(n_in, n_out, self.filter)
            ent = self._tabs[key] = (torch.from_numpy(t).to(dev), t.shape[1] - 2)
        return ent

    def _lut_on(self, dev):
        lut = self._lut.get(dev)
        if lut is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('FrameIngest: first use on this device inside a graph capture: run it once before capturing')
            lut = self._lut[dev] = self._lut_cpu.to(dev)
        return lut

    def prepare(self, H, W, device=None):
        """build (outside a capture) the tables a later captured call on H x W frames needs"""
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._lut_on(dev)
        self._table(dev, int(H), self.size[0])
        self._table(dev, int(W), self.size[1])
        return self

    def forward(self, frames, flip=None):
        items = list(frames) if isinstance(frames, (list, tuple)) else [frames]
        lead = None
        flat = []
        for t in items:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError('svol_amd FrameIngest runs on the MI355X HIP kernels only (no CPU path): pass device tensors')
            if t.dtype != torch.uint8:
                raise TypeError(f'FrameIngest takes uint8 frames, got {t.dtype}')
            if not (t.dim() == 3 or (t.dim() in (4, 5) and t.shape[-1] in (1, 3))):
                raise ValueError(f'frames must be [n,H,W,3] or [B,T,H,W,3], or grey [n,H,W], [n,H,W,1] or [B,T,H,W,1], got {tuple(t.shape)}')
            if t.dim() == 5:
                if not isinstance(frames, (list, tuple)):
                    lead = tuple(t.shape[:2])
                t = t.flatten(0, 1)   # a view where the strides allow it
            if t.dim() == 4 and t.shape[3] == 1:
                t = t[..., 0]         # grey: [n,H,W], any strides
            elif t.dim() == 4 and t.shape[0] and t.stride(3) != 1:
                t = t.contiguous()
            flat.append(t)
        dev = flat[0].device
        n = sum(t.shape[0] for t in flat)
        OH, OW = self.size
        dt = _OUT[self.out]
        nchw = self.out == 'nchw_f32'
        out = torch.empty((n, 3, OH, OW) if nchw else (n, OH, OW, 3), dtype=dt, device=dev)
        if flip is not None:
            if not flip.is_cuda or flip.dtype != torch.uint8 or flip.numel() != n:
                raise ValueError(f'flip must be a uint8 device tensor with one entry per frame ({n})')
            flip = flip.contiguous().view(-1)
        lut = self._lut_on(dev) if n else None
        i = 0
        for t in flat:
            m, H, W = t.shape[0], t.shape[1], t.shape[2]
            if m == 0:
                continue
            (ytab, ky), (xtab, kx) = self._table(dev, H, OH), self._table(dev, W, OW)
            o = out[i:i + m]
            strides = (o.stride(0), o.stride(1), o.stride(2), o.stride(3)) if nchw else (o.stride(0), o.stride(3), o.stride(1), o.stride(2))
            fl = flip[i:i + m] if flip is not None else None
            if t.dim() == 4 and self.filter == 'bilinear' and not self.invert:
                ops.ingest_resize(t, xtab, kx, ytab, ky, lut, fl, o, strides, OH, OW)
            else:
                ops.ingest_resample(t, xtab, kx, ytab, ky, lut, fl, o, strides, OH, OW, invert=self.invert)
            i += m
        return out.view(*lead, *out.shape[1:]) if lead is not None else out
