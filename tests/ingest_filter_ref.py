"""numpy restatement of Pillow's 8-bit resample (Resample.c: ImagingResampleHorizontal_8bpc, then ImagingResampleVertical_8bpc) for
any of its filters, from svol_amd.ingest.resample_tables(in, out, filter): signed taps, an int32 accumulator from 2^21, an arithmetic
shift by 22, a clamp to [0, 255] after each pass.  The reference of the svol_ingest_resample tests.  It does not import PIL;
tests/test_ingest_filter_tables.py pins it against the Pillow goldens of tests/golden/ingest_filter_cases.npz and, where Pillow is
installed, against live Pillow."""
import numpy as np

from svol_amd.ingest import PRECISION_BITS, resample_tables

FILTERS = ('box', 'bilinear', 'hamming', 'bicubic', 'lanczos')
MAX_TAPS = 64      # include/svol_hip.h: kx, ky <= 64


def _pass(img, tab, axis, stats=None):
    """one pass along `axis` (0 rows / 1 columns) of a uint8 [H, W, C] image with the table of that axis; `stats` (a list) receives
    the smallest and the largest accumulator BEFORE the shift and the clamp"""
    k = tab.shape[1] - 2
    src = np.moveaxis(img.astype(np.int64), axis, 0)          # [in, other, C]
    idx = tab[:, :1].astype(np.int64) + np.arange(k)[None, :]  # [out, k]
    valid = np.arange(k)[None, :] < tab[:, 1:2]
    idx = np.where(valid, idx, 0)
    w = np.where(valid, tab[:, 2:], 0).astype(np.int64)        # taps past the count are not read
    acc = np.full((tab.shape[0],) + src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for i in range(k):
        acc += src[idx[:, i]] * w[:, i][:, None, None]
    assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31       # the kernel's int32 accumulator is enough
    if stats is not None:
        stats.append((int(acc.min()), int(acc.max())))
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)   # (>> of a negative numpy integer: arithmetic)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, size, filter='bilinear', invert=False, stats=None):
    """uint8 [H, W] (grey) or [H, W, C] -> uint8 [OH, OW] / [OH, OW, C]: the source inverted first if asked, the horizontal pass,
    ROUNDED to uint8, then the vertical pass (Pillow's order).  An axis of unchanged size runs through its table, which is the
    identity's (Pillow skips that pass).  stats: see _pass — [horizontal, vertical]."""
    OH, OW = size
    grey = img.ndim == 2
    x = np.ascontiguousarray(img[..., None] if grey else img)
    if invert:
        x = 255 - x
    H, W = x.shape[:2]
    t = _pass(x, resample_tables(W, OW, filter), 1, stats)
    y = _pass(t, resample_tables(H, OH, filter), 0, stats)
    return y[..., 0] if grey else y


def noise(seed, H, W, C=3):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, C) if C else (H, W), dtype=np.uint8)
