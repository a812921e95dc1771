"""numpy restatement of Pillow's 8-bit bilinear resample (Resample.c: ImagingResampleHorizontal_8bpc, then
ImagingResampleVertical_8bpc) from svol_amd.ingest.resample_tables, in integer arithmetic: the reference of the ingest tests.
It does not import PIL; tests/test_ingest_tables.py pins it against the Pillow goldens and, where Pillow is installed, against
live Pillow."""
import numpy as np

from svol_amd.ingest import PRECISION_BITS, resample_tables


def _pass(img, tab, axis):
    """one pass along `axis` (0 rows / 1 columns) of a uint8 [H, W, C] image with the table of that axis"""
    k = tab.shape[1] - 2
    src = np.moveaxis(img.astype(np.int64), axis, 0)          # [in, other, C]
    idx = tab[:, :1].astype(np.int64) + np.arange(k)[None, :]  # [out, k]
    valid = np.arange(k)[None, :] < tab[:, 1:2]
    idx = np.where(valid, idx, 0)
    w = np.where(valid, tab[:, 2:], 0).astype(np.int64)        # taps past the count are not read
    acc = np.full((tab.shape[0],) + src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for i in range(k):
        acc += src[idx[:, i]] * w[:, i][:, None, None]
    assert acc.max() < 2 ** 31 and acc.min() >= 0          # the kernel's int32 accumulator is enough
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, size):
    """uint8 [H, W, C] -> uint8 [OH, OW, C]: horizontal pass, ROUNDED to uint8, then the vertical pass (Pillow's order)"""
    OH, OW = size
    H, W = img.shape[:2]
    t = _pass(np.ascontiguousarray(img), resample_tables(W, OW), 1)
    return _pass(t, resample_tables(H, OH), 0)


def noise(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
