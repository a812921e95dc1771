"""Writes tests/golden/ingest_filter_cases.npz: seeded uint8 inputs, grey (mode L) and RGB, with what Pillow's Image.resize makes of
them under each of BOX, BILINEAR, HAMMING, BICUBIC and LANCZOS (one stacked array per case and mode, in that order; the grey source
of a case is the green channel of its RGB source, as a mode-L image); the QuickDraw line itself (a 28 x 28 bitmap, inverted, BICUBIC
to 224 x 224: the reference's preprocess/quickdraw_array_to_pil.py:36); and 0 / 255 inputs under BICUBIC and LANCZOS, whose
overshoot reaches both clamps in both passes.

    python tests/golden/make_golden_ingest_filters.py        # needs Pillow; nothing else

Small outputs on purpose: the file stays under 500 KB."""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = {'box': Image.BOX, 'bilinear': Image.BILINEAR, 'hamming': Image.HAMMING, 'bicubic': Image.BICUBIC, 'lanczos': Image.LANCZOS}
# (H, W) -> (OH, OW): upscale; downscale; one axis up, one down; identity; one axis unchanged; degenerate; taps clipped at both ends
# (lanczos k = 51 along the 200); a sliver
CASES = [((37, 53), (64, 64)), ((96, 128), (40, 56)), ((75, 77), (74, 78)), ((64, 64), (64, 64)), ((64, 40), (64, 56)), ((1, 1), (8, 8)),
         ((2, 200), (16, 24)), ((300, 7), (24, 16))]
# 0 / 255 inputs (bicubic and lanczos only): RGB and grey
BW_CASES = [((37, 53, 3), (64, 64)), ((20, 24), (48, 40))]


def resize(x, size, flt):
    OH, OW = size
    y = np.asarray(Image.fromarray(x, 'L' if x.ndim == 2 else 'RGB').resize((OW, OH), FILTERS[flt]))
    assert y.shape == (OH, OW) + x.shape[2:] and y.dtype == np.uint8
    return y


def quickdraw_bitmap(seed=7):
    """a 28 x 28 bitmap in QuickDraw's convention (strokes bright on black): a few seeded random walks with soft edges"""
    rng = np.random.default_rng(seed)
    b = np.zeros((28, 28), np.int64)
    for _ in range(4):
        y, x = rng.integers(4, 24, size=2)
        for _ in range(30):
            b[y, x] = 255
            for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0)):
                yy, xx = y + dy, x + dx
                if 0 <= yy < 28 and 0 <= xx < 28:
                    b[yy, xx] = max(b[yy, xx], int(rng.integers(40, 200)))
            y = int(np.clip(y + rng.integers(-1, 2), 0, 27))
            x = int(np.clip(x + rng.integers(-1, 2), 0, 27))
    return b.astype(np.uint8)


def main():
    out = {'n': np.int64(len(CASES)), 'n_bw': np.int64(len(BW_CASES))}
    for i, ((H, W), size) in enumerate(CASES):
        rgb = np.random.default_rng(2000 + i).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        out[f'c{i}/x'] = rgb                                    # the grey source is its green channel, as a mode-L image
        for mode, x in (('grey', np.ascontiguousarray(rgb[..., 1])), ('rgb', rgb)):
            out[f'c{i}/{mode}'] = np.stack([resize(x, size, flt) for flt in FILTERS])    # [5, OH, OW(, 3)] in FILTERS' order
    bitmap = quickdraw_bitmap()
    out['qd/x'] = bitmap          # the raw bitmap, NOT inverted
    out['qd/y'] = np.asarray(Image.fromarray(255 - bitmap.reshape(28, 28)).resize((224, 224), Image.BICUBIC))
    for j, (shape, size) in enumerate(BW_CASES):
        x = (np.random.default_rng(3000 + j).integers(0, 2, size=shape) * 255).astype(np.uint8)
        out[f'bw{j}/x'] = x
        out[f'bw{j}/y'] = np.stack([resize(x, size, flt) for flt in ('bicubic', 'lanczos')])
    path = os.path.join(HERE, 'ingest_filter_cases.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
