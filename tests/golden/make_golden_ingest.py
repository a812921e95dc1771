"""Writes tests/golden/ingest_cases.npz: seeded uint8 RGB inputs with what Pillow's Image.resize(size, BILINEAR) makes of them, and
the three preset tables as torch (ToTensor's arithmetic), torchvision's constants and transformers' ViTImageProcessor produce them.

    python tests/golden/make_golden_ingest.py        # needs Pillow and transformers; nothing else

Small outputs on purpose: the file stays well under 700 KB."""
import os

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
# (H, W) -> (OH, OW): upscale with 159-byte rows; scale 2.4 / 2.29; near-identity, mixed up and down; identity; 1 x 1;
# 25 x horizontal with clipped taps at both ends; a tall sliver
CASES = [((37, 53), (64, 64)), ((96, 128), (40, 56)), ((75, 77), (74, 78)), ((64, 64), (64, 64)), ((1, 1), (8, 8)),
         ((2, 600), (16, 24)), ((300, 7), (24, 16))]


def main():
    out = {'n': np.int64(len(CASES))}
    for i, ((H, W), (OH, OW)) in enumerate(CASES):
        x = np.random.default_rng(1000 + i).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        y = np.asarray(Image.fromarray(x, 'RGB').resize((OW, OH), Image.BILINEAR))
        assert y.shape == (OH, OW, 3) and y.dtype == np.uint8
        out[f'c{i}/x'], out[f'c{i}/y'] = x, y
    v = torch.arange(256, dtype=torch.uint8)
    tt = v.float().div(255)     # torchvision.transforms.functional.to_tensor: img.to(float32).div(255)
    out['lut/totensor'] = tt.expand(3, 256).numpy().copy()
    mean = torch.tensor((0.485, 0.456, 0.406))[:, None]
    std = torch.tensor((0.229, 0.224, 0.225))[:, None]
    out['lut/imagenet'] = ((tt[None] - mean) / std).numpy()      # torchvision.transforms.Normalize on ToTensor's output
    from transformers import ViTImageProcessor
    proc = ViTImageProcessor(do_resize=False, do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=[0.5] * 3,
                             image_std=[0.5] * 3)     # preprocessor_config.json of google/vit-base-patch16-224-in21k, resize aside
    img = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (4, 256, 3)).copy()     # every byte value in every channel
    pv = proc(images=[img], return_tensors='np')['pixel_values'][0]   # [3, 4, 256]
    assert pv.dtype == np.float32 and (pv == pv[:, :1]).all()
    out['lut/vit'] = pv[:, 0, :].copy()
    path = os.path.join(HERE, 'ingest_cases.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
