#!/usr/bin/env python3
"""Frame ingest (svol_ingest_resize) against a device-to-device copy, and the host-side Pillow time it replaces.

    python tools/bench_ingest.py [--frames 256] [--blocks 9] [--iters 10] [--no-host]

Per case (256 frames 360 x 480 -> 224 and 224 -> 224, fp32 NCHW and bf16 NHWC): the kernel and two copies are timed in ALTERNATING
blocks of `iters` launches between device events in one run; the figure is the median block.  The yardsticks: a copy OF
(bytes read + bytes written) bytes — the bar of profiles/ingest.md is kernel <= 2 x this one — and, for reference, a copy that MOVES
that many bytes (half the size: the same memory traffic as the kernel).  Bytes are the algorithm's: every source byte read once,
every output element written once.  The host figure is PIL resize + ToTensor's arithmetic for the same frames on this machine's
CPUs (one thread, and a 16-thread pool: Pillow releases the GIL while it resamples)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from svol_amd.ingest import FrameIngest


def blocks_ms(fns, blocks, iters):
    """median ms per call of each fn, blocks alternating fn by fn"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def host_ms(frames, size, threads):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    def one(f):
        img = Image.fromarray(f, 'RGB').resize((size[1], size[0]), Image.BILINEAR)
        return torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(255)      # torchvision's to_tensor
    t0 = time.perf_counter()
    if threads == 1:
        for f in frames:
            one(f)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, frames))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ingest.py measures on the MI355X; there is no CPU figure for a kernel'
    n, size = a.frames, (224, 224)
    rng = np.random.default_rng(0)
    print(f'# frame ingest, {n} frames -> {size[0]} x {size[1]}; median [min, max] of {a.blocks} alternating blocks of {a.iters} launches')
    print('| source | output | kernel ms | read+written MB | kernel GB/s | copy of (r+w) bytes ms | kernel / copy | same-traffic copy ms | kernel / same-traffic |')
    print('|---|---|---|---|---|---|---|---|---|')
    for H, W in ((360, 480), (224, 224)):
        x = torch.from_numpy(rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)).cuda()
        for out in ('nchw_f32', 'nhwc_bf16'):
            m = FrameIngest(size, 'totensor', out=out)
            y = m(x)
            nbytes = x.numel() + y.numel() * y.element_size()
            big_s, big_d = (torch.empty(nbytes, dtype=torch.uint8, device='cuda') for _ in range(2))
            half_s, half_d = big_s[:nbytes // 2], big_d[:nbytes // 2]
            (k, klo, khi), (c, clo, chi), (h, hlo, hhi) = blocks_ms([lambda: m(x), lambda: big_d.copy_(big_s), lambda: half_d.copy_(half_s)],
                                                                  a.blocks, a.iters)
            print(f'| {H} x {W} | {out} | {k:.3f} [{klo:.3f}, {khi:.3f}] | {nbytes / 1e6:.1f} | {nbytes / k / 1e6:.0f} | '
                  f'{c:.3f} [{clo:.3f}, {chi:.3f}] | {k / c:.2f} | {h:.3f} [{hlo:.3f}, {hhi:.3f}] | {k / h:.2f} |', flush=True)
            del big_s, big_d, y
    if not a.no_host:
        frames = rng.integers(0, 256, size=(n, 360, 480, 3), dtype=np.uint8)
        torch.set_num_threads(1)   # one core per frame: the pool below is the parallelism
        host_ms(frames[:8], size, 1)
        t1 = host_ms(frames, size, 1)
        t16 = host_ms(frames, size, 16)
        print(f'\nhost: PIL resize 360 x 480 -> 224 + ToTensor, {n} frames: {t1:.0f} ms on one thread ({t1 / n:.2f} ms per frame), '
              f'{t16:.0f} ms on a 16-thread pool')


if __name__ == '__main__':
    main()
