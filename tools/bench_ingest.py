#!/usr/bin/env python3
"""Frame ingest (svol_ingest_resize) against a device-to-device copy, and the host-side Pillow time it replaces.

    python tools/bench_ingest.py [--frames 256] [--blocks 9] [--iters 10] [--no-host]
    python tools/bench_ingest.py --filter bicubic --grey --invert --source 28 28      # one row of svol_ingest_resample
    python tools/bench_ingest.py --filter-rows                                        # the rows of profiles/ingest_filters.md

Per case (256 frames 360 x 480 -> 224 and 224 -> 224, fp32 NCHW and bf16 NHWC): the kernel and two copies are timed in ALTERNATING
blocks of `iters` launches between device events in one run; the figure is the median block.  The yardsticks: a copy OF
(bytes read + bytes written) bytes — the bar of profiles/ingest.md is kernel <= 2 x this one — and, for reference, a copy that MOVES
that many bytes (half the size: the same memory traffic as the kernel).  Bytes are the algorithm's: every source byte read once,
every output element written once.  The host figure is PIL resize + ToTensor's arithmetic for the same frames on this machine's
CPUs (one thread, and a 16-thread pool: Pillow releases the GIL while it resamples).

--filter / --grey / --invert / --source H W time svol_ingest_resample on one case instead (fp32 NCHW and bf16 NHWC), with the same
yardsticks.  Where the case has a partner on the existing entry it is timed in the same alternating blocks: a grey bilinear source
beside svol_ingest_resize on the same images replicated to three channels (the gate of profiles/ingest_filters.md: grey must not be
slower), an RGB bilinear source (--new-entry forces it through svol_ingest_resample) beside svol_ingest_resize on the same images."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from svol_amd import ops
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


def resample_call(m, x, out):
    """m's forward on x [n,H,W,3] / [n,H,W] forced through svol_ingest_resample (FrameIngest sends RGB + bilinear to the old entry)"""
    (ytab, ky), (xtab, kx) = m._table(x.device, x.shape[1], m.size[0]), m._table(x.device, x.shape[2], m.size[1])
    lut = m._lut_on(x.device)
    nchw = m.out == 'nchw_f32'
    st = tuple(out.stride()) if nchw else (out.stride(0), out.stride(3), out.stride(1), out.stride(2))
    return lambda: ops.ingest_resample(x, xtab, kx, ytab, ky, lut, None, out, st, m.size[0], m.size[1], invert=m.invert)


def filter_row(n, H, W, size, flt, grey, invert, new_entry, blocks, iters, rng):
    """one case through svol_ingest_resample in both layouts; returns the (new, partner) medians of the rows that have a partner"""
    x = torch.from_numpy(rng.integers(0, 256, size=(n, H, W) if grey else (n, H, W, 3), dtype=np.uint8)).cuda()
    pairs = []
    for out in ('nchw_f32', 'nhwc_bf16'):
        m = FrameIngest(size, 'totensor', out=out, filter=flt, invert=invert)
        y = m(x)
        fn = resample_call(m, x, y) if new_entry else (lambda: m(x))
        nbytes = x.numel() + y.numel() * y.element_size()
        big_s, big_d = (torch.empty(nbytes, dtype=torch.uint8, device='cuda') for _ in range(2))
        fns = [fn, lambda: big_d.copy_(big_s)]
        partner = ''
        if flt == 'bilinear' and not invert:      # the existing entry on the same images (replicated to three channels if grey)
            x3 = x[..., None].expand(n, H, W, 3).contiguous() if grey else x
            old = FrameIngest(size, 'totensor', out=out)
            assert torch.equal(old(x3), fn())
            fns.append(lambda: old(x3))
        res = blocks_ms(fns, blocks, iters)
        (k, klo, khi), (c, clo, chi) = res[:2]
        if len(res) == 3:
            o, olo, ohi = res[2]
            partner = f'{o:.3f} [{olo:.3f}, {ohi:.3f}] | {k / o:.2f}'
            pairs.append((k, o))
        else:
            partner = '- | -'
        what = f"{'grey' if grey else 'RGB'} {H} x {W}, {flt}{', inverted' if invert else ''}{', new entry' if new_entry and not grey else ''}"
        print(f'| {what} | {out} | {k:.3f} [{klo:.3f}, {khi:.3f}] | {nbytes / 1e6:.1f} | {nbytes / k / 1e6:.0f} | '
              f'{c:.3f} [{clo:.3f}, {chi:.3f}] | {k / c:.2f} | {partner} |', flush=True)
        del big_s, big_d, y
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--filter', default=None, choices=['box', 'bilinear', 'hamming', 'bicubic', 'lanczos'], help='time svol_ingest_resample with this filter')
    ap.add_argument('--grey', action='store_true', help='single-channel sources [n,H,W]')
    ap.add_argument('--invert', action='store_true', help='255 - byte at the source read')
    ap.add_argument('--new-entry', action='store_true', help='send RGB + bilinear through svol_ingest_resample too')
    ap.add_argument('--source', type=int, nargs=2, default=None, metavar=('H', 'W'), help='source size of the --filter / --grey / --invert case')
    ap.add_argument('--filter-rows', action='store_true', help='the rows of profiles/ingest_filters.md, and its gate')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ingest.py measures on the MI355X; there is no CPU figure for a kernel'
    n, size = a.frames, (224, 224)
    rng = np.random.default_rng(0)
    if a.filter_rows or a.filter or a.grey or a.invert or a.new_entry:
        print(f'# svol_ingest_resample, {n} images -> {size[0]} x {size[1]}; median [min, max] of {a.blocks} alternating blocks of {a.iters} launches')
        print('| source | output | kernel ms | read+written MB | kernel GB/s | copy of (r+w) bytes ms | kernel / copy | svol_ingest_resize on the same images (x 3 if grey) ms | new / old |')
        print('|---|---|---|---|---|---|---|---|---|')
        if a.filter_rows:
            gate = filter_row(n, 1111, 1111, size, 'bilinear', True, False, True, a.blocks, a.iters, rng)
            filter_row(n, 28, 28, size, 'bicubic', True, True, True, a.blocks, a.iters, rng)
            filter_row(n, 360, 480, size, 'bicubic', False, False, True, a.blocks, a.iters, rng)
            filter_row(n, 360, 480, size, 'lanczos', False, False, True, a.blocks, a.iters, rng)
            filter_row(n, 360, 480, size, 'bilinear', False, False, True, a.blocks, a.iters, rng)
            ok = all(k <= o for k, o in gate)
            print(f"\ngate (grey 1111 x 1111 bilinear median <= svol_ingest_resize on the replicated images, same run): {'met' if ok else 'MISSED'} "
                  + ', '.join(f'{k:.3f} vs {o:.3f} ms' for k, o in gate))
            sys.exit(0 if ok else 1)
        H, W = a.source or (360, 480)
        filter_row(n, H, W, size, a.filter or 'bilinear', a.grey, a.invert, a.new_entry or a.grey or a.invert or (a.filter or 'bilinear') != 'bilinear',
                   a.blocks, a.iters, rng)
        return
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
