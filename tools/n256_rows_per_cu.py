"""Is the deep-K N = 256 GEMM bound per CU or chip-wide?  Times svol_gemm_nt alone at N = 256, K = 2048, fp32 output with bias and
residual (fc2's call) at M = 128 C, 128 C + 1024, 196 C and 256 C rows (C = the device's CU count): HIP events, warm-up, 20 launches.

With 128-row tiles, a time that steps with the largest number of tiles on one CU (128 C + 1024 costs what 256 C costs) says per CU;
a time in proportion to M says chip-wide.  profiles/n256_balanced.md holds the numbers.

    python tools/n256_rows_per_cu.py [--dtype bf16|fp16] [--k 2048]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svol_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    ap.add_argument('--k', type=int, default=2048)
    ap.add_argument('--launches', type=int, default=20)
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float16
    C = torch.cuda.get_device_properties(0).multi_processor_count
    K, N = a.k, 256
    out = {'cus': C, 'K': K, 'dtype': a.dtype, 'us': {}}
    W = (torch.randn((N, K), device='cuda') / K ** 0.5).to(dt)
    bias = torch.randn((N,), device='cuda')
    for name, M in (('128C', 128 * C), ('128C+1024', 128 * C + 1024), ('196C', 196 * C), ('256C', 256 * C)):
        A = torch.randn((M, K), device='cuda').to(dt)
        R = torch.randn((M, N), device='cuda')
        Cout = torch.empty((M, N), device='cuda')
        for _ in range(5):
            ops.gemm_nt(A, W, bias, residual=R, out_f32=True, out=Cout)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.launches + 1)]
        ev[0].record()
        for i in range(a.launches):
            ops.gemm_nt(A, W, bias, residual=R, out_f32=True, out=Cout)
            ev[i + 1].record()
        torch.cuda.synchronize()
        t = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(a.launches))
        out['us'][name] = {'M': M, 'median': round(t[len(t) // 2], 1), 'min': round(t[0], 1), 'max': round(t[-1], 1)}
        print(f'M = {name:10s} ({M:6d} rows): median {t[len(t) // 2]:7.1f} us   min {t[0]:7.1f}   max {t[-1]:7.1f}', flush=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
