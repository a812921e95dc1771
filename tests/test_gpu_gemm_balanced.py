"""The balanced deep-K N = 256 GEMM (gemm_n256_bf16.hip: one workgroup per CU, equal rows each), taken when M > 128 * CUs.

Every case is checked twice:
  * same bits as the 128-row-tile kernel: the result equals the concatenation of the same call on row chunks of 16384 rows (those route
    to the 128-row kernel; a row's result does not depend on the chunk it is computed in, so the last chunk is the LAST 16384 rows);
  * against fp64 on the device over a fixed row sample that holds the first and the last 300 rows, with the bars of
    tests/gpu_checks.py::check_gemm_nt: TOL[dt], and 1e-5 for the fp32-output variants.
"""
import math

import pytest
import torch

from tests.gpu_checks import TOL

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CHUNK = 16384
KS = (512, 544, 2048)
M_KINDS = ('128C+1', '144C', '196C', '256C+77')   # one valid row in the last tile / an exact multiple / bench rows per workgroup / two workgroups per CU


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _m(kind):
    C = _cus()
    return {'128C+1': 128 * C + 1, '144C': 144 * C, '196C': 196 * C, '256C+77': 256 * C + 77}[kind]


_cache = {}


def _operands(dt, K):
    """A (the largest M, sliced by rows per case; 2K wide: the column-slice variant reads its right half), W, bias, residual: made once"""
    key = (dt, K)
    if key not in _cache:
        _cache.clear()   # (one K and dtype at a time: the widest A is 0.5 GiB)
        g = torch.Generator(device=DEV).manual_seed(1000 + K)
        Mx = _m('256C+77')
        wide = torch.randn((Mx, 2 * K), generator=g, device=DEV, dtype=torch.float32).to(dt)
        W = (torch.randn((256, K), generator=g, device=DEV, dtype=torch.float32) / math.sqrt(K)).to(dt)
        bias = torch.randn((256,), generator=g, device=DEV, dtype=torch.float32)
        res = torch.randn((Mx, 256), generator=g, device=DEV, dtype=torch.float32)
        _cache[key] = (wide, W, bias, res)
    return _cache[key]


def _rows(M):
    mid = torch.arange(300, M - 300, max(1, (M - 600) // 424), device=DEV)[:424]
    return torch.cat([torch.arange(0, 300, device=DEV), mid, torch.arange(M - 300, M, device=DEV)])


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _chunked(call, M):
    """`call(r0, r1)` on chunks of CHUNK rows, concatenated; the last chunk is the last CHUNK rows, of which the new ones are kept"""
    parts = []
    r = 0
    while r < M:
        if r + CHUNK <= M:
            parts.append(call(r, r + CHUNK))
        else:
            parts.append(call(M - CHUNK, M)[CHUNK - (M - r):])
        r += CHUNK
    return torch.cat(parts)


def _rel(got, ref):
    assert torch.isfinite(got).all()
    return float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-12))


@pytest.mark.parametrize('kind', M_KINDS)
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_balanced_gemm(dt, K, kind):
    from svol_amd import ops
    C = _cus()
    assert 128 * C >= CHUNK, 'the row chunks must route to the 128-row-tile kernel'
    M = _m(kind)
    wide, W, bias, res = _operands(dt, K)
    A = wide[:M, :K].contiguous()
    Asl = wide[:M, K:]          # a column slice: lda = 2K
    R = res[:M]
    rows = _rows(M)
    W64 = W.double()
    pre = {False: A[rows].double() @ W64.t() + bias.double(), True: Asl[rows].double() @ W64.t() + bias.double()}

    # fp32 output with bias and fp32 residual (fc2); A dense and as a column slice
    for sl, a in ((False, A), (True, Asl)):
        got = ops.gemm_nt(a, W, bias, residual=R, out_f32=True)
        want = _chunked(lambda r0, r1: ops.gemm_nt(a[r0:r1], W, bias, residual=R[r0:r1], out_f32=True), M)
        assert torch.equal(got, want), f'out_f32 slice={sl}: {int((got != want).sum())} elements differ from the 128-row kernel'
        e = _rel(got[rows], pre[sl] + R[rows].double())
        print(f'out_f32 slice={sl} M={M} K={K} {dt}: err {e:.3e} (bar 1e-5)')
        assert e < 1e-5
    # 16-bit output, NONE / RELU / GELU (the dX products; RELU / GELU epilogues)
    for act, f in ((ops.ACT_NONE, lambda x: x), (ops.ACT_RELU, torch.relu), (ops.ACT_GELU, _gelu64)):
        got = ops.gemm_nt(A, W, bias, act)
        want = _chunked(lambda r0, r1: ops.gemm_nt(A[r0:r1], W, bias, act), M)
        assert torch.equal(got, want), f'act {act}: {int((got != want).sum())} elements differ from the 128-row kernel'
        e = _rel(got[rows], f(pre[False]))
        print(f'act{act} M={M} K={K} {dt}: err {e:.3e} (bar {TOL[dt]})')
        assert e < TOL[dt]
    got = ops.gemm_nt(Asl, W)
    want = _chunked(lambda r0, r1: ops.gemm_nt(Asl[r0:r1], W), M)
    assert torch.equal(got, want)
    assert _rel(got[rows], pre[True] - bias.double()) < TOL[dt]


@pytest.mark.parametrize('kind', M_KINDS)
def test_balanced_gemm_split_weights(kind):
    """svol_gemm_nt_split at K = 512 (A is 256 wide and read twice: [hi | lo] weights), bf16 only; output into a column slice"""
    from svol_amd import ops
    dt = torch.bfloat16
    M = _m(kind)
    wide, W, bias, _ = _operands(dt, 512)   # W [256, 512] = [hi | lo]
    A = wide[:M, 256:512]                   # lda = 1024
    rows = _rows(M)
    out = torch.full((M, 320), 3.0, dtype=dt, device=DEV)
    ops.gemm_nt_split(A, W, bias, out=out[:, 64:])
    got = out[:, 64:]
    want = _chunked(lambda r0, r1: ops.gemm_nt_split(A[r0:r1], W, bias), M)
    assert torch.equal(got, want), f'{int((got != want).sum())} elements differ from the 128-row kernel'
    assert float((out[:, :64].float() - 3.0).abs().max()) == 0.0
    ref = A[rows].double() @ (W[:, :256].double() + W[:, 256:].double()).t() + bias.double()
    e = _rel(got[rows], ref)
    print(f'split M={M}: err {e:.3e} (bar {TOL[dt]})')
    assert e < TOL[dt]
