// Sketch-ViT classification fine-tuning (preprocess/sketch_vit_finetune.py): the objective reads ONE row per image, the [CLS] state of
// the last block, so that block's attention is one query per (image, head) against all L <= 256 keys, and its loss is a softmax
// cross-entropy over <= 1024 classes.
//
//   svol_attn_cls_fwd   o = softmax(q k^T * scale) v for one query row per image: q [n, H dh], k / v [n L, >= H dh] views, bf16
//                       (or, through svol_attn_cls_*_h16, fp16) operands, every product and sum in fp32 (a VALU kernel: one query has no MFMA shape; P is never rounded).
//                       One wave per (image, head), four per workgroup.  Phase 1, lane = key (<= 4 keys per lane, 16-byte loads of
//                       the K row against q broadcast from LDS): t_j = s_j c, maximum and sum by wave reduction.  Phase 2, lane =
//                       channel: P from LDS, V rows read coalesced; at dh = 32 the two half-waves take alternate keys.
//   svol_attn_cls_bwd   P_j = exp2(t_j - lse2), dS_j = P_j (dout . v_j - delta); dk_j = scale dS_j q and dv_j = P_j dout by the key's
//                       lane (16-byte stores), dq = scale sum_j dS_j k_j by the channel's lane.  delta = dout . o is formed as
//                       sum_j P_j (dout . v_j) from the very products dS uses (a wave reduction), NOT from the stored bf16 o: where P is
//                       nearly one-hot dS is a small difference and the rounding of o would be most of it (the bf16 emulation of a
//                       two-key head missed the element bar 14-fold with it).  At L = 1 the sum is 1 * (dout . v_0) + zeros, so dS is
//                       exactly 0; t_j is the same rounded product as in the forward, so P is exactly 1 there.  No atomics: one wave
//                       owns all outputs of its (image, head).
//   svol_softmax_xent   mean cross-entropy of fp32 logits, dlogits = (softmax - onehot) / n and the top-1 hit count, ONE workgroup:
//                       a wave per row in turn, the row losses summed wave by wave and then over the waves in index order.
//
// Built with -ffp-contract=off (svol_amd/build.py): t_j = s_j c is one rounded product, the same in both attention kernels; every fma
// here is written out (__builtin_fmaf).
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int CLS_WAVES = 4;     // (image, head) pairs of a workgroup
constexpr int CLS_LMAX = 256;
constexpr int CLS_KPL = CLS_LMAX / 64;   // keys per lane

// T = bf16_t or f16_t, the operand type.  Every operand is widened to fp32 as it is read and P, dS, delta stay fp32; T is met again only
// at the stores of o, dq, dk and dv.  No constant here is rounded to T (the -inf of an empty key slot lives in an fp32 register).
template <typename T>
struct ClsArgs {
    const T *q, *k, *v, *dout;
    T *out, *dq, *dk, *dv;
    float* lse2;         // [n, H]: written by the forward, read by the backward
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int64_t pairs;       // n * H
    int H, L;
    float scale, scale_log2e;
};

// sum_c vec[c] * row[c] over DH channels, one fma chain in channel order: the ONE dot product of both kernels
template <typename T, int DH>
__device__ __forceinline__ float row_dot(const float* vec, const T* row) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < DH / 8; ++c) {
        const auto b = __builtin_bit_cast(typename H16<T>::v8, *reinterpret_cast<const uint4*>(row + c * 8));
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __builtin_fmaf((float)b[e], vec[c * 8 + e], acc);
    }
    return acc;
}

// sum_j w[j] * rows[j][channel of this lane] over j < L (lane = channel; dh = 32: the half-waves take alternate rows)
template <typename T, int DH>
__device__ __forceinline__ float weighted_rows(const float* w, const T* rows, int64_t ld, int L, int lane) {
    float acc = 0.f;
    if constexpr (DH == 64) {
#pragma unroll 4
        for (int j = 0; j < L; ++j) acc = __builtin_fmaf(w[j], (float)rows[(int64_t)j * ld + lane], acc);
    } else {
        const int ch = lane & 31;
#pragma unroll 4
        for (int j = lane >> 5; j < L; j += 2) acc = __builtin_fmaf(w[j], (float)rows[(int64_t)j * ld + ch], acc);
        acc += __shfl_xor(acc, 32, 64);
    }
    return acc;
}

template <typename T, int DH>
__global__ __launch_bounds__(64 * CLS_WAVES) void attn_cls_fwd_kernel(ClsArgs<T> p) {
    __shared__ float sQ[CLS_WAVES][64];
    __shared__ float sP[CLS_WAVES][CLS_LMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * CLS_WAVES + wave;
    const bool valid = pair < p.pairs;      // the tail of the last workgroup: its waves only keep the barriers company
    const int64_t img = valid ? pair / p.H : 0;
    const int hh = valid ? (int)(pair % p.H) : 0;
    const T* K = p.k + img * p.L * p.ldk + hh * DH;
    const T* V = p.v + img * p.L * p.ldv + hh * DH;
    if (valid && lane < DH) sQ[wave][lane] = to_f32(p.q[img * p.ldq + hh * DH + lane]);
    __syncthreads();
    float l = 0.f, tm = 0.f;
    if (valid) {
        float t[CLS_KPL];
        tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < CLS_KPL; ++i) {
            const int j = lane + 64 * i;
            t[i] = -INFINITY;
            if (j < p.L) t[i] = row_dot<T, DH>(sQ[wave], K + (int64_t)j * p.ldk) * p.scale_log2e;
            tm = fmaxf(tm, t[i]);
        }
        tm = wave_max(tm);
#pragma unroll
        for (int i = 0; i < CLS_KPL; ++i) {
            const int j = lane + 64 * i;
            const float e = j < p.L ? __builtin_amdgcn_exp2f(t[i] - tm) : 0.f;
            if (j < p.L) sP[wave][j] = e;
            l += e;
        }
        l = wave_sum(l);
    }
    __syncthreads();
    if (valid) {
        const float acc = weighted_rows<T, DH>(sP[wave], V, p.ldv, p.L, lane);
        if (lane < DH) p.out[img * p.ldo + hh * DH + lane] = from_f32<T>(acc / l);
        if (lane == 0) p.lse2[pair] = tm + log2f(l);
    }
}

template <typename T, int DH>
__global__ __launch_bounds__(64 * CLS_WAVES) void attn_cls_bwd_kernel(ClsArgs<T> p) {
    __shared__ float sQ[CLS_WAVES][64];
    __shared__ float sD[CLS_WAVES][64];
    __shared__ float sS[CLS_WAVES][CLS_LMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * CLS_WAVES + wave;
    const bool valid = pair < p.pairs;
    const int64_t img = valid ? pair / p.H : 0;
    const int hh = valid ? (int)(pair % p.H) : 0;
    const int64_t row0 = img * p.L;
    const T* K = p.k + row0 * p.ldk + hh * DH;
    const T* V = p.v + row0 * p.ldv + hh * DH;
    if (valid && lane < DH) {
        sQ[wave][lane] = to_f32(p.q[img * p.ldq + hh * DH + lane]);
        sD[wave][lane] = to_f32(p.dout[img * p.lddo + hh * DH + lane]);
    }
    __syncthreads();
    if (valid) {
        const float lse = p.lse2[pair];
        float pj[CLS_KPL], dp[CLS_KPL];
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < CLS_KPL; ++i) {
            const int j = lane + 64 * i;
            pj[i] = dp[i] = 0.f;
            if (j < p.L) {
                const float t = row_dot<T, DH>(sQ[wave], K + (int64_t)j * p.ldk) * p.scale_log2e;
                pj[i] = __builtin_amdgcn_exp2f(t - lse);
                dp[i] = row_dot<T, DH>(sD[wave], V + (int64_t)j * p.ldv);
            }
            part = __builtin_fmaf(pj[i], dp[i], part);
        }
        const float delta = wave_sum(part);     // = dout . o for the unrounded o; L = 1: 1 * dp_0 + zeros = dp_0 exactly
#pragma unroll
        for (int i = 0; i < CLS_KPL; ++i) {
            const int j = lane + 64 * i;
            if (j < p.L) {
                const float ds = pj[i] * (dp[i] - delta);
                sS[wave][j] = ds;
                const float dsc = ds * p.scale;
                T* dk = p.dk + (row0 + j) * p.lddk + hh * DH;
                T* dv = p.dv + (row0 + j) * p.lddv + hh * DH;
#pragma unroll
                for (int c = 0; c < DH / 8; ++c) {
                    f32x4 a[2], b[2];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        a[e >> 2][e & 3] = dsc * sQ[wave][c * 8 + e];
                        b[e >> 2][e & 3] = pj[i] * sD[wave][c * 8 + e];
                    }
                    *reinterpret_cast<typename H16<T>::v8*>(dk + c * 8) =
                        __builtin_shufflevector(H16<T>::cvt4(a[0]), H16<T>::cvt4(a[1]), 0, 1, 2, 3, 4, 5, 6, 7);
                    *reinterpret_cast<typename H16<T>::v8*>(dv + c * 8) =
                        __builtin_shufflevector(H16<T>::cvt4(b[0]), H16<T>::cvt4(b[1]), 0, 1, 2, 3, 4, 5, 6, 7);
                }
            }
        }
    }
    __syncthreads();
    if (valid) {
        const float acc = weighted_rows<T, DH>(sS[wave], K, p.ldk, p.L, lane);
        if (lane < DH) p.dq[img * p.lddq + hh * DH + lane] = from_f32<T>(acc * p.scale);
    }
}

// ---- softmax cross-entropy ------------------------------------------------------------------------------------------------------
constexpr int XE_WAVES = 16;
constexpr int XE_CMAX = 1024;
constexpr int XE_PER_LANE = XE_CMAX / 64;

__global__ __launch_bounds__(64 * XE_WAVES) void softmax_xent_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ targets,
                                                                     float* __restrict__ loss, float* __restrict__ dlogits, int64_t lddl,
                                                                     int* __restrict__ correct, int64_t n, int C) {
    __shared__ float sLoss[XE_WAVES];
    __shared__ int sHit[XE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_n = 1.f / (float)n;
    float part = 0.f;
    int hits = 0;
    for (int64_t r = wave; r < n; r += XE_WAVES) {
        const float* x = logits + r * ld;
        float xv[XE_PER_LANE];
        float m = -INFINITY;
        int am = 0;
#pragma unroll
        for (int i = 0; i < XE_PER_LANE; ++i) {
            const int c = lane + 64 * i;
            xv[i] = c < C ? x[c] : -INFINITY;
            if (xv[i] > m) { m = xv[i]; am = c; }     // (the lane's columns ascend: its first maximum)
        }
        const float mm = wave_max(m);
        // the lowest column that holds the maximum
        int cand = (m == mm) ? am : 0x7fffffff;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) cand = min(cand, __shfl_xor(cand, s, 64));
        float l = 0.f;
#pragma unroll
        for (int i = 0; i < XE_PER_LANE; ++i) {
            xv[i] = lane + 64 * i < C ? expf(xv[i] - mm) : 0.f;
            l += xv[i];
        }
        l = wave_sum(l);
        const int64_t tg = targets[r];
        const bool ok = tg >= 0 && tg < C;      // checked BEFORE it is an index: nothing is read at a bad one
        const float xt = ok ? x[tg] : 0.f;
        const float rl = ok ? (mm - xt) + logf(l) : __builtin_nanf("");
#pragma unroll
        for (int i = 0; i < XE_PER_LANE; ++i) {
            const int c = lane + 64 * i;
            if (c < C) dlogits[r * lddl + c] = ok ? (xv[i] / l - (c == tg ? 1.f : 0.f)) * inv_n : __builtin_nanf("");
        }
        part += rl;
        hits += (ok && cand == (int)tg) ? 1 : 0;
    }
    if (lane == 0) {
        sLoss[wave] = part;
        sHit[wave] = hits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.f;
        int h = 0;
        for (int w = 0; w < XE_WAVES; ++w) {
            tot += sLoss[w];
            h += sHit[w];
        }
        *loss = tot * inv_n;
        *correct = h;
    }
}

// h16: the *_h16 entry points, which take SVOL_F16 besides SVOL_BF16 (the entries without the suffix keep refusing it)
int cls_check(const void* const* ptrs16, int n16, const int64_t* lds, int nld, const float* lse2, int64_t n, int64_t H, int64_t L, int64_t dh,
              int dtype, bool h16) {
    for (int i = 0; i < n16; ++i)
        if (!ptrs16[i]) return SVOL_E_INVALID;
    if (!lse2 || n <= 0 || H <= 0 || L <= 0) return SVOL_E_INVALID;
    if (!(dtype == SVOL_BF16 || (h16 && dtype == SVOL_F16)) || (dh != 32 && dh != 64) || L > CLS_LMAX || n > (1ll << 24) || H > 4096) return SVOL_E_UNSUPPORTED;
    for (int i = 0; i < nld; ++i)
        if (lds[i] % 8 || lds[i] < H * dh) return SVOL_E_UNSUPPORTED;
    for (int i = 0; i < n16; ++i)
        if (!aligned16(ptrs16[i])) return SVOL_E_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(lse2) & 3) return SVOL_E_UNSUPPORTED;
    return SVOL_OK;
}

template <typename T>
int cls_fwd_go(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse2, int64_t n,
               int64_t H, int64_t L, int64_t dh, float scale, void* stream) {
    ClsArgs<T> p{};
    p.q = (const T*)q, p.k = (const T*)k, p.v = (const T*)v, p.out = (T*)o, p.lse2 = lse2;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    p.pairs = n * H, p.H = (int)H, p.L = (int)L, p.scale = scale, p.scale_log2e = scale * LOG2E;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((p.pairs + CLS_WAVES - 1) / CLS_WAVES));
    if (dh == 64) hipLaunchKernelGGL((attn_cls_fwd_kernel<T, 64>), grid, dim3(64 * CLS_WAVES), 0, s, p);
    else hipLaunchKernelGGL((attn_cls_fwd_kernel<T, 32>), grid, dim3(64 * CLS_WAVES), 0, s, p);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int cls_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse2, int64_t n,
            int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream, bool h16) {
    const void* ptrs[] = {q, k, v, o};
    const int64_t lds[] = {ldq, ldk, ldv, ldo};
    const int rc = cls_check(ptrs, 4, lds, 4, lse2, n, H, L, dh, dtype, h16);
    if (rc != SVOL_OK) return rc;
    if (dtype == SVOL_F16) return cls_fwd_go<f16_t>(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n, H, L, dh, scale, stream);
    return cls_fwd_go<bf16_t>(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n, H, L, dh, scale, stream);
}

template <typename T>
int cls_bwd_go(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t ldo, const void* dout, int64_t lddo,
               const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t n, int64_t H, int64_t L,
               int64_t dh, float scale, void* stream) {
    ClsArgs<T> p{};
    p.q = (const T*)q, p.k = (const T*)k, p.v = (const T*)v, p.dout = (const T*)dout;
    p.dq = (T*)dq, p.dk = (T*)dk, p.dv = (T*)dv, p.lse2 = const_cast<float*>(lse2);
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddo = lddo, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
    p.pairs = n * H, p.H = (int)H, p.L = (int)L, p.scale = scale, p.scale_log2e = scale * LOG2E;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((p.pairs + CLS_WAVES - 1) / CLS_WAVES));
    if (dh == 64) hipLaunchKernelGGL((attn_cls_bwd_kernel<T, 64>), grid, dim3(64 * CLS_WAVES), 0, s, p);
    else hipLaunchKernelGGL((attn_cls_bwd_kernel<T, 32>), grid, dim3(64 * CLS_WAVES), 0, s, p);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int cls_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo, const void* dout,
            int64_t lddo, const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t n, int64_t H,
            int64_t L, int64_t dh, float scale, int dtype, void* stream, bool h16) {
    const void* ptrs[] = {q, k, v, o, dout, dq, dk, dv};
    const int64_t lds[] = {ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv};
    const int rc = cls_check(ptrs, 8, lds, 8, lse2, n, H, L, dh, dtype, h16);
    if (rc != SVOL_OK) return rc;
    if (dtype == SVOL_F16)
        return cls_bwd_go<f16_t>(q, ldq, k, ldk, v, ldv, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n, H, L, dh, scale, stream);
    return cls_bwd_go<bf16_t>(q, ldq, k, ldk, v, ldv, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n, H, L, dh, scale, stream);
}

}  // namespace

extern "C" {

int svol_attn_cls_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse2,
                      int64_t n, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return cls_fwd(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n, H, L, dh, scale, dtype, stream, false);
}

int svol_attn_cls_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                      const void* dout, int64_t lddo, const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                      int64_t lddv, int64_t n, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return cls_bwd(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n, H, L, dh, scale, dtype, stream, false);
}

int svol_attn_cls_fwd_h16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse2,
                          int64_t n, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return cls_fwd(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n, H, L, dh, scale, dtype, stream, true);
}

int svol_attn_cls_bwd_h16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                          const void* dout, int64_t lddo, const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                          int64_t lddv, int64_t n, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return cls_bwd(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n, H, L, dh, scale, dtype, stream, true);
}

int svol_softmax_xent(const float* logits, int64_t ld, const int64_t* targets, float* loss, float* dlogits, int64_t lddl, int32_t* correct,
                      int64_t n, int64_t C, void* stream) {
    if (!logits || !targets || !loss || !dlogits || !correct || n <= 0 || C <= 0 || ld < C || lddl < C) return SVOL_E_INVALID;
    if (C > XE_CMAX || n > (1ll << 30)) return SVOL_E_UNSUPPORTED;
    if (((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(dlogits) |
          reinterpret_cast<uintptr_t>(correct)) & 3) || (reinterpret_cast<uintptr_t>(targets) & 7))
        return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(softmax_xent_kernel, dim3(1), dim3(64 * XE_WAVES), 0, s, logits, ld, targets, loss, dlogits, lddl, correct, n, (int)C);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // extern "C"
