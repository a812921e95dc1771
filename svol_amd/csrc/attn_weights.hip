// Head-averaged attention weights of the decoder's query -> memory cross-attention: the second value
// nn.MultiheadAttention returns with need_weights=True, which the reference's TransformerDecoder stacks per layer
// (transformer.py:139-152, 258-262 `att`).  The fused attention kernels never materialise probabilities, so the few
// (N = 100 queries) rows that someone asks for are recomputed here from q, k and the saved log-sum-exp:
//
//     att[b, n, l] = 1/H * sum_h exp2(q[b,n,h,:].k[b,l,h,:] * c + kbias[b,l]*log2e - lse2[b,h,n])
//
// Lane = key (coalesced att rows), a workgroup takes 256 keys x QT queries of one batch element; the query tile and its
// lse sit in LDS (broadcast reads), each lane loads one head of its key row at a time and reuses it for all QT queries.
// VALU work (B*Lq*Lk*d FMAs = 1.3 G at the benchmark size), no gradient (the reference's consumers discard `att`).
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int QT = 20;

template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_weights_mean_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k,
                                                                 int64_t ldk, const float* __restrict__ lse2,
                                                                 const float* __restrict__ kbias, float* __restrict__ att, int H,
                                                                 int Lq, int Lk, float c) {
    extern __shared__ float smem[];
    const int d = H * DH;
    float* qs = smem;            // [QT][d]
    float* ls = smem + QT * d;   // [QT][H]
    const int tid = threadIdx.x;
    const int b = blockIdx.z, n0 = blockIdx.y * QT;
    const int nq = min(QT, Lq - n0);
    for (int i = tid; i < QT * d; i += 256) {
        const int n = i / d, e = i - n * d;
        qs[i] = n < nq ? to_f32(q[((int64_t)b * Lq + n0 + n) * ldq + e]) * c : 0.f;
    }
    for (int i = tid; i < QT * H; i += 256) {
        const int n = i / H, h = i - n * H;
        ls[i] = n < nq ? lse2[((int64_t)b * H + h) * Lq + n0 + n] : INFINITY;
    }
    __syncthreads();
    const int l = blockIdx.x * 256 + tid;
    if (l >= Lk) return;
    const float kb = kbias ? kbias[(int64_t)b * Lk + l] * LOG2E : 0.f;
    const T* krow = k + ((int64_t)b * Lk + l) * ldk;
    float acc[QT];
#pragma unroll
    for (int n = 0; n < QT; ++n) acc[n] = 0.f;
    for (int h = 0; h < H; ++h) {
        float kr[DH];
#pragma unroll
        for (int e = 0; e < DH; ++e) kr[e] = to_f32(krow[h * DH + e]);
#pragma unroll
        for (int n = 0; n < QT; ++n) {
            const float* qv = qs + n * d + h * DH;
            float s = kb - ls[n * H + h];
#pragma unroll
            for (int e = 0; e < DH; ++e) s = fmaf(kr[e], qv[e], s);
            acc[n] += __builtin_amdgcn_exp2f(s);
        }
    }
    const float inv = 1.f / (float)H;
    for (int n = 0; n < nq; ++n) att[((int64_t)b * Lq + n0 + n) * Lk + l] = acc[n] * inv;
}

template <typename T>
int launch(const void* q, int64_t ldq, const void* k, int64_t ldk, const float* lse2, const float* kbias, float* att, int64_t B,
           int64_t H, int64_t Lq, int64_t Lk, int64_t dh, float c, hipStream_t s) {
    const dim3 grid((unsigned)((Lk + 255) / 256), (unsigned)((Lq + QT - 1) / QT), (unsigned)B);
    const size_t sh = (size_t)QT * (H * dh + H) * sizeof(float);
    if (sh > 64 * 1024) return SVOL_E_UNSUPPORTED;
#define SVOL_AW(DH_)                                                                                                            \
    hipLaunchKernelGGL((attn_weights_mean_kernel<T, DH_>), grid, dim3(256), sh, s, (const T*)q, ldq, (const T*)k, ldk, lse2, kbias, \
                       att, (int)H, (int)Lq, (int)Lk, c)
    if (dh == 8) SVOL_AW(8);
    else if (dh == 16) SVOL_AW(16);
    else if (dh == 32) SVOL_AW(32);
    else if (dh == 40) SVOL_AW(40);   // the widths svol_attn_fwd serves above 32 (attention.hip, two d-tiles)
    else if (dh == 48) SVOL_AW(48);
    else if (dh == 56) SVOL_AW(56);
    else if (dh == 64) SVOL_AW(64);
    else return SVOL_E_UNSUPPORTED;
#undef SVOL_AW
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // namespace

extern "C" int svol_attn_weights_mean(const void* q, int64_t ldq, const void* k, int64_t ldk, const float* lse2, const float* kbias,
                                      float* att, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, float scale,
                                      float q_premul, int dtype, void* stream) {
    if (!q || !k || !lse2 || !att || B < 0 || H <= 0 || Lq < 0 || Lk < 0 || dh <= 0) return SVOL_E_INVALID;
    if (B == 0 || Lq == 0 || Lk == 0) return SVOL_OK;
    if (B > 65535 || (Lq + QT - 1) / QT > 65535) return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // q already carries d_h^-1/2 * log2(e) when q_premul != 0 (bf16 projection epilogue), as in svol_attn_fwd
    const float c = q_premul != 0.f ? 1.f : scale * LOG2E;
    if (dtype == SVOL_BF16) return launch<bf16_t>(q, ldq, k, ldk, lse2, kbias, att, B, H, Lq, Lk, dh, c, s);
    if (dtype == SVOL_F16) return launch<f16_t>(q, ldq, k, ldk, lse2, kbias, att, B, H, Lq, Lk, dh, c, s);
    if (dtype == SVOL_F32) return launch<float>(q, ldq, k, ldk, lse2, kbias, att, B, H, Lq, Lk, dh, c, s);
    return SVOL_E_INVALID;
}
