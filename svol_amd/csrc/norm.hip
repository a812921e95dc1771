// LayerNorm (+dropout, +positional add) and sine positional encoding — HBM-bound row kernels.
// The backward row (prefetched operands, reduce, dx, column sums and their fold) lives in ln_row.h: ln_bwd_kernel is its plain user at
// WPR = 1 and WPR = 4.  The forward kernels keep their own text.  One wave (64 lanes) per row, 4 contiguous elements per lane per pass (8 B bf16 / 16 B f32 coalesced loads), fp32
// statistics, wave shuffle reductions (no LDS): WPR = 1.  Rows wider than 1024 columns (up to 4096): one workgroup of four waves per
// row, the row sums exchanged through LDS: lnw_fwd_kernel, and the WPR = 4 instances of ln_bwd_kernel.
#include "ln_row.h"

namespace {

constexpr int LN_MAX_PASSES = 4;  // one wave per row: D <= 4 * 64 * 4 = 1024; wider rows (to LNW_MAX_D) take the WPR = 4 instances
// wide rows: 1024 < D <= 4096 (pre-extracted 2048-d features, ResNet-50 tokens, concat_to_seq on ViT features), NP = passes of 1024
// columns: 2, 3 or 4 — at most 16 columns per lane per array
constexpr int LNW_MAX_D = 4096;

// The two forward kernels keep their own text (they are not built on LnFwdRow of ln_row.h): their multi-pass instances carry roundings
// that no shared body reproduces — which of the first two squares of the variance sum is rounded before the fused chain starts is the
// compiler's pick per instantiation (profiles/ln_row.md) — and svol_layernorm_fwd's outputs stay the parent's to the bit.
// T  = element type of the compute-dtype outputs / gradients, TX = element type of the LN input
// (float when the input is the fp32 residual stream).
template <typename T, typename TX, int NP>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const TX* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ y32,
                                                     T* __restrict__ y, T* __restrict__ ypos, const T* __restrict__ pos,
                                                     int64_t pos_rows, float* __restrict__ mean, float* __restrict__ rstd,
                                                     int64_t M, int D, float p, float inv_keep, uint64_t seed0,
                                                     const int64_t* __restrict__ soff) {
    const uint64_t seed = seed0 + (soff ? ((uint64_t)soff[0] << 8) : 0ull);  // device-side step counter (same stride as the host-side one): graph replays draw fresh masks
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const TX* xr = x + row * D;
    float v[NP][4];
    float s = 0.f;
    // every global load of the wave's one row goes out before the first reduction: one memory latency per wave, not two
    // (x, then pos / gamma / beta behind the statistics: 39 us per [50176, 256] launch; NP = passes of 256 columns)
    const T* pr = pos ? pos + (row % pos_rows) * D : nullptr;
    Vec4<TX> t[NP];
    Vec4<T> pv[NP];
    Vec4<float> gv[NP], bv[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < D) {
            t[j].load(xr + c);
            if (pr) pv[j].load(pr + c);
            gv[j].load(gamma + c);
            bv[j].load(beta + c);
        }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int c = (lane + 64 * j) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[j][e] = c < D ? t[j].get(e) : 0.f;
            s += v[j][e];
        }
    }
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < D) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[j][e] - mu; q += d * d; }
        }
    }
    const float rs = rsqrtf(wave_sum(q) / (float)D + 1e-5f);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < D) {
            Vec4<T> o, op;
            Vec4<float> o32;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float r = (v[j][e] - mu) * rs * gv[j].get(e) + bv[j].get(e);
                if (p > 0.f) r *= dropout_scale(seed, (uint64_t)row, (uint32_t)(c + e), p, inv_keep);
                o.set(e, r);
                o32.set(e, r);
                if (pr) op.set(e, r + pv[j].get(e));
            }
            if (y32) o32.store(y32 + row * D + c);
            if (y) o.store(y + row * D + c);
            if (ypos) op.store(ypos + row * D + c);
        }
    }
}

// wide rows (WPR = 4 in the backward's terms): thread t owns the 4-column vectors (t + 256 j) * 4, j < NV, the two row sums go wave_sum ->
// four LDS words -> one barrier
template <typename T, typename TX, int NV>
__global__ __launch_bounds__(256) void lnw_fwd_kernel(const TX* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ y32,
                                                      T* __restrict__ y, T* __restrict__ ypos, const T* __restrict__ pos,
                                                      int64_t pos_rows, float* __restrict__ mean, float* __restrict__ rstd,
                                                      int64_t M, int D, float p, float inv_keep, uint64_t seed0,
                                                      const int64_t* __restrict__ soff) {
    __shared__ float red[2][4];
    const uint64_t seed = seed0 + (soff ? ((uint64_t)soff[0] << 8) : 0ull);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;   // one row per workgroup (grid = M)
    const TX* xr = x + row * D;
    const T* pr = pos ? pos + (row % pos_rows) * D : nullptr;
    // as in the narrow kernel: every load of the row goes out before the first reduction
    Vec4<TX> t[NV];
    Vec4<T> pv[NV];
    Vec4<float> gv[NV], bv[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = (tid + 256 * j) * 4;
        if (c < D) {
            t[j].load(xr + c);
            if (pr) pv[j].load(pr + c);
            gv[j].load(gamma + c);
            bv[j].load(beta + c);
        }
    }
    float v[NV][4];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = (tid + 256 * j) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[j][e] = c < D ? t[j].get(e) : 0.f;
            s += v[j][e];
        }
    }
    s = wave_sum(s);
    if (lane == 0) red[0][wave] = s;
    __syncthreads();
    const float mu = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = (tid + 256 * j) * 4;
        if (c < D) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[j][e] - mu; q += d * d; }
        }
    }
    q = wave_sum(q);
    if (lane == 0) red[1][wave] = q;
    __syncthreads();
    const float rs = rsqrtf(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)D + 1e-5f);
    if (tid == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = (tid + 256 * j) * 4;
        if (c < D) {
            Vec4<T> o, op;
            Vec4<float> o32;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float r = (v[j][e] - mu) * rs * gv[j].get(e) + bv[j].get(e);
                if (p > 0.f) r *= dropout_scale(seed, (uint64_t)row, (uint32_t)(c + e), p, inv_keep);
                o.set(e, r);
                o32.set(e, r);
                if (pr) op.set(e, r + pv[j].get(e));
            }
            if (y32) o32.store(y32 + row * D + c);
            if (y) o.store(y + row * D + c);
            if (ypos) op.store(ypos + row * D + c);
        }
    }
}

// (NP, WPR) of the launch ladder -> the forward kernel
template <typename T, typename TX, int NP, int WPR>
constexpr auto ln_fwd_pick() {
    if constexpr (WPR == 1) return &ln_fwd_kernel<T, TX, NP>;
    else return &lnw_fwd_kernel<T, TX, NP>;
}

// An owner (wave at WPR = 1, workgroup at WPR = 4) walks `rows_per_owner` consecutive rows, the next row's operands in flight while
// the current one is reduced.  WPR = 4: one barrier per row — the LDS words of the row sums alternate by row parity, so a wave that
// runs ahead writes the other set — and r0, rend are uniform over the workgroup: every thread meets every barrier.
template <typename T, typename TX, int NP, int WPR>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy32, const T* __restrict__ dy,
                                                     const T* __restrict__ dy2, const TX* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, float* __restrict__ dx32,
                                                     T* __restrict__ dx, float* __restrict__ dgamma,
                                                     float* __restrict__ dbeta, float* __restrict__ dxsum, int64_t M, int D,
                                                     float p, float inv_keep, uint64_t seed0, const int64_t* __restrict__ soff, int rows_per_owner,
                                                     float* __restrict__ det_part) {
    using Own = LnOwner<WPR>;
    using Rows = LnBwdRows<T, TX, NP, WPR>;
    const uint64_t seed = seed0 + (soff ? ((uint64_t)soff[0] << 8) : 0ull);
    const int64_t r0 = Own::index() * rows_per_owner;
    const int64_t rend = (r0 + rows_per_owner < M) ? r0 + rows_per_owner : M;
    Rows ln{dy32, dy, dy2, x, mean, rstd, D};
    ln.init(gamma);
    float (*slot)[4] = Own::template slots<4>();
    typename Rows::Row cur, nxt;
    if (r0 < rend) ln.fetch(r0, cur);
    int par = 0;
    for (int64_t row = r0; row < rend; ++row) {
        if (row + 1 < rend) ln.fetch(row + 1, nxt);
        if constexpr (WPR == 4) ln.row(cur, row, dx32, dx, p, inv_keep, seed, slot + 2 * par);
        else ln.row(cur, row, dx32, dx, p, inv_keep, seed, nullptr);
        par ^= 1;
        cur = nxt;
    }
    float* const sinks[3] = {dgamma, dbeta, dxsum};
    ln_fold_columns<WPR>(ln.acc, sinks, det_part ? det_part + (int64_t)blockIdx.x * 3 * D : nullptr, D);
}

// position_encoding.py:51-71 — one workgroup per batch row: inclusive scan of the mask over L,
// then pos[l, 2i] = sin(x / t_i), pos[l, 2i+1] = cos(x / t_i) with x = cumsum/(last+1e-6)*2pi.
// grid = (ceil(L/64), B): every block re-reduces the (tiny) mask prefix it needs, then writes 64 tokens.
template <typename T>
__global__ __launch_bounds__(256) void posenc_kernel(const float* __restrict__ mask, T* __restrict__ pos, int L, int D) {
    __shared__ float red[2][4];
    __shared__ float xe[64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* mr = mask + (int64_t)b * L;
    const int l0 = blockIdx.x * 64;
    float before = 0.f, all = 0.f;
    for (int l = tid; l < L; l += 256) {
        const float v = (mr[l] != 0.f) ? 1.f : 0.f;
        all += v;
        if (l < l0) before += v;
    }
    before = wave_sum(before);
    all = wave_sum(all);
    if (lane == 0) { red[0][wave] = before; red[1][wave] = all; }
    __syncthreads();
    if (tid == 0) {
        float run = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        const float denom = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) + 1e-6f;
        for (int i = 0; i < 64 && l0 + i < L; ++i) {
            run += (mr[l0 + i] != 0.f) ? 1.f : 0.f;
            xe[i] = run / denom * 6.283185307179586f;
        }
    }
    __syncthreads();
    const int ntok = min(64, L - l0);
    // a thread keeps its column(s): the frequency 10000^(2*floor(i/2)/D) is computed once, not per element
    for (int i = tid; i < D; i += 256) {
        const float dim_t = powf(10000.f, (float)(2 * (i / 2)) / (float)D);
        const bool odd = i & 1;
        T* out = pos + ((int64_t)b * L + l0) * D + i;
        if constexpr (sizeof(T) == 4) {   // fp32 (the parity mode): the reference's own arithmetic — a true division, libm sin / cos
            for (int t = 0; t < ntok; ++t) {
                const float a = xe[t] / dim_t;
                out[(int64_t)t * D] = from_f32<T>(odd ? cosf(a) : sinf(a));
            }
        } else {
            // 16-bit outputs (8 / 11 significant bits): the argument lies in [0, 2 pi] (x is normalised to 2 pi, dim_t >= 1), where the
            // hardware sine / cosine (v_sin_f32 / v_cos_f32 on revolutions) are good to ~1e-6 absolute — libm's range reduction and
            // polynomial made this kernel VALU-bound at 51 us for a 26 MB output (round 6: the step's first kernels are a serial chain)
            const float inv = 0.15915494309189535f / dim_t;   // revolutions per unit of x
            for (int t = 0; t < ntok; ++t) {
                const float rev = xe[t] * inv;
                out[(int64_t)t * D] = from_f32<T>(odd ? __builtin_amdgcn_cosf(rev) : __builtin_amdgcn_sinf(rev));
            }
        }
    }
}


// ---- stand-alone dropout (the enc/dec Transformer's residual / FFN dropouts, transformer.py:165-215,225-295) -------------------------
// Stateless keep mask of (row, column) of the [n / row_len, row_len] view (dropout_scale, common.h): forward and backward regenerate
// the same mask from (seed, row, column).  A thread walks along a row chunk: the row's share of the hash is computed once per chunk.
template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n, int64_t row_len, float p,
                                                      float inv_keep, uint64_t seed, const int64_t* __restrict__ step) {
    const uint32_t s0 = drop_seed32(drop_seed_at(seed, step));
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (; i < n; i += stride) {
        int64_t r = i / row_len;
        int64_t k = i - r * row_len;
        uint32_t rm = drop_row(s0, (uint64_t)r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i + e >= n) break;
            y[i + e] = from_f32<T>(to_f32(x[i + e]) * drop_scale_rk(rm, (uint32_t)k, p, inv_keep));
            if (++k == row_len) { k = 0; ++r; rm = drop_row(s0, (uint64_t)r); }
        }
    }
}
// (t, res and out may alias — ops.dropout_add runs in place on t: no __restrict__)
__global__ __launch_bounds__(256) void dropout_add_kernel(const float* t, const float* res, float* out, int64_t n, int64_t row_len, float p,
                                                          float inv_keep, uint64_t seed, const int64_t* __restrict__ step) {
    const uint32_t s0 = drop_seed32(drop_seed_at(seed, step));
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (; i < n; i += stride) {
        int64_t r = i / row_len;
        int64_t k = i - r * row_len;
        uint32_t rm = drop_row(s0, (uint64_t)r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i + e >= n) break;
            out[i + e] = res[i + e] + t[i + e] * drop_scale_rk(rm, (uint32_t)k, p, inv_keep);
            if (++k == row_len) { k = 0; ++r; rm = drop_row(s0, (uint64_t)r); }
        }
    }
}
}  // namespace

// The one ladder of the two LayerNorm launchers below (undefined after them; it reads their dtype, x_f32 and D): dtype x x_f32 ->
// (T, TX), width -> (NP, WPR).  LAUNCH(T, TX, NP, WPR) is the caller's.
#define SVOL_LN_WIDTH(LAUNCH, TT, TXX)                         \
    do {                                                       \
        if (D <= 256) LAUNCH(TT, TXX, 1, 1);                   \
        else if (D <= 512) LAUNCH(TT, TXX, 2, 1);              \
        else if (D <= LN_MAX_PASSES * 256) LAUNCH(TT, TXX, 4, 1); \
        else if (D <= 2048) LAUNCH(TT, TXX, 2, 4);             \
        else if (D <= 3072) LAUNCH(TT, TXX, 3, 4);             \
        else LAUNCH(TT, TXX, 4, 4);                            \
    } while (0)
#define SVOL_LN_DISPATCH(LAUNCH)                                                   \
    do {                                                                           \
        if (dtype == SVOL_BF16 && x_f32) SVOL_LN_WIDTH(LAUNCH, bf16_t, float);     \
        else if (dtype == SVOL_BF16) SVOL_LN_WIDTH(LAUNCH, bf16_t, bf16_t);        \
        else if (dtype == SVOL_F16 && x_f32) SVOL_LN_WIDTH(LAUNCH, f16_t, float);  \
        else if (dtype == SVOL_F16) SVOL_LN_WIDTH(LAUNCH, f16_t, f16_t);           \
        else SVOL_LN_WIDTH(LAUNCH, float, float);                                  \
    } while (0)

extern "C" {

int svol_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, float* y32, void* y,
                       void* ypos, const void* pos, int64_t pos_rows, float* mean, float* rstd, int64_t M, int64_t D,
                       float dropout_p, uint64_t seed, const int64_t* seed_offset_dev, int dtype, void* stream) {
    if (!x || !gamma || !beta || (!y && !y32) || !mean || !rstd || M < 0 || D <= 0) return SVOL_E_INVALID;
    if (!aligned16(gamma) || !aligned16(beta)) return SVOL_E_INVALID;   // (16-byte vector loads of the affine parameters)
    if ((ypos != nullptr) != (pos != nullptr)) return SVOL_E_INVALID;
    if (pos && pos_rows <= 0) return SVOL_E_INVALID;
    if (D % 4 || D > LNW_MAX_D) return SVOL_E_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return SVOL_E_INVALID;
    if (!svol_is16(dtype) && dtype != SVOL_F32) return SVOL_E_INVALID;
    if (M == 0) return SVOL_OK;
    const float inv_keep = 1.f / (1.f - dropout_p);
    const bool wide = D > LN_MAX_PASSES * 256;
    if (wide && M > 0x7fffffffll) return SVOL_E_UNSUPPORTED;   // (one workgroup per row)
    const unsigned grid = wide ? (unsigned)M : (unsigned)((M + 3) / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define SVOL_LNF(TT, TXX, NPP, WPRR)                                                                                        \
    hipLaunchKernelGGL((ln_fwd_pick<TT, TXX, NPP, WPRR>()), dim3(grid), dim3(256), 0, s, (const TXX*)x, gamma, beta, y32, (TT*)y, \
                       (TT*)ypos, (const TT*)pos, pos_rows, mean, rstd, M, (int)D, dropout_p, inv_keep, seed, seed_offset_dev)
    SVOL_LN_DISPATCH(SVOL_LNF);
#undef SVOL_LNF
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int svol_layernorm_bwd(const float* dy32, const void* dy, const void* dy2, const void* x, int x_f32, const float* gamma,
                       const float* mean, const float* rstd, float* dx32, void* dx, float* dgamma, float* dbeta,
                       float* dx_colsum, int64_t M, int64_t D, float dropout_p, uint64_t seed, const int64_t* seed_offset_dev,
                       int dtype, void* stream) {
    if ((!dy32 && !dy && !dy2) || !x || !gamma || !mean || !rstd || (!dx && !dx32) || !dgamma || !dbeta || M < 0 || D <= 0)
        return SVOL_E_INVALID;
    if (D % 4 || D > LNW_MAX_D) return SVOL_E_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return SVOL_E_INVALID;
    if (!svol_is16(dtype) && dtype != SVOL_F32) return SVOL_E_INVALID;
    if (M == 0) return SVOL_OK;
    const float inv_keep = 1.f / (1.f - dropout_p);
    // ~2048 waves (512 workgroups); each wave walks `rpw` consecutive rows; one set of atomics per workgroup
    // (wide rows: as many workgroups as are resident at once — three to four per CU at NP = 2, two at NP = 3 / 4 — each walking `rpw`
    // consecutive rows with all four waves on one row.  Fewer leave HBM latency uncovered, more only add sink atomics:
    // profiles/layernorm_wide.md)
    const bool wide = D > LN_MAX_PASSES * 256;
    const int64_t lnw_wgs = D <= 2048 ? 1024 : 512;
    int64_t rpw = wide ? (M + lnw_wgs - 1) / lnw_wgs : (M + 2047) / 2048;
    if (rpw < 1) rpw = 1;
    const int64_t waves = (M + rpw - 1) / rpw;
    const unsigned grid = wide ? (unsigned)waves : (unsigned)((waves + 3) / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool det_mode = svol_deterministic();
    DetScratch det(det_mode ? (size_t)grid * 3 * (size_t)D : 0, s);   // deterministic mode: per-workgroup rows, folded below
    if (det_mode && !det.p) return SVOL_E_LAUNCH;
    // NP = passes of 256 columns per row: the accumulator / operand arrays are sized by it (NP = 1 at d = 256: 76 VGPRs
    // instead of the 166 of the 4-pass instantiation; 46 us instead of 50 at [50176, 256] = 5.0 TB/s.  More waves or a next-row
    // prefetch do not help further: the end-of-workgroup atomics, then HBM, bound it)
#define SVOL_LNB(TT, TXX, NPP, WPRR)                                                                                                 \
    hipLaunchKernelGGL((ln_bwd_kernel<TT, TXX, NPP, WPRR>), dim3(grid), dim3(256), 0, s, dy32, (const TT*)dy, (const TT*)dy2, (const TXX*)x, \
                       gamma, mean, rstd, dx32, (TT*)dx, dgamma, dbeta, dx_colsum, M, (int)D, dropout_p, inv_keep, seed,                  \
                       seed_offset_dev, (int)rpw, det.p)
    SVOL_LN_DISPATCH(SVOL_LNB);
#undef SVOL_LNB
    if (det_mode) {
        det_fold(det.p, (int)grid, 3 * D, dgamma, D, s);
        det_fold(det.p + D, (int)grid, 3 * D, dbeta, D, s);
        det_fold(det.p + 2 * D, (int)grid, 3 * D, dx_colsum, D, s);
    }
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

#undef SVOL_LN_DISPATCH
#undef SVOL_LN_WIDTH

int svol_dropout_sd(const void* x, void* y, int64_t n, int64_t row_len, float p, uint64_t seed, const int64_t* seed_step_dev, int dtype,
                    void* stream) {
    if (!x || !y || n < 0 || row_len <= 0 || row_len > 0xffffffffll || !(p >= 0.f && p < 1.f)) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    const float inv = 1.f / (1.f - p);
    int64_t g = (n + 1023) / 1024;
    if (g > 8192) g = 8192;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == SVOL_F32) hipLaunchKernelGGL(dropout_kernel<float>, dim3((unsigned)g), dim3(256), 0, s, (const float*)x, (float*)y, n, row_len, p, inv, seed, seed_step_dev);
    else if (dtype == SVOL_BF16) hipLaunchKernelGGL(dropout_kernel<bf16_t>, dim3((unsigned)g), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, n, row_len, p, inv, seed, seed_step_dev);
    else if (dtype == SVOL_F16) hipLaunchKernelGGL(dropout_kernel<f16_t>, dim3((unsigned)g), dim3(256), 0, s, (const f16_t*)x, (f16_t*)y, n, row_len, p, inv, seed, seed_step_dev);
    else return SVOL_E_INVALID;
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int svol_dropout(const void* x, void* y, int64_t n, int64_t row_len, float p, uint64_t seed, int dtype, void* stream) {
    return svol_dropout_sd(x, y, n, row_len, p, seed, nullptr, dtype, stream);
}

int svol_dropout_add_sd(const float* t32, const float* res32, float* out32, int64_t n, int64_t row_len, float p, uint64_t seed,
                        const int64_t* seed_step_dev, void* stream) {
    if (!t32 || !res32 || !out32 || n < 0 || row_len <= 0 || row_len > 0xffffffffll || !(p >= 0.f && p < 1.f)) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    int64_t g = (n + 1023) / 1024;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(dropout_add_kernel, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), t32, res32, out32, n,
                       row_len, p, 1.f / (1.f - p), seed, seed_step_dev);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}
int svol_dropout_add(const float* t32, const float* res32, float* out32, int64_t n, int64_t row_len, float p, uint64_t seed, void* stream) {
    return svol_dropout_add_sd(t32, res32, out32, n, row_len, p, seed, nullptr, stream);
}

int svol_posenc_sine(const float* mask, void* pos, int64_t B, int64_t L, int64_t D, int dtype, void* stream) {
    if (!mask || !pos || B <= 0 || L <= 0 || D <= 0) return SVOL_E_INVALID;
    if (L > (1 << 24) || D > 4096) return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (B > 65535) return SVOL_E_UNSUPPORTED;
    dim3 grid((unsigned)((L + 63) / 64), (unsigned)B);
    if (dtype == SVOL_BF16)
        hipLaunchKernelGGL(posenc_kernel<bf16_t>, grid, dim3(256), 0, s, mask, (bf16_t*)pos, (int)L, (int)D);
    else if (dtype == SVOL_F16)
        hipLaunchKernelGGL(posenc_kernel<f16_t>, grid, dim3(256), 0, s, mask, (f16_t*)pos, (int)L, (int)D);
    else if (dtype == SVOL_F32)
        hipLaunchKernelGGL(posenc_kernel<float>, grid, dim3(256), 0, s, mask, (float*)pos, (int)L, (int)D);
    else return SVOL_E_INVALID;
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // extern "C"
