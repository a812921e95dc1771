// The LayerNorm row, shared: the backward of svol_layernorm_bwd at both row layouts (LnBwdRows), the forward of the gate's apply pass and
// of the fused-score kernel (LnFwdRow), and the workgroup fold of per-column sums (ln_fold_columns: the LayerNorm backward and the gate's
// du).  Three kernels keep their own copy of the arithmetic, because their compiled roundings could not be met from here
// (profiles/ln_row.md): the forward kernels of svol_layernorm_fwd (norm.hip) and gate_bwd_ln_kernel (gate.hip).
// A lane owns 4 contiguous columns per pass (8 B 16-bit / 16 B f32 coalesced accesses), statistics are fp32, and every summation order
// and every rounding here is part of the contract: the outputs are compared bit for bit across kernels (tests/gpu_checks.py) and were
// compared with the copies they replaced (profiles/ln_row.md).  So the bodies compile with floating-point contraction off and name their fused multiply-adds where
// the code they replace had them (left to the compiler, whether a product is fused into the sum that follows depends on what the SLP
// vectoriser packed first, and a helper meets it in another shape than a kernel with the text pasted in).
#pragma once
#include "common.h"

namespace {

// Who owns a row.  WPR = waves per row: 1 = one wave per row, four rows (forward) or row ranges (backward) per workgroup, rows of up
// to 4 passes of 256 columns; 4 = the four waves of a workgroup share a row of up to 4 passes of 1024 columns, thread t owning the
// vectors (t + 256 j) * 4 (one wave per row would hold 64 values per lane per array at D = 4096: the backward's three per-column
// accumulators alone would be 192 registers).
template <int WPR>
struct LnOwner {
    static_assert(WPR == 1 || WPR == 4, "a row belongs to one wave or to the four waves of a workgroup");
    static __device__ __forceinline__ int lane() { return WPR == 1 ? threadIdx.x & 63 : threadIdx.x; }   // lane-in-row id
    static __device__ __forceinline__ int col(int j) { return (lane() + 64 * WPR * j) * 4; }            // first column of pass j
    // which row (forward) or row range (backward) of the launch this owner has
    static __device__ __forceinline__ int64_t index() { return WPR == 1 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x; }
    // N sets of four LDS words for sum() (none for WPR = 1: the narrow kernels keep their static LDS at what the column fold needs)
    template <int N>
    static __device__ __forceinline__ float (*slots())[4] {
        if constexpr (WPR == 4) {
            __shared__ float s[N][4];
            return s;
        } else {
            return nullptr;
        }
    }
    // K row sums, in every lane of the row: wave_sum, and for WPR = 4 four LDS words per sum, ONE barrier, (s0 + s1) + (s2 + s3).
    // slot: K sets from slots(), not reused before every wave has passed the next barrier.
    template <int K>
    static __device__ __forceinline__ void sum(float (&v)[K], float (*slot)[4]) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
        if constexpr (WPR == 4) {
            if ((threadIdx.x & 63) == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) slot[k][threadIdx.x >> 6] = v[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = (slot[k][0] + slot[k][1]) + (slot[k][2] + slot[k][3]);
        }
    }
};

// ---- forward (one wave per row): y = (x * scale - mu) * rs * gamma + beta, three steps ---------------------------------------------------
// The gate's apply pass and the fused-score kernel (gate.hip).  T = element type of the compute-dtype outputs and of pos, NP = passes of
// 256 columns.  The two hooks: `scale`, a per-row factor on x (the gate's 1 + a; the literal 1.f folds away), and `tp`, where store()
// leaves y + pos in fp32 (the fused score epilogue; the literal nullptr folds away).  svol_layernorm_fwd's own kernels (norm.hip) are
// NOT built on this: the fused-score kernel's promise of their bits at one pass rests on both rounding alike — squares rounded before they
// are summed, the affine step one fused multiply-add — and is asserted by tests/gpu_checks.py::check_gate_scores_fused.
template <typename T, int NP>
struct LnFwdRow {
    using Own = LnOwner<1>;
    Vec4<float> t[NP], gv[NP], bv[NP];
    Vec4<T> pv[NP];
    float v[NP][4], mu, rs;

    // every global load of the row goes out before the first reduction: one memory latency per wave, not two.  The row's own vectors
    // first, then the affine parameters every row shares: the two 64-bit row addresses are dead before gamma and beta take their registers.
    __device__ __forceinline__ void load(const float* __restrict__ x, const T* __restrict__ pos, int64_t row, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, int D) {
        const float* xl = x + row * D + Own::col(0);   // this lane's columns of pass 0; pass j is a constant further on
        const T* pl = pos + row * D + Own::col(0);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (Own::col(j) < D) {
                t[j].load(xl + 256 * j);
                pv[j].load(pl + 256 * j);
            }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = Own::col(j);
            if (c < D) {
                gv[j].load(gamma + c);
                bv[j].load(beta + c);
            }
        }
    }
    // two-pass mean and rstd of x * scale
    __device__ __forceinline__ void stats(float scale, int D) {
#pragma clang fp contract(off)
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = Own::col(j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[j][e] = c < D ? t[j].get(e) * scale : 0.f;
                s += v[j][e];
            }
        }
        mu = wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (Own::col(j) < D) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[j][e] - mu; q += d * d; }
            }
        }
        rs = rsqrtf(wave_sum(q) / (float)D + 1e-5f);
    }
    // normalise and store to the three sinks (each may be null)
    __device__ __forceinline__ void store(int64_t row, float* __restrict__ y32, T* __restrict__ y, T* __restrict__ ypos, int D,
                                          float (*tp)[4]) const {
#pragma clang fp contract(off)
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = Own::col(j);
            if (c < D) {
                Vec4<T> o, op;
                Vec4<float> o32;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float r = __builtin_fmaf((v[j][e] - mu) * rs, gv[j].get(e), bv[j].get(e));
                    o.set(e, r);
                    o32.set(e, r);
                    op.set(e, r + pv[j].get(e));
                    if (tp) tp[j][e] = r + pv[j].get(e);
                }
                if (y32) o32.store(y32 + row * D + c);
                if (y) o.store(y + row * D + c);
                if (ypos) op.store(ypos + row * D + c);
            }
        }
    }
};

// ---- backward: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = (dy32 + dy + dy2) * gamma (dropout mask applied first),
// xhat = (x - mean) * rstd -----------------------------------------------------------------------------------------------------------
// An owner walks consecutive rows: a dependent load -> reduce -> store chain, so the caller fetches the NEXT row's operand vectors and
// statistics into a second Row before it calls row() on the current one (58 -> 4x us per [50176, 256] launch).  acc holds the
// per-column sums over the owner's rows: [0] dgamma, [1] dbeta, [2] the column sums of dx.  gamma sits in registers.
template <typename T, typename TX, int NP, int WPR>
struct LnBwdRows {
    using Own = LnOwner<WPR>;
    struct Row { Vec4<float> a32[NP]; Vec4<T> a[NP], b[NP]; Vec4<TX> xv[NP]; float mu, rs; };
    const float* __restrict__ dy32;   // the three gradient operands: each may be null
    const T* __restrict__ dy;
    const T* __restrict__ dy2;
    const TX* __restrict__ x;
    const float* __restrict__ mean;
    const float* __restrict__ rstd;
    int D;
    float acc[3][NP][4], gm[NP][4];

    __device__ __forceinline__ void init(const float* __restrict__ gamma) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = Own::col(j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][j][e] = acc[1][j][e] = acc[2][j][e] = 0.f;
                gm[j][e] = c < D ? gamma[c + e] : 0.f;
            }
        }
    }
    __device__ __forceinline__ void fetch(int64_t row, Row& r) const {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = Own::col(j);
            if (c < D) {
                if (dy32) r.a32[j].load(dy32 + row * D + c);
                if (dy) r.a[j].load(dy + row * D + c);
                if (dy2) r.b[j].load(dy2 + row * D + c);
                r.xv[j].load(x + row * D + c);
            }
        }
        r.mu = mean[row];
        r.rs = rstd[row];
    }
    // One row: accumulates acc, stores dx (fp32 and / or T; either may be null).  slot: two sets of LnOwner::slots() (null at WPR = 1).
    __device__ __forceinline__ void row(const Row& cur, int64_t row, float* __restrict__ dx32, T* __restrict__ dx, float p, float inv_keep,
                                        uint64_t seed, float (*slot)[4]) {
#pragma clang fp contract(off)
        const float mu = cur.mu, rs = cur.rs;
        float g[NP][4], xh[NP][4];
        float s[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = Own::col(j);
            if (c < D) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float d = (dy32 ? cur.a32[j].get(e) : 0.f) + (dy ? cur.a[j].get(e) : 0.f) + (dy2 ? cur.b[j].get(e) : 0.f);
                    if (p > 0.f) d *= dropout_scale(seed, (uint64_t)row, (uint32_t)(c + e), p, inv_keep);
                    const float h = (cur.xv[j].get(e) - mu) * rs;
                    xh[j][e] = h;
                    acc[0][j][e] = __builtin_fmaf(d, h, acc[0][j][e]);
                    acc[1][j][e] += d;
                    const float gg = d * gm[j][e];
                    g[j][e] = gg;
                    s[0] += gg;
                    s[1] += gg * h;
                }
            }
        }
        Own::sum(s, slot);
        const float s1 = s[0] / (float)D, s2 = s[1] / (float)D;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = Own::col(j);
            if (c < D) {
                Vec4<T> o;
                Vec4<float> o32;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ds = rs * __builtin_fmaf(-xh[j][e], s2, g[j][e] - s1);
                    acc[2][j][e] += ds;
                    o.set(e, ds);
                    o32.set(e, ds);
                }
                if (dx32) o32.store(dx32 + row * D + c);
                if (dx) o.store(dx + row * D + c);
            }
        }
    }
};

// ---- column fold: K per-column register arrays of every owner of the workgroup -> LDS [K][NP * 256 * WPR] ------------------------------
// WPR = 1: the four waves hold partial sums of the same columns and fold one after another, w = 0..3 with a barrier each.  WPR = 4:
// every column has ONE owner in the workgroup and nothing is folded; the sums still pass through LDS so that consecutive lanes reach
// consecutive addresses afterwards (a lane owns 4 neighbouring columns: straight from registers a wave's atomic instruction would
// spread over 8 cache lines, and each line would be visited by 4 instructions).
template <int WPR, int K, int NP>
__device__ __forceinline__ const float* ln_fold_columns(const float (&part)[K][NP][4], int D) {
    using Own = LnOwner<WPR>;
    __shared__ float red[K][NP * 256 * WPR];
    const int wave = threadIdx.x >> 6;
    for (int w = 0; w < (WPR == 1 ? 4 : 1); ++w) {
        if (WPR == 4 || wave == w) {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int c = Own::col(j);
                if (c < D) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            if (w == 0) red[k][c + e] = part[k][j][e];
                            else red[k][c + e] += part[k][j][e];
                        }
                }
            }
        }
        __syncthreads();
    }
    return &red[0][0];
}
// ... and on to the sinks: one set of atomics per WORKGROUP, in lane order (every wave of every workgroup adding to the same D
// addresses is the contended-atomic worst case; a null sink is skipped), or — deterministic mode (common.h) — this workgroup's row
// [K * D] of the scratch, which the launcher folds in index order with det_fold.
template <int WPR, int K, int NP>
__device__ __forceinline__ void ln_fold_columns(const float (&part)[K][NP][4], float* const (&sink)[K], float* __restrict__ det_row, int D) {
    const float* red = ln_fold_columns<WPR>(part, D);
    for (int c = threadIdx.x; c < D; c += 256) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float v = red[k * NP * 256 * WPR + c];
            if (det_row) det_row[k * D + c] = v;
            else if (sink[k]) atomicAdd(sink[k] + c, v);
        }
    }
}

}  // namespace
