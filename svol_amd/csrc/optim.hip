// The flat optimizers' update kernels and the dynamic loss scaler (parallel._FlatOptimizer, parallel.DynamicLossScaler): the
// reference's three --optimizer choices (train.py:94-99: torch.optim.SGD(lr, momentum=0.9, weight_decay=wd), torch.optim.Adam and
// torch.optim.AdamW(lr, weight_decay=wd)) over a flat, 16-byte aligned fp32 range of parameters p with gradients g and one (SGD: the
// momentum buffer) or two (Adam, AdamW: exp_avg, exp_avg_sq) state arrays.  Each rule's per-element arithmetic is written once
// (sgd_update, adam_update<DECOUPLED>: AdamW is Adam with decoupled weight decay), and each family has one kernel, an HBM-bound
// streaming pass: 4 parameters per thread (16-byte accesses), thread n / 4 takes the n % 4 tail, every array read once and written
// once.  SGD moves 20 bytes per parameter, Adam and AdamW 28; ZERO adds 4.
//   ZERO:   the gradient range is zeroed behind its read (optimizer.zero_grad() of the next iteration, train.py:222, folded into the
//           step: the step boundary loses the caller's fill launches).
//   SCALED: the update reads a state vector of four floats on the device: [0] loss scale, [1] overflow flag of the current step
//           (0 / 1), [2] clean steps since the last change of the scale, [3] optimizer steps really taken.  Nothing is written when
//           [1] is set (an overflowed step is skipped whole: parameters and state keep their values), the gradient is multiplied by
//           gscale / [0], and Adam's bias-correction step is [3] + 1.  The vector is a DynamicLossScaler's state (svol_grad_finite
//           sets [1], svol_loss_scaler_update moves [0], [2], [3] and clears [1]: no host synchronisation anywhere) or the clip state
//           of svol_grad_clip_state (gradnorm.hip), whose first four floats have this layout.
// Where a constant is computed decides its bits: the plain entries take Adam's step_size and 1 / sqrt(bc2) from the host in double
// and AdamW's decay = 1 - lr * wd in host float, the SCALED ones compute all three on the device in float.
// The two kernels stay separate functions with scalar parameters on purpose: which product of a sum the compiler contracts into an
// fma depends on how the body reaches the kernel, and a body shared through a rule type or a further inlined function made
// another choice in the SGD and Adam updates (other result bits).
// The grouped kernels (several param groups, a capturable step) are a third and fourth function beside them, further down: they read
// every hyper-parameter and the step count from device tables and promise the parity bar, not the bits of the entries above.
// The weight average (ema_flat_kernel, behind them) is a fifth, for the same reason: it shares nothing with the update bodies.
#include "common.h"

namespace {

__device__ __forceinline__ void sgd_update(float& p, float g, float& buf, float lr, float mom, float wd, float gscale) {
    const float d = g * gscale + wd * p;   // grad.add(param, alpha=weight_decay)
    buf = mom * buf + d;                   // buf.mul_(momentum).add_(grad)       (dampening 0; a zero buffer gives torch's first-step clone)
    p -= lr * buf;                         // param.add_(buf, alpha=-lr)
}

template <bool ZERO, bool SCALED>
__global__ __launch_bounds__(256) void sgd_flat_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, int64_t n4,
                                                       int64_t n, float lr, float mom, float wd, float gscale,
                                                       const float* __restrict__ state) {
    if constexpr (SCALED) {
        if (state[1] != 0.f) return;   // an overflowed step is skipped whole
        gscale = gscale / state[0];
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        f32x4 pp = *reinterpret_cast<f32x4*>(p + 4 * i), bb = *reinterpret_cast<f32x4*>(buf + 4 * i);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // (a vector element does not bind to a reference)
            float pe = pp[e], be = bb[e];
            sgd_update(pe, gg[e], be, lr, mom, wd, gscale);
            pp[e] = pe; bb[e] = be;
        }
        *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
        *reinterpret_cast<f32x4*>(buf + 4 * i) = bb;
        if constexpr (ZERO) *reinterpret_cast<f32x4*>(g + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else if (i == n4) {  // scalar tail (n % 4 elements)
        for (int64_t j = 4 * n4; j < n; ++j) {
            float pj = p[j], bj = buf[j];
            sgd_update(pj, g[j], bj, lr, mom, wd, gscale);
            p[j] = pj; buf[j] = bj;
            if constexpr (ZERO) g[j] = 0.f;
        }
    }
}

// DECOUPLED: AdamW's param.mul_(1 - lr * weight_decay) in place of Adam's grad.add(param, alpha=weight_decay).  A compile-time choice,
// not a zero coefficient: 0 * inf must not enter either rule's gradient.
template <bool DECOUPLED>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float wd, float decay, float b1, float b2, float step_size,
                                            float inv_bc2_sqrt, float eps, float gscale) {
    float gr;
    if constexpr (DECOUPLED) {
        gr = g * gscale;
        p *= decay;
    } else {
        gr = g * gscale + wd * p;
    }
    m = m + (gr - m) * (1.f - b1);                   // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + (1.f - b2) * gr * gr;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    p -= step_size * (m / (sqrtf(v) * inv_bc2_sqrt + eps));
}

template <bool DECOUPLED, bool ZERO, bool SCALED>
__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n4, int64_t n, float lr, float wd, float b1, float b2,
                                                        float step_size, float inv_bc2_sqrt, float eps, float gscale,
                                                        const float* __restrict__ state, float decay) {
    if constexpr (SCALED) {
        if (state[1] != 0.f) return;
        gscale = gscale / state[0];
        const float step = state[3] + 1.f;
        if constexpr (DECOUPLED) decay = 1.f - lr * wd;
        step_size = lr / (1.f - powf(b1, step));
        inv_bc2_sqrt = 1.f / sqrtf(1.f - powf(b2, step));
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        f32x4 pp = *reinterpret_cast<f32x4*>(p + 4 * i), mm = *reinterpret_cast<f32x4*>(m + 4 * i), vv = *reinterpret_cast<f32x4*>(v + 4 * i);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], me = mm[e], ve = vv[e];
            adam_update<DECOUPLED>(pe, gg[e], me, ve, wd, decay, b1, b2, step_size, inv_bc2_sqrt, eps, gscale);
            pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
        *reinterpret_cast<f32x4*>(m + 4 * i) = mm;
        *reinterpret_cast<f32x4*>(v + 4 * i) = vv;
        if constexpr (ZERO) *reinterpret_cast<f32x4*>(g + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else if (i == n4) {
        for (int64_t j = 4 * n4; j < n; ++j) {
            float pj = p[j], mj = m[j], vj = v[j];
            adam_update<DECOUPLED>(pj, g[j], mj, vj, wd, decay, b1, b2, step_size, inv_bc2_sqrt, eps, gscale);
            p[j] = pj; m[j] = mj; v[j] = vj;
            if constexpr (ZERO) g[j] = 0.f;
        }
    }
}

// What every launch checks first: SVOL_E_INVALID on a null array, n < 0 or !args_ok, SVOL_E_UNSUPPORTED on an array off a 16-byte
// boundary or a grid that would not fit; blocks: one thread per 4 parameters plus the tail thread, 0 (with SVOL_OK) when n == 0.
template <class... P>
int flat_grid(int64_t n, bool args_ok, unsigned& blocks, const P*... arrays) {
    blocks = 0;
    if ((... || !arrays) || n < 0 || !args_ok) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if ((... || !aligned16(arrays))) return SVOL_E_UNSUPPORTED;
    const int64_t b = (n / 4 + 1 + 255) / 256;
    if (b >= (1ll << 31)) return SVOL_E_UNSUPPORTED;
    blocks = (unsigned)b;
    return SVOL_OK;
}

// (g: only the ZERO kernels write it, and their entries take it non-const)
template <bool ZERO, bool SCALED>
int sgd_flat_launch(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                    const float* state, void* stream) {
    unsigned blocks;
    const int rc = flat_grid(n, !SCALED || state, blocks, p, g, buf);
    if (!blocks) return rc;
    hipLaunchKernelGGL((sgd_flat_kernel<ZERO, SCALED>), dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p,
                       const_cast<float*>(g), buf, n / 4, n, lr, momentum, weight_decay, grad_scale, state);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

template <bool DECOUPLED, bool ZERO, bool SCALED>
int adam_flat_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int64_t step, float grad_scale, const float* state, void* stream) {
    unsigned blocks;
    const int rc = flat_grid(n, SCALED ? state != nullptr : step > 0, blocks, p, g, m, v);
    if (!blocks) return rc;
    float step_size = 0.f, inv_bc2_sqrt = 0.f;
    if (!SCALED) {   // the plain entries' constants: bias corrections in double; decay in float, below
        const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
        step_size = (float)((double)lr / bc1);
        inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    }
    hipLaunchKernelGGL((adam_flat_kernel<DECOUPLED, ZERO, SCALED>), dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p,
                       const_cast<float*>(g), m, v, n / 4, n, lr, weight_decay, beta1, beta2, step_size, inv_bc2_sqrt, eps, grad_scale, state,
                       1.f - lr * weight_decay);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

// The grouped entries: the same streaming pass with every hyper-parameter and the step count read from device memory, per RUN of
// the range (a maximal stretch of adjacent parameters of one param group; runs end on 16-byte boundaries, seg_end counts float4s).
// One float4 per thread, 256 per workgroup, no scalar tail (n % 4 == 0).  A workgroup looks up the run of its FIRST vector with
// a binary search over seg_end whose every index derives from blockIdx and kernel arguments (wave-uniform: the table reads are
// scalar loads); a thread at or past that run's end (a workgroup that straddles runs: at most one per run boundary) searches on
// from there for itself.  The searches clamp to [0, nseg) and the group index to [0, ngroups): whatever the tables hold, every
// table read is inside the tables, and the arrays are only touched below n4.  Adam's bias corrections are computed in float from
// the run's row, as the SCALED branch above does from its arguments, but once per WORKGROUP for the run of its first vector: two
// powf, a square root and two divisions are ~400 VALU instructions against ~130 for the four elements' update, and per thread they
// cost the pass 17 % (measured: 0.1125 against 0.0957 ms per step over 19.1 M parameters).  One lane computes them while the
// workgroup's loads are in flight and hands them on through LDS; the wave that does so rotates with the workgroup index, so that the
// work spreads over a CU's four SIMDs.  A thread in a later run computes its own.

// first run s in [lo, nseg) with seg_end[s] > i; nseg - 1 when there is none
__device__ __forceinline__ int run_of(const int32_t* __restrict__ seg_end, int nseg, int lo, int64_t i) {
    int hi = nseg - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)seg_end[mid] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ const float* row_of(const int32_t* __restrict__ seg_group, int s, const float* __restrict__ hyper, int ngroups) {
    return hyper + 8 * min(max(seg_group[s], 0), ngroups - 1);
}

__device__ __forceinline__ void adam_constants(const float* __restrict__ h, float step, float& step_size, float& inv_bc2_sqrt, float& decay) {
    decay = 1.f - h[0] * h[4];
    step_size = h[0] / (1.f - powf(h[1], step));
    inv_bc2_sqrt = 1.f / sqrtf(1.f - powf(h[2], step));
}

template <bool ZERO>
__global__ __launch_bounds__(256) void sgd_grouped_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, int64_t n4,
                                                          const int32_t* __restrict__ seg_end, const int32_t* __restrict__ seg_group,
                                                          int nseg, const float* __restrict__ hyper, int ngroups,
                                                          const float* __restrict__ state, float gscale) {
    if (state) {
        if (state[1] != 0.f) return;   // an overflowed step is skipped whole
        gscale = gscale / state[0];
    }
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + threadIdx.x;
    if (i >= n4) return;
    f32x4 pp = *reinterpret_cast<f32x4*>(p + 4 * i), bb = *reinterpret_cast<f32x4*>(buf + 4 * i);
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * i);
    int s = run_of(seg_end, nseg, 0, i0);                                                // the workgroup's first vector: uniform
    if (i >= (int64_t)seg_end[s]) s = run_of(seg_end, nseg, min(s + 1, nseg - 1), i);    // this thread lies in a later run
    const float* h = row_of(seg_group, s, hyper, ngroups);
    const float lr = h[0], mom = h[1], wd = h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = pp[e], be = bb[e];
        sgd_update(pe, gg[e], be, lr, mom, wd, gscale);
        pp[e] = pe; bb[e] = be;
    }
    *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
    *reinterpret_cast<f32x4*>(buf + 4 * i) = bb;
    if constexpr (ZERO) *reinterpret_cast<f32x4*>(g + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
}

template <bool DECOUPLED, bool ZERO>
__global__ __launch_bounds__(256) void adam_grouped_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, int64_t n4, const int32_t* __restrict__ seg_end,
                                                           const int32_t* __restrict__ seg_group, int nseg,
                                                           const float* __restrict__ hyper, int ngroups, const float* __restrict__ state,
                                                           const float* __restrict__ step_count, float gscale) {
    if (state) {
        if (state[1] != 0.f) return;
        gscale = gscale / state[0];
    }
    __shared__ float first[3];   // step_size, 1 / sqrt(bc2), decay of the run of the workgroup's first vector
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + threadIdx.x;
    const bool live = i < n4;    // (no return in front of the barrier)
    f32x4 pp, mm, vv, gg;
    if (live) {
        pp = *reinterpret_cast<f32x4*>(p + 4 * i); mm = *reinterpret_cast<f32x4*>(m + 4 * i); vv = *reinterpret_cast<f32x4*>(v + 4 * i);
        gg = *reinterpret_cast<const f32x4*>(g + 4 * i);
    }
    const float step = *step_count + 1.f;
    const int s0 = run_of(seg_end, nseg, 0, i0);   // uniform
    const float* h = row_of(seg_group, s0, hyper, ngroups);
    float step_size, inv_bc2_sqrt, decay;
    if (threadIdx.x == (blockIdx.x & 3) * 64) {
        adam_constants(h, step, step_size, inv_bc2_sqrt, decay);
        first[0] = step_size; first[1] = inv_bc2_sqrt; first[2] = decay;
    }
    __syncthreads();
    if (!live) return;
    if (i < (int64_t)seg_end[s0]) {
        step_size = first[0]; inv_bc2_sqrt = first[1]; decay = first[2];
    } else {                                       // this thread lies in a later run
        h = row_of(seg_group, run_of(seg_end, nseg, min(s0 + 1, nseg - 1), i), hyper, ngroups);
        adam_constants(h, step, step_size, inv_bc2_sqrt, decay);
    }
    const float b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        adam_update<DECOUPLED>(pe, gg[e], me, ve, wd, decay, b1, b2, step_size, inv_bc2_sqrt, eps, gscale);
        pp[e] = pe; mm[e] = me; vv[e] = ve;
    }
    *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
    *reinterpret_cast<f32x4*>(m + 4 * i) = mm;
    *reinterpret_cast<f32x4*>(v + 4 * i) = vv;
    if constexpr (ZERO) *reinterpret_cast<f32x4*>(g + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// What the grouped launches check first, after the pattern of flat_grid; blocks: one thread per float4, 0 (with SVOL_OK) when n == 0.
template <class... P>
int grouped_grid(int64_t n, const void* seg_end, const void* seg_group, int nseg, const void* hyper, int ngroups, bool args_ok,
                 unsigned& blocks, const P*... arrays) {
    blocks = 0;
    if ((... || !arrays) || !seg_end || !seg_group || !hyper || n < 0 || nseg < 1 || ngroups < 1 || !args_ok) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if ((... || !aligned16(arrays)) || n % 4 != 0 || n / 4 >= (1ll << 31)) return SVOL_E_UNSUPPORTED;   // (seg_end is int32)
    blocks = (unsigned)((n / 4 + 255) / 256);
    return SVOL_OK;
}

template <bool DECOUPLED>
int adam_grouped_launch(float* p, float* g, float* m, float* v, int64_t n, const int32_t* seg_end, const int32_t* seg_group, int32_t nseg,
                        const float* hyper, int32_t ngroups, const float* state, const float* step_count, float grad_mul, int zero,
                        void* stream) {
    unsigned blocks;
    const int rc = grouped_grid(n, seg_end, seg_group, nseg, hyper, ngroups, step_count != nullptr, blocks, p, g, m, v);
    if (!blocks) return rc;
    auto k = zero ? adam_grouped_kernel<DECOUPLED, true> : adam_grouped_kernel<DECOUPLED, false>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, g, m, v, n / 4, seg_end, seg_group, nseg,
                       hyper, ngroups, state, step_count, grad_mul);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

// The weight average beside the update (parallel._FlatOptimizer(ema_decay=...)): ema += (1 - d) * (p - ema) over a flat range, one
// more streaming pass behind the update launch (8 bytes read, 4 written per parameter).  A kernel of its own, not a flag of the
// update kernels: see the header on what another way into those bodies does to their bits.  d is uniform: decay, or under warm-up
// min(decay, (1 + t) / (10 + t)) with t the 1-based index of the update being averaged, read where that update read its count:
// *step_count + 1 (grouped path), else state[3] + 1 (scaler or clip state), else the host's step.  Formed once per wave in double
// (one division), so that 1 - d carries a single fp32 rounding; the element arithmetic is one explicit fma.  Nothing is written
// when state[1] is set: the update was skipped, the average of the steps taken does not move.
__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n4, float decay,
                                                       int warmup, float step, const float* __restrict__ state,
                                                       const float* __restrict__ step_count) {
    if (state && state[1] != 0.f) return;   // an overflowed step is skipped whole
    double d = (double)decay;
    if (warmup) {
        const double t = step_count ? (double)*step_count + 1.0 : state ? (double)state[3] + 1.0 : (double)step;
        d = fmin(d, (1.0 + t) / (10.0 + t));
    }
    const float w = (float)(1.0 - d);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 ee = *reinterpret_cast<f32x4*>(ema + 4 * i);
    const f32x4 pp = *reinterpret_cast<const f32x4*>(p + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) ee[e] = fmaf(w, pp[e] - ee[e], ee[e]);
    *reinterpret_cast<f32x4*>(ema + 4 * i) = ee;
}

__global__ void flat_step_advance_kernel(float* step_count, const float* state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!state || state[1] == 0.f) *step_count += 1.f;
}

__global__ __launch_bounds__(256) void grad_finite_kernel(const float* __restrict__ g, int64_t n4, int64_t n, float* __restrict__ state) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) bad |= nonfinite(v[e]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t j = 4 * n4; j < n; ++j) bad |= nonfinite(g[j]);
    if (__any(bad) && (threadIdx.x & 63) == 0) state[1] = 1.f;   // (benign race: every writer stores the same value)
}

__global__ void loss_scaler_update_kernel(float* state, float growth, float backoff, float interval, float min_scale, float max_scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (state[1] != 0.f) {
        state[0] = fmaxf(state[0] * backoff, min_scale);
        state[2] = 0.f;
    } else {
        state[3] += 1.f;
        state[2] += 1.f;
        if (state[2] >= interval) { state[0] = fminf(state[0] * growth, max_scale); state[2] = 0.f; }
    }
    state[1] = 0.f;
}

}  // namespace

extern "C" {

int svol_sgd_flat(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                  void* stream) {
    return sgd_flat_launch<false, false>(p, g, buf, n, lr, momentum, weight_decay, grad_scale, nullptr, stream);
}
int svol_sgd_flat_zero(float* p, float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                       void* stream) {
    return sgd_flat_launch<true, false>(p, g, buf, n, lr, momentum, weight_decay, grad_scale, nullptr, stream);
}
int svol_sgd_flat_scaled(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_mul,
                         const float* scaler_state, void* stream) {
    return sgd_flat_launch<false, true>(p, g, buf, n, lr, momentum, weight_decay, grad_mul, scaler_state, stream);
}

int svol_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t step, float grad_scale, void* stream) {
    return adam_flat_launch<false, false, false>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, stream);
}
int svol_adam_flat_zero(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, float grad_scale, void* stream) {
    return adam_flat_launch<false, true, false>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, stream);
}
int svol_adam_flat_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, float grad_mul, const float* scaler_state, void* stream) {
    return adam_flat_launch<false, false, true>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, 0, grad_mul, scaler_state, stream);
}

int svol_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, float grad_scale, void* stream) {
    return adam_flat_launch<true, false, false>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, stream);
}
int svol_adamw_flat_zero(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int64_t step, float grad_scale, void* stream) {
    return adam_flat_launch<true, true, false>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, stream);
}
int svol_adamw_flat_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, float grad_mul, const float* scaler_state, void* stream) {
    return adam_flat_launch<true, false, true>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, 0, grad_mul, scaler_state, stream);
}

int svol_sgd_flat_grouped(float* p, float* g, float* buf, int64_t n, const int32_t* seg_end, const int32_t* seg_group, int32_t nseg,
                          const float* hyper, int32_t ngroups, const float* state, float grad_mul, int zero, void* stream) {
    unsigned blocks;
    const int rc = grouped_grid(n, seg_end, seg_group, nseg, hyper, ngroups, true, blocks, p, g, buf);
    if (!blocks) return rc;
    hipLaunchKernelGGL(zero ? sgd_grouped_kernel<true> : sgd_grouped_kernel<false>, dim3(blocks), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), p, g, buf, n / 4, seg_end, seg_group, nseg, hyper, ngroups, state, grad_mul);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}
int svol_adam_flat_grouped(float* p, float* g, float* m, float* v, int64_t n, const int32_t* seg_end, const int32_t* seg_group,
                           int32_t nseg, const float* hyper, int32_t ngroups, const float* state, const float* step_count,
                           float grad_mul, int zero, void* stream) {
    return adam_grouped_launch<false>(p, g, m, v, n, seg_end, seg_group, nseg, hyper, ngroups, state, step_count, grad_mul, zero, stream);
}
int svol_adamw_flat_grouped(float* p, float* g, float* m, float* v, int64_t n, const int32_t* seg_end, const int32_t* seg_group,
                            int32_t nseg, const float* hyper, int32_t ngroups, const float* state, const float* step_count,
                            float grad_mul, int zero, void* stream) {
    return adam_grouped_launch<true>(p, g, m, v, n, seg_end, seg_group, nseg, hyper, ngroups, state, step_count, grad_mul, zero, stream);
}
int svol_flat_step_advance(float* step_count, const float* state, void* stream) {
    if (!step_count) return SVOL_E_INVALID;
    hipLaunchKernelGGL(flat_step_advance_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), step_count, state);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int svol_ema_flat(float* ema, const float* p, int64_t n, float decay, int warmup, int64_t step, const float* state,
                  const float* step_count, void* stream) {
    if (!ema || !p || n < 0 || !(decay >= 0.f && decay <= 1.f) || (!state && !step_count && step < 1)) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if (n % 4 != 0 || !aligned16(ema) || !aligned16(p)) return SVOL_E_UNSUPPORTED;
    const int64_t blocks = (n / 4 + 255) / 256;
    if (blocks >= (1ll << 31)) return SVOL_E_UNSUPPORTED;
    hipLaunchKernelGGL(ema_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), ema, p, n / 4, decay,
                       warmup, (float)step, state, step_count);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int svol_grad_finite(const float* g, int64_t n, float* scaler_state, void* stream) {
    if (!g || !scaler_state || n < 0) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if (!aligned16(g)) return SVOL_E_UNSUPPORTED;
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(grad_finite_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, n4, n, scaler_state);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int svol_loss_scaler_update(float* scaler_state, float growth_factor, float backoff_factor, int64_t growth_interval, float min_scale,
                            float max_scale, void* stream) {
    if (!scaler_state || growth_factor < 1.f || backoff_factor <= 0.f || backoff_factor > 1.f || growth_interval < 1) return SVOL_E_INVALID;
    hipLaunchKernelGGL(loss_scaler_update_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), scaler_state, growth_factor,
                       backoff_factor, (float)growth_interval, min_scale, max_scale);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // extern "C"
