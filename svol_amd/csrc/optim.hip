// SGD with momentum and Adam with coupled L2 over a flat fp32 range: the reference's other two --optimizer choices
// (train.py:94-97: torch.optim.SGD(lr, momentum=0.9, weight_decay=wd), torch.optim.Adam(lr, weight_decay=wd)); AdamW is in norm.hip.
// HBM-bound streaming passes shaped like adamw_flat_kernel: 4 parameters per thread (16-byte accesses), thread n/4 takes the n % 4
// tail, every array read once and written once.  SGD moves 20 bytes per parameter (p, g, buf in; p, buf out), Adam 28; ZERO adds 4.
#include "common.h"

namespace {

// ZERO:   the gradient range is zeroed behind its read (optimizer.zero_grad() of the next iteration folded into the step).
// SCALED: dynamic loss scaling, the contract of adamw_flat_scaled_kernel (norm.hip) — nothing is written when state[1] is set,
//         the gradient is multiplied by gscale / state[0], Adam's bias-correction step is state[3] + 1.

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

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float wd, float b1, float b2, float step_size,
                                            float inv_bc2_sqrt, float eps, float gscale) {
    const float gr = g * gscale + wd * p;            // grad.add(param, alpha=weight_decay): coupled L2, no p *= 1 - lr*wd
    m = m + (gr - m) * (1.f - b1);                   // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + (1.f - b2) * gr * gr;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    p -= step_size * (m / (sqrtf(v) * inv_bc2_sqrt + eps));
}

template <bool ZERO, bool SCALED>
__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n4, int64_t n, float lr, float wd, float b1, float b2,
                                                        float step_size, float inv_bc2_sqrt, float eps, float gscale,
                                                        const float* __restrict__ state) {
    if constexpr (SCALED) {
        if (state[1] != 0.f) return;
        gscale = gscale / state[0];
        const float step = state[3] + 1.f;
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
            adam_update(pe, gg[e], me, ve, wd, b1, b2, step_size, inv_bc2_sqrt, eps, gscale);
            pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
        *reinterpret_cast<f32x4*>(m + 4 * i) = mm;
        *reinterpret_cast<f32x4*>(v + 4 * i) = vv;
        if constexpr (ZERO) *reinterpret_cast<f32x4*>(g + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else if (i == n4) {
        for (int64_t j = 4 * n4; j < n; ++j) {
            float pj = p[j], mj = m[j], vj = v[j];
            adam_update(pj, g[j], mj, vj, wd, b1, b2, step_size, inv_bc2_sqrt, eps, gscale);
            p[j] = pj; m[j] = mj; v[j] = vj;
            if constexpr (ZERO) g[j] = 0.f;
        }
    }
}

// one thread per 4 parameters plus the tail thread; 0 when the grid would not fit
inline unsigned flat_blocks(int64_t n) {
    const int64_t blocks = (n / 4 + 1 + 255) / 256;
    return blocks >= (1ll << 31) ? 0u : (unsigned)blocks;
}

template <bool ZERO, bool SCALED>
int sgd_flat_launch(float* p, float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                    const float* state, void* stream) {
    if (!p || !g || !buf || n < 0 || (SCALED && !state)) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if (!aligned16(p) || !aligned16(g) || !aligned16(buf)) return SVOL_E_UNSUPPORTED;
    const unsigned blocks = flat_blocks(n);
    if (!blocks) return SVOL_E_UNSUPPORTED;
    hipLaunchKernelGGL((sgd_flat_kernel<ZERO, SCALED>), dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, g, buf, n / 4, n,
                       lr, momentum, weight_decay, grad_scale, state);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

template <bool ZERO, bool SCALED>
int adam_flat_launch(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int64_t step, float grad_scale, const float* state, void* stream) {
    if (!p || !g || !m || !v || n < 0 || (SCALED ? !state : step <= 0)) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return SVOL_E_UNSUPPORTED;
    const unsigned blocks = flat_blocks(n);
    if (!blocks) return SVOL_E_UNSUPPORTED;
    float step_size = 0.f, inv_bc2_sqrt = 0.f;
    if (!SCALED) {   // bias corrections in double on the host, as adamw_flat_launch computes them
        const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
        step_size = (float)((double)lr / bc1);
        inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    }
    hipLaunchKernelGGL((adam_flat_kernel<ZERO, SCALED>), dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, g, m, v, n / 4, n,
                       lr, weight_decay, beta1, beta2, step_size, inv_bc2_sqrt, eps, grad_scale, state);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // namespace

extern "C" {

int svol_sgd_flat(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                  void* stream) {
    return sgd_flat_launch<false, false>(p, const_cast<float*>(g), buf, n, lr, momentum, weight_decay, grad_scale, nullptr, stream);
}
int svol_sgd_flat_zero(float* p, float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                       void* stream) {
    return sgd_flat_launch<true, false>(p, g, buf, n, lr, momentum, weight_decay, grad_scale, nullptr, stream);
}
int svol_sgd_flat_scaled(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_mul,
                         const float* scaler_state, void* stream) {
    return sgd_flat_launch<false, true>(p, const_cast<float*>(g), buf, n, lr, momentum, weight_decay, grad_mul, scaler_state, stream);
}

int svol_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t step, float grad_scale, void* stream) {
    return adam_flat_launch<false, false>(p, const_cast<float*>(g), m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr,
                                          stream);
}
int svol_adam_flat_zero(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, float grad_scale, void* stream) {
    return adam_flat_launch<true, false>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, stream);
}
int svol_adam_flat_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, float grad_mul, const float* scaler_state, void* stream) {
    return adam_flat_launch<false, true>(p, const_cast<float*>(g), m, v, n, lr, beta1, beta2, eps, weight_decay, 1, grad_mul, scaler_state,
                                         stream);
}

}  // extern "C"
