// Global gradient-norm clipping for the flat optimizers (stands in for torch.nn.utils.clip_grad_norm_ between backward() and step(),
// the place of train.py:231-234 in the reference's loop): the sum of squares of one flat fp32 gradient range, and the one-thread
// kernel that turns the per-bucket sums into the state vector the *_flat_scaled update kernels read (optim.hip).
// No floating-point atomics anywhere: a fixed grid, a fixed reduction order, the same bits in every run.
#include "common.h"

namespace {

constexpr int SQ_BLOCK = 256;
constexpr int SQ_MAX_BLOCKS = 2048;   // the cap of svol_grad_finite: 8 blocks per CU, a grid-stride loop above it

inline int sq_blocks(int64_t n) {
    const int64_t blocks = (n / 4 + 1 + SQ_BLOCK - 1) / SQ_BLOCK;   // one thread per 4 floats plus the tail thread
    return (int)(blocks > SQ_MAX_BLOCKS ? SQ_MAX_BLOCKS : blocks);
}

// Stage 1: part[blockIdx.x] = the block's share of sum g^2.  Streaming read, 16 bytes per lane and iteration; the thread whose stride
// reaches index n / 4 adds the n % 4 tail.  Adder chains in fp32: one accumulator per vector element (ceil(n4 / threads) adds: 16 at
// n = 2^25), 2 to join the four, 1 for the tail, 6 wave steps, 3 across the block's waves = 28 at n = 2^25; the rest of the sum runs in double.
__global__ __launch_bounds__(SQ_BLOCK) void grad_sqnorm_partial_kernel(const float* __restrict__ g, int64_t n4, int64_t n,
                                                                       float* __restrict__ part) {
    __shared__ float wsum[SQ_BLOCK / 64];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float tail = 0.f;
    const int64_t stride = (int64_t)gridDim.x * SQ_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * SQ_BLOCK + threadIdx.x; i <= n4; i += stride) {
        if (i < n4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(v[e], v[e], acc[e]);
        } else {
            for (int64_t j = 4 * n4; j < n; ++j) tail = fmaf(g[j], g[j], tail);
        }
    }
    float s = wave_sum(((acc[0] + acc[1]) + (acc[2] + acc[3])) + tail);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// Stage 2 (one block, behind stage 1 on the stream): the block partials in index order, in double; *out = (float) sum.
__global__ __launch_bounds__(SQ_BLOCK) void grad_sqnorm_final_kernel(const float* __restrict__ part, int parts, float* __restrict__ out) {
    __shared__ double sh[SQ_BLOCK];
    double a = 0.0;
    for (int i = threadIdx.x; i < parts; i += SQ_BLOCK) a += (double)part[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int w = SQ_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (float)sh[0];   // past fp32's range: inf, the overflow signal
}

// One thread.  state_out: [0] scale / coef (the *_flat_scaled kernels multiply the gradient by grad_mul / [0]), [1] overflow flag,
// [2] 0, [3] updates taken so far, [4] total norm of the true gradient before clipping, [5] coef, [6..7] 0.
__global__ void grad_clip_state_kernel(const float* __restrict__ sq, int nb, float gmul, float max_norm, float loss_scale, float steps_taken,
                                       float* scaler_state, float* __restrict__ state_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sum = 0.0;
    for (int b = 0; b < nb; ++b) sum += (double)sq[b];
    const float scale = scaler_state ? scaler_state[0] : loss_scale;
    const float taken = scaler_state ? scaler_state[3] : steps_taken;
    const float total = (float)(sqrt(sum) * (double)gmul / (double)scale);
    const float c = max_norm / (total + 1e-6f);
    const float coef = c > 1.f ? 1.f : c;             // torch's clamp(max=1): a NaN stays a NaN
    float flag = 0.f;
    if (scaler_state) {
        if (nonfinite(total)) scaler_state[1] = 1.f;   // svol_loss_scaler_update backs the scale off
        flag = scaler_state[1];
    }
    state_out[0] = scale / coef;
    state_out[1] = flag;
    state_out[2] = 0.f;
    state_out[3] = taken;
    state_out[4] = total;
    state_out[5] = coef;
    state_out[6] = 0.f;
    state_out[7] = 0.f;
}

}  // namespace

extern "C" {

int64_t svol_grad_sqnorm_ws_bytes(int64_t n) {
    if (n < 0) return SVOL_E_INVALID;
    return ((int64_t)sq_blocks(n) * 4 + 15) / 16 * 16;
}

int svol_grad_sqnorm(const float* g, int64_t n, float* ws, float* out, void* stream) {
    if (!g || !ws || !out || n < 0) return SVOL_E_INVALID;
    if (!aligned16(g) || !aligned16(ws)) return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int blocks = n == 0 ? 0 : sq_blocks(n);
    if (blocks) {
        hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3((unsigned)blocks), dim3(SQ_BLOCK), 0, s, g, n / 4, n, ws);
        SVOL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(SQ_BLOCK), 0, s, ws, blocks, out);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int svol_grad_clip_state(const float* sq, int32_t nb, float grad_mul, float max_norm, float loss_scale, int64_t steps_taken,
                         float* scaler_state, float* state_out, void* stream) {
    if (!sq || !state_out || nb < 1 || steps_taken < 0 || !(max_norm > 0.f) || (!scaler_state && !(loss_scale > 0.f))) return SVOL_E_INVALID;
    hipLaunchKernelGGL(grad_clip_state_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sq, (int)nb, grad_mul, max_norm,
                       loss_scale, (float)steps_taken, scaler_state, state_out);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // extern "C"
