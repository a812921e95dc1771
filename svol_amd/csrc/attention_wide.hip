// Multi-head attention at head widths 32 < d_h <= 64 (d_h % 8 == 0: 40, 48, 56, 64) for gfx950: --nheads 4 at hidden_dim 256,
// --hidden_dim 512 / 384 at eight heads.  f32 (v_mfma_f32_32x32x2_f32, exact fp32), bf16 and fp16 (v_mfma_f32_32x32x16_{bf16,f16}) from ONE
// template on the element type.
//
// The scheme is attention.hip's generic one (the "swapped" product: softmax statistics lane-local, the first product's accumulator
// fed to the second MFMA from registers), widened from one 32-column d-tile to two:
//
//   first product : X[reg row][lane row] = A_tile[reg row][0:64] . B_block[lane row][0:64]      (twice the d-chunks)
//   second product: Y_t[d][lane row]    += A_tileT[32 t + d][reg row] * f(X)[reg row][lane row]  (t = 0, 1: two accumulator tiles)
//
//   forward : lane = queries, reg = keys : X = K Q^T -> P ; O^T += V^T P
//   dq      : lane = queries, reg = keys : P, dP = V dO^T -> dS ; dQ^T += K^T dS
//   dk/dv   : lane = keys, reg = queries : P, dV^T += dO^T P ; dP = dO V^T -> dS ; dK^T += Q^T dS
//
// Columns >= d_h are zero in registers and LDS.  Plain compiler-scheduled HIP: no key split, no single pass, no atomics, no workspace —
// results are bit-reproducible, and the same under SVOL_DETERMINISTIC=1.  The contract (leading dimensions, lse2 in log2 units, kbias,
// q_premul, the dropout keep mask, delta in the first B H Lq floats of the scratch) is that of attention.hip's d_h <= 32 kernels.
//
// LDS per workgroup (bytes; 64 rows x 64 d natural image, [64 d][64 rows] transposed image with a padded row stride):
//            natural   transposed   forward   dq       dk/dv
//   16-bit     8192       9216       17664    25856    35328
//   f32       16384      17408       34048    50432    68096     (two workgroups per CU: 136192 of 163840)
#include "attn_call.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// EPC: elements per 16-byte chunk; CPR: chunks per 64-wide row; NA1: chunks a lane feeds to the first product; NA2: 16-byte operands
// of one d-tile's second product (32 reg-side rows)
template <typename T> struct WT {
    static constexpr bool H = sizeof(T) == 2;
    static constexpr int EPC = H ? 8 : 4, CPR = H ? 8 : 16, NA1 = H ? 4 : 8, NA2 = H ? 2 : 4;
    static constexpr int NAT_ROW = H ? 128 : 256, TR_STRIDE = H ? 64 * 2 + 16 : 64 * 4 + 16;
    static constexpr int NAT = 64 * NAT_ROW, TR = 64 * TR_STRIDE;
};

// ---- staging ---------------------------------------------------------------
// natural image: [64 rows][64 d] (zero padded), 16-byte chunks XOR-swizzled against bank conflicts
template <typename T>
__device__ __forceinline__ int nat_off(int row, int ch) {
    return row * WT<T>::NAT_ROW + ((ch ^ (row & (WT<T>::CPR - 1))) << 4);
}

// Stage 64 rows starting at row0 of a [rows, ld] matrix (head column offset already applied) into the natural image `nat` and/or the
// transposed image `tr`.
template <typename T>
__device__ __forceinline__ void stage_tile(char* nat, char* tr, const T* g, int64_t ld, int row0, int limit, int dh, int tid) {
    constexpr int EPC = WT<T>::EPC, CPR = WT<T>::CPR, ST = WT<T>::TR_STRIDE;
    for (int c = tid; c < 64 * CPR; c += 256) {
        const int row = c / CPR, ch = c % CPR;
        const int d0 = ch * EPC;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row0 + row < limit && d0 < dh) v = *reinterpret_cast<const uint4*>(g + (int64_t)(row0 + row) * ld + d0);
        if (nat) *reinterpret_cast<uint4*>(nat + nat_off<T>(row, ch)) = v;
        if (tr) {
            if constexpr (WT<T>::H) {
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    *reinterpret_cast<uint16_t*>(tr + (d0 + j) * ST + row * 2) = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
            } else {
                const f32x4 e = __builtin_bit_cast(f32x4, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<float*>(tr + (d0 + j) * ST + row * 4) = e[j];
            }
        }
    }
}

// the d-chunk that slot i of half h (= lane >> 5) feeds to the first product: 16-bit, MFMA step i contracts d in [16 i, 16 i + 16), eight
// per half; f32, half h owns d in [32 h, 32 h + 32) and step (i, e) contracts d = 4 i + e of both halves
template <typename T>
__device__ __forceinline__ int first_chunk(int i, int h) {
    return WT<T>::H ? (2 * i + h) : (8 * h + i);
}

// lane-side block: this lane's row (r = lane & 31), the d-chunks its half feeds to the MFMA
template <typename T>
__device__ __forceinline__ void load_lane_block(uint4 (&out)[WT<T>::NA1], const T* g, int64_t ld, int row, bool valid, int dh, int h) {
#pragma unroll
    for (int i = 0; i < WT<T>::NA1; ++i) {
        const int d0 = first_chunk<T>(i, h) * WT<T>::EPC;
        out[i] = (valid && d0 < dh) ? *reinterpret_cast<const uint4*>(g + (int64_t)row * ld + d0) : make_uint4(0, 0, 0, 0);
    }
}

// A operand of the first product from the natural image: tile row `row`, contraction over d
template <typename T>
__device__ __forceinline__ void read_nat(uint4 (&a)[WT<T>::NA1], const char* nat, int row, int h) {
#pragma unroll
    for (int i = 0; i < WT<T>::NA1; ++i) a[i] = *reinterpret_cast<const uint4*>(nat + nat_off<T>(row, first_chunk<T>(i, h)));
}

// A operand of the second product from the transposed image: row d (0..63), contraction over the 32 reg-side rows of sub-tile t, in the
// order the accumulator registers of the first product present them (register 4 g + e holds reg-side row 8 g + 4 h + e)
template <typename T>
__device__ __forceinline__ void read_tr(uint4 (&a)[WT<T>::NA2], const char* tr, int d, int h, int t) {
    constexpr int ST = WT<T>::TR_STRIDE;
    if constexpr (WT<T>::H) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int col = 32 * t + 16 * s + 4 * h;
            const uint2 p0 = *reinterpret_cast<const uint2*>(tr + d * ST + col * 2);
            const uint2 p1 = *reinterpret_cast<const uint2*>(tr + d * ST + (col + 8) * 2);
            a[s] = make_uint4(p0.x, p0.y, p1.x, p1.y);
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = 32 * t + 8 * g + 4 * h;
            a[g] = *reinterpret_cast<const uint4*>(tr + d * ST + col * 4);
        }
    }
}

template <typename T>
__device__ __forceinline__ void mma_first(f32x16& acc, const uint4 (&a)[WT<T>::NA1], const uint4 (&b)[WT<T>::NA1]) {
    if constexpr (WT<T>::H) {
        typedef typename H16<T>::v8 v8;
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = H16<T>::mfma32(__builtin_bit_cast(v8, a[s]), __builtin_bit_cast(v8, b[s]), acc);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f32x4 af = __builtin_bit_cast(f32x4, a[j]), bf = __builtin_bit_cast(f32x4, b[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
        }
    }
}

// the accumulator tile of the first product as the B operand of the second: rounded to T once, used for both d-tiles
template <typename T>
__device__ __forceinline__ void acc_operand(uint4 (&b)[WT<T>::NA2], const f32x16& x) {
    if constexpr (WT<T>::H) {
        typedef typename H16<T>::v4 v4;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const v4 lo = H16<T>::cvt4(f32x4{x[8 * s + 0], x[8 * s + 1], x[8 * s + 2], x[8 * s + 3]});
            const v4 hi = H16<T>::cvt4(f32x4{x[8 * s + 4], x[8 * s + 5], x[8 * s + 6], x[8 * s + 7]});
            const uint2 l = __builtin_bit_cast(uint2, lo), u = __builtin_bit_cast(uint2, hi);
            b[s] = make_uint4(l.x, l.y, u.x, u.y);
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) b[g] = __builtin_bit_cast(uint4, f32x4{x[4 * g + 0], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]});
    }
}

// acc += A_tr * X
template <typename T>
__device__ __forceinline__ void mma_second(f32x16& acc, const uint4 (&a)[WT<T>::NA2], const uint4 (&b)[WT<T>::NA2]) {
    if constexpr (WT<T>::H) {
        typedef typename H16<T>::v8 v8;
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = H16<T>::mfma32(__builtin_bit_cast(v8, a[s]), __builtin_bit_cast(v8, b[s]), acc);
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 af = __builtin_bit_cast(f32x4, a[g]), bf = __builtin_bit_cast(f32x4, b[g]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
        }
    }
}

// both d-tiles of the second product: Y_t += trT[32 t + r][sub-tile `sub`] * x
template <typename T>
__device__ __forceinline__ void mma_second2(f32x16& y0, f32x16& y1, const char* tr, int r, int h, int sub, const f32x16& x) {
    uint4 xb[WT<T>::NA2], a[WT<T>::NA2];
    acc_operand<T>(xb, x);
    read_tr<T>(a, tr, r, h, sub);
    mma_second<T>(y0, a, xb);
    read_tr<T>(a, tr, 32 + r, h, sub);
    mma_second<T>(y1, a, xb);
}

// accumulator tile t [d - 32 t][lane row] -> out[row][d] (T), optionally scaled
template <typename T>
__device__ __forceinline__ void store_acc_T(const f32x16& acc, int t, T* out, int64_t ld, int row, bool valid, int dh, int h, float mul) {
    if (!valid) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int d0 = 32 * t + 8 * g + 4 * h;
        if (d0 < dh) {
            Vec4<T> v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v.set(e, acc[4 * g + e] * mul);
            v.store(out + (int64_t)row * ld + d0);
        }
    }
}

struct WideArgs {
    const void *q, *k, *v, *o, *d_o;
    void *out_o, *dq, *dk, *dv;
    const float* kbias;
    float *lse2, *delta;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, Lq, Lk, dh;
    float scale;
    float premul;
    // attention-probability dropout: the keep mask of attention.hip (0 or 1/(1-p) by element ((b*H + h)*Lq + q, key)) on the numerators
    // that feed P V; row sums / lse2 stay those of the undropped softmax; both backward passes regenerate it
    float drop_p, drop_inv;
    uint64_t drop_seed;
    const int64_t* drop_step;   // device step counter (drop_seed_at), or null
};

// keep-mask scale of score element (row, key); row = (b*H + h)*Lq + q
__device__ __forceinline__ float attn_drop(uint64_t seed, uint64_t row, int key, float p, float inv) {
    return dropout_scale(seed, row, (uint32_t)key, p, inv);
}

// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void attn_wide_fwd_kernel(WideArgs p) {
    const uint64_t dseed = drop_seed_at(p.drop_seed, p.drop_step);   // (one uniform load per kernel)
    __shared__ __attribute__((aligned(16))) char smem[WT<T>::NAT + WT<T>::TR + 64 * 4];
    char* sK = smem;
    char* sVt = smem + WT<T>::NAT;
    float* sbias = reinterpret_cast<float*>(smem + WT<T>::NAT + WT<T>::TR);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hh = blockIdx.y;
    const int qrow = blockIdx.x * 128 + wave * 32 + r;
    const bool qvalid = qrow < p.Lq;
    const T* Q = reinterpret_cast<const T*>(p.q) + (int64_t)b * p.Lq * p.ldq + hh * p.dh;
    const T* K = reinterpret_cast<const T*>(p.k) + (int64_t)b * p.Lk * p.ldk + hh * p.dh;
    const T* V = reinterpret_cast<const T*>(p.v) + (int64_t)b * p.Lk * p.ldv + hh * p.dh;
    const float* kb = p.kbias ? p.kbias + (int64_t)b * p.Lk : nullptr;
    const float sc = p.premul != 0.f ? 1.f : p.scale * LOG2E;
    const uint64_t drow = ((uint64_t)b * p.H + hh) * p.Lq + (qvalid ? qrow : 0);

    uint4 qb[WT<T>::NA1];
    load_lane_block<T>(qb, Q, p.ldq, qrow, qvalid, p.dh, h);

    float m = -INFINITY, l = 0.f;
    f32x16 O0, O1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { O0[i] = 0.f; O1[i] = 0.f; }

    for (int kt = 0; kt < p.Lk; kt += 64) {
        __syncthreads();
        stage_tile<T>(sK, nullptr, K, p.ldk, kt, p.Lk, p.dh, tid);
        stage_tile<T>(nullptr, sVt, V, p.ldv, kt, p.Lk, p.dh, tid);
        if (tid < 64) {
            const int key = kt + tid;
            sbias[tid] = key < p.Lk ? (kb ? kb[key] * LOG2E : 0.f) : -INFINITY;
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            f32x16 S;
#pragma unroll
            for (int i = 0; i < 16; ++i) S[i] = 0.f;
            {
                uint4 ka[WT<T>::NA1];
                read_nat<T>(ka, sK, sub * 32 + r, h);
                mma_first<T>(S, ka, qb);
            }
            float mloc = -INFINITY;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(sbias + sub * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    S[4 * g + e] = S[4 * g + e] * sc + bb[e];
                    mloc = fmaxf(mloc, S[4 * g + e]);
                }
            }
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m, mloc);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m - m_use);
            float ls = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                S[i] = __builtin_amdgcn_exp2f(S[i] - m_use);
                ls += S[i];
            }
            l = l * alpha + ls;
            m = m_new;
#pragma unroll
            for (int i = 0; i < 16; ++i) { O0[i] *= alpha; O1[i] *= alpha; }
            if (p.drop_p > 0.f) {
                const uint32_t rm = drop_row(drop_seed32(dseed), drow);
                const uint32_t thr = drop_thr16(p.drop_p);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; e += 2) {   // (the lane's keys 8g + 4h + e: an even / odd pair shares one generator call)
                        const uint32_t bits = drop_bits(rm, (uint32_t)(kt + sub * 32 + 8 * g + 4 * h + e) >> 1);
                        S[4 * g + e] *= drop_pick(bits, 0u, thr, p.drop_inv);
                        S[4 * g + e + 1] *= drop_pick(bits, 1u, thr, p.drop_inv);
                    }
            }
            mma_second2<T>(O0, O1, sVt, r, h, sub, S);
        }
    }
    const float lt = l + __shfl_xor(l, 32, 64);
    const float inv = lt > 0.f ? 1.f / lt : 0.f;
    T* Oo = reinterpret_cast<T*>(p.out_o) + (int64_t)b * p.Lq * p.ldo + hh * p.dh;
    store_acc_T<T>(O0, 0, Oo, p.ldo, qrow, qvalid, p.dh, h, inv);
    store_acc_T<T>(O1, 1, Oo, p.ldo, qrow, qvalid, p.dh, h, inv);
    if (qvalid && h == 0) p.lse2[((int64_t)b * p.H + hh) * p.Lq + qrow] = m + __builtin_amdgcn_logf(lt);
}

// delta[b,h,q] = sum_d dO[q, h*dh + d] * O[q, h*dh + d]
template <typename T>
__global__ __launch_bounds__(256) void attn_wide_delta_kernel(WideArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)p.B * p.Lq * p.H;
    if (idx >= total) return;
    const int hh = (int)(idx % p.H);
    const int64_t row = idx / p.H;  // b*Lq + q
    const int b = (int)(row / p.Lq), q = (int)(row % p.Lq);
    const T* o = reinterpret_cast<const T*>(p.o) + row * p.ldo + hh * p.dh;
    const T* d = reinterpret_cast<const T*>(p.d_o) + row * p.lddo + hh * p.dh;
    float s = 0.f;
    for (int i = 0; i < p.dh; i += 4) {
        Vec4<T> a, c;
        a.load(o + i);
        c.load(d + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += a.get(e) * c.get(e);
    }
    p.delta[((int64_t)b * p.H + hh) * p.Lq + q] = s;
}

// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void attn_wide_bwd_dq_kernel(WideArgs p) {
    const uint64_t dseed = drop_seed_at(p.drop_seed, p.drop_step);   // (one uniform load per kernel)
    __shared__ __attribute__((aligned(16))) char smem[2 * WT<T>::NAT + WT<T>::TR + 64 * 4];
    char* sK = smem;
    char* sV = smem + WT<T>::NAT;
    char* sKt = smem + 2 * WT<T>::NAT;
    float* sbias = reinterpret_cast<float*>(smem + 2 * WT<T>::NAT + WT<T>::TR);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hh = blockIdx.y;
    const int qrow = blockIdx.x * 128 + wave * 32 + r;
    const bool qvalid = qrow < p.Lq;
    const T* Q = reinterpret_cast<const T*>(p.q) + (int64_t)b * p.Lq * p.ldq + hh * p.dh;
    const T* dO = reinterpret_cast<const T*>(p.d_o) + (int64_t)b * p.Lq * p.lddo + hh * p.dh;
    const T* K = reinterpret_cast<const T*>(p.k) + (int64_t)b * p.Lk * p.ldk + hh * p.dh;
    const T* V = reinterpret_cast<const T*>(p.v) + (int64_t)b * p.Lk * p.ldv + hh * p.dh;
    const float* kb = p.kbias ? p.kbias + (int64_t)b * p.Lk : nullptr;
    const float sc = p.premul != 0.f ? 1.f : p.scale * LOG2E;
    const uint64_t drow = ((uint64_t)b * p.H + hh) * p.Lq + (qvalid ? qrow : 0);

    uint4 qb[WT<T>::NA1], dob[WT<T>::NA1];
    load_lane_block<T>(qb, Q, p.ldq, qrow, qvalid, p.dh, h);
    load_lane_block<T>(dob, dO, p.lddo, qrow, qvalid, p.dh, h);
    const int64_t sidx = ((int64_t)b * p.H + hh) * p.Lq + qrow;
    const float lse = qvalid ? p.lse2[sidx] : INFINITY;
    const float dl = qvalid ? p.delta[sidx] : 0.f;

    f32x16 dQ0, dQ1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { dQ0[i] = 0.f; dQ1[i] = 0.f; }

    for (int kt = 0; kt < p.Lk; kt += 64) {
        __syncthreads();
        stage_tile<T>(sK, sKt, K, p.ldk, kt, p.Lk, p.dh, tid);
        stage_tile<T>(sV, nullptr, V, p.ldv, kt, p.Lk, p.dh, tid);
        if (tid < 64) {
            const int key = kt + tid;
            sbias[tid] = key < p.Lk ? (kb ? kb[key] * LOG2E : 0.f) : -INFINITY;
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            f32x16 S, dP;
#pragma unroll
            for (int i = 0; i < 16; ++i) { S[i] = 0.f; dP[i] = 0.f; }
            {
                uint4 a[WT<T>::NA1];
                read_nat<T>(a, sK, sub * 32 + r, h);
                mma_first<T>(S, a, qb);
                read_nat<T>(a, sV, sub * 32 + r, h);
                mma_first<T>(dP, a, dob);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(sbias + sub * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(S[4 * g + e] * sc + bb[e] - lse);
                    float dpe = dP[4 * g + e];
                    if (p.drop_p > 0.f) dpe *= attn_drop(dseed, drow, kt + sub * 32 + 8 * g + 4 * h + e, p.drop_p, p.drop_inv);
                    S[4 * g + e] = pe * (dpe - dl) * p.scale;
                }
            }
            mma_second2<T>(dQ0, dQ1, sKt, r, h, sub, S);
        }
    }
    T* dQo = reinterpret_cast<T*>(p.dq) + (int64_t)b * p.Lq * p.lddq + hh * p.dh;
    store_acc_T<T>(dQ0, 0, dQo, p.lddq, qrow, qvalid, p.dh, h, 1.f);
    store_acc_T<T>(dQ1, 1, dQo, p.lddq, qrow, qvalid, p.dh, h, 1.f);
}

// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void attn_wide_bwd_dkdv_kernel(WideArgs p) {
    const uint64_t dseed = drop_seed_at(p.drop_seed, p.drop_step);   // (one uniform load per kernel)
    __shared__ __attribute__((aligned(16))) char smem[2 * WT<T>::NAT + 2 * WT<T>::TR + 128 * 4];
    char* sQ = smem;
    char* sdO = smem + WT<T>::NAT;
    char* sQt = smem + 2 * WT<T>::NAT;
    char* sdOt = smem + 2 * WT<T>::NAT + WT<T>::TR;
    float* slse = reinterpret_cast<float*>(smem + 2 * WT<T>::NAT + 2 * WT<T>::TR);
    float* sdl = slse + 64;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hh = blockIdx.y;
    const int krow = blockIdx.x * 128 + wave * 32 + r;
    const bool kvalid = krow < p.Lk;
    const T* Q = reinterpret_cast<const T*>(p.q) + (int64_t)b * p.Lq * p.ldq + hh * p.dh;
    const T* dO = reinterpret_cast<const T*>(p.d_o) + (int64_t)b * p.Lq * p.lddo + hh * p.dh;
    const T* K = reinterpret_cast<const T*>(p.k) + (int64_t)b * p.Lk * p.ldk + hh * p.dh;
    const T* V = reinterpret_cast<const T*>(p.v) + (int64_t)b * p.Lk * p.ldv + hh * p.dh;
    const float sc = p.premul != 0.f ? 1.f : p.scale * LOG2E;
    const float kbl = kvalid ? (p.kbias ? p.kbias[(int64_t)b * p.Lk + krow] * LOG2E : 0.f) : -INFINITY;
    const float* lse_g = p.lse2 + ((int64_t)b * p.H + hh) * p.Lq;
    const float* dl_g = p.delta + ((int64_t)b * p.H + hh) * p.Lq;

    uint4 kbk[WT<T>::NA1], vbk[WT<T>::NA1];
    load_lane_block<T>(kbk, K, p.ldk, krow, kvalid, p.dh, h);
    load_lane_block<T>(vbk, V, p.ldv, krow, kvalid, p.dh, h);

    f32x16 dK0, dK1, dV0, dV1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { dK0[i] = 0.f; dK1[i] = 0.f; dV0[i] = 0.f; dV1[i] = 0.f; }

    for (int qt = 0; qt < p.Lq; qt += 64) {
        __syncthreads();
        stage_tile<T>(sQ, sQt, Q, p.ldq, qt, p.Lq, p.dh, tid);
        stage_tile<T>(sdO, sdOt, dO, p.lddo, qt, p.Lq, p.dh, tid);
        if (tid < 64) {
            const int qi = qt + tid;
            slse[tid] = qi < p.Lq ? lse_g[qi] : INFINITY;
            sdl[tid] = qi < p.Lq ? dl_g[qi] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            f32x16 S, dP;
#pragma unroll
            for (int i = 0; i < 16; ++i) { S[i] = 0.f; dP[i] = 0.f; }
            {
                uint4 a[WT<T>::NA1];
                read_nat<T>(a, sQ, sub * 32 + r, h);
                mma_first<T>(S, a, kbk);  // S[q][key]
                read_nat<T>(a, sdO, sub * 32 + r, h);
                mma_first<T>(dP, a, vbk);  // dP[q][key] = dO V^T
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 ls = *reinterpret_cast<const f32x4*>(slse + sub * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) S[4 * g + e] = __builtin_amdgcn_exp2f(S[4 * g + e] * sc + kbl - ls[e]);
            }
            if (p.drop_p > 0.f) {   // the keep-mask scales of this block go onto P for dV and onto dP for dS
                f32x16 Pd;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int qi = min(qt + sub * 32 + 8 * g + 4 * h + e, p.Lq - 1);
                        const float ms = attn_drop(dseed, ((uint64_t)b * p.H + hh) * p.Lq + qi, kvalid ? krow : 0, p.drop_p, p.drop_inv);
                        Pd[4 * g + e] = S[4 * g + e] * ms;
                        dP[4 * g + e] *= ms;
                    }
                mma_second2<T>(dV0, dV1, sdOt, r, h, sub, Pd);  // dV^T += dO^T (P . mask)
            } else {
                mma_second2<T>(dV0, dV1, sdOt, r, h, sub, S);  // dV^T += dO^T P
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 dd = *reinterpret_cast<const f32x4*>(sdl + sub * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) S[4 * g + e] = S[4 * g + e] * (dP[4 * g + e] - dd[e]) * p.scale;
            }
            mma_second2<T>(dK0, dK1, sQt, r, h, sub, S);  // dK^T += Q^T dS
        }
    }
    T* dKo = reinterpret_cast<T*>(p.dk) + (int64_t)b * p.Lk * p.lddk + hh * p.dh;
    T* dVo = reinterpret_cast<T*>(p.dv) + (int64_t)b * p.Lk * p.lddv + hh * p.dh;
    const float kmul = p.premul != 0.f ? 1.f / p.premul : 1.f;
    store_acc_T<T>(dK0, 0, dKo, p.lddk, krow, kvalid, p.dh, h, kmul);
    store_acc_T<T>(dK1, 1, dKo, p.lddk, krow, kvalid, p.dh, h, kmul);
    store_acc_T<T>(dV0, 0, dVo, p.lddv, krow, kvalid, p.dh, h, 1.f);
    store_acc_T<T>(dV1, 1, dVo, p.lddv, krow, kvalid, p.dh, h, 1.f);
}

template <typename T>
int fwd_launch(const AttnCall& c) {
    WideArgs p{};
    attn_fill(p, c);
    dim3 grid((unsigned)((c.Lq + 127) / 128), (unsigned)c.H, (unsigned)c.B);
    hipLaunchKernelGGL(attn_wide_fwd_kernel<T>, grid, dim3(256), 0, c.stream, p);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

template <typename T>
int bwd_launch(const AttnCall& c) {
    WideArgs p{};
    attn_fill(p, c);
    const int64_t total = (int64_t)c.B * c.Lq * c.H;
    dim3 gd((unsigned)((total + 255) / 256));
    dim3 gq((unsigned)((c.Lq + 127) / 128), (unsigned)c.H, (unsigned)c.B);
    dim3 gk((unsigned)((c.Lk + 127) / 128), (unsigned)c.H, (unsigned)c.B);
    hipLaunchKernelGGL(attn_wide_delta_kernel<T>, gd, dim3(256), 0, c.stream, p);
    hipLaunchKernelGGL(attn_wide_bwd_dq_kernel<T>, gq, dim3(256), 0, c.stream, p);
    hipLaunchKernelGGL(attn_wide_bwd_dkdv_kernel<T>, gk, dim3(256), 0, c.stream, p);
    if (c.ev_prep) (void)hipEventRecord(static_cast<hipEvent_t>(c.ev_prep), c.stream);   // behind the last launch: nothing here uses a workspace
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // namespace

// a validated call (check_call) with 32 < dh <= 64
int svol_attn_wide_fwd_launch(const AttnCall& c, int dtype) {
    if (c.dh <= 32 || c.dh > 64 || c.dh % 8) return SVOL_E_UNSUPPORTED;
    return dtype == SVOL_BF16 ? fwd_launch<bf16_t>(c) : dtype == SVOL_F16 ? fwd_launch<f16_t>(c) : fwd_launch<float>(c);
}
int svol_attn_wide_bwd_launch(const AttnCall& c, int dtype) {
    if (c.dh <= 32 || c.dh > 64 || c.dh % 8) return SVOL_E_UNSUPPORTED;
    return dtype == SVOL_BF16 ? bwd_launch<bf16_t>(c) : dtype == SVOL_F16 ? bwd_launch<f16_t>(c) : bwd_launch<float>(c);
}
