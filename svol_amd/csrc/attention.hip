// Multi-head attention core for the SVOL head (gfx950 / CDNA4): flash-style forward and backward that
// never materialise the Lq x Lk score matrix (the reference's nn.MultiheadAttention writes
// [B*h, L, L] = 9.4 GiB per layer at the benchmark size; cross_modal_transformer.py:139).
//
// This file holds the C-ABI entries and ONE generic kernel template on the element type T and the number ND of 32-column
// d-tiles that span the head: ND = 1 for d_h <= 32 (d_h = 32 at the benchmark size, 8 at the CPU config), ND = 2 for
// 32 < d_h <= 64 (d_h % 8 == 0: --nheads 4 at hidden_dim 256, --hidden_dim 512 / 384 at eight heads).  All three kernels share one
// scheme built on the "swapped" product so that softmax statistics are lane-local (MI355X guide: swapped QK^T,
// accumulator-as-next-operand):
//
//   "lane side"  : a block of 32 rows held in registers as the MFMA B operand (one row per lane&31)
//   "reg side"   : 64-row tiles streamed through LDS, used as the MFMA A operand
//   first product : X[reg row][lane row] = A_tile[reg row][0:32 ND] . B_block[lane row][0:32 ND]     (contract d)
//   second product: Y_t[d][lane row]    += A_tileT[32 t + d][reg row] * f(X)[reg row][lane row]      (t < ND: one accumulator tile each)
//                   f(X) is fed straight from the accumulator registers (no LDS round trip).
//
//   forward : lane = queries, reg = keys : X = K Q^T -> P ; O^T += V^T P
//   dq      : lane = queries, reg = keys : P, dP = V dO^T -> dS ; dQ^T += K^T dS
//   dk/dv   : lane = keys, reg = queries : P, dV^T += dO^T P ; dP = dO V^T -> dS ; dK^T += Q^T dS
//
// dQ is produced by its own pass instead of fp32 atomics: with d_h = 32 there are only 64 FLOP per
// atomic byte and the chip-wide atomic rate (~1.3 TB/s) would bound the kernel (guide, Guideline 12).
//
// Columns >= d_h are zero in registers and LDS.  Plain compiler-scheduled HIP: no key split, no single pass, no atomics, no workspace —
// results are bit-reproducible, and the same under SVOL_DETERMINISTIC=1.  Softmax runs in the log2 domain with fp32 statistics; exp via
// v_exp_f32.
//
// Instances: <float, 1>, <float, 2> (v_mfma_f32_32x32x2_f32, exact fp32 — the parity mode), <bf16, 2>, <fp16, 2>
// (v_mfma_f32_32x32x16_{bf16,f16}).  16-bit operands at d_h <= 32 are dispatched to the tuned kernels of attention_bf16.hip.
//
// LDS per workgroup (bytes; 64 rows x 32 ND d natural image, [32 ND d][64 rows] transposed image with a padded row stride):
//                  natural   transposed   forward   dq       dk/dv
//   f32,    ND = 1   8192       8704       17152    25344    34304
//   16-bit, ND = 2   8192       9216       17664    25856    35328
//   f32,    ND = 2  16384      17408       34048    50432    68096     (two workgroups per CU: 136192 of 163840)
#include "attn_call.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// EPC: elements per 16-byte chunk; CPR: chunks per 32 ND-wide row; NA1: chunks a lane feeds to the first product; NA2: 16-byte operands
// of one d-tile's second product (32 reg-side rows)
template <typename T_, int ND_> struct AT {
    typedef T_ T;
    static constexpr int ND = ND_;
    static constexpr bool H = sizeof(T) == 2;
    // 16 bits at one d-tile belongs to attention_bf16.hip; the natural image's swizzle below is not the one that layout would need
    static_assert(ND == 2 || (ND == 1 && !H), "instances: <float, 1>, <float, 2>, <bf16_t, 2>, <f16_t, 2>");
    static constexpr int EPC = H ? 8 : 4, CPR = (H ? 4 : 8) * ND, NA1 = (H ? 2 : 4) * ND, NA2 = H ? 2 : 4;
    static constexpr int NAT_ROW = (H ? 64 : 128) * ND, TR_STRIDE = H ? 64 * 2 + 16 : 64 * 4 + 16;
    static constexpr int NAT = 64 * NAT_ROW, TR = 32 * ND * TR_STRIDE;
};

// ---- staging ---------------------------------------------------------------
// natural image: [64 rows][32 ND d] (zero padded), 16-byte chunks XOR-swizzled against bank conflicts
template <typename W>
__device__ __forceinline__ int nat_off(int row, int ch) {
    return row * W::NAT_ROW + ((ch ^ (row & (W::CPR - 1))) << 4);
}

// Stage 64 rows starting at row0 of a [rows, ld] matrix (head column offset already applied) into the natural image `nat` and/or the
// transposed image `tr`.
template <typename W>
__device__ __forceinline__ void stage_tile(char* nat, char* tr, const typename W::T* g, int64_t ld, int row0, int limit, int dh, int tid) {
    constexpr int EPC = W::EPC, CPR = W::CPR, ST = W::TR_STRIDE;
    for (int c = tid; c < 64 * CPR; c += 256) {
        const int row = c / CPR, ch = c % CPR;
        const int d0 = ch * EPC;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row0 + row < limit && d0 < dh) v = *reinterpret_cast<const uint4*>(g + (int64_t)(row0 + row) * ld + d0);
        if (nat) *reinterpret_cast<uint4*>(nat + nat_off<W>(row, ch)) = v;
        if (tr) {
            if constexpr (W::H) {
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
// per half; f32, half h owns d in [16 ND h, 16 ND h + 16 ND) and step (i, e) contracts d = 4 i + e of both halves
template <typename W>
__device__ __forceinline__ int first_chunk(int i, int h) {
    return W::H ? (2 * i + h) : (4 * W::ND * h + i);
}

// lane-side block: this lane's row (r = lane & 31), the d-chunks its half feeds to the MFMA
template <typename W>
__device__ __forceinline__ void load_lane_block(uint4 (&out)[W::NA1], const typename W::T* g, int64_t ld, int row, bool valid, int dh, int h) {
#pragma unroll
    for (int i = 0; i < W::NA1; ++i) {
        const int d0 = first_chunk<W>(i, h) * W::EPC;
        out[i] = (valid && d0 < dh) ? *reinterpret_cast<const uint4*>(g + (int64_t)row * ld + d0) : make_uint4(0, 0, 0, 0);
    }
}

// A operand of the first product from the natural image: tile row `row`, contraction over d
template <typename W>
__device__ __forceinline__ void read_nat(uint4 (&a)[W::NA1], const char* nat, int row, int h) {
#pragma unroll
    for (int i = 0; i < W::NA1; ++i) a[i] = *reinterpret_cast<const uint4*>(nat + nat_off<W>(row, first_chunk<W>(i, h)));
}

// A operand of the second product from the transposed image: row d (0 .. 32 ND - 1), contraction over the 32 reg-side rows of sub-tile
// t, in the order the accumulator registers of the first product present them (register 4 g + e holds reg-side row 8 g + 4 h + e)
template <typename W>
__device__ __forceinline__ void read_tr(uint4 (&a)[W::NA2], const char* tr, int d, int h, int t) {
    constexpr int ST = W::TR_STRIDE;
    if constexpr (W::H) {
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

template <typename W>
__device__ __forceinline__ void mma_first(f32x16& acc, const uint4 (&a)[W::NA1], const uint4 (&b)[W::NA1]) {
    if constexpr (W::H) {
        typedef typename H16<typename W::T>::v8 v8;
#pragma unroll
        for (int s = 0; s < 2 * W::ND; ++s) acc = H16<typename W::T>::mfma32(__builtin_bit_cast(v8, a[s]), __builtin_bit_cast(v8, b[s]), acc);
    } else {
#pragma unroll
        for (int j = 0; j < 4 * W::ND; ++j) {
            const f32x4 af = __builtin_bit_cast(f32x4, a[j]), bf = __builtin_bit_cast(f32x4, b[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
        }
    }
}

// the accumulator tile of the first product as the B operand of the second: rounded to T once, used for every d-tile
template <typename W>
__device__ __forceinline__ void acc_operand(uint4 (&b)[W::NA2], const f32x16& x) {
    if constexpr (W::H) {
        typedef H16<typename W::T> HT;
        typedef typename HT::v4 v4;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const v4 lo = HT::cvt4(f32x4{x[8 * s + 0], x[8 * s + 1], x[8 * s + 2], x[8 * s + 3]});
            const v4 hi = HT::cvt4(f32x4{x[8 * s + 4], x[8 * s + 5], x[8 * s + 6], x[8 * s + 7]});
            const uint2 l = __builtin_bit_cast(uint2, lo), u = __builtin_bit_cast(uint2, hi);
            b[s] = make_uint4(l.x, l.y, u.x, u.y);
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) b[g] = __builtin_bit_cast(uint4, f32x4{x[4 * g + 0], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]});
    }
}

// acc += A_tr * X
template <typename W>
__device__ __forceinline__ void mma_second(f32x16& acc, const uint4 (&a)[W::NA2], const uint4 (&b)[W::NA2]) {
    if constexpr (W::H) {
        typedef typename H16<typename W::T>::v8 v8;
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = H16<typename W::T>::mfma32(__builtin_bit_cast(v8, a[s]), __builtin_bit_cast(v8, b[s]), acc);
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 af = __builtin_bit_cast(f32x4, a[g]), bf = __builtin_bit_cast(f32x4, b[g]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
        }
    }
}

// The accumulator tiles of a second product, Y_t[d - 32 t][lane row].  Two named tiles, not f32x16[ND]: under the array the compiler
// assigns the two-tile kernels' registers differently, which cost the 16-bit dQ kernel 1.2 % (profiles/attn_generic.md).  At ND = 1
// nothing reads t1 and what the kernels do to it is dead code.
struct Tiles {
    f32x16 t0, t1;
    __device__ __forceinline__ void fill(float x) {
#pragma unroll
        for (int i = 0; i < 16; ++i) { t0[i] = x; t1[i] = x; }
    }
};

// every d-tile of the second product: Y_t += trT[32 t + r][sub-tile `sub`] * x
template <typename W>
__device__ __forceinline__ void mma_second_tiles(Tiles& y, const char* tr, int r, int h, int sub, const f32x16& x) {
    uint4 xb[W::NA2], a[W::NA2];
    acc_operand<W>(xb, x);
    read_tr<W>(a, tr, r, h, sub);
    mma_second<W>(y.t0, a, xb);
    if constexpr (W::ND > 1) {
        read_tr<W>(a, tr, 32 + r, h, sub);
        mma_second<W>(y.t1, a, xb);
    }
}

// accumulator tile t -> out[row][32 t + d] (T), optionally scaled
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
template <typename W>
__device__ __forceinline__ void store_tiles(const Tiles& y, typename W::T* out, int64_t ld, int row, bool valid, int dh, int h, float mul) {
    store_acc_T(y.t0, 0, out, ld, row, valid, dh, h, mul);
    if constexpr (W::ND > 1) store_acc_T(y.t1, 1, out, ld, row, valid, dh, h, mul);
}

struct AttnArgs {
    const void *q, *k, *v, *o, *d_o;
    void *out_o, *dq, *dk, *dv;
    const float* kbias;
    float *lse2, *delta;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, Lq, Lk, dh;
    float scale;
    float premul;
    // attention-probability dropout (nn.MultiheadAttention(dropout=p) in training mode, transformer.py:158-160,216-222): the
    // softmax numerators that feed P V are multiplied by a stateless keep mask (0 or 1/(1-p)) of the element index
    // ((b*H + h)*Lq + q)*Lk + key — the row sums / lse stay those of the undropped softmax; both backward passes regenerate the mask
    float drop_p, drop_inv;
    uint64_t drop_seed;
    const int64_t* drop_step;   // device step counter (drop_seed_at), or null
};

// keep-mask scale of score element (row, key); row = (b*H + h)*Lq + q
__device__ __forceinline__ float attn_drop(uint64_t seed, uint64_t row, int key, float p, float inv) {
    return dropout_scale(seed, row, (uint32_t)key, p, inv);
}
// the same for keys key0 (EVEN) and key0 + 1 of one row, onto x[i] and x[i + 1]: one generator call for the pair
__device__ __forceinline__ void attn_drop2(f32x16& x, int i, uint32_t rowmix, int key0, uint32_t thr16, float inv) {
    const uint32_t bits = drop_bits(rowmix, (uint32_t)key0 >> 1);
    x[i] *= drop_pick(bits, 0u, thr16, inv);
    x[i + 1] *= drop_pick(bits, 1u, thr16, inv);
}

// ---------------------------------------------------------------------------
template <typename T, int ND>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnArgs p) {
    typedef AT<T, ND> W;
    const uint64_t dseed = drop_seed_at(p.drop_seed, p.drop_step);   // (one uniform load per kernel)
    __shared__ __attribute__((aligned(16))) char smem[W::NAT + W::TR + 64 * 4];
    char* sK = smem;
    char* sVt = smem + W::NAT;
    float* sbias = reinterpret_cast<float*>(smem + W::NAT + W::TR);

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

    uint4 qb[W::NA1];
    load_lane_block<W>(qb, Q, p.ldq, qrow, qvalid, p.dh, h);

    float m = -INFINITY, l = 0.f;
    Tiles O;
    O.fill(0.f);

    for (int kt = 0; kt < p.Lk; kt += 64) {
        __syncthreads();
        stage_tile<W>(sK, nullptr, K, p.ldk, kt, p.Lk, p.dh, tid);
        stage_tile<W>(nullptr, sVt, V, p.ldv, kt, p.Lk, p.dh, tid);
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
                uint4 ka[W::NA1];
                read_nat<W>(ka, sK, sub * 32 + r, h);
                mma_first<W>(S, ka, qb);
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
            for (int i = 0; i < 16; ++i) { O.t0[i] *= alpha; O.t1[i] *= alpha; }
            if (p.drop_p > 0.f) {
                const uint32_t rm = drop_row(drop_seed32(dseed), drow);
                const uint32_t thr = drop_thr16(p.drop_p);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; e += 2) {   // (the lane's keys 8g + 4h + e: an even / odd pair shares one generator call)
                        attn_drop2(S, 4 * g + e, rm, kt + sub * 32 + 8 * g + 4 * h + e, thr, p.drop_inv);
                    }
            }
            mma_second_tiles<W>(O, sVt, r, h, sub, S);
        }
    }
    const float lt = l + __shfl_xor(l, 32, 64);
    const float inv = lt > 0.f ? 1.f / lt : 0.f;
    T* Oo = reinterpret_cast<T*>(p.out_o) + (int64_t)b * p.Lq * p.ldo + hh * p.dh;
    store_tiles<W>(O, Oo, p.ldo, qrow, qvalid, p.dh, h, inv);
    if (qvalid && h == 0) p.lse2[((int64_t)b * p.H + hh) * p.Lq + qrow] = m + __builtin_amdgcn_logf(lt);
}

// delta[b,h,q] = sum_d dO[q, h*dh + d] * O[q, h*dh + d]
template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(AttnArgs p) {
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
template <typename T, int ND>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(AttnArgs p) {
    typedef AT<T, ND> W;
    const uint64_t dseed = drop_seed_at(p.drop_seed, p.drop_step);   // (one uniform load per kernel)
    __shared__ __attribute__((aligned(16))) char smem[2 * W::NAT + W::TR + 64 * 4];
    char* sK = smem;
    char* sV = smem + W::NAT;
    char* sKt = smem + 2 * W::NAT;
    float* sbias = reinterpret_cast<float*>(smem + 2 * W::NAT + W::TR);

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

    uint4 qb[W::NA1], dob[W::NA1];
    load_lane_block<W>(qb, Q, p.ldq, qrow, qvalid, p.dh, h);
    load_lane_block<W>(dob, dO, p.lddo, qrow, qvalid, p.dh, h);
    const int64_t sidx = ((int64_t)b * p.H + hh) * p.Lq + qrow;
    const float lse = qvalid ? p.lse2[sidx] : INFINITY;
    const float dl = qvalid ? p.delta[sidx] : 0.f;

    Tiles dQ;
    dQ.fill(0.f);

    for (int kt = 0; kt < p.Lk; kt += 64) {
        __syncthreads();
        stage_tile<W>(sK, sKt, K, p.ldk, kt, p.Lk, p.dh, tid);
        stage_tile<W>(sV, nullptr, V, p.ldv, kt, p.Lk, p.dh, tid);
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
                uint4 a[W::NA1];
                read_nat<W>(a, sK, sub * 32 + r, h);
                mma_first<W>(S, a, qb);
                read_nat<W>(a, sV, sub * 32 + r, h);
                mma_first<W>(dP, a, dob);
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
            mma_second_tiles<W>(dQ, sKt, r, h, sub, S);
        }
    }
    T* dQo = reinterpret_cast<T*>(p.dq) + (int64_t)b * p.Lq * p.lddq + hh * p.dh;
    store_tiles<W>(dQ, dQo, p.lddq, qrow, qvalid, p.dh, h, 1.f);
}

// ---------------------------------------------------------------------------
template <typename T, int ND>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkdv_kernel(AttnArgs p) {
    typedef AT<T, ND> W;
    const uint64_t dseed = drop_seed_at(p.drop_seed, p.drop_step);   // (one uniform load per kernel)
    __shared__ __attribute__((aligned(16))) char smem[2 * W::NAT + 2 * W::TR + 128 * 4];
    char* sQ = smem;
    char* sdO = smem + W::NAT;
    char* sQt = smem + 2 * W::NAT;
    char* sdOt = smem + 2 * W::NAT + W::TR;
    float* slse = reinterpret_cast<float*>(smem + 2 * W::NAT + 2 * W::TR);
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

    uint4 kbk[W::NA1], vbk[W::NA1];
    load_lane_block<W>(kbk, K, p.ldk, krow, kvalid, p.dh, h);
    load_lane_block<W>(vbk, V, p.ldv, krow, kvalid, p.dh, h);

    Tiles dK, dV;
    dK.fill(0.f);
    dV.fill(0.f);

    for (int qt = 0; qt < p.Lq; qt += 64) {
        __syncthreads();
        stage_tile<W>(sQ, sQt, Q, p.ldq, qt, p.Lq, p.dh, tid);
        stage_tile<W>(sdO, sdOt, dO, p.lddo, qt, p.Lq, p.dh, tid);
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
                uint4 a[W::NA1];
                read_nat<W>(a, sQ, sub * 32 + r, h);
                mma_first<W>(S, a, kbk);  // S[q][key]
                read_nat<W>(a, sdO, sub * 32 + r, h);
                mma_first<W>(dP, a, vbk);  // dP[q][key] = dO V^T
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 ls = *reinterpret_cast<const f32x4*>(slse + sub * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) S[4 * g + e] = __builtin_amdgcn_exp2f(S[4 * g + e] * sc + kbl - ls[e]);
            }
            f32x16 Pd = S;   // P as the dV product takes it
            if (p.drop_p > 0.f) {   // the keep-mask scales of this block go onto P for dV and onto dP for dS
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int qi = min(qt + sub * 32 + 8 * g + 4 * h + e, p.Lq - 1);
                        const float ms = attn_drop(dseed, ((uint64_t)b * p.H + hh) * p.Lq + qi, kvalid ? krow : 0, p.drop_p, p.drop_inv);
                        Pd[4 * g + e] = S[4 * g + e] * ms;
                        dP[4 * g + e] *= ms;
                    }
            }
            mma_second_tiles<W>(dV, sdOt, r, h, sub, Pd);  // dV^T += dO^T (P . mask)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 dd = *reinterpret_cast<const f32x4*>(sdl + sub * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) S[4 * g + e] = S[4 * g + e] * (dP[4 * g + e] - dd[e]) * p.scale;
            }
            mma_second_tiles<W>(dK, sQt, r, h, sub, S);  // dK^T += Q^T dS
        }
    }
    T* dKo = reinterpret_cast<T*>(p.dk) + (int64_t)b * p.Lk * p.lddk + hh * p.dh;
    T* dVo = reinterpret_cast<T*>(p.dv) + (int64_t)b * p.Lk * p.lddv + hh * p.dh;
    store_tiles<W>(dK, dKo, p.lddk, krow, kvalid, p.dh, h, p.premul != 0.f ? 1.f / p.premul : 1.f);
    store_tiles<W>(dV, dVo, p.lddv, krow, kvalid, p.dh, h, 1.f);
}

// a validated call (check_call): dh <= 32 ND
template <typename T, int ND>
int fwd_launch(const AttnCall& c) {
    AttnArgs p{};
    attn_fill(p, c);
    dim3 grid((unsigned)((c.Lq + 127) / 128), (unsigned)c.H, (unsigned)c.B);
    hipLaunchKernelGGL((attn_fwd_kernel<T, ND>), grid, dim3(256), 0, c.stream, p);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

template <typename T, int ND>
int bwd_launch(const AttnCall& c) {
    AttnArgs p{};
    attn_fill(p, c);
    const int64_t total = (int64_t)c.B * c.Lq * c.H;
    dim3 gd((unsigned)((total + 255) / 256));
    dim3 gq((unsigned)((c.Lq + 127) / 128), (unsigned)c.H, (unsigned)c.B);
    dim3 gk((unsigned)((c.Lk + 127) / 128), (unsigned)c.H, (unsigned)c.B);
    hipLaunchKernelGGL(attn_delta_kernel<T>, gd, dim3(256), 0, c.stream, p);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<T, ND>), gq, dim3(256), 0, c.stream, p);
    hipLaunchKernelGGL((attn_bwd_dkdv_kernel<T, ND>), gk, dim3(256), 0, c.stream, p);
    if (c.ev_prep) (void)hipEventRecord(static_cast<hipEvent_t>(c.ev_prep), c.stream);   // behind the last launch: nothing here uses a workspace
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int check_common(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, int dtype) {
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || dh <= 0) return SVOL_E_INVALID;
    if (!svol_is16(dtype) && dtype != SVOL_F32) return SVOL_E_INVALID;
    if (dh > 64 || dh % 8) return SVOL_E_UNSUPPORTED;
    if (B > 65535 || H > 65535 || Lq > (1 << 24) || Lk > (1 << 24)) return SVOL_E_UNSUPPORTED;
    return SVOL_OK;
}
bool ld_ok(int64_t ld, int dtype) { return ld % (svol_is16(dtype) ? 8 : 4) == 0; }

// validates one call (a forward's four operands or a backward's eight) and stores the dims once they are known to fit
int check_call(AttnCall& c, bool bwd, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, int dtype) {
    const void* ptr[8] = {c.q, c.k, c.v, bwd ? c.o : c.out_o, c.d_o, c.dq, c.dk, c.dv};
    const int64_t ld[8] = {c.ldq, c.ldk, c.ldv, c.ldo, c.lddo, c.lddq, c.lddk, c.lddv};
    bool null = !c.lse2 || (bwd && !c.delta), ld_bad = false, unaligned = false;
    for (int i = 0; i < (bwd ? 8 : 4); ++i) {
        null |= !ptr[i];
        ld_bad |= !ld_ok(ld[i], dtype);
        unaligned |= !aligned16(ptr[i]);
    }
    if (null || !(c.drop_p >= 0.f && c.drop_p < 1.f)) return SVOL_E_INVALID;
    if (const int rc = check_common(B, H, Lq, Lk, dh, dtype)) return rc;
    if (ld_bad) return SVOL_E_UNSUPPORTED;
    if (unaligned) return SVOL_E_INVALID;
    c.B = (int)B; c.H = (int)H; c.Lq = (int)Lq; c.Lk = (int)Lk; c.dh = (int)dh;
    if (!aligned16(c.ws)) c.ws = nullptr;
    return SVOL_OK;
}

}  // namespace

extern "C" {

int64_t svol_attn_ws_bytes(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh) {
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || dh <= 0 || B > (1 << 24) || Lq > (1 << 24) || Lk > (1 << 24)) return 0;
    if (dh > 32) return 0;   // the generic kernels use no workspace
    return 4 * svol_attn_ws_floats_bf16((int)B, (int)H, (int)Lq, (int)Lk, (int)dh);
}

int svol_attn_fwd_dropout_sd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                             int64_t ldo, float* lse2, const float* kbias, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh,
                             float scale, float q_premul, void* ws, int64_t ws_bytes, float dropout_p, uint64_t seed,
                             const int64_t* seed_step_dev, int dtype, void* stream) {
    AttnCall c{};
    c.q = q; c.k = k; c.v = v; c.out_o = o; c.lse2 = lse2; c.kbias = kbias;
    c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.ldo = ldo;
    c.scale = scale; c.premul = q_premul; c.ws = static_cast<float*>(ws); c.ws_bytes = ws_bytes;
    c.drop_p = dropout_p; c.drop_seed = seed; c.drop_step = seed_step_dev; c.stream = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = check_call(c, false, B, H, Lq, Lk, dh, dtype)) return rc;
    if (dh > 32) return dtype == SVOL_BF16 ? fwd_launch<bf16_t, 2>(c) : dtype == SVOL_F16 ? fwd_launch<f16_t, 2>(c) : fwd_launch<float, 2>(c);
    if (svol_is16(dtype)) return (dtype == SVOL_BF16 ? svol_attn_fwd_bf16_launch : svol_attn_fwd_f16_launch)(c);
    return fwd_launch<float, 1>(c);
}
int svol_attn_fwd_dropout(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                          int64_t ldo, float* lse2, const float* kbias, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh,
                          float scale, float q_premul, void* ws, int64_t ws_bytes, float dropout_p, uint64_t seed, int dtype,
                          void* stream) {
    return svol_attn_fwd_dropout_sd(q, ldq, k, ldk, v, ldv, o, ldo, lse2, kbias, B, H, Lq, Lk, dh, scale, q_premul, ws, ws_bytes,
                                    dropout_p, seed, nullptr, dtype, stream);
}
int svol_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                  int64_t ldo, float* lse2, const float* kbias, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh,
                  float scale, float q_premul, void* ws, int64_t ws_bytes, int dtype, void* stream) {
    return svol_attn_fwd_dropout(q, ldq, k, ldk, v, ldv, o, ldo, lse2, kbias, B, H, Lq, Lk, dh, scale, q_premul, ws, ws_bytes, 0.f, 0,
                                 dtype, stream);
}

static int attn_bwd_impl(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                         int64_t ldo, const void* d_o, int64_t lddo, const float* lse2, float* delta, const float* kbias, void* dq,
                         int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t B, int64_t H, int64_t Lq, int64_t Lk,
                         int64_t dh, float scale, float q_premul, void* ws, int64_t ws_bytes, float drop_p, uint64_t drop_seed,
                         const int64_t* drop_step, int dtype, void* stream, int flags = 0, void* ev_prep = nullptr) {
    AttnCall c{};
    c.q = q; c.k = k; c.v = v; c.o = o; c.d_o = d_o; c.lse2 = const_cast<float*>(lse2); c.delta = delta; c.kbias = kbias;
    c.dq = dq; c.dk = dk; c.dv = dv;
    c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.ldo = ldo; c.lddo = lddo; c.lddq = lddq; c.lddk = lddk; c.lddv = lddv;
    c.scale = scale; c.premul = q_premul; c.ws = static_cast<float*>(ws); c.ws_bytes = ws_bytes;
    c.drop_p = drop_p; c.drop_seed = drop_seed; c.drop_step = drop_step; c.flags = flags; c.ev_prep = ev_prep; c.stream = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = check_call(c, true, B, H, Lq, Lk, dh, dtype)) return rc;
    // (the generic kernels keep no dQ image: SVOL_ATTN_DQ_PREZEROED means nothing to them)
    if (dh > 32) return dtype == SVOL_BF16 ? bwd_launch<bf16_t, 2>(c) : dtype == SVOL_F16 ? bwd_launch<f16_t, 2>(c) : bwd_launch<float, 2>(c);
    if (svol_is16(dtype)) return (dtype == SVOL_BF16 ? svol_attn_bwd_bf16_launch : svol_attn_bwd_f16_launch)(c);
    return bwd_launch<float, 1>(c);
}

int svol_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                  int64_t ldo, const void* d_o, int64_t lddo, const float* lse2, float* delta, const float* kbias, void* dq,
                  int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t B, int64_t H, int64_t Lq, int64_t Lk,
                  int64_t dh, float scale, float q_premul, void* ws, int64_t ws_bytes, int dtype, void* stream) {
    return attn_bwd_impl(q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, lse2, delta, kbias, dq, lddq, dk, lddk, dv, lddv, B, H, Lq, Lk, dh,
                         scale, q_premul, ws, ws_bytes, 0.f, 0, nullptr, dtype, stream);
}
int svol_attn_bwd_ex(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                     int64_t ldo, const void* d_o, int64_t lddo, const float* lse2, float* delta, const float* kbias, void* dq,
                     int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t B, int64_t H, int64_t Lq, int64_t Lk,
                     int64_t dh, float scale, float q_premul, void* ws, int64_t ws_bytes, int dtype, int flags, void* ev_prep,
                     void* stream) {
    if (flags & ~SVOL_ATTN_DQ_PREZEROED) return SVOL_E_INVALID;
    return attn_bwd_impl(q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, lse2, delta, kbias, dq, lddq, dk, lddk, dv, lddv, B, H, Lq, Lk, dh,
                         scale, q_premul, ws, ws_bytes, 0.f, 0, nullptr, dtype, stream, flags, ev_prep);
}
int64_t svol_attn_bwd_sp_image_bytes(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, int64_t ws_bytes, int dtype) {
    if (!svol_is16(dtype) || dh > 32 || check_common(B, H, Lq, Lk, dh, dtype)) return 0;
    return (dtype == SVOL_BF16 ? svol_attn_sp_image_bytes_bf16 : svol_attn_sp_image_bytes_f16)((int)B, (int)H, (int)Lq, (int)Lk, (int)dh,
                                                                                              ws_bytes);
}
int svol_attn_bwd_zero_ws(void* ws, int64_t ws_bytes, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, int dtype, void* stream) {
    if (!ws || !aligned16(ws)) return SVOL_E_INVALID;
    if (!svol_is16(dtype)) return SVOL_E_UNSUPPORTED;
    const int rc = check_common(B, H, Lq, Lk, dh, dtype);
    if (rc) return rc;
    if (dh > 32) return SVOL_E_UNSUPPORTED;   // no single-pass plan, no dQ image at the wide head widths
    return (dtype == SVOL_BF16 ? svol_attn_sp_zero_bf16_launch : svol_attn_sp_zero_f16_launch)(
        static_cast<float*>(ws), ws_bytes, (int)B, (int)H, (int)Lq, (int)Lk, (int)dh, reinterpret_cast<hipStream_t>(stream));
}
int svol_attn_bwd_dropout(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                          int64_t ldo, const void* d_o, int64_t lddo, const float* lse2, float* delta, const float* kbias, void* dq,
                          int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t B, int64_t H, int64_t Lq, int64_t Lk,
                          int64_t dh, float scale, float q_premul, void* ws, int64_t ws_bytes, float dropout_p, uint64_t seed,
                          int dtype, void* stream) {
    return attn_bwd_impl(q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, lse2, delta, kbias, dq, lddq, dk, lddk, dv, lddv, B, H, Lq, Lk, dh,
                         scale, q_premul, ws, ws_bytes, dropout_p, seed, nullptr, dtype, stream);
}
int svol_attn_bwd_dropout_sd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                             int64_t ldo, const void* d_o, int64_t lddo, const float* lse2, float* delta, const float* kbias,
                             void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t B, int64_t H, int64_t Lq,
                             int64_t Lk, int64_t dh, float scale, float q_premul, void* ws, int64_t ws_bytes, float dropout_p,
                             uint64_t seed, const int64_t* seed_step_dev, int dtype, void* stream) {
    return attn_bwd_impl(q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, lse2, delta, kbias, dq, lddq, dk, lddk, dv, lddv, B, H, Lq, Lk, dh,
                         scale, q_premul, ws, ws_bytes, dropout_p, seed, seed_step_dev, dtype, stream);
}

}  // extern "C"
