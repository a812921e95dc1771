// ViT-B/16 feature extractor pieces (Hugging Face ViTModel semantics; forward, and the attention backward of the
// trainable extractor):
//
//   svol_patchify        pixel_values [n,C,H,W] fp32 -> patch rows [n*P, C*p*p] (the im2col of the stride-p conv, in the
//                        conv weight's own (c, ky, kx) order) so that the patch embedding is ONE MFMA GEMM
//   svol_vit_embed       tokens = [cls; patch_proj] + position embeddings, fp32 residual stream + compute-dtype copy
//   svol_attn_small_fwd  softmax(Q K^T / sqrt(d_h)) V for SHORT sequences (L <= 256: 197 tokens per image), d_h = 32 or
//                        64, bf16 or fp16 operands (the kernels are templates on the operand type; the fp16 instances sit behind
//                        the *_h16 entry points).  One workgroup per (image, head): K and V sit in LDS once (row-major images with
//                        XOR-swizzled 16-byte chunks, V read back through ds_read_b64_tr_b16), a wave owns 32 queries
//                        at a time with the WHOLE score row of its query in registers (<= 8 accumulator tiles), so the
//                        softmax is a plain two-pass one — no running maximum, no rescale; swapped products keep the
//                        statistics lane-local and feed P to the second MFMA straight from the accumulators, as in
//                        attention_bf16.hip.  Attention is 4 % of ViT-B's FLOPs; the GEMMs (gemm_bf16.hip) carry it.
//   svol_attn_small_fwd_lse  the same forward, plus lse2 per query (template flag: the plain forward's code is untouched)
//   svol_attn_small_bwd      its backward, one workgroup per (image, head) (see attn_small_bwd_kernel)
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// ---- patchify -------------------------------------------------------------------------------------------------
// one thread per (patch, c, ky): 16-float contiguous read (p = 16 -> kx run), p outputs
template <typename T>
__global__ void patchify_kernel(const float* __restrict__ pix, T* __restrict__ out, int n, int C, int H, int W, int p) {
    const int gw = W / p, gh = H / p;
    const int64_t total = (int64_t)n * gh * gw * C * p;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ky = (int)(i % p);
    const int c = (int)((i / p) % C);
    const int64_t patch = i / ((int64_t)p * C);
    const int px = (int)(patch % gw), py = (int)((patch / gw) % gh);
    const int64_t img = patch / ((int64_t)gw * gh);
    const float* src = pix + ((img * C + c) * H + (py * p + ky)) * (int64_t)W + px * p;
    T* dst = out + patch * ((int64_t)C * p * p) + ((int64_t)c * p + ky) * p;
    for (int kx = 0; kx < p; ++kx) dst[kx] = from_f32<T>(src[kx]);
}

// ---- cls + position embeddings ----------------------------------------------------------------------------------
template <typename T>
__global__ void vit_embed_kernel(const float* __restrict__ proj, const float* __restrict__ cls, const float* __restrict__ pos,
                                 float* __restrict__ x32, T* __restrict__ x, int64_t n, int P, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per 4 channels
    const int64_t total = n * (P + 1) * (D / 4);
    if (i >= total) return;
    const int c = (int)(i % (D / 4)) * 4;
    const int64_t row = i / (D / 4);
    const int tok = (int)(row % (P + 1));
    const int64_t img = row / (P + 1);
    const f32x4 pe = *reinterpret_cast<const f32x4*>(pos + (int64_t)tok * D + c);
    const f32x4 src = tok == 0 ? *reinterpret_cast<const f32x4*>(cls + c)
                               : *reinterpret_cast<const f32x4*>(proj + (img * P + tok - 1) * D + c);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = src[e] + pe[e];
    *reinterpret_cast<f32x4*>(x32 + row * D + c) = v;
    if (x) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[row * D + c + e] = from_f32<T>(v[e]);
    }
}

// ---- short-sequence attention -------------------------------------------------------------------------------------
// T = bf16_t or f16_t, the operand type (H16<T> of common.h: the MFMA, the transposed LDS read, the packed conversion).  Nothing between
// the two products is rounded to T but P <= 1 and dS = P (dP - delta), |dS| <= 2 max |dP|; the padded key lanes of the backward's
// key-stationary phase hold P = exp2(0 - lse2), inf as a bf16 operand from lse2 <= -128 and as an fp16 operand from lse2 <= -16: a B
// column that only reaches the output column of the same padded key, which is never stored.
template <typename T>
struct SmallArgs {
    const T *q, *k, *v;
    T* o;
    int64_t ldq, ldk, ldv, ldo;
    int H, L, nkb;  // nkb = ceil(L / 32) <= 8
    float scale_log2e;
    float* lse2;    // [n_seq, H, L] log2-sum-exp of the scaled scores (LSE instantiation only)
};
// image: row-major, DH bf16 per row (DH*2 bytes = DH/8 chunks of 16 bytes), chunk index XOR-ed with the row
// 16 bytes from global memory, or zeros (a branch, not a select between the source and a zero local: that select puts the
// local on the scratch stack and turns every staging load into a flat load)
template <typename T> __device__ __forceinline__ uint4 ld16_or_zero(const T* src, bool valid) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (valid) v = *reinterpret_cast<const uint4*>(src);
    return v;
}

template <int DH> __device__ __forceinline__ int img_off(int row, int ch) {
    constexpr int CPR = DH / 8;
    return row * (DH * 2) + (((ch ^ (row >> (DH == 32 ? 2 : 0))) & (CPR - 1)) << 4);
}

template <typename T> __device__ __forceinline__ typename H16<T>::v8 as_v8(const uint4& x) { return __builtin_bit_cast(typename H16<T>::v8, x); }

// A operand [row = column db*32 + (lane & 31) of the image][k = image rows r0 + 8(j>>2) + 4h + (j&3)]: per 16-lane group, lane 4q+pp
// supplies the address of image row q (of 4), columns 4pp..4pp+3 of its 16-column group
template <typename T, int DH> __device__ __forceinline__ typename H16<T>::v8 tr_frag(const char* img, int r0, int db, int lane) {
    typedef typename H16<T>::lds_v4_ptr lds_ptr;
    const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pp = i16 & 3, hb = g >> 1;
    const int col = db * 32 + 16 * (g & 1) + 4 * pp;
    const int r1 = r0 + 4 * hb + q4;
    const auto lo = H16<T>::read_tr((lds_ptr)(img + img_off<DH>(r1, col >> 3) + (col & 7) * 2));
    const auto hi = H16<T>::read_tr((lds_ptr)(img + img_off<DH>(r1 + 8, col >> 3) + (col & 7) * 2));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// registers 8s .. 8s + 7 of an accumulator as a B fragment
template <typename T> __device__ __forceinline__ typename H16<T>::v8 acc_frag(const f32x16& x, int s) {
    const auto lo = H16<T>::cvt4(f32x4{x[8 * s], x[8 * s + 1], x[8 * s + 2], x[8 * s + 3]});
    const auto hi = H16<T>::cvt4(f32x4{x[8 * s + 4], x[8 * s + 5], x[8 * s + 6], x[8 * s + 7]});
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// rows of a [*, DH] output from an accumulator with the row on the lane and the columns in the registers
template <typename T, int DB> __device__ __forceinline__ void store_rows(T* out, const f32x16 (&acc)[DB], float mul, int h) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<typename H16<T>::v4*>(out + db * 32 + 8 * g + 4 * h) =
                H16<T>::cvt4(f32x4{acc[db][4 * g] * mul, acc[db][4 * g + 1] * mul, acc[db][4 * g + 2] * mul, acc[db][4 * g + 3] * mul});
}

template <typename T, int DH, bool LSE>
__global__ __launch_bounds__(256, 2) void attn_small_kernel(SmallArgs<T> p) {
    constexpr int CPR = DH / 8, KS = DH / 16, DB = DH / 32;
    constexpr int LMAX = 256;
    __shared__ __attribute__((aligned(16))) char smem[2 * LMAX * DH * 2];
    char* sK = smem;
    char* sV = smem + LMAX * DH * 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int seq = blockIdx.y, hh = blockIdx.x;
    const T* Q = p.q + (int64_t)seq * p.L * p.ldq + hh * DH;
    const T* K = p.k + (int64_t)seq * p.L * p.ldk + hh * DH;
    const T* V = p.v + (int64_t)seq * p.L * p.ldv + hh * DH;
    const int Lp = p.nkb * 32;
    // stage K and V (zero rows past L)
    for (int c = tid; c < Lp * CPR; c += 256) {
        const int row = c / CPR, ch = c % CPR;
        *reinterpret_cast<uint4*>(sK + img_off<DH>(row, ch)) = ld16_or_zero(K + (int64_t)row * p.ldk + ch * 8, row < p.L);
        *reinterpret_cast<uint4*>(sV + img_off<DH>(row, ch)) = ld16_or_zero(V + (int64_t)row * p.ldv + ch * 8, row < p.L);
    }
    __syncthreads();
    for (int qb = wave; qb < p.nkb; qb += 4) {
        const int qrow = qb * 32 + r;
        const bool qvalid = qrow < p.L;
        uint4 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            qf[ks] = ld16_or_zero(Q + (int64_t)qrow * p.ldq + ks * 16 + h * 8, qvalid);
        // scores of this lane's query against every key: S[kb][i] <-> key kb*32 + 8*(i/4) + 4*h + i%4
        f32x16 S[8];
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            if (kb < p.nkb) {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const uint4 kf = *reinterpret_cast<const uint4*>(sK + img_off<DH>(kb * 32 + r, ks * 2 + h));
                    acc = H16<T>::mfma32(as_v8<T>(kf), as_v8<T>(qf[ks]), acc);
                }
                S[kb] = acc;
            }
        }
        // mask keys >= L (only the last block can hold them), row maximum over registers then across the two half-waves
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            if (kb < p.nkb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = kb * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
                    if (key >= p.L) S[kb][i] = -INFINITY;
                    m = fmaxf(m, S[kb][i]);
                }
            }
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        const float mc = -m * p.scale_log2e;
        float l = 0.f;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            if (kb < p.nkb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    S[kb][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[kb][i], p.scale_log2e, mc));
                    l += S[kb][i];
                }
            }
        }
        l += __shfl_xor(l, 32, 64);
        // O^T[d][q] += V^T[d][keys] * P^T[keys][q]
        f32x16 O[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) O[db][i] = 0.f;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            if (kb < p.nkb) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const auto pb = acc_frag<T>(S[kb], s);
#pragma unroll
                    for (int db = 0; db < DB; ++db)   // transposed fragment of V: lane (r -> column d = db*32 + r)
                        O[db] = H16<T>::mfma32(tr_frag<T, DH>(sV, kb * 32 + 16 * s, db, lane), pb, O[db]);
                }
            }
        }
        if (qvalid) {
            const float inv = 1.f / l;
            store_rows<T, DB>(p.o + ((int64_t)seq * p.L + qrow) * p.ldo + hh * DH, O, inv, h);
            // lse2 = log2 sum_j exp2(s_j * scale_log2e) = m * scale_log2e + log2(l): P = exp2(s * scale_log2e - lse2)
            if constexpr (LSE)
                if (h == 0) p.lse2[((int64_t)seq * p.H + hh) * p.L + qrow] = -mc + log2f(l);
        }
    }
}

// ---- short-sequence attention backward ------------------------------------------------------------------------------
// One workgroup of 8 waves per (image, head) owns ALL of that head's dQ / dK / dV: no atomics, bit-reproducible.  Q, K, V and
// dO sit in LDS (same XOR-swizzled images as the forward, 4 x 32 KB at L = 256, dh = 64), with lse2 and
// delta = rowsum(dO * O) beside them (the diagonal of an MFMA dO O^T: the same chain as dP).  P = exp2(s * scale_log2e - lse2)
// and dS = P (dP - delta) are recomputed in two phases that need no barrier between them (the images are read-only after staging):
//   key-stationary    wave w owns keys [32w, 32w + 32): X = S[q][key] = mfma(Q rows, K rows) has the key on the lane and the
//                     queries in the registers, so dV^T += dO^T P and dK^T += Q^T dS take P / dS straight from the
//                     accumulators (dO^T and Q^T through ds_read_tr16_b64, as V in the forward)
//   query-stationary  wave w owns queries [32w, 32w + 32): S^T = mfma(K rows, Q rows) as in the forward (lse2 / delta lane-local),
//                     dQ^T += K^T dS^T
// Outputs are stored like the forward's O (lane = row, 4 consecutive columns per store); rows >= L are never written, padded
// keys and queries get P = 0.
template <typename T>
struct SmallBwdArgs {
    const T *q, *k, *v, *o, *dout;
    const float* lse2;
    T *dq, *dk, *dv;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int H, L, nkb;
    float scale, scale_log2e;
};

template <int DH> __device__ __forceinline__ uint4 row_frag(const char* img, int row, int ch) {
    return *reinterpret_cast<const uint4*>(img + img_off<DH>(row, ch));
}

template <typename T, int DH>
__device__ __forceinline__ void attn_small_bwd_body(const SmallBwdArgs<T>& p) {
    constexpr int CPR = DH / 8, KS = DH / 16, DB = DH / 32;
    constexpr int LMAX = 256, IMG = LMAX * DH * 2;
    __shared__ __attribute__((aligned(16))) char smem[4 * IMG];
    __shared__ __attribute__((aligned(16))) float sLse[LMAX];
    __shared__ __attribute__((aligned(16))) float sDel[LMAX];
    char* sQ = smem;
    char* sK = smem + IMG;
    char* sV = smem + 2 * IMG;
    char* sD = smem + 3 * IMG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int seq = blockIdx.y, hh = blockIdx.x;
    const int64_t row0 = (int64_t)seq * p.L;
    const T* Q = p.q + row0 * p.ldq + hh * DH;
    const T* K = p.k + row0 * p.ldk + hh * DH;
    const T* V = p.v + row0 * p.ldv + hh * DH;
    const T* O = p.o + row0 * p.ldo + hh * DH;
    const T* dO = p.dout + row0 * p.lddo + hh * DH;
    const float* lse = p.lse2 + ((int64_t)seq * p.H + hh) * p.L;
    const int Lp = p.nkb * 32;
    // this wave's O rows (block `wave`: nkb <= 8 waves have one) as MFMA B fragments, in flight while the images are staged
    const int orow = wave * 32 + r;
    uint4 ob[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) ob[ks] = ld16_or_zero(O + (int64_t)orow * p.ldo + (ks * 2 + h) * 8, orow < p.L);
    // stage Q, K, V, dO (zero rows past L)
    for (int c = tid; c < Lp * CPR; c += 512) {
        const int row = c / CPR, ch = c % CPR;
        const bool valid = row < p.L;
        const uint4 qv = ld16_or_zero(Q + (int64_t)row * p.ldq + ch * 8, valid);
        const uint4 kv = ld16_or_zero(K + (int64_t)row * p.ldk + ch * 8, valid);
        const uint4 vv = ld16_or_zero(V + (int64_t)row * p.ldv + ch * 8, valid);
        const uint4 dv = ld16_or_zero(dO + (int64_t)row * p.lddo + ch * 8, valid);
        *reinterpret_cast<uint4*>(sQ + img_off<DH>(row, ch)) = qv;
        *reinterpret_cast<uint4*>(sK + img_off<DH>(row, ch)) = kv;
        *reinterpret_cast<uint4*>(sV + img_off<DH>(row, ch)) = vv;
        *reinterpret_cast<uint4*>(sD + img_off<DH>(row, ch)) = dv;
        if (ch == 0) sLse[row] = valid ? lse[row] : 0.f;
    }
    __syncthreads();
    // delta of wave w's 32 rows = the diagonal of dO O^T, from the SAME MFMA chain that forms dP = dO V^T below: where P is one-hot,
    // O is a V row bit for bit and dP - delta is then exactly 0, which an fma chain over the same products is not.  Element [m][m]
    // sits on lane m + 32 ((m >> 2) & 1) in register 4 (m >> 3) + (m & 3).
    if (wave < p.nkb) {
        f32x16 D;
#pragma unroll
        for (int i = 0; i < 16; ++i) D[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4 da = row_frag<DH>(sD, orow, ks * 2 + h);
            D = H16<T>::mfma32(as_v8<T>(da), as_v8<T>(ob[ks]), D);
        }
        const int idx = 4 * (r >> 3) + (r & 3);
        float dl = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i == idx) dl = D[i];
        if (h == ((r >> 2) & 1)) sDel[orow] = dl;
    }
    __syncthreads();
    const float c2 = p.scale_log2e;
    // ---- key-stationary: dK, dV of this wave's 32 keys
    for (int kb = wave; kb < p.nkb; kb += 8) {
        uint4 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = row_frag<DH>(sK, kb * 32 + r, ks * 2 + h);
            vf[ks] = row_frag<DH>(sV, kb * 32 + r, ks * 2 + h);
        }
        f32x16 dVt[DB], dKt[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) dVt[db][i] = dKt[db][i] = 0.f;
        for (int qb = 0; qb < p.nkb; ++qb) {
            // X[q][key] (lane = key, register i <-> query qb*32 + 8(i>>2) + 4h + (i&3)): scores and dP = dO V^T
            f32x16 S, dP;
#pragma unroll
            for (int i = 0; i < 16; ++i) S[i] = dP[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 qa = row_frag<DH>(sQ, qb * 32 + r, ks * 2 + h);
                const uint4 da = row_frag<DH>(sD, qb * 32 + r, ks * 2 + h);
                S = H16<T>::mfma32(as_v8<T>(qa), as_v8<T>(kf[ks]), S);
                dP = H16<T>::mfma32(as_v8<T>(da), as_v8<T>(vf[ks]), dP);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q0 = qb * 32 + 8 * g + 4 * h;
                const f32x4 ls = *reinterpret_cast<const f32x4*>(sLse + q0);
                const f32x4 dl = *reinterpret_cast<const f32x4*>(sDel + q0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pv = q0 + e < p.L ? __builtin_amdgcn_exp2f(__builtin_fmaf(S[4 * g + e], c2, -ls[e])) : 0.f;
                    S[4 * g + e] = pv;
                    dP[4 * g + e] = pv * (dP[4 * g + e] - dl[e]);
                }
            }
            // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T[d][key] += Q^T[d][q] dS[q][key]
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const auto pb = acc_frag<T>(S, s), sb = acc_frag<T>(dP, s);
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    dVt[db] = H16<T>::mfma32(tr_frag<T, DH>(sD, qb * 32 + 16 * s, db, lane), pb, dVt[db]);
                    dKt[db] = H16<T>::mfma32(tr_frag<T, DH>(sQ, qb * 32 + 16 * s, db, lane), sb, dKt[db]);
                }
            }
        }
        const int key = kb * 32 + r;
        if (key < p.L) {
            store_rows<T, DB>(p.dv + (row0 + key) * p.lddv + hh * DH, dVt, 1.f, h);
            store_rows<T, DB>(p.dk + (row0 + key) * p.lddk + hh * DH, dKt, p.scale, h);
        }
    }
    // ---- query-stationary: dQ of this wave's 32 queries
    for (int qb = wave; qb < p.nkb; qb += 8) {
        const int qrow = qb * 32 + r;
        uint4 qf[KS], df[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = row_frag<DH>(sQ, qrow, ks * 2 + h);
            df[ks] = row_frag<DH>(sD, qrow, ks * 2 + h);
        }
        const float ls = sLse[qrow], dl = sDel[qrow];
        f32x16 dQt[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) dQt[db][i] = 0.f;
        for (int kb = 0; kb < p.nkb; ++kb) {
            // S^T[key][q] (lane = query, register i <-> key kb*32 + 8(i>>2) + 4h + (i&3)) and dP^T = V dO^T
            f32x16 S, dP;
#pragma unroll
            for (int i = 0; i < 16; ++i) S[i] = dP[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 ka = row_frag<DH>(sK, kb * 32 + r, ks * 2 + h);
                const uint4 va = row_frag<DH>(sV, kb * 32 + r, ks * 2 + h);
                S = H16<T>::mfma32(as_v8<T>(ka), as_v8<T>(qf[ks]), S);
                dP = H16<T>::mfma32(as_v8<T>(va), as_v8<T>(df[ks]), dP);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kb * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
                const float pv = key < p.L ? __builtin_amdgcn_exp2f(__builtin_fmaf(S[i], c2, -ls)) : 0.f;
                dP[i] = pv * (dP[i] - dl);
            }
            // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const auto sb = acc_frag<T>(dP, s);
#pragma unroll
                for (int db = 0; db < DB; ++db)
                    dQt[db] = H16<T>::mfma32(tr_frag<T, DH>(sK, kb * 32 + 16 * s, db, lane), sb, dQt[db]);
            }
        }
        if (qrow < p.L) store_rows<T, DB>(p.dq + (row0 + qrow) * p.lddq + hh * DH, dQt, p.scale, h);
    }
}

// the two instances of the body as kernels.  The fp16 one carries a name of its own: tests/test_vit_train_cli.py counts the kernels called
// attn_small_bwd_kernel in this file's code object (d_h = 32 and 64) and holds every kernel here to no scratch and no spill.
template <int DH>
__global__ __launch_bounds__(512, 1) void attn_small_bwd_kernel(SmallBwdArgs<bf16_t> p) { attn_small_bwd_body<bf16_t, DH>(p); }
template <int DH>
__global__ __launch_bounds__(512, 1) void attn_small_bwd_f16_kernel(SmallBwdArgs<f16_t> p) { attn_small_bwd_body<f16_t, DH>(p); }

}  // namespace

template <typename T>
static void attn_small_fwd_go(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                              float* lse2, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, hipStream_t s) {
    SmallArgs<T> p{(const T*)q, (const T*)k, (const T*)v, (T*)o, ldq, ldk, ldv, ldo, (int)H, (int)L, (int)((L + 31) / 32), scale * LOG2E, lse2};
    const dim3 grid((unsigned)H, (unsigned)n_seq);
    if (lse2) {
        if (dh == 64) hipLaunchKernelGGL((attn_small_kernel<T, 64, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((attn_small_kernel<T, 32, true>), grid, dim3(256), 0, s, p);
    } else {
        if (dh == 64) hipLaunchKernelGGL((attn_small_kernel<T, 64, false>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((attn_small_kernel<T, 32, false>), grid, dim3(256), 0, s, p);
    }
}

// h16: the *_h16 entry points, which take SVOL_F16 besides SVOL_BF16 (the entries without the suffix keep refusing it)
static int attn_small_launch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                             float* lse2, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream, bool h16) {
    if (!q || !k || !v || !o || n_seq <= 0 || H <= 0 || L <= 0) return SVOL_E_INVALID;
    if (!(dtype == SVOL_BF16 || (h16 && dtype == SVOL_F16)) || (dh != 32 && dh != 64) || L > 256 || n_seq > 65535) return SVOL_E_UNSUPPORTED;
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4 || !aligned16(q) || !aligned16(k) || !aligned16(v) || (reinterpret_cast<uintptr_t>(o) & 7))
        return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == SVOL_F16) attn_small_fwd_go<f16_t>(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n_seq, H, L, dh, scale, s);
    else attn_small_fwd_go<bf16_t>(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n_seq, H, L, dh, scale, s);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

static void launch_small_bwd(const SmallBwdArgs<bf16_t>& p, int64_t dh, dim3 grid, hipStream_t s) {
    if (dh == 64) hipLaunchKernelGGL(attn_small_bwd_kernel<64>, grid, dim3(512), 0, s, p);
    else hipLaunchKernelGGL(attn_small_bwd_kernel<32>, grid, dim3(512), 0, s, p);
}
static void launch_small_bwd(const SmallBwdArgs<f16_t>& p, int64_t dh, dim3 grid, hipStream_t s) {
    if (dh == 64) hipLaunchKernelGGL(attn_small_bwd_f16_kernel<64>, grid, dim3(512), 0, s, p);
    else hipLaunchKernelGGL(attn_small_bwd_f16_kernel<32>, grid, dim3(512), 0, s, p);
}

template <typename T>
static void attn_small_bwd_go(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                              const void* dout, int64_t lddo, const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                              int64_t lddv, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, hipStream_t s) {
    SmallBwdArgs<T> p{(const T*)q, (const T*)k, (const T*)v, (const T*)o, (const T*)dout, lse2, (T*)dq, (T*)dk, (T*)dv,
                      ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv, (int)H, (int)L, (int)((L + 31) / 32), scale, scale * LOG2E};
    launch_small_bwd(p, dh, dim3((unsigned)H, (unsigned)n_seq), s);
}

static int attn_small_bwd_launch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                                 const void* dout, int64_t lddo, const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                                 int64_t lddv, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream, bool h16) {
    if (!q || !k || !v || !o || !dout || !lse2 || !dq || !dk || !dv || n_seq <= 0 || H <= 0 || L <= 0) return SVOL_E_INVALID;
    if (!(dtype == SVOL_BF16 || (h16 && dtype == SVOL_F16)) || (dh != 32 && dh != 64) || L > 256 || n_seq > 65535) return SVOL_E_UNSUPPORTED;
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8 || lddo % 8 || !aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) ||
        !aligned16(dout) || (reinterpret_cast<uintptr_t>(lse2) & 3))
        return SVOL_E_UNSUPPORTED;
    if (lddq % 4 || lddk % 4 || lddv % 4 || ((reinterpret_cast<uintptr_t>(dq) | reinterpret_cast<uintptr_t>(dk) | reinterpret_cast<uintptr_t>(dv)) & 7))
        return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == SVOL_F16) attn_small_bwd_go<f16_t>(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n_seq, H, L, dh, scale, s);
    else attn_small_bwd_go<bf16_t>(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n_seq, H, L, dh, scale, s);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}


extern "C" {

int svol_patchify(const float* pixel_values, void* out, int64_t n, int64_t C, int64_t H, int64_t W, int64_t p, int dtype,
                  void* stream) {
    if (!pixel_values || !out || n <= 0 || C <= 0 || H <= 0 || W <= 0 || p <= 0) return SVOL_E_INVALID;
    if (H % p || W % p) return SVOL_E_UNSUPPORTED;
    const int64_t total = n * (H / p) * (W / p) * C * p;
    if (total > (1ll << 40)) return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == SVOL_BF16) hipLaunchKernelGGL(patchify_kernel<bf16_t>, grid, dim3(256), 0, s, pixel_values, (bf16_t*)out, (int)n, (int)C, (int)H, (int)W, (int)p);
    else if (dtype == SVOL_F16) hipLaunchKernelGGL(patchify_kernel<f16_t>, grid, dim3(256), 0, s, pixel_values, (f16_t*)out, (int)n, (int)C, (int)H, (int)W, (int)p);
    else if (dtype == SVOL_F32) hipLaunchKernelGGL(patchify_kernel<float>, grid, dim3(256), 0, s, pixel_values, (float*)out, (int)n, (int)C, (int)H, (int)W, (int)p);
    else return SVOL_E_INVALID;
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

int svol_vit_embed(const float* patch_proj, const float* cls_token, const float* pos_embed, float* x32, void* x, int64_t n,
                   int64_t P, int64_t D, int dtype, void* stream) {
    if (!patch_proj || !cls_token || !pos_embed || !x32 || n <= 0 || P <= 0 || D <= 0) return SVOL_E_INVALID;
    if (D % 4) return SVOL_E_UNSUPPORTED;
    const int64_t total = n * (P + 1) * (D / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == SVOL_BF16) hipLaunchKernelGGL(vit_embed_kernel<bf16_t>, grid, dim3(256), 0, s, patch_proj, cls_token, pos_embed, x32, (bf16_t*)x, n, (int)P, (int)D);
    else if (dtype == SVOL_F16) hipLaunchKernelGGL(vit_embed_kernel<f16_t>, grid, dim3(256), 0, s, patch_proj, cls_token, pos_embed, x32, (f16_t*)x, n, (int)P, (int)D);
    else if (dtype == SVOL_F32) hipLaunchKernelGGL(vit_embed_kernel<float>, grid, dim3(256), 0, s, patch_proj, cls_token, pos_embed, x32, (float*)x, n, (int)P, (int)D);
    else return SVOL_E_INVALID;
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}


int svol_attn_small_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                        int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return attn_small_launch(q, ldq, k, ldk, v, ldv, o, ldo, nullptr, n_seq, H, L, dh, scale, dtype, stream, false);
}

int svol_attn_small_fwd_lse(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                            float* lse2, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    if (!lse2) return SVOL_E_INVALID;
    return attn_small_launch(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n_seq, H, L, dh, scale, dtype, stream, false);
}

int svol_attn_small_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                        const void* dout, int64_t lddo, const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                        int64_t lddv, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return attn_small_bwd_launch(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n_seq, H, L, dh, scale, dtype,
                                 stream, false);
}

int svol_attn_small_fwd_h16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                            int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return attn_small_launch(q, ldq, k, ldk, v, ldv, o, ldo, nullptr, n_seq, H, L, dh, scale, dtype, stream, true);
}

int svol_attn_small_fwd_lse_h16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                                float* lse2, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    if (!lse2) return SVOL_E_INVALID;
    return attn_small_launch(q, ldq, k, ldk, v, ldv, o, ldo, lse2, n_seq, H, L, dh, scale, dtype, stream, true);
}

int svol_attn_small_bwd_h16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                            const void* dout, int64_t lddo, const float* lse2, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                            int64_t lddv, int64_t n_seq, int64_t H, int64_t L, int64_t dh, float scale, int dtype, void* stream) {
    return attn_small_bwd_launch(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse2, dq, lddq, dk, lddk, dv, lddv, n_seq, H, L, dh, scale, dtype,
                                 stream, true);
}

}  // extern "C"
