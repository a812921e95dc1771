// Many queries, few keys: every video token attends to the sketch's tokens (the reference's "V2 (7x7)" lines,
// cross_modal_transformer.py:129-135): Lq = L = 1568 .. 6272 per video against Lk = 49 .. 256 keys.  The contract is svol_attn_fwd /
// svol_attn_bwd's (row-major operands with their own leading dimensions, head h in columns [h dh, (h+1) dh), kbias [B, Lk] fp32 0 / -inf
// or NULL, lse2 [B, H, Lq] in the log2 domain, q_premul as there), for bf16 / fp16 operands, dh in {32, 64} and 1 <= Lk <= 256.
//
// K and V of one (batch, head) are at most 2 x 256 x 64 x 2 B = 64 KiB: a workgroup stages them ONCE into LDS (the XOR-swizzled row
// images of csrc/vit.hip's short-sequence kernels, whose MFMA fragment layouts these kernels share) and then walks a CHUNK of queries,
// fk_chunk_rows(Lq) = 256 ceil(Lq / 2048) rows: a function of Lq alone, at most 8 chunks per (batch, head).  A row of K / V whose key
// is masked (kbias = -inf) or >= Lk is staged as zeros and its score bias is -inf: P = exp2(-inf) = 0 exactly, dP = dO . 0 = 0, so
// its dk / dv rows are exactly 0 whatever its K / V rows hold (NaN included); rows >= Lk / >= Lq are never read or written.
//
//   attn_fewkeys_fwd_kernel   4 waves; a wave takes 32-query tiles of the chunk in turn.  S^T[key][q] = mfma(K rows, Q rows) for ALL
//                             keys (<= 8 accumulator tiles, the query on the lane): one maximum, one exp2 pass, no streaming rescale;
//                             O^T += V^T P^T with P rounded to the operand type (V^T through ds_read_tr16_b64).
//   attn_fewkeys_bwd_kernel   8 waves; the chunk in tiles of 256 queries whose Q and dO rows are staged beside K and V, with lse2 and
//                             delta = the diagonal of the MFMA dO O^T (the chain dP uses: a one-hot P gives dS = 0 exactly).
//                               key-stationary    the waves split the 32-key blocks: with P2 = nkb rounded up to a power of two, wave w owns
//                                                 key block w % P2 and the query blocks w / P2, w / P2 + 8 / P2, .. of every tile, so
//                                                 that at 49 keys (two blocks) all eight waves work.  dV^T / dK^T stay in 2 x dh / 32
//                                                 accumulator tiles per wave over the whole chunk: no spill.
//                               query-stationary  wave w owns query block w of the tile: dQ^T += K^T dS^T, stored at once.
//                             After the last tile the waves that share a key block add their accumulators through LDS in wave order and
//                             one of them stores the block's fp32 partial into ws[b][h][chunk][dV | dK][key][dh].
//   attn_fewkeys_sum_kernel   dv / dk = the chunk partials added in chunk order, dk times scale (/ q_premul), rounded: no atomics, the
//                             same bits every run.
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int FK_LMAX = 256;        // keys
constexpr int FK_TILE = 256;        // queries of a backward tile: 8 waves x 32
constexpr int FK_MAXCHUNKS = 8;     // chunks of a (batch, head) at most

inline int64_t fk_chunk_rows(int64_t Lq) { return FK_TILE * ((Lq + FK_TILE * FK_MAXCHUNKS - 1) / (FK_TILE * FK_MAXCHUNKS)); }
inline int64_t fk_ws_bytes(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh) {
    const int64_t chunk = fk_chunk_rows(Lq), nchunks = (Lq + chunk - 1) / chunk, Lp = (Lk + 31) / 32 * 32;
    return B * H * nchunks * 2 * Lp * dh * (int64_t)sizeof(float);
}

template <typename T>
struct FkArgs {
    const T *q, *k, *v, *o, *dout;
    T *out, *dq;
    float* lse2;          // [B, H, Lq]: written by the forward, read by the backward
    const float* kbias;   // [B, Lk] or null
    float* ws;            // backward: [B, H, nchunks, 2, nkb * 32, dh] fp32
    int64_t ldq, ldk, ldv, ldo, lddo, lddq;
    int H, Lq, Lk, nkb;   // nkb = ceil(Lk / 32) <= 8
    int chunk, nchunks;
    float c2, scale;      // c2: raw MFMA score -> log2 domain (1 for a pre-multiplied q)
};

// 16 bytes from global memory, or zeros (a branch, not a select: see csrc/vit.hip)
template <typename T> __device__ __forceinline__ uint4 fk_ld16(const T* src, bool valid) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (valid) v = *reinterpret_cast<const uint4*>(src);
    return v;
}
// image: row-major, DH operands per row (DH / 8 chunks of 16 bytes), chunk index XOR-ed with the row
template <int DH> __device__ __forceinline__ int fk_off(int row, int ch) {
    constexpr int CPR = DH / 8;
    return row * (DH * 2) + (((ch ^ (row >> (DH == 32 ? 2 : 0))) & (CPR - 1)) << 4);
}
template <int DH> __device__ __forceinline__ uint4 fk_row(const char* img, int row, int ch) {
    return *reinterpret_cast<const uint4*>(img + fk_off<DH>(row, ch));
}
template <typename T> __device__ __forceinline__ typename H16<T>::v8 fk_v8(const uint4& x) { return __builtin_bit_cast(typename H16<T>::v8, x); }
// A operand [row = column db*32 + (lane & 31) of the image][k = image rows r0 .. r0 + 15]
template <typename T, int DH> __device__ __forceinline__ typename H16<T>::v8 fk_tr(const char* img, int r0, int db, int lane) {
    typedef typename H16<T>::lds_v4_ptr lds_ptr;
    const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pp = i16 & 3, hb = g >> 1;
    const int col = db * 32 + 16 * (g & 1) + 4 * pp;
    const int r1 = r0 + 4 * hb + q4;
    const auto lo = H16<T>::read_tr((lds_ptr)(img + fk_off<DH>(r1, col >> 3) + (col & 7) * 2));
    const auto hi = H16<T>::read_tr((lds_ptr)(img + fk_off<DH>(r1 + 8, col >> 3) + (col & 7) * 2));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// registers 8s .. 8s + 7 of an accumulator, rounded to T, as a B fragment
template <typename T> __device__ __forceinline__ typename H16<T>::v8 fk_acc(const f32x16& x, int s) {
    const auto lo = H16<T>::cvt4(f32x4{x[8 * s], x[8 * s + 1], x[8 * s + 2], x[8 * s + 3]});
    const auto hi = H16<T>::cvt4(f32x4{x[8 * s + 4], x[8 * s + 5], x[8 * s + 6], x[8 * s + 7]});
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// rows of a [*, DH] output from accumulators with the row on the lane and the columns in the registers
template <typename T, int DB> __device__ __forceinline__ void fk_store(T* out, const f32x16 (&acc)[DB], float mul, int h) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<typename H16<T>::v4*>(out + db * 32 + 8 * g + 4 * h) =
                H16<T>::cvt4(f32x4{acc[db][4 * g] * mul, acc[db][4 * g + 1] * mul, acc[db][4 * g + 2] * mul, acc[db][4 * g + 3] * mul});
}

// K and V rows [0, nkb * 32) of (b, hh) into their images and the keys' score bias (log2 domain) into sBias; NT threads
template <typename T, int DH, int NT>
__device__ __forceinline__ void fk_stage_kv(const FkArgs<T>& p, int b, int hh, char* sK, char* sV, float* sBias, int tid) {
    constexpr int CPR = DH / 8;
    const T* K = p.k + (int64_t)b * p.Lk * p.ldk + hh * DH;
    const T* V = p.v + (int64_t)b * p.Lk * p.ldv + hh * DH;
    const float* kb = p.kbias ? p.kbias + (int64_t)b * p.Lk : nullptr;
    const int Lp = p.nkb * 32;
    for (int c = tid; c < Lp * CPR; c += NT) {
        const int row = c / CPR, ch = c % CPR;
        bool valid = row < p.Lk;
        if (valid && kb) valid = kb[row] != -INFINITY;
        *reinterpret_cast<uint4*>(sK + fk_off<DH>(row, ch)) = fk_ld16(K + (int64_t)row * p.ldk + ch * 8, valid);
        *reinterpret_cast<uint4*>(sV + fk_off<DH>(row, ch)) = fk_ld16(V + (int64_t)row * p.ldv + ch * 8, valid);
    }
    for (int j = tid; j < FK_LMAX; j += NT) {
        float bias = -INFINITY;
        if (j < p.Lk) bias = kb ? kb[j] * LOG2E : 0.f;
        sBias[j] = bias;
    }
}

template <typename T, int DH>
__global__ __launch_bounds__(256, 2) void attn_fewkeys_fwd_kernel(FkArgs<T> p) {
    constexpr int KS = DH / 16, DB = DH / 32;
    constexpr int IMG = FK_LMAX * DH * 2;
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG];
    __shared__ __attribute__((aligned(16))) float sBias[FK_LMAX];
    char* sK = smem;
    char* sV = smem + IMG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hh = blockIdx.y;
    fk_stage_kv<T, DH, 256>(p, b, hh, sK, sV, sBias, tid);
    __syncthreads();
    const int q0 = blockIdx.x * p.chunk;
    const int qend = min(p.Lq, q0 + p.chunk);
    const int64_t row0 = (int64_t)b * p.Lq;
    for (int qt = q0 + wave * 32; qt < qend; qt += 128) {
        const int qrow = qt + r;
        const bool qvalid = qrow < qend;
        uint4 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = fk_ld16(p.q + (row0 + qrow) * p.ldq + hh * DH + ks * 16 + h * 8, qvalid);
        // t of this lane's query against every key, log2 domain: S[kb][i] <-> key kb*32 + 8*(i/4) + 4*h + i%4
        f32x16 S[8];
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            if (kb < p.nkb) {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = H16<T>::mfma32(fk_v8<T>(fk_row<DH>(sK, kb * 32 + r, ks * 2 + h)), fk_v8<T>(qf[ks]), acc);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bias = *reinterpret_cast<const f32x4*>(sBias + kb * 32 + 8 * g + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[4 * g + e] = __builtin_fmaf(acc[4 * g + e], p.c2, bias[e]);
                        m = fmaxf(m, acc[4 * g + e]);
                    }
                }
                S[kb] = acc;
            }
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.f;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            if (kb < p.nkb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    S[kb][i] = __builtin_amdgcn_exp2f(S[kb][i] - m);
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
                    const auto pb = fk_acc<T>(S[kb], s);
#pragma unroll
                    for (int db = 0; db < DB; ++db) O[db] = H16<T>::mfma32(fk_tr<T, DH>(sV, kb * 32 + 16 * s, db, lane), pb, O[db]);
                }
            }
        }
        if (qvalid) {
            fk_store<T, DB>(p.out + (row0 + qrow) * p.ldo + hh * DH, O, 1.f / l, h);
            if (h == 0) p.lse2[((int64_t)b * p.H + hh) * p.Lq + qrow] = m + log2f(l);
        }
    }
}

template <typename T, int DH>
__device__ __forceinline__ void fk_bwd_body(const FkArgs<T>& p) {
    constexpr int CPR = DH / 8, KS = DH / 16, DB = DH / 32;
    constexpr int IMG = FK_LMAX * DH * 2;
    static_assert(FK_TILE == FK_LMAX, "the Q / dO images of a tile are as large as the K / V images");
    __shared__ __attribute__((aligned(16))) char smem[4 * IMG];
    __shared__ __attribute__((aligned(16))) float sLse[FK_TILE];
    __shared__ __attribute__((aligned(16))) float sDel[FK_TILE];
    __shared__ __attribute__((aligned(16))) float sBias[FK_LMAX];
    char* sK = smem;
    char* sV = smem + IMG;
    char* sQ = smem + 2 * IMG;
    char* sD = smem + 3 * IMG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hh = blockIdx.y;
    const int64_t row0 = (int64_t)b * p.Lq;
    const T* Q = p.q + row0 * p.ldq + hh * DH;
    const T* O = p.o + row0 * p.ldo + hh * DH;
    const T* dO = p.dout + row0 * p.lddo + hh * DH;
    const float* lse = p.lse2 + ((int64_t)b * p.H + hh) * p.Lq;
    fk_stage_kv<T, DH, 512>(p, b, hh, sK, sV, sBias, tid);
    __syncthreads();
    // the key-stationary split: P2 = nkb rounded up to a power of two key blocks, G = 8 / P2 waves per key block
    const int P2 = p.nkb <= 1 ? 1 : p.nkb <= 2 ? 2 : p.nkb <= 4 ? 4 : 8;
    const int G = 8 / P2;
    const int kbw = wave & (P2 - 1), grp = wave / P2;
    const bool kactive = kbw < p.nkb;
    uint4 kf[KS], vf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        kf[ks] = fk_row<DH>(sK, kbw * 32 + r, ks * 2 + h);     // (kbw < 8: inside the image; a block past nkb was not staged, and its wave is not kactive: the values are never used)
        vf[ks] = fk_row<DH>(sV, kbw * 32 + r, ks * 2 + h);
    }
    const float kbias_l = sBias[kbw * 32 + r];
    f32x16 dVt[DB], dKt[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) dVt[db][i] = dKt[db][i] = 0.f;
    const float c2 = p.c2;
    const int q0 = blockIdx.x * p.chunk;
    const int qend = min(p.Lq, q0 + p.chunk);
    for (int t0 = q0; t0 < qend; t0 += FK_TILE) {
        const int nq = min(FK_TILE, qend - t0);
        const int nqb = (nq + 31) >> 5;
        // this wave's O rows (query block `wave` of the tile) as MFMA B fragments, in flight while the tile is staged
        const int trow = wave * 32 + r;
        uint4 ob[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ob[ks] = fk_ld16(O + (int64_t)(t0 + trow) * p.ldo + (ks * 2 + h) * 8, trow < nq);
        __syncthreads();   // the previous tile's images are no longer read
        for (int c = tid; c < nqb * 32 * CPR; c += 512) {
            const int row = c / CPR, ch = c % CPR;
            const bool valid = row < nq;
            const uint4 qv = fk_ld16(Q + (int64_t)(t0 + row) * p.ldq + ch * 8, valid);
            const uint4 dv = fk_ld16(dO + (int64_t)(t0 + row) * p.lddo + ch * 8, valid);
            *reinterpret_cast<uint4*>(sQ + fk_off<DH>(row, ch)) = qv;
            *reinterpret_cast<uint4*>(sD + fk_off<DH>(row, ch)) = dv;
            if (ch == 0) {
                float ls = 0.f;
                if (valid) ls = lse[t0 + row];
                sLse[row] = ls;
            }
        }
        __syncthreads();
        // delta of the wave's 32 rows = the diagonal of dO O^T: element [m][m] sits on lane m + 32 ((m >> 2) & 1), register 4 (m >> 3) + (m & 3)
        if (wave < nqb) {
            f32x16 D;
#pragma unroll
            for (int i = 0; i < 16; ++i) D[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) D = H16<T>::mfma32(fk_v8<T>(fk_row<DH>(sD, trow, ks * 2 + h)), fk_v8<T>(ob[ks]), D);
            const int idx = 4 * (r >> 3) + (r & 3);
            float dl = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i == idx) dl = D[i];
            if (h == ((r >> 2) & 1)) sDel[trow] = dl;
        }
        __syncthreads();
        // ---- key-stationary: dK, dV of key block kbw over this wave's query blocks
        if (kactive) {
            for (int qb = grp; qb < nqb; qb += G) {
                // X[q][key] (lane = key, register i <-> query qb*32 + 8(i>>2) + 4h + (i&3)): scores and dP = dO V^T
                f32x16 S, dP;
#pragma unroll
                for (int i = 0; i < 16; ++i) S[i] = dP[i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    S = H16<T>::mfma32(fk_v8<T>(fk_row<DH>(sQ, qb * 32 + r, ks * 2 + h)), fk_v8<T>(kf[ks]), S);
                    dP = H16<T>::mfma32(fk_v8<T>(fk_row<DH>(sD, qb * 32 + r, ks * 2 + h)), fk_v8<T>(vf[ks]), dP);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int qq = qb * 32 + 8 * g + 4 * h;
                    const f32x4 ls = *reinterpret_cast<const f32x4*>(sLse + qq);
                    const f32x4 dl = *reinterpret_cast<const f32x4*>(sDel + qq);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float pv = qq + e < nq ? __builtin_amdgcn_exp2f(__builtin_fmaf(S[4 * g + e], c2, kbias_l) - ls[e]) : 0.f;
                        S[4 * g + e] = pv;
                        dP[4 * g + e] = pv * (dP[4 * g + e] - dl[e]);
                    }
                }
                // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T[d][key] += Q^T[d][q] dS[q][key]
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const auto pb = fk_acc<T>(S, s), sb = fk_acc<T>(dP, s);
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        dVt[db] = H16<T>::mfma32(fk_tr<T, DH>(sD, qb * 32 + 16 * s, db, lane), pb, dVt[db]);
                        dKt[db] = H16<T>::mfma32(fk_tr<T, DH>(sQ, qb * 32 + 16 * s, db, lane), sb, dKt[db]);
                    }
                }
            }
        }
        // ---- query-stationary: dQ of query block `wave`
        if (wave < nqb) {
            uint4 qf[KS], df[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                qf[ks] = fk_row<DH>(sQ, trow, ks * 2 + h);
                df[ks] = fk_row<DH>(sD, trow, ks * 2 + h);
            }
            const float ls = sLse[trow], dl = sDel[trow];
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
                    S = H16<T>::mfma32(fk_v8<T>(fk_row<DH>(sK, kb * 32 + r, ks * 2 + h)), fk_v8<T>(qf[ks]), S);
                    dP = H16<T>::mfma32(fk_v8<T>(fk_row<DH>(sV, kb * 32 + r, ks * 2 + h)), fk_v8<T>(df[ks]), dP);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bias = *reinterpret_cast<const f32x4*>(sBias + kb * 32 + 8 * g + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(S[4 * g + e], c2, bias[e]) - ls);
                        dP[4 * g + e] = pv * (dP[4 * g + e] - dl);
                    }
                }
                // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const auto sb = fk_acc<T>(dP, s);
#pragma unroll
                    for (int db = 0; db < DB; ++db) dQt[db] = H16<T>::mfma32(fk_tr<T, DH>(sK, kb * 32 + 16 * s, db, lane), sb, dQt[db]);
                }
            }
            if (trow < nq) fk_store<T, DB>(p.dq + (row0 + t0 + trow) * p.lddq + hh * DH, dQt, p.scale, h);
        }
    }
    // ---- the waves of a key block add their accumulators in wave order through LDS (the Q / dO images: G > 1 means P2 <= 4 slots of
    //      2 DB x 16 x 64 floats = 2 IMG bytes), then wave kbw stores the block's partial of this chunk
    __syncthreads();
    float* sRed = reinterpret_cast<float*>(sQ);
    for (int g = 1; g < G; ++g) {
        if (kactive && grp == g) {
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sRed[(((kbw * 2 + 0) * DB + db) * 16 + i) * 64 + lane] = dVt[db][i];
                    sRed[(((kbw * 2 + 1) * DB + db) * 16 + i) * 64 + lane] = dKt[db][i];
                }
        }
        __syncthreads();
        if (kactive && grp == 0) {
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    dVt[db][i] += sRed[(((kbw * 2 + 0) * DB + db) * 16 + i) * 64 + lane];
                    dKt[db][i] += sRed[(((kbw * 2 + 1) * DB + db) * 16 + i) * 64 + lane];
                }
        }
        __syncthreads();
    }
    if (kactive && grp == 0) {
        const int Lp = p.nkb * 32;
        float* wv = p.ws + ((((int64_t)b * p.H + hh) * p.nchunks + blockIdx.x) * 2) * (int64_t)Lp * DH + (int64_t)(kbw * 32 + r) * DH;
        float* wk = wv + (int64_t)Lp * DH;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<f32x4*>(wv + db * 32 + 8 * g + 4 * h) = f32x4{dVt[db][4 * g], dVt[db][4 * g + 1], dVt[db][4 * g + 2], dVt[db][4 * g + 3]};
                *reinterpret_cast<f32x4*>(wk + db * 32 + 8 * g + 4 * h) = f32x4{dKt[db][4 * g], dKt[db][4 * g + 1], dKt[db][4 * g + 2], dKt[db][4 * g + 3]};
            }
    }
}

template <typename T, int DH>
__global__ __launch_bounds__(512, 1) void attn_fewkeys_bwd_kernel(FkArgs<T> p) { fk_bwd_body<T, DH>(p); }

// dv / dk rows [0, Lk) of every (batch, head): the chunk partials in chunk order; one thread per four columns
template <typename T>
__global__ __launch_bounds__(256) void attn_fewkeys_sum_kernel(const float* __restrict__ ws, T* __restrict__ dk, int64_t lddk, T* __restrict__ dv,
                                                               int64_t lddv, int H, int Lk, int Lp, int dh, int nchunks, int64_t total, float mulk) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int which = blockIdx.y;   // 0: dv, 1: dk
    const int c4 = dh / 4;
    const int col = (int)(idx % c4) * 4;
    const int key = (int)((idx / c4) % Lk);
    const int64_t bh = idx / ((int64_t)c4 * Lk);
    const int64_t b = bh / H;
    const int hh = (int)(bh % H);
    const int64_t part = (int64_t)Lp * dh;
    const float* src = ws + (bh * nchunks * 2 + which) * part + (int64_t)key * dh + col;
    f32x4 acc = *reinterpret_cast<const f32x4*>(src);
    for (int c = 1; c < nchunks; ++c) acc += *reinterpret_cast<const f32x4*>(src + (int64_t)c * 2 * part);
    const float mul = which ? mulk : 1.f;
    T* dst = which ? dk + (b * Lk + key) * lddk : dv + (b * Lk + key) * lddv;
    *reinterpret_cast<typename H16<T>::v4*>(dst + hh * dh + col) = H16<T>::cvt4(f32x4{acc[0] * mul, acc[1] * mul, acc[2] * mul, acc[3] * mul});
}

int fk_check(const void* const* ptrs16, int n16, const int64_t* lds, int nld, const float* lse2, const float* kbias, int64_t B, int64_t H,
             int64_t Lq, int64_t Lk, int64_t dh, int dtype) {
    if (!svol_is16(dtype) || (dh != 32 && dh != 64) || Lk < 1 || Lk > FK_LMAX) return SVOL_E_UNSUPPORTED;
    for (int i = 0; i < n16; ++i)
        if (!ptrs16[i]) return SVOL_E_INVALID;
    if (!lse2 || B <= 0 || H <= 0 || Lq <= 0) return SVOL_E_INVALID;
    if (B > 65535 || H > 65535 || Lq > (1ll << 30)) return SVOL_E_UNSUPPORTED;
    for (int i = 0; i < nld; ++i)
        if (lds[i] % 8 || lds[i] < H * dh) return SVOL_E_UNSUPPORTED;
    for (int i = 0; i < n16; ++i)
        if (!aligned16(ptrs16[i])) return SVOL_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(lse2) | reinterpret_cast<uintptr_t>(kbias)) & 3) return SVOL_E_UNSUPPORTED;
    return SVOL_OK;
}

template <typename T>
void fk_shape(FkArgs<T>& p, int64_t H, int64_t Lq, int64_t Lk, float scale, float q_premul) {
    p.H = (int)H, p.Lq = (int)Lq, p.Lk = (int)Lk, p.nkb = (int)((Lk + 31) / 32);
    p.chunk = (int)fk_chunk_rows(Lq);
    p.nchunks = (int)((Lq + p.chunk - 1) / p.chunk);
    p.c2 = q_premul != 0.f ? 1.f : scale * LOG2E;
    p.scale = scale;
}

template <typename T>
int fk_fwd_go(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse2,
              const float* kbias, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, float scale, float q_premul, void* stream) {
    FkArgs<T> p{};
    p.q = (const T*)q, p.k = (const T*)k, p.v = (const T*)v, p.out = (T*)o, p.lse2 = lse2, p.kbias = kbias;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    fk_shape(p, H, Lq, Lk, scale, q_premul);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)p.nchunks, (unsigned)H, (unsigned)B);
    if (dh == 64) hipLaunchKernelGGL((attn_fewkeys_fwd_kernel<T, 64>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((attn_fewkeys_fwd_kernel<T, 32>), grid, dim3(256), 0, s, p);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

template <typename T>
int fk_bwd_go(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo, const void* d_o,
              int64_t lddo, const float* lse2, const float* kbias, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
              int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, float scale, float q_premul, void* ws, void* stream) {
    FkArgs<T> p{};
    p.q = (const T*)q, p.k = (const T*)k, p.v = (const T*)v, p.o = (const T*)o, p.dout = (const T*)d_o, p.dq = (T*)dq;
    p.lse2 = const_cast<float*>(lse2), p.kbias = kbias, p.ws = static_cast<float*>(ws);
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddo = lddo, p.lddq = lddq;
    fk_shape(p, H, Lq, Lk, scale, q_premul);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)p.nchunks, (unsigned)H, (unsigned)B);
    if (dh == 64) hipLaunchKernelGGL((attn_fewkeys_bwd_kernel<T, 64>), grid, dim3(512), 0, s, p);
    else hipLaunchKernelGGL((attn_fewkeys_bwd_kernel<T, 32>), grid, dim3(512), 0, s, p);
    SVOL_CHECK_LAUNCH();
    const int64_t total = B * H * Lk * (dh / 4);
    hipLaunchKernelGGL((attn_fewkeys_sum_kernel<T>), dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, s, p.ws, (T*)dk, lddk, (T*)dv, lddv,
                       (int)H, (int)Lk, p.nkb * 32, (int)dh, p.nchunks, total, q_premul != 0.f ? scale / q_premul : scale);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // namespace

extern "C" {

int64_t svol_attn_fewkeys_chunk_rows(int64_t Lq) { return Lq >= 1 ? fk_chunk_rows(Lq) : 0; }

int64_t svol_attn_fewkeys_ws_bytes(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh) {
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk < 1 || Lk > FK_LMAX || (dh != 32 && dh != 64)) return 0;
    return fk_ws_bytes(B, H, Lq, Lk, dh);
}

int svol_attn_fewkeys_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse2,
                          const float* kbias, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, float scale, float q_premul, int dtype,
                          void* stream) {
    const void* ptrs[] = {q, k, v, o};
    const int64_t lds[] = {ldq, ldk, ldv, ldo};
    const int rc = fk_check(ptrs, 4, lds, 4, lse2, kbias, B, H, Lq, Lk, dh, dtype);
    if (rc != SVOL_OK) return rc;
    if (dtype == SVOL_F16) return fk_fwd_go<f16_t>(q, ldq, k, ldk, v, ldv, o, ldo, lse2, kbias, B, H, Lq, Lk, dh, scale, q_premul, stream);
    return fk_fwd_go<bf16_t>(q, ldq, k, ldk, v, ldv, o, ldo, lse2, kbias, B, H, Lq, Lk, dh, scale, q_premul, stream);
}

int svol_attn_fewkeys_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                          const void* d_o, int64_t lddo, const float* lse2, const float* kbias, void* dq, int64_t lddq, void* dk, int64_t lddk,
                          void* dv, int64_t lddv, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, float scale, float q_premul,
                          void* ws, int64_t ws_bytes, int dtype, void* stream) {
    const void* ptrs[] = {q, k, v, o, d_o, dq, dk, dv};
    const int64_t lds[] = {ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv};
    const int rc = fk_check(ptrs, 8, lds, 8, lse2, kbias, B, H, Lq, Lk, dh, dtype);
    if (rc != SVOL_OK) return rc;
    if (!ws || ws_bytes < fk_ws_bytes(B, H, Lq, Lk, dh)) return SVOL_E_INVALID;
    if (!aligned16(ws)) return SVOL_E_UNSUPPORTED;
    if (dtype == SVOL_F16)
        return fk_bwd_go<f16_t>(q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, lse2, kbias, dq, lddq, dk, lddk, dv, lddv, B, H, Lq, Lk, dh, scale,
                                q_premul, ws, stream);
    return fk_bwd_go<bf16_t>(q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, lse2, kbias, dq, lddq, dk, lddk, dv, lddv, B, H, Lq, Lk, dh, scale,
                             q_premul, ws, stream);
}

}  // extern "C"
