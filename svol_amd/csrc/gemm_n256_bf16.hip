// bf16 NT GEMM with N a multiple of 256 and deep K (fc2: K = 2048, the MLP / q|k dX products: K = 2048 / 512; the ViT
// extractor's projections: K = 768 / 3072, N = 768 ... 3072), gfx950.
//
// With a 128x128 tiling these launches stream A twice (two column tiles) and re-stage a W tile per 128 rows:
// 812 MB through the L2 -> LDS path for fc2 at B = 8, which is what bounds them (~9.5 TB/s measured), on a
// two-stage ring that drains at every barrier.  Here a workgroup owns 128 rows x ALL 256 columns:
//
//  * A is streamed exactly once, W once per 128 rows: 597 MB for fc2;
//  * 32-deep K slabs (A 8 KiB + W 16 KiB) through a 3-slot LDS ring filled by LDS-DMA, one slab always in flight
//    across the raw barrier (counted s_waitcnt vmcnt), fragment reads in inline asm with immediate slot offsets
//    (the loop is unrolled over the ring), 12 ds_read_b128 per wave for 32 MFMAs;
//  * operands swapped and W's rows permuted in its LDS image (as in gemm_ws_bf16.hip) so that a lane owns 8
//    consecutive output columns: bias / fp32 residual / 16-byte stores straight from the accumulators.
//
// Balanced variant (N == 256 and more rows than 128 per CU: fc2, the MLP / in-projection dX products at the video stream's row count).
// With 128-row tiles 392 workgroups meet 256 CUs: some CUs carry two tiles, the rest one (a tail below the fill path's chip-wide rate,
// which is what bounds the launch: profiles/n256_balanced.md), and every tile re-stages all of W.  Here ONE workgroup per CU (C * ceil(M / 256 C) workgroups) owns ceil(M / workgroups) <= 256 consecutive
// rows: eight waves (the two-per-SIMD residency of two co-resident 128-row workgroups), W staged once per workgroup, equal fill on every
// CU.  Same slabs, same W image, same MFMA and the same slab order along K as the 128-row kernel, so every output element sees the same
// accumulation sequence: the two return the same bits.  The workgroup's 16-row MFMA tiles are dealt to the four wave rows as evenly as they
// go (13 tiles: 3 3 3 4); a wave skips the tiles it does not have.
#include <type_traits>

#include "gemm_call.h"

namespace {

struct N256Args {
    const h16_t* A; const h16_t* W; void* C;
    const float* bias; const float* res;
    int64_t lda, ldw, ldc, ldr;
    int M, K, act, nrt;  // nrt: row tiles per column group (padded to a multiple of 8 when there are several groups)
    int rpw;             // balanced variant: rows per workgroup (<= 256)
    int kwt;             // A's contraction index wraps every kwt slabs (kwt = K / BK: no wrap).  Split weights: C = A [W_hi | W_lo]^T
                         // reads the K-concatenated [A | A] without materialising it
};

typedef __attribute__((address_space(3))) void* lds_void_ptr;

constexpr int BM = 128, BN = 256, BK = 32, BAL_BM = 256;
constexpr int W_ST = BN * BK * 2;   // 16 KiB
// the LDS ring of a variant.  128-row tiles: 3 slots of [A 8 KiB | W 16 KiB], 72 KiB, two workgroups per CU.  Balanced: BAL_STG slots,
// A's (16 KiB each) first, then W's, so that the slot offset of a fragment read still fits ds_read's 16-bit immediate.  Three slots
// (96 KiB) leave 64 KiB of the CU's LDS to the side streams' workgroups (the weight-gradient ring); four measured the same alone and
// in the step (profiles/n256_balanced.md).
constexpr int BAL_STG = 3;
template <bool BAL> struct Ring {
    static constexpr int bm = BAL ? BAL_BM : BM, waves = bm / 32, stg = BAL ? BAL_STG : 3;
    static constexpr int a_st = bm * BK * 2, slot = a_st + W_ST, bytes = stg * slot;
    static constexpr int wpw = 16 / waves;       // W pieces (1 KiB LDS-DMA instructions) per wave and slab; A: 2
    static constexpr int pieces = 2 + wpw;
    static constexpr int w_base = BAL ? stg * a_st : 0;   // folded into the W fragment addresses
    static constexpr int offa(int s) { return BAL ? s * a_st : s * slot; }
    static constexpr int offw(int s) { return BAL ? s * W_ST : s * slot + a_st; }   // (on top of w_base)
    static_assert(offa(stg - 1) < 65536 && offw(stg - 1) < 65536 && bytes <= 160 * 1024, "ring does not fit");
};

// 64-byte rows, four 16-byte chunks: chunk permutation that makes the 16 lanes of a fragment read hit 16 distinct slots
__device__ __forceinline__ int slot32(int row, int ch) { return ch ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3); }
__device__ __forceinline__ int wcol(int nt, int i) { return (nt >> 1) * 32 + (i >> 2) * 8 + (nt & 1) * 4 + (i & 3); }

template <int N> __device__ __forceinline__ void n256_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// all but the newest min(fly, F) slabs (PIECES instructions each) have landed
template <int PIECES, int F> __device__ __forceinline__ void n256_wait_slabs(int fly) {
    if constexpr (F == 0) n256_wait_vm<0>();
    else if (fly >= F) n256_wait_vm<PIECES * F>();
    else n256_wait_slabs<PIECES, F - 1>(fly);
}

template <int OFFA, int OFFW>
__device__ __forceinline__ void read_frags(uint4 (&af)[4], uint4 (&wf)[8], const unsigned (&aa)[4], const unsigned (&wa)[8]) {
    asm volatile(
        "ds_read_b128 %0, %12 offset:%c24\n\t"
        "ds_read_b128 %1, %13 offset:%c24\n\t"
        "ds_read_b128 %2, %14 offset:%c24\n\t"
        "ds_read_b128 %3, %15 offset:%c24\n\t"
        "ds_read_b128 %4, %16 offset:%c25\n\t"
        "ds_read_b128 %5, %17 offset:%c25\n\t"
        "ds_read_b128 %6, %18 offset:%c25\n\t"
        "ds_read_b128 %7, %19 offset:%c25\n\t"
        "ds_read_b128 %8, %20 offset:%c25\n\t"
        "ds_read_b128 %9, %21 offset:%c25\n\t"
        "ds_read_b128 %10, %22 offset:%c25\n\t"
        "ds_read_b128 %11, %23 offset:%c25\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(af[0]), "=&v"(af[1]), "=&v"(af[2]), "=&v"(af[3]), "=&v"(wf[0]), "=&v"(wf[1]), "=&v"(wf[2]), "=&v"(wf[3]),
          "=&v"(wf[4]), "=&v"(wf[5]), "=&v"(wf[6]), "=&v"(wf[7])
        : "v"(aa[0]), "v"(aa[1]), "v"(aa[2]), "v"(aa[3]), "v"(wa[0]), "v"(wa[1]), "v"(wa[2]), "v"(wa[3]), "v"(wa[4]), "v"(wa[5]),
          "v"(wa[6]), "v"(wa[7]), "n"(OFFA), "n"(OFFW)
        : "memory");
}

// one pass over the ring (slots S .. STG-1 at slabs kt + S ...), and the up to STG - 1 steps behind the last whole pass
template <int S, int STG, class F> __device__ __forceinline__ void ring_pass(F& step, int kt) {
    if constexpr (S < STG) { step(std::integral_constant<int, S>{}, kt + S); ring_pass<S + 1, STG>(step, kt); }
}
template <int S, int STG, class F> __device__ __forceinline__ void ring_tail(F& step, int kt, int nk) {
    if constexpr (S < STG - 1) {
        if (kt < nk) { step(std::integral_constant<int, S>{}, kt); ring_tail<S + 1, STG>(step, kt + 1, nk); }
    }
}

template <bool OUT_F32, bool BAL>
__device__ __forceinline__ void gemm_n256_body(const N256Args& p) {
    using R = Ring<BAL>;
    constexpr int STG = R::stg;
    __shared__ __attribute__((aligned(1024))) char smem[R::bytes];  // 72 KiB (balanced: 96 KiB)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    // 1-D grid, row tile fastest: the column groups of one row tile land on the same XCD (ids differ by a multiple of 8)
    // and share its L2 for the A rows they all read.  (Balanced: one column group, p.rpw rows per workgroup.)
    const int rt = BAL ? blockIdx.x : blockIdx.x % p.nrt, cg = BAL ? 0 : blockIdx.x / p.nrt;
    const int bm = rt * (BAL ? p.rpw : BM);
    if (bm >= p.M) return;  // padding workgroups of the XCD-aligned grid
    const int rows = min(BAL ? p.rpw : BM, p.M - bm);
    const int bn = cg * BN;
    // the wave row's MFMA tiles: four from row wm * 64 on; balanced: tiles t0 .. t0 + cnt - 1 (cnt <= 4) of the workgroup's ceil(rows / 16)
    const int ntile = (rows + 15) >> 4;
    const int t0 = BAL ? (wm * ntile) >> 2 : wm * 4;
    const int cnt = BAL ? (((wm + 1) * ntile) >> 2) - t0 : 4;

    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.A + (int64_t)bm * p.lda), 0, (int)((((int64_t)rows - 1) * p.lda + p.kwt * BK) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rW =
        __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (int64_t)bn * p.ldw), 0, (int)((((int64_t)BN - 1) * p.ldw + p.K) * 2), 0x00020000);
    // DMA: one instruction = 16 image rows x 4 chunks.  A: instructions 2w, 2w+1; W: 4w .. 4w+3 (balanced, eight waves: 2w, 2w+1).
    // Rows past the workgroup's last are past the descriptor's end: they land as zeros.
    // image row rho of W holds global row  (rho/128)*128 + wcol((rho%128)/16, rho%16)
    int voffA[2], voffW[R::wpw];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = (wave * 2 + j) * 16 + (lane >> 2);
        voffA[j] = (int)(((int64_t)row * p.lda + slot32(row, lane & 3) * 8) * 2);
    }
#pragma unroll
    for (int j = 0; j < R::wpw; ++j) {
        const int rho = (wave * R::wpw + j) * 16 + (lane >> 2);
        const int n = (rho >> 7) * 128 + wcol((rho & 127) >> 4, rho & 15);
        voffW[j] = (int)(((int64_t)n * p.ldw + slot32(rho, lane & 3) * 8) * 2);
    }
    auto issue = [&](int slot, int kt) {
        char* slA = smem + (BAL ? slot * R::a_st : slot * R::slot);
        char* slW = smem + (BAL ? R::w_base + slot * W_ST : slot * R::slot + R::a_st);
        const int so = kt * BK * 2;
        const int soA = (kt >= p.kwt ? kt - p.kwt : kt) * BK * 2;   // (at most one wrap: K <= 2 * kwt * BK)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_void_ptr)(slA + (wave * 2 + j) * 1024), 16, voffA[j], soA, 0, 0);
#pragma unroll
        for (int j = 0; j < R::wpw; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void_ptr)(slW + (wave * R::wpw + j) * 1024), 16, voffW[j], so, 0, 0);
    };

    // fragment addresses (slot 0): A rows (t0 + mt)*16 + fr, W image rows wn*128 + nt*16 + fr, chunk fq
    const unsigned lds0 = (unsigned)(size_t)(lds_void_ptr)smem;
    unsigned aa[4], wa[8];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int row = (t0 + mt) * 16 + fr;   // (balanced, mt >= cnt: still inside A's slot, read and not used)
        aa[mt] = lds0 + (unsigned)(row * 64 + (slot32(row, fq) << 4));
    }
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const int rho = wn * 128 + nt * 16 + fr;
        wa[nt] = lds0 + (unsigned)(R::w_base + rho * 64 + (slot32(rho, fq) << 4));
    }

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / BK;
#pragma unroll
    for (int s = 0; s < STG - 1; ++s)
        if (s < nk) issue(s, s);
    auto step = [&](auto slot_tag, int kt) {
        constexpr int S = decltype(slot_tag)::value;
        n256_wait_slabs<R::pieces, STG - 2>(nk - 1 - kt);  // slab kt has landed; up to STG - 2 later ones may still fly
        __builtin_amdgcn_s_barrier();
        if (kt + STG - 1 < nk) issue((S + STG - 1) % STG, kt + STG - 1);   // (the slot read in step kt - 1: every wave is past that read)
        uint4 af[4], wf[8];
        read_frags<R::offa(S), R::offw(S)>(af, wf, aa, wa);
        if constexpr (BAL) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                if (mt < cnt) {
#pragma unroll
                    for (int nt = 0; nt < 8; ++nt)
                        acc[nt][mt] = SVOL_MFMA_16x16x32_H16(__builtin_bit_cast(h16x8, wf[nt]),
                                                                              __builtin_bit_cast(h16x8, af[mt]), acc[nt][mt], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int nt = 0; nt < 8; ++nt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    acc[nt][mt] = SVOL_MFMA_16x16x32_H16(__builtin_bit_cast(h16x8, wf[nt]),
                                                                          __builtin_bit_cast(h16x8, af[mt]), acc[nt][mt], 0, 0, 0);
        }
    };
    int kt = 0;
    for (; kt + STG <= nk; kt += STG) ring_pass<0, STG>(step, kt);
    ring_tail<0, STG>(step, kt, nk);

    // ---- epilogue from the accumulators: lane (fr = row, fq): columns wn*128 + pr*32 + fq*8 + [0,8) ----------------
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int lr = (t0 + mt) * 16 + fr;   // row inside the workgroup's block
        const int m = bm + lr;
        if (mt >= cnt || lr >= rows) continue;
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) {
            const int n0 = bn + wn * 128 + pr * 32 + fq * 8;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = acc[2 * pr + (e >> 2)][mt][e & 3];
            if (p.bias) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += p.bias[n0 + e];
            }
            if constexpr (OUT_F32) {
                float* C = reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n0;
                if (p.res) {
                    const float* R = p.res + (int64_t)m * p.ldr + n0;
                    const f32x4 r0 = *reinterpret_cast<const f32x4*>(R), r1 = *reinterpret_cast<const f32x4*>(R + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] += r0[e]; v[4 + e] += r1[e]; }
                }
                *reinterpret_cast<f32x4*>(C) = f32x4{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>(C + 4) = f32x4{v[4], v[5], v[6], v[7]};
            } else {
                if (act_is_gelu(p.act)) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = gelu_fast(v[e]);
                }
                if (p.act == SVOL_ACT_RELU) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                h16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (h16_t)v[e];
                *reinterpret_cast<h16x8*>(reinterpret_cast<h16_t*>(p.C) + (int64_t)m * p.ldc + n0) = o;
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void gemm_n256_bf16_f32(N256Args p) { gemm_n256_body<true, false>(p); }
__global__ __launch_bounds__(256, 2) void gemm_n256_bf16_b16(N256Args p) { gemm_n256_body<false, false>(p); }
__global__ __launch_bounds__(512, 2) void gemm_n256_bal_bf16_f32(N256Args p) { gemm_n256_body<true, true>(p); }
__global__ __launch_bounds__(512, 2) void gemm_n256_bal_bf16_b16(N256Args p) { gemm_n256_body<false, true>(p); }

}  // namespace

// compute units of the current device, read once (0: unknown, the balanced variant is then never taken)
static int n256_cus() {
    static const int n = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        return cus;
    }();
    return n;
}

// plan of one call: refuses it (the call does not fit, gemm_call.h) or yields the kernel arguments, the grid and the variant
static int n256_plan(const GemmCall& c, N256Args& p, dim3& grid, bool& bal) {
    const int64_t M = c.M, N = c.N, K = c.K;
    if (N % BN || K % BK || K < 512 || M < 4096) return SVOL_E_UNSUPPORTED;
    if (c.epi != 0 || c.pre || c.colscale) return SVOL_E_UNSUPPORTED;
    if (c.kwrap != K && (c.kwrap % BK || 2 * c.kwrap != K)) return SVOL_E_UNSUPPORTED;
    if (c.act != SVOL_ACT_NONE && ((c.act != SVOL_ACT_GELU && c.act != SVOL_ACT_RELU) || c.out_f32)) return SVOL_E_UNSUPPORTED;   // (GELU_D: needs `pre`, not here)
    if (c.res && !c.out_f32) return SVOL_E_UNSUPPORTED;
    if (c.lda % 8 || c.ldb % 8 || !aligned16(c.A) || !aligned16(c.B) || !aligned16(c.C)) return SVOL_E_UNSUPPORTED;
    if (c.out_f32 ? (c.ldc % 4 || (c.res && (c.ldr % 4 || !aligned16(c.res)))) : (c.ldc % 8 != 0)) return SVOL_E_UNSUPPORTED;
    if ((int64_t)BM * c.lda * 2 >= (1ll << 31) || (int64_t)BN * c.ldb * 2 >= (1ll << 31)) return SVOL_E_UNSUPPORTED;
    const int64_t ncg = N / BN, cus = n256_cus();
    // one column group and more than a 128-row tile per CU: one workgroup per CU (and per round of 256 C rows), equal rows each
    bal = ncg == 1 && cus > 0 && M > BM * cus && (int64_t)BAL_BM * c.lda * 2 < (1ll << 31);
    int64_t nrt = (M + BM - 1) / BM, rpw = 0;
    if (bal) {
        nrt = cus * ((M + BAL_BM * cus - 1) / (BAL_BM * cus));
        rpw = (M + nrt - 1) / nrt;
    } else if (ncg > 1) nrt = (nrt + 7) / 8 * 8;
    if (nrt * ncg > (1ll << 30)) return SVOL_E_UNSUPPORTED;
    p = N256Args{(const h16_t*)c.A, (const h16_t*)c.B, c.C, c.bias, (const float*)c.res, c.lda, c.ldb, c.ldc, c.ldr, (int)M, (int)K, c.act,
                 (int)nrt, (int)rpw, (int)(c.kwrap / BK)};
    grid = dim3((unsigned)(nrt * ncg));
    return SVOL_OK;
}

int svol_gemm_n256_bf16(const GemmCall& c) {
    N256Args p; dim3 grid; bool bal;
    if (const int rc = n256_plan(c, p, grid, bal)) return rc;
    if (bal) hipLaunchKernelGGL(c.out_f32 ? gemm_n256_bal_bf16_f32 : gemm_n256_bal_bf16_b16, grid, dim3(512), 0, c.stream, p);
    else hipLaunchKernelGGL(c.out_f32 ? gemm_n256_bf16_f32 : gemm_n256_bf16_b16, grid, dim3(256), 0, c.stream, p);
    return hipGetLastError() == hipSuccess ? SVOL_OK : SVOL_E_LAUNCH;
}
