// One GEMM call as it crosses from the C-ABI entries (gemm.hip) to the 16-bit kernel families (built for bf16 and for fp16), and the
// order in which they are asked: a family's plan function refuses a call that does not fit (SVOL_E_UNSUPPORTED) and the next is asked.
//
// NT (svol_gemm_nt, svol_gemm_nt_split, svol_gemm_nt_dact -> gemm_nt_dispatch, gemm.hip).  The plain product (epi 0) is validated
// first; the fused backward step (epi 1) meets those checks only in its composition, and under SVOL_DETERMINISTIC its column sums
// are a svol_colsum behind the call without them.  16-bit dtype and no A2: svol_gemm_nt_*_fast
// (gemm_bf16.hip: K % 32 == 0, 16-byte aligned A / B rows, vector-aligned C / res / pre / aux rows), which asks
//   1. weight-stationary, gemm_ws_bf16.hip: K == 256 (no wrap), N % 64 == 0, M >= 4096; bf16 out: no residual, act NONE / GELU / RELU /
//      GELU_D; fp32 out: residual, no act / pre / colscale; epi 1: aux, bf16 out; 16-byte aligned rows
//   2. full-width tiles, gemm_n256_bf16.hip: N % 256 == 0, K % 32 == 0, K >= 512, M >= 4096, epi 0, no pre / colscale; bf16 out: act
//      NONE / GELU / RELU, no residual; fp32 out: act NONE; 16-byte aligned rows.  Two grids, same bits: 128-row tiles; with N == 256 and
//      M > 128 x the device's CU count the balanced variant — one eight-wave workgroup per CU for every 256 x CUs rows, equal rows (<= 256) each
//   3. skinny split-K, gemm_bf16.hip: M <= 2048, K % 256 == 0, N % 64 == 0
//   4. 128 x 128 tiles, gemm_bf16.hip: everything else up to 65535 row tiles; 64-deep K steps when K % 64 == 0 and K >= 1024
// and when none of them takes the call (or the dtype is fp32, or A2 is set), gemm.hip goes on with
//   5. fp32 skinny: dtype fp32, no A2, M <= 2048, K % 128 == 0, N % 32 == 0, 16-byte aligned rows
//   6. epi 0: the generic kernel (any dtype, A2 / n_split; fp32 with fewer than 256 tiles of 128 x 128: 64 x 64 tiles)
//      epi 1: dense C and aux only: the plain product through this cascade, then svol_act_bwd, then svol_colsum
// TN (svol_gemm_tn, svol_gemm_tn_grouped, gemm.hip; one svol_tn_problem per product):
//   1. 16-bit dtype: svol_gemm_tn_*_fast / _grouped (tn_plan, gemm_tn_bf16.hip): N, K, lda, ldb % 8 == 0, 16-byte aligned A / B,
//      sizes <= 2^30, a row chunk within 32-bit byte offsets; grouped: 2 .. SVOL_TN_GROUP_MAX problems that all fit
//   2. the generic kernel (tn_generic_plan, gemm.hip): N, K, lda, ldb on the 16-byte grid, aligned A / B; grouped for fp32 only
//   A group that does not fit as a whole is issued problem by problem.  svol_conv_wgrad_*_fast is tn_plan on an im2col view.
// svol_conv_nhwc (one C-ABI entry, gemm_bf16.hip) picks svol_conv_nhwc_*_launch by dtype: the 128 x 128 NT tile kernel with its A operand
// gathered from an NHWC activation.
#pragma once
#include "common.h"

struct GemmCall {
    // C[M,N] = epilogue(A[M,K] * B[N,K]^T) under the names of the kernel argument structs (FastArgs, WsArgs, N256Args, SkArgs, NtArgs);
    // epi 0: act((A B^T + bias) * colscale) + res, the pre-activation (gelu' under SVOL_ACT_GELU_D) copied to `pre`; epi 1:
    // (A B^T) * act'(aux), column sums added to `colsum`.  Optional operands are null.
    const void *A, *B, *res, *aux;
    void *C, *pre;
    const float *bias, *colscale;
    float* colsum;
    int64_t lda, ldb, ldc, ldp, ldr, ldaux, M, N, K, kwrap;   // A's contraction index is k % kwrap (== K: plain; svol_gemm_nt_split: K == 2 * kwrap)
    int act, epi, out_f32;   // out_f32: C and res are fp32 whatever the operands' type
    hipStream_t stream;
};

// the entry points of the 16-bit files, declared once for both of their builds (an fp16 build sees the bf16 names through common.h's
// renaming macros as well, which makes them a second declaration of its own)
#define SVOL_GEMM_H16_ENTRIES(T)                                                                                                  \
    int svol_gemm_nt_##T##_fast(const GemmCall& c);                                                                               \
    int svol_gemm_ws_##T(const GemmCall& c);                                                                                      \
    int svol_gemm_n256_##T(const GemmCall& c);                                                                                    \
    int svol_gemm_tn_##T##_fast(const svol_tn_problem& q, hipStream_t s);                                                         \
    int svol_gemm_tn_##T##_grouped(const svol_tn_problem* pr, int n, hipStream_t s);                                              \
    int svol_conv_wgrad_##T##_fast(const void* dz, const void* x, float* dwp, int64_t N, int64_t H, int64_t W, int64_t C,         \
                                   int64_t Cout, int64_t kh, int64_t kw, int64_t stride, int64_t pad, int64_t Kp, hipStream_t s);  \
    int svol_conv_nhwc_##T##_launch(const void* x, const void* w, int64_t ldw, void* y, const float* bias, int act,               \
                                    const void* residual, int64_t N, int64_t H, int64_t W, int64_t C, int64_t Cout, int64_t kh,  \
                                    int64_t kw, int64_t stride, int64_t pad, hipStream_t s);
SVOL_GEMM_H16_ENTRIES(bf16)
SVOL_GEMM_H16_ENTRIES(f16)
#undef SVOL_GEMM_H16_ENTRIES
