// One attention call as it crosses from the C-ABI entries (attention.hip) to the 16-bit launchers (attention_bf16.hip, built for bf16
// and for fp16): a plain host record in place of 22 / 33 positional parameters.
#pragma once
#include "common.h"

struct AttnCall {
    // operands under the names of the kernel argument structs (AttnArgs, Args): a forward writes out_o / lse2, a backward reads
    // o / d_o / lse2 and writes dq / dk / dv (delta: its 3 x [B,H,Lq] fp32 scratch)
    const void *q, *k, *v, *o, *d_o;
    void *out_o, *dq, *dk, *dv;
    const float* kbias;
    float *lse2, *delta;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, Lq, Lk, dh;
    float scale, premul, drop_p;
    uint64_t drop_seed;
    const int64_t* drop_step;   // device step counter of the *_sd entries (drop_seed_at, common.h), or null
    float* ws;   // scratch of ws_bytes (svol_attn_ws_bytes), or null
    int64_t ws_bytes;
    int flags;       // SVOL_ATTN_* (backward)
    void* ev_prep;   // hipEvent_t or null (backward): recorded where work on the caller's OTHER workspace may begin
    hipStream_t stream;
};

// the fields a kernel argument struct shares with the record
template <typename A> static inline void attn_fill(A& p, const AttnCall& c) {
    p.q = c.q; p.k = c.k; p.v = c.v; p.o = c.o; p.d_o = c.d_o; p.out_o = c.out_o; p.dq = c.dq; p.dk = c.dk; p.dv = c.dv;
    p.kbias = c.kbias; p.lse2 = c.lse2; p.delta = c.delta;
    p.ldq = c.ldq; p.ldk = c.ldk; p.ldv = c.ldv; p.ldo = c.ldo; p.lddo = c.lddo; p.lddq = c.lddq; p.lddk = c.lddk; p.lddv = c.lddv;
    p.B = c.B; p.H = c.H; p.Lq = c.Lq; p.Lk = c.Lk; p.dh = c.dh; p.scale = c.scale; p.premul = c.premul;
    p.drop_p = c.drop_p; p.drop_inv = c.drop_p > 0.f ? 1.f / (1.f - c.drop_p) : 1.f; p.drop_seed = c.drop_seed; p.drop_step = c.drop_step;
}

// attention_bf16.hip's entry points, declared once for both of its builds (an fp16 build sees the bf16 names through common.h's
// renaming macros as well, which makes them a second declaration of its own)
#define SVOL_ATTN_H16_ENTRIES(T)                                                                                      \
    int svol_attn_fwd_##T##_launch(const AttnCall& c);                                                                \
    int svol_attn_bwd_##T##_launch(const AttnCall& c);                                                                \
    int64_t svol_attn_ws_floats_##T(int B, int H, int Lq, int Lk, int dh);                                            \
    int64_t svol_attn_sp_image_bytes_##T(int B, int H, int Lq, int Lk, int dh, int64_t ws_bytes);                     \
    int svol_attn_sp_zero_##T##_launch(float* ws, int64_t ws_bytes, int B, int H, int Lq, int Lk, int dh, hipStream_t s);
SVOL_ATTN_H16_ENTRIES(bf16)
SVOL_ATTN_H16_ENTRIES(f16)
#undef SVOL_ATTN_H16_ENTRIES
