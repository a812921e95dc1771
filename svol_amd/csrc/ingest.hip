// Frame ingest (reference lib/modeling/backbone.py:31,49: ViTFeatureExtractor(images=[frame]) inside ViTBackbone.forward;
// lib/dataset/svol_dataset.py:218-229: Resize((224,224)) + ToTensor() per frame): raw uint8 frames [n,H,W,3] -> the backbone's
// input, on the device.
//
//   svol_ingest_resize   Pillow's 8-bit bilinear resample, bit for bit: a horizontal pass with fixed-point taps (22 fraction bits),
//                        the intermediate ROUNDED TO uint8 as Pillow does between its passes, a vertical pass, then a 256-entry
//                        table per channel (the /255, mean / std arithmetic is done once on the host, so the float stage has
//                        no rounding of its own) and a store through element strides in fp32 / bf16 / fp16.
//   svol_ingest_resample the same contract for the sketch input (reference preprocess/quickdraw_array_to_pil.py:36: 255 - bitmap,
//                        28 x 28 -> 224 x 224 with Image.BICUBIC; lib/dataset/svol_dataset.py:212-229: .convert('RGB')) and for any of
//                        Pillow's box / bilinear / hamming / bicubic / lanczos tables: SIGNED taps (int32 accumulators from 2^21, an
//                        arithmetic shift by 22, a clamp to [0, 255] after each pass), one or three source channels (one channel goes
//                        through both passes, three source rows per wave at a time where an RGB wave takes one, and becomes
//                        lut[c][u] for c = 0, 1, 2 at the store), and an inversion where the source byte is staged.  Same kernel
//                        body, other template arguments: svol_ingest_resize's instances are unchanged.
//
// One launch, both passes through LDS.  A workgroup owns one image and a tile of R output rows x CW output columns:
//   1. its four waves walk the source rows [ys[r0], ys[r1-1] + cnt[r1-1]) the tile's rows touch, each wave every fourth row: the bytes
//      [3 xs[c0], 3 (xs[c1-1] + cnt[c1-1])) of the row go to the wave's LDS staging buffer with 16-byte loads where the address allows
//      (rows are only byte-aligned: head and tail bytes one by one, nothing outside the span is read), then the wave resamples the
//      row from LDS into one row of the uint8 intermediate image, also in LDS — a lane per output pixel, the tile's taps read from an
//      LDS copy once for the three channels; no workgroup barrier inside this pass (a wave only reads what it staged itself);
//   2. every thread takes 4 neighbouring bytes of an intermediate row (one dword read per tap), runs the vertical taps, looks the four
//      results up in the LDS copy of the table and stores them: as ONE 4-element vector when the four destinations are consecutive
//      and aligned, else one by one.  The intermediate is laid out the way the destination is — channel planes when the output's
//      x stride is 1 (NCHW), pixel-interleaved otherwise (NHWC) — so both consumers get vector stores; a mirrored image is
//      mirrored when the intermediate is written, so its stores stay ascending.
// The tile is chosen on the host (choose_tile): the (R, CW) whose LDS need fits the budget with the least staging work per
// output.  Plain vector loads and stores only: no atomics, no scratch, no allocation, no synchronisation.
#include "common.h"

namespace {

constexpr int INGEST_MAX_TAPS = 64;        // table width per axis (Pillow's bilinear: 2 ceil(scale) + 1, i.e. a downscale up to 31)
constexpr int INGEST_MAX_OUT = 16384;      // OH, OW
constexpr int INGEST_MAX_IN = 1 << 24;     // H, W
constexpr int INGEST_LUT_BYTES = 3 * 256 * 4;
constexpr size_t INGEST_LDS_PREFERRED = 40 * 1024;   // four workgroups per CU
constexpr size_t INGEST_LDS_MAX = 64 * 1024;
constexpr int INGEST_ROW_OVERHEAD = 192;           // tile choice: the fixed cost of staging one source row, in source pixels

struct IngestArgs {
    const unsigned char* src;
    int64_t s_n, s_h, s_w;
    int H, W;
    const int32_t* xtab;
    const int32_t* ytab;
    int kx, ky;
    const float* lut;
    const unsigned char* flip;
    void* out;
    int64_t o_n, o_c, o_h, o_w;
    int OH, OW;
    int R, CW, tiles_x, tiles_y;
    int cap_rows, cap_span;   // what the LDS images hold: intermediate rows, source pixels per staged row
    int pitch, planar, rowbuf;   // bytes per intermediate row; 1 = channel planes of CW bytes, 0 = interleaved; bytes per staging buffer
    int invert;                  // svol_ingest_resample only: 1 = a source byte b is staged as 255 - b
};

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a wave hands LDS data from some of its lanes to others: the LDS executes one wave's instructions in order, so all it takes is that
// the compiler keeps the stores in front of the loads
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the accumulator of a pass and its rounding to a byte: unsigned for svol_ingest_resize's non-negative taps, signed for svol_ingest_resample
template <bool GEN> struct IngestAcc { using type = uint32_t; };
template <> struct IngestAcc<true> { using type = int32_t; };
__device__ __forceinline__ uint32_t clip8(uint32_t acc) { return min(acc >> 22, 255u); }
__device__ __forceinline__ uint32_t clip8(int32_t acc) { return (uint32_t)clampi(acc >> 22, 0, 255); }   // (>> of a negative int: arithmetic)

// One body for both entries.  <TO, 3, false> is svol_ingest_resize.  GEN = true is svol_ingest_resample: SC source channels (1: one
// channel through both passes, an intermediate of CW bytes per row, the three output channels made at the store), signed taps, and
// a.invert applied where the row is staged.
template <typename TO, int SC, bool GEN>
__global__ __launch_bounds__(256) void ingest_resize_kernel(const IngestArgs a) {
    using acc_t = typename IngestAcc<GEN>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char ingest_smem[];
    float* lut_s = reinterpret_cast<float*>(ingest_smem);
    int32_t* xt_s = reinterpret_cast<int32_t*>(ingest_smem + INGEST_LUT_BYTES);
    const int xts = 2 + a.kx, yts = 2 + a.ky;
    int32_t* yt_s = xt_s + round_up(a.CW * xts, 4);
    unsigned char* rowbufs = reinterpret_cast<unsigned char*>(yt_s + round_up(a.R * yts, 4));
    unsigned char* inter = rowbufs + 4 * a.rowbuf;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned b = blockIdx.x;
    const int tx = (int)(b % (unsigned)a.tiles_x);
    b /= (unsigned)a.tiles_x;
    const int ty = (int)(b % (unsigned)a.tiles_y);
    const int64_t img = b / (unsigned)a.tiles_y;
    const int c0 = tx * a.CW, c1 = min(c0 + a.CW, a.OW), cw = c1 - c0;
    const int r0 = ty * a.R, r1 = min(r0 + a.R, a.OH), nr = r1 - r0;
    const bool fl = a.flip != nullptr && a.flip[img] != 0;

    for (int i = tid; i < 768; i += 256) lut_s[i] = a.lut[i];
    for (int i = tid; i < cw * xts; i += 256) xt_s[i] = a.xtab[(int64_t)c0 * xts + i];
    for (int i = tid; i < nr * yts; i += 256) yt_s[i] = a.ytab[(int64_t)r0 * yts + i];

    // the source window of this tile, clamped to the image and to what the LDS images hold (a table that asks for more than the
    // bound the host sized them by loses taps; it never reads or writes outside)
    const int32_t* ya = a.ytab + (int64_t)r0 * yts;
    const int32_t* yb = a.ytab + (int64_t)(r1 - 1) * yts;
    const int y0 = clampi(ya[0], 0, a.H - 1);
    const int y1 = clampi(clampi(yb[0], 0, a.H) + clampi(yb[1], 0, a.ky), y0, a.H);
    const int nrows = min(y1 - y0, a.cap_rows);
    const int32_t* xa_t = a.xtab + (int64_t)c0 * xts;
    const int32_t* xb_t = a.xtab + (int64_t)(c1 - 1) * xts;
    const int xa = clampi(xa_t[0], 0, a.W - 1);
    const int xb = clampi(clampi(xb_t[0], 0, a.W) + clampi(xb_t[1], 0, a.kx), xa, a.W);
    const int span = min(xb - xa, a.cap_span);
    __syncthreads();

    // ---- horizontal pass: source rows -> uint8 intermediate rows.  A wave stages a row into ITS buffer and resamples it, row after
    // row, without a workgroup barrier: the four waves drift apart and one's load latency hides under another's arithmetic ------------
    const unsigned char* img_p = a.src + img * a.s_n;
    unsigned char* rb = rowbufs + wave * a.rowbuf;
    if constexpr (SC == 1) {
        // a grey row is a third of the bytes and a third of the arithmetic, but one row at a time it costs the same chain of latencies
        // (global load, LDS, a tap loop of dependent LDS reads) as an RGB row.  So a wave stages THREE neighbouring rows at a time (three
        // staging buffers of a.rowbuf / 3 bytes; the loads of the three are issued together) and resamples them together, the taps
        // read once for the three — the shape of the three-channel loop, with a third of the round trips.  Behind the last row the
        // last row is taken again (the same bytes written to the same place), so nothing needs a guard.
        const int rb1 = a.rowbuf / 3;
        const uint32_t inv = a.invert ? 0xffffffffu : 0u;   // 255 - b == b ^ 255
        for (int yl = 3 * wave; yl < nrows; yl += 12) {
            const unsigned char* p[3];
            unsigned char* trow[3];
            int shift[3] = {0, 0, 0};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int yr = min(yl + r, nrows - 1);
                p[r] = img_p + (int64_t)(y0 + yr) * a.s_h + (int64_t)xa * a.s_w;
                trow[r] = inter + yr * a.pitch;
            }
            if (a.s_w == 1) {
                int head[3], nv[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    shift[r] = (int)(reinterpret_cast<uintptr_t>(p[r]) & 15u);
                    head[r] = min((16 - shift[r]) & 15, span);
                    nv[r] = (span - head[r]) >> 4;
                }
                const int nvmax = max(nv[0], max(nv[1], nv[2]));
                for (int j = lane; j < nvmax; j += 64) {
                    uint4 v[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        if (j < nv[r]) v[r] = *reinterpret_cast<const uint4*>(p[r] + head[r] + 16 * j);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        if (j < nv[r]) {
                            v[r].x ^= inv, v[r].y ^= inv, v[r].z ^= inv, v[r].w ^= inv;
                            *reinterpret_cast<uint4*>(rb + r * rb1 + shift[r] + head[r] + 16 * j) = v[r];
                        }
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    unsigned char* d = rb + r * rb1 + shift[r];
                    if (lane < head[r]) d[lane] = p[r][lane] ^ (unsigned char)inv;
                    for (int j = head[r] + 16 * nv[r] + lane; j < span; j += 64) d[j] = p[r][j] ^ (unsigned char)inv;
                }
            } else {   // any other pixel stride (one channel of an interleaved image): byte gathers
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    for (int j = lane; j < span; j += 64) rb[r * rb1 + j] = p[r][(int64_t)j * a.s_w] ^ (unsigned char)inv;
            }
            wave_lds_order();
            for (int xl = lane; xl < cw; xl += 64) {   // one output pixel per lane: its taps are read once for the three rows
                const int32_t* t = xt_s + xl * xts;
                const int st = clampi(t[0], 0, a.W) - xa;
                const int cnt = clampi(t[1], 0, a.kx);
                const int lo = max(0, -st), hi = min(cnt, span - st);   // the taps [lo, hi) fall inside the staged span
                acc_t acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
                const unsigned char* s0 = rb + shift[0] + st;
                const unsigned char* s1 = rb + rb1 + shift[1] + st;
                const unsigned char* s2 = rb + 2 * rb1 + shift[2] + st;
                for (int i = lo; i < hi; ++i) {
                    const acc_t w = (acc_t)t[2 + i];
                    acc0 += (acc_t)s0[i] * w;
                    acc1 += (acc_t)s1[i] * w;
                    acc2 += (acc_t)s2[i] * w;
                }
                const int xo = fl ? cw - 1 - xl : xl;
                trow[0][xo] = (unsigned char)clip8(acc0);
                trow[1][xo] = (unsigned char)clip8(acc1);
                trow[2][xo] = (unsigned char)clip8(acc2);
            }
            wave_lds_order();   // the next rows' staging overwrites rb
        }
    } else {
        for (int yl = wave; yl < nrows; yl += 4) {
            const unsigned char* p = img_p + (int64_t)(y0 + yl) * a.s_h + (int64_t)xa * a.s_w;
            int shift = 0;
            uint32_t inv = 0;   // 255 - b == b ^ 255
            if constexpr (GEN) inv = a.invert ? 0xffffffffu : 0u;
            if (a.s_w == SC) {
                // byte b of the span sits at rb[shift + b], shift = p mod 16: 16-byte-aligned global chunks are 16-byte-aligned in LDS
                const int nb = span * SC;
                shift = (int)(reinterpret_cast<uintptr_t>(p) & 15u);
                const int head = min((16 - shift) & 15, nb);
                const int nv = (nb - head) >> 4;
                if constexpr (GEN) {
                    for (int j = lane; j < nv; j += 64) {
                        uint4 v = *reinterpret_cast<const uint4*>(p + head + 16 * j);
                        v.x ^= inv, v.y ^= inv, v.z ^= inv, v.w ^= inv;
                        *reinterpret_cast<uint4*>(rb + shift + head + 16 * j) = v;
                    }
                    if (lane < head) rb[shift + lane] = p[lane] ^ (unsigned char)inv;
                    for (int j = head + 16 * nv + lane; j < nb; j += 64) rb[shift + j] = p[j] ^ (unsigned char)inv;
                } else {
                    for (int j = lane; j < nv; j += 64)
                        *reinterpret_cast<uint4*>(rb + shift + head + 16 * j) = *reinterpret_cast<const uint4*>(p + head + 16 * j);
                    if (lane < head) rb[shift + lane] = p[lane];
                    for (int j = head + 16 * nv + lane; j < nb; j += 64) rb[shift + j] = p[j];
                }
            } else {   // any other pixel stride (an RGBA view's first three channels): byte gathers
                for (int j = lane; j < span * SC; j += 64) {
                    const int px = j / SC, c = j - px * SC;
                    if constexpr (GEN) rb[j] = p[(int64_t)px * a.s_w + c] ^ (unsigned char)inv;
                    else rb[j] = p[(int64_t)px * a.s_w + c];
                }
            }
            wave_lds_order();
            unsigned char* trow = inter + yl * a.pitch;
            for (int xl = lane; xl < cw; xl += 64) {   // one output pixel per lane: its taps are read once for the three channels
                const int32_t* t = xt_s + xl * xts;
                const int st = clampi(t[0], 0, a.W) - xa;
                const int cnt = clampi(t[1], 0, a.kx);
                const int lo = max(0, -st), hi = min(cnt, span - st);   // the taps [lo, hi) fall inside the staged span
                const int xo = fl ? cw - 1 - xl : xl;
                if constexpr (SC == 3) {
                    acc_t acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
                    int si = shift + (st + lo) * 3;
                    for (int i = lo; i < hi; ++i, si += 3) {
                        const acc_t w = (acc_t)t[2 + i];
                        acc0 += (acc_t)rb[si] * w;
                        acc1 += (acc_t)rb[si + 1] * w;
                        acc2 += (acc_t)rb[si + 2] * w;
                    }
                    unsigned char* d = trow + (a.planar ? xo : xo * 3);
                    const int cs = a.planar ? a.CW : 1;
                    d[0] = (unsigned char)clip8(acc0);
                    d[cs] = (unsigned char)clip8(acc1);
                    d[2 * cs] = (unsigned char)clip8(acc2);
                }
            }
            wave_lds_order();   // the next row's staging overwrites rb
        }
    }
    __syncthreads();

    // ---- vertical pass + table + strided store: 4 neighbouring intermediate bytes per thread -----------------------------------
    const int groups = a.pitch >> 2;
    TO* outp = reinterpret_cast<TO*>(a.out) + img * a.o_n;
    const int xbase = fl ? a.OW - c1 : c0;
    const bool dense = a.planar || (a.o_c == 1 && a.o_w == 3);   // 4 neighbouring intermediate bytes = 4 neighbouring destinations
    for (int idx = tid; idx < nr * groups; idx += 256) {
        const int rl = idx / groups, g = idx - rl * groups;
        const int32_t* t = yt_s + rl * yts;
        const int st = clampi(t[0], 0, a.H) - y0;
        const int cnt = clampi(t[1], 0, a.ky);
        const int lo = max(0, -st), hi = min(cnt, nrows - st);
        acc_t acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
        const unsigned char* col = inter + (st + lo) * a.pitch + 4 * g;
        for (int j = lo; j < hi; ++j, col += a.pitch) {
            const acc_t w = (acc_t)t[2 + j];
            const uint32_t v = *reinterpret_cast<const uint32_t*>(col);
            acc[0] += (acc_t)(v & 255u) * w;
            acc[1] += (acc_t)((v >> 8) & 255u) * w;
            acc[2] += (acc_t)((v >> 16) & 255u) * w;
            acc[3] += (acc_t)(v >> 24) * w;
        }
        const int e0 = 4 * g;
        if constexpr (SC == 1) {
            const int64_t rowoff = (int64_t)(r0 + rl) * a.o_h;
            // four neighbouring pixels of the one channel: each becomes the three output channels here
            const int nvalid = cw - e0;   // (<= 0: the padding behind the tile's last column)
            int u[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) u[q] = (int)clip8(acc[q]);
            if (a.planar) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    Vec4<TO> val;
#pragma unroll
                    for (int q = 0; q < 4; ++q) val.set(q, lut_s[c * 256 + u[q]]);
                    TO* d0 = outp + rowoff + c * a.o_c + (int64_t)(xbase + e0) * a.o_w;
                    if (nvalid >= 4 && (reinterpret_cast<uintptr_t>(d0) & (4 * sizeof(TO) - 1)) == 0) {
                        val.store(d0);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (q < nvalid) d0[q] = from_f32<TO>(val.get(q));
                    }
                }
            } else if (a.o_c == 1 && a.o_w == 3) {   // NHWC: the four pixels are 12 consecutive elements
                TO* d0 = outp + rowoff + (int64_t)(xbase + e0) * 3;
                const bool vec = nvalid >= 4 && (reinterpret_cast<uintptr_t>(d0) & (4 * sizeof(TO) - 1)) == 0;
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    Vec4<TO> val;
#pragma unroll
                    for (int q = 0; q < 4; ++q) val.set(q, lut_s[((4 * v + q) % 3) * 256 + u[(4 * v + q) / 3]]);
                    if (vec) {
                        val.store(d0 + 4 * v);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (4 * v + q < 3 * nvalid) d0[4 * v + q] = from_f32<TO>(val.get(q));
                    }
                }
            } else {   // any destination strides
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    for (int c = 0; c < 3; ++c)
                        if (q < nvalid) outp[rowoff + c * a.o_c + (int64_t)(xbase + e0 + q) * a.o_w] = from_f32<TO>(lut_s[c * 256 + u[q]]);
            }
            continue;
        }
        int c, xl;
        if (a.planar) {
            c = e0 / a.CW;
            xl = e0 - c * a.CW;
        } else {
            xl = e0 / 3;
            c = e0 - xl * 3;
        }
        const int64_t rowoff = (int64_t)(r0 + rl) * a.o_h;
        Vec4<TO> val;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int cq = a.planar ? c : c + q;
            cq = cq >= 3 ? cq - 3 : cq;
            val.set(q, lut_s[cq * 256 + (int)clip8(acc[q])]);
        }
        if (dense) {
            const int nvalid = a.planar ? cw - xl : 3 * cw - e0;   // (<= 0: the padding behind the tile's last column)
            TO* d0 = outp + rowoff + c * a.o_c + (int64_t)(xbase + xl) * a.o_w;
            if (nvalid >= 4 && (reinterpret_cast<uintptr_t>(d0) & (4 * sizeof(TO) - 1)) == 0) {
                val.store(d0);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nvalid) d0[q] = from_f32<TO>(val.get(q));
            }
        } else {   // interleaved intermediate, any destination strides
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int xq = (e0 + q) / 3, cq = e0 + q - xq * 3;
                if (xq < cw) outp[rowoff + cq * a.o_c + (int64_t)(xbase + xq) * a.o_w] = from_f32<TO>(val.get(q));
            }
        }
    }
}

// source pixels (rows) that `t` neighbouring outputs of an `in` -> `out` axis with k-wide taps touch, at most: Pillow's windows are
// [int(c - s + .5), int(c + s + .5)) around c = (i + .5) in/out with s = support * max(in/out, 1) and k = 2 ceil(s) + 1 >= 2 s + 1,
// whatever the filter's support (0.5 box, 1 bilinear / hamming, 2 bicubic, 3 lanczos): the last window ends at most (t-1) in/out + 2 s + 1
// behind the first one's start
inline int64_t span_bound(int64_t t, int64_t in, int64_t out, int64_t k) {
    const int64_t s = ((t - 1) * in + out - 1) / out + k;
    return s < in ? s : in;
}

// the tile: among the (R, CW) whose LDS images fit, the one with the least staging work (source pixels + a per-row constant) per output pixel
// (sc source channels: a staged row and an intermediate row hold sc bytes per pixel)
bool choose_tile(IngestArgs& a, size_t& lds_bytes, int sc = 3) {
    const int ow4 = round_up(a.OW, 4);
    const int cws[] = {ow4, 256, 128, 64, 32, 16}, rs[] = {32, 16, 8, 4, 2, 1};
    for (size_t budget : {INGEST_LDS_PREFERRED, INGEST_LDS_MAX}) {
        double best = -1.0;
        for (int ci = 0; ci < 6; ++ci) {
            const int CW = cws[ci];
            if (CW > ow4 || (ci > 0 && CW == ow4)) continue;
            const int cols = CW < a.OW ? CW : a.OW;
            const int64_t spanx = span_bound(cols, a.W, a.OW, a.kx);
            // (a grey wave stages three rows at a time: three buffers)
            const int64_t rowbuf = sc == 3 ? (spanx * 3 + 15 + 15) / 16 * 16 : 3 * ((spanx + 15 + 15) / 16 * 16);
            const int64_t xt_bytes = round_up(CW * (2 + a.kx), 4) * 4;
            const int pitch = sc * CW;   // CW % 4 == 0
            for (int R : rs) {
                const int rows_out = R < a.OH ? R : a.OH;
                const int64_t rows = span_bound(rows_out, a.H, a.OH, a.ky);
                const int64_t lds = INGEST_LUT_BYTES + xt_bytes + round_up(R * (2 + a.ky), 4) * 4 + 4 * rowbuf + (rows * pitch + 15) / 16 * 16;
                if (lds > (int64_t)budget) continue;
                // per staged row: its source pixels, plus the two barriers and the load latency a row costs however short it is
                const double cost = (double)rows * (double)(spanx + INGEST_ROW_OVERHEAD) / ((double)rows_out * cols);
                if (best < 0.0 || cost < best) {
                    best = cost;
                    a.R = R, a.CW = CW, a.cap_rows = (int)rows, a.cap_span = (int)spanx, a.pitch = pitch, a.rowbuf = (int)rowbuf;
                    lds_bytes = (size_t)lds;
                }
            }
        }
        if (best >= 0.0) return true;
    }
    return false;
}

// both entries: sc source channels; gen = svol_ingest_resample's kernels (signed taps, invert)
int ingest_launch(const uint8_t* src, int64_t n, int64_t H, int64_t W, int64_t s_n, int64_t s_h, int64_t s_w, const int32_t* xtab, int64_t kx,
                  const int32_t* ytab, int64_t ky, const float* lut, const uint8_t* flip, void* out, int64_t o_n, int64_t o_c, int64_t o_h,
                  int64_t o_w, int64_t OH, int64_t OW, int out_dtype, int sc, int invert, bool gen, void* stream) {
    if (!src || !xtab || !ytab || !lut || !out || n < 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || kx < 1 || ky < 1 || s_n < 0 ||
        s_h < 0 || s_w < 0 || o_n < 0 || o_c < 0 || o_h < 0 || o_w < 0)
        return SVOL_E_INVALID;
    if (out_dtype != SVOL_F32 && out_dtype != SVOL_BF16 && out_dtype != SVOL_F16) return SVOL_E_INVALID;
    if ((sc != 1 && sc != 3) || (invert != 0 && invert != 1)) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if (kx > INGEST_MAX_TAPS || ky > INGEST_MAX_TAPS || OH > INGEST_MAX_OUT || OW > INGEST_MAX_OUT || H > INGEST_MAX_IN || W > INGEST_MAX_IN)
        return SVOL_E_UNSUPPORTED;
    IngestArgs a;
    a.src = src, a.s_n = s_n, a.s_h = s_h, a.s_w = s_w, a.H = (int)H, a.W = (int)W;
    a.xtab = xtab, a.ytab = ytab, a.kx = (int)kx, a.ky = (int)ky, a.lut = lut, a.flip = flip;
    a.out = out, a.o_n = o_n, a.o_c = o_c, a.o_h = o_h, a.o_w = o_w, a.OH = (int)OH, a.OW = (int)OW;
    a.planar = o_w == 1 ? 1 : 0;
    a.invert = invert;
    size_t lds = 0;
    if (!choose_tile(a, lds, sc)) return SVOL_E_UNSUPPORTED;
    a.tiles_x = (a.OW + a.CW - 1) / a.CW, a.tiles_y = (a.OH + a.R - 1) / a.R;
    const int64_t blocks = n * a.tiles_x * a.tiles_y;
    if (blocks >= (1ll << 31)) return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(256);
#define INGEST_LAUNCH(SC, GEN)                                                                                          \
    do {                                                                                                                \
        if (out_dtype == SVOL_F32) hipLaunchKernelGGL((ingest_resize_kernel<float, SC, GEN>), grid, block, lds, s, a);  \
        else if (out_dtype == SVOL_BF16) hipLaunchKernelGGL((ingest_resize_kernel<bf16_t, SC, GEN>), grid, block, lds, s, a); \
        else hipLaunchKernelGGL((ingest_resize_kernel<f16_t, SC, GEN>), grid, block, lds, s, a);                        \
    } while (0)
    if (!gen) INGEST_LAUNCH(3, false);
    else if (sc == 3) INGEST_LAUNCH(3, true);
    else INGEST_LAUNCH(1, true);
#undef INGEST_LAUNCH
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}

}  // namespace

extern "C" int svol_ingest_resize(const uint8_t* src, int64_t n, int64_t H, int64_t W, int64_t s_n, int64_t s_h, int64_t s_w,
                                  const int32_t* xtab, int64_t kx, const int32_t* ytab, int64_t ky, const float* lut, const uint8_t* flip,
                                  void* out, int64_t o_n, int64_t o_c, int64_t o_h, int64_t o_w, int64_t OH, int64_t OW, int out_dtype,
                                  void* stream) {
    return ingest_launch(src, n, H, W, s_n, s_h, s_w, xtab, kx, ytab, ky, lut, flip, out, o_n, o_c, o_h, o_w, OH, OW, out_dtype, 3, 0, false, stream);
}

extern "C" int svol_ingest_resample(const uint8_t* src, int64_t n, int64_t H, int64_t W, int64_t s_n, int64_t s_h, int64_t s_w,
                                    int src_channels, int invert, const int32_t* xtab, int64_t kx, const int32_t* ytab, int64_t ky,
                                    const float* lut, const uint8_t* flip, void* out, int64_t o_n, int64_t o_c, int64_t o_h, int64_t o_w,
                                    int64_t OH, int64_t OW, int out_dtype, void* stream) {
    return ingest_launch(src, n, H, W, s_n, s_h, s_w, xtab, kx, ytab, ky, lut, flip, out, o_n, o_c, o_h, o_w, OH, OW, out_dtype, src_channels,
                         invert, true, stream);
}
