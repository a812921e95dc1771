// Frame ingest (reference lib/modeling/backbone.py:31,49: ViTFeatureExtractor(images=[frame]) inside ViTBackbone.forward;
// lib/dataset/svol_dataset.py:218-229: Resize((224,224)) + ToTensor() per frame): raw uint8 frames [n,H,W,3] -> the backbone's
// input, on the device.
//
//   svol_ingest_resize   Pillow's 8-bit bilinear resample, bit for bit: a horizontal pass with fixed-point taps (22 fraction bits),
//                        the intermediate ROUNDED TO uint8 as Pillow does between its passes, a vertical pass, then a 256-entry
//                        table per channel (the /255, mean / std arithmetic is done once on the host, so the float stage has
//                        no rounding of its own) and a store through element strides in fp32 / bf16 / fp16.
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

template <typename TO>
__global__ __launch_bounds__(256) void ingest_resize_kernel(const IngestArgs a) {
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
    for (int yl = wave; yl < nrows; yl += 4) {
        const unsigned char* p = img_p + (int64_t)(y0 + yl) * a.s_h + (int64_t)xa * a.s_w;
        int shift = 0;
        if (a.s_w == 3) {
            // byte b of the span sits at rb[shift + b], shift = p mod 16: 16-byte-aligned global chunks are 16-byte-aligned in LDS
            const int nb = span * 3;
            shift = (int)(reinterpret_cast<uintptr_t>(p) & 15u);
            const int head = min((16 - shift) & 15, nb);
            const int nv = (nb - head) >> 4;
            for (int j = lane; j < nv; j += 64)
                *reinterpret_cast<uint4*>(rb + shift + head + 16 * j) = *reinterpret_cast<const uint4*>(p + head + 16 * j);
            if (lane < head) rb[shift + lane] = p[lane];
            for (int j = head + 16 * nv + lane; j < nb; j += 64) rb[shift + j] = p[j];
        } else {   // any other pixel stride (an RGBA view's first three channels): byte gathers
            for (int j = lane; j < span * 3; j += 64) {
                const int px = j / 3, c = j - px * 3;
                rb[j] = p[(int64_t)px * a.s_w + c];
            }
        }
        wave_lds_order();
        unsigned char* trow = inter + yl * a.pitch;
        for (int xl = lane; xl < cw; xl += 64) {   // one output pixel per lane: its taps are read once for the three channels
            const int32_t* t = xt_s + xl * xts;
            const int st = clampi(t[0], 0, a.W) - xa;
            const int cnt = clampi(t[1], 0, a.kx);
            const int lo = max(0, -st), hi = min(cnt, span - st);   // the taps [lo, hi) fall inside the staged span
            uint32_t acc0 = 1u << 21, acc1 = 1u << 21, acc2 = 1u << 21;
            int si = shift + (st + lo) * 3;
            for (int i = lo; i < hi; ++i, si += 3) {
                const uint32_t w = (uint32_t)t[2 + i];
                acc0 += (uint32_t)rb[si] * w;
                acc1 += (uint32_t)rb[si + 1] * w;
                acc2 += (uint32_t)rb[si + 2] * w;
            }
            const int xo = fl ? cw - 1 - xl : xl;
            unsigned char* d = trow + (a.planar ? xo : xo * 3);
            const int cs = a.planar ? a.CW : 1;
            d[0] = (unsigned char)min(acc0 >> 22, 255u);
            d[cs] = (unsigned char)min(acc1 >> 22, 255u);
            d[2 * cs] = (unsigned char)min(acc2 >> 22, 255u);
        }
        wave_lds_order();   // the next row's staging overwrites rb
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
        uint32_t acc[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
        const unsigned char* col = inter + (st + lo) * a.pitch + 4 * g;
        for (int j = lo; j < hi; ++j, col += a.pitch) {
            const uint32_t w = (uint32_t)t[2 + j];
            const uint32_t v = *reinterpret_cast<const uint32_t*>(col);
            acc[0] += (v & 255u) * w;
            acc[1] += ((v >> 8) & 255u) * w;
            acc[2] += ((v >> 16) & 255u) * w;
            acc[3] += (v >> 24) * w;
        }
        const int e0 = 4 * g;
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
            val.set(q, lut_s[cq * 256 + (int)min(acc[q] >> 22, 255u)]);
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
// [int(c - s + .5), int(c + s + .5)) around c = (i + .5) in/out with s = max(in/out, 1) and k = 2 ceil(s) + 1 >= 2 s + 1
inline int64_t span_bound(int64_t t, int64_t in, int64_t out, int64_t k) {
    const int64_t s = ((t - 1) * in + out - 1) / out + k;
    return s < in ? s : in;
}

// the tile: among the (R, CW) whose LDS images fit, the one with the least staging work (source pixels + a per-row constant) per output pixel
bool choose_tile(IngestArgs& a, size_t& lds_bytes) {
    const int ow4 = round_up(a.OW, 4);
    const int cws[] = {ow4, 256, 128, 64, 32, 16}, rs[] = {32, 16, 8, 4, 2, 1};
    for (size_t budget : {INGEST_LDS_PREFERRED, INGEST_LDS_MAX}) {
        double best = -1.0;
        for (int ci = 0; ci < 6; ++ci) {
            const int CW = cws[ci];
            if (CW > ow4 || (ci > 0 && CW == ow4)) continue;
            const int cols = CW < a.OW ? CW : a.OW;
            const int64_t spanx = span_bound(cols, a.W, a.OW, a.kx);
            const int64_t rowbuf = (spanx * 3 + 15 + 15) / 16 * 16;
            const int64_t xt_bytes = round_up(CW * (2 + a.kx), 4) * 4;
            const int pitch = 3 * CW;   // CW % 4 == 0
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

}  // namespace

extern "C" int svol_ingest_resize(const uint8_t* src, int64_t n, int64_t H, int64_t W, int64_t s_n, int64_t s_h, int64_t s_w,
                                  const int32_t* xtab, int64_t kx, const int32_t* ytab, int64_t ky, const float* lut, const uint8_t* flip,
                                  void* out, int64_t o_n, int64_t o_c, int64_t o_h, int64_t o_w, int64_t OH, int64_t OW, int out_dtype,
                                  void* stream) {
    if (!src || !xtab || !ytab || !lut || !out || n < 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || kx < 1 || ky < 1 || s_n < 0 ||
        s_h < 0 || s_w < 0 || o_n < 0 || o_c < 0 || o_h < 0 || o_w < 0)
        return SVOL_E_INVALID;
    if (out_dtype != SVOL_F32 && out_dtype != SVOL_BF16 && out_dtype != SVOL_F16) return SVOL_E_INVALID;
    if (n == 0) return SVOL_OK;
    if (kx > INGEST_MAX_TAPS || ky > INGEST_MAX_TAPS || OH > INGEST_MAX_OUT || OW > INGEST_MAX_OUT || H > INGEST_MAX_IN || W > INGEST_MAX_IN)
        return SVOL_E_UNSUPPORTED;
    IngestArgs a;
    a.src = src, a.s_n = s_n, a.s_h = s_h, a.s_w = s_w, a.H = (int)H, a.W = (int)W;
    a.xtab = xtab, a.ytab = ytab, a.kx = (int)kx, a.ky = (int)ky, a.lut = lut, a.flip = flip;
    a.out = out, a.o_n = o_n, a.o_c = o_c, a.o_h = o_h, a.o_w = o_w, a.OH = (int)OH, a.OW = (int)OW;
    a.planar = o_w == 1 ? 1 : 0;
    size_t lds = 0;
    if (!choose_tile(a, lds)) return SVOL_E_UNSUPPORTED;
    a.tiles_x = (a.OW + a.CW - 1) / a.CW, a.tiles_y = (a.OH + a.R - 1) / a.R;
    const int64_t blocks = n * a.tiles_x * a.tiles_y;
    if (blocks >= (1ll << 31)) return SVOL_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(256);
    if (out_dtype == SVOL_F32) hipLaunchKernelGGL(ingest_resize_kernel<float>, grid, block, lds, s, a);
    else if (out_dtype == SVOL_BF16) hipLaunchKernelGGL(ingest_resize_kernel<bf16_t>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(ingest_resize_kernel<f16_t>, grid, block, lds, s, a);
    SVOL_CHECK_LAUNCH();
    return SVOL_OK;
}
