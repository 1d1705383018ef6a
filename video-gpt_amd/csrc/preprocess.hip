// Frame preprocessing (include/vgpt.h, "frame preprocessing"): the 8-bit BOX / BICUBIC resampler of Pillow's Image.resize,
// the centre crop and ToTensor + Normalize(0.5, 0.5), on (N, H, W, 3) uint8 frames.  Everything up to the normalisation is
// integer arithmetic on a coefficient table the host builds in double precision, so the results are Pillow's bit for bit.
//   vgpt_resample_coeffs        : the table of one pass (host; contraction off: an fma in the weights moves a rounding).
//   resample_h_kernel           : a workgroup owns TW output pixels x a walk over row batches.  The (TW, ksize) slice of the
//                                 table stays in LDS for the whole walk; every batch stages the source span of RB rows.
//   resample_v_kernel<FUSED>    : a workgroup owns TH output rows x CB byte columns of one frame and stages the source rows
//                                 of that column strip.  FUSED writes the cropped, normalised planar fp32 instead of bytes.
//   u8_to_chw_norm_kernel       : crop + HWC -> planar + normalise, a 256-pixel row piece per step.
// A 3-byte pixel row starts at any byte, so no row is dword-aligned as a whole.  Global memory is read as ALIGNED dwords
// into an LDS row that keeps the row's misalignment (byte g of the row lies at row[off + g], off = address & 3); a dword that
// sticks out of the source buffer at either end is put together from the bytes inside it, so nothing outside [src, src +
// total) is ever read.  Every lane produces one aligned dword of the destination (four bytes, two pixels' worth); the
// dwords at the two ends of a row piece fall back to byte stores.  pixel x coefficient is a 24-bit multiply-add: |k| < 2^23.
// The tables are device memory the caller filled: every bound read from them is clamped to the staged span, so a corrupt
// table gives wrong pixels, never an access outside LDS or the buffers.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int KSIZE_MAX = VGPT_RESAMPLE_MAX_KSIZE;
constexpr int LDS_BUDGET = 48 * 1024;   // three workgroups per CU at the largest tile
constexpr int DIM_MAX = 1 << 24;         // 3 * side and side * ksize stay far inside int32

// ---------------------------------------------------------------------------------------------------------------------
// host: the coefficient table of one pass
// ---------------------------------------------------------------------------------------------------------------------
double filter_box(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }

double filter_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct PassGeom {
    double scale, support, ss;
    int ksize;
};

int pass_geom(const char* who, int in, int out, int filter, PassGeom* g) {
    VGPT_REQUIRE(in >= 1 && out >= 1, VGPT_ERR_INVALID, "%s: bad size in = %d out = %d", who, in, out);
    VGPT_REQUIRE(filter == VGPT_FILTER_BOX || filter == VGPT_FILTER_BICUBIC, VGPT_ERR_INVALID,
                 "%s: unknown filter = %d (VGPT_FILTER_BOX = 0, VGPT_FILTER_BICUBIC = 1)", who, filter);
    const double S = filter == VGPT_FILTER_BOX ? 0.5 : 2.0;
    g->scale = (double)in / (double)out;
    const double fs = g->scale < 1.0 ? 1.0 : g->scale;
    g->support = S * fs;
    g->ss = 1.0 / fs;
    const double kd = 2.0 * ceil(g->support) + 1.0;
    VGPT_REQUIRE(kd <= (double)KSIZE_MAX, VGPT_ERR_UNSUPPORTED, "%s: ksize = %.0f for in = %d out = %d exceeds %d", who, kd, in,
                 out, KSIZE_MAX);
    g->ksize = (int)kd;
    return VGPT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------------------------------
// the aligned dword at address p; the bytes of it that lie outside [lo, hi) read as 0 and are never touched
__device__ __forceinline__ uint32_t load_dword_inside(uintptr_t p, uintptr_t lo, uintptr_t hi) {
    if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (p + j >= lo && p + j < hi) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(p + j) << (8 * j);
    return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one output byte: taps p[0], p[stride], ... against k[0..n)
__device__ __forceinline__ uint32_t resample_byte(const uint8_t* p, int stride, const int32_t* k, int n) {
    int acc = 1 << 21;
    for (int x = 0; x < n; ++x) acc += __mul24((int)p[x * stride], k[x]);
    return (uint32_t)clampi(acc >> 22, 0, 255);
}

__device__ __forceinline__ float norm_entry(int b) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)b, 255.0f), 0.5f), 0.5f);
}

// this tile's slice of the table: s_coef (tn, ksize), s_min[i] relative to the first staged index, s_cnt[i] taps.  Returns
// the first source index s0 and the staged length through *span (<= span_cap).  All threads call it; ends with a barrier.
__device__ __forceinline__ int stage_table(const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs, int ksize,
                                           int t0, int tn, int in_len, int span_cap, int32_t* s_coef, int32_t* s_min,
                                           int32_t* s_cnt, int* span) {
    const int tid = threadIdx.x;
    const int s0 = clampi(bounds[2 * t0], 0, in_len);
    const int lmin = clampi(bounds[2 * (t0 + tn - 1)], 0, in_len);
    const int lend = lmin + clampi(bounds[2 * (t0 + tn - 1) + 1], 0, in_len - lmin);
    int sp = lend - s0;
    sp = sp < 0 ? 0 : (sp > span_cap ? span_cap : sp);
    for (int i = tid; i < tn; i += blockDim.x) {
        const int mn = clampi(bounds[2 * (t0 + i)], 0, in_len) - s0;
        int cnt = bounds[2 * (t0 + i) + 1];
        cnt = cnt > ksize ? ksize : cnt;
        if (mn < 0) cnt = 0;
        if (cnt > sp - mn) cnt = sp - mn;
        s_min[i] = mn < 0 ? 0 : mn;
        s_cnt[i] = cnt < 0 ? 0 : cnt;
    }
    const int32_t* c = coeffs + (int64_t)t0 * ksize;
    for (int i = tid; i < tn * ksize; i += blockDim.x) s_coef[i] = c[i];
    *span = sp;
    __syncthreads();
    return s0;
}

// ---------------------------------------------------------------------------------------------------------------------
// horizontal pass: (rows, in_w, 3) -> (rows, out_w, 3)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs,
                                                         int ksize, int64_t rows, int in_w, int out_w, int TW, int RB,
                                                         int span_cap, int pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int32_t* s_coef = reinterpret_cast<int32_t*>(smem);
    int32_t* s_min = s_coef + TW * ksize;
    int32_t* s_cnt = s_min + TW;
    uint8_t* s_src = reinterpret_cast<uint8_t*>(s_cnt + TW);

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW;
    const int tw = min(TW, out_w - x0);
    int span;
    const int s0 = stage_table(bounds, coeffs, ksize, x0, tw, in_w, span_cap, s_coef, s_min, s_cnt, &span);

    const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)(rows * in_w * 3);
    const int pd = pitch >> 2;                  // dwords of an LDS row
    const int L = tw * 3;                       // bytes of a destination row piece
    const int nd_max = (L + 3 + 3) >> 2;        // aligned dwords that can touch it
    for (int64_t r0 = (int64_t)blockIdx.y * RB; r0 < rows; r0 += (int64_t)gridDim.y * RB) {
        const int rb = rows - r0 < RB ? (int)(rows - r0) : RB;
        for (int idx = tid; idx < rb * pd; idx += 256) {
            const int r = idx / pd, d = idx - r * pd;
            const uintptr_t a = lo + (uintptr_t)(((r0 + r) * in_w + s0) * 3);
            const int off = (int)(a & 3);
            if (4 * d < off + span * 3)
                reinterpret_cast<uint32_t*>(s_src + r * pitch)[d] = load_dword_inside(a - off + 4 * (uintptr_t)d, lo, hi);
        }
        __syncthreads();
        for (int idx = tid; idx < rb * nd_max; idx += 256) {
            const int r = idx / nd_max, d = idx - r * nd_max;
            const int soff = (int)((lo + (uintptr_t)(((r0 + r) * in_w + s0) * 3)) & 3);
            const uint8_t* row = s_src + r * pitch + soff;
            uint8_t* g = dst + ((r0 + r) * out_w + x0) * 3;
            const int aoff = (int)((uintptr_t)g & 3);
            const int i0 = 4 * d - aoff;        // first byte of this dword, as an index into the row piece
            if (i0 >= L) continue;
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j;
                if (i >= 0 && i < L) {
                    const int px = i / 3, c = i - 3 * px;
                    v |= resample_byte(row + s_min[px] * 3 + c, 3, s_coef + px * ksize, s_cnt[px]) << (8 * j);
                }
            }
            if (i0 >= 0 && i0 + 4 <= L) {
                *reinterpret_cast<uint32_t*>(g + i0) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i0 + j >= 0 && i0 + j < L) g[i0 + j] = (uint8_t)(v >> (8 * j));
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// vertical pass: (N, in_h, W, 3) -> (N, out_h, W, 3) bytes, or FUSED: -> the window (y0, x0, h, w) of it as (N, 3, h, w) fp32
// ---------------------------------------------------------------------------------------------------------------------
template <bool FUSED>
struct VCfg {
    static constexpr int CB = FUSED ? 192 : 256;   // byte columns of a strip (FUSED: 64 whole pixels)
    static constexpr int PITCH = CB + 4;            // + the row's misalignment
};

template <bool FUSED>
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         float* __restrict__ dst_f32, const int32_t* __restrict__ bounds,
                                                         const int32_t* __restrict__ coeffs, int ksize, int n_frames, int in_h,
                                                         int out_h, int W, int TH, int span_cap, int y0, int x0, int h, int w,
                                                         int col_tiles, int row_tiles) {
    constexpr int CB = VCfg<FUSED>::CB, PITCH = VCfg<FUSED>::PITCH, PD = PITCH / 4;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int32_t* s_coef = reinterpret_cast<int32_t*>(smem);
    int32_t* s_min = s_coef + TH * ksize;
    int32_t* s_cnt = s_min + TH;
    float* s_lut = reinterpret_cast<float*>(s_cnt + TH);
    uint8_t* s_src = reinterpret_cast<uint8_t*>(s_lut + (FUSED ? 256 : 0));

    const int tid = threadIdx.x;
    const int ct = blockIdx.x % col_tiles;
    const int rt = (blockIdx.x / col_tiles) % row_tiles;
    const int64_t n = blockIdx.x / col_tiles / row_tiles;
    const int WB = W * 3;
    const int cb0 = (FUSED ? x0 * 3 : 0) + ct * CB;                 // first byte column of the strip
    const int cbn = min(CB, (FUSED ? (x0 + w) * 3 : WB) - cb0);
    const int yy0 = (FUSED ? y0 : 0) + rt * TH;                     // first output row of the tile
    const int th = min(TH, (FUSED ? y0 + h : out_h) - yy0);
    if (FUSED) s_lut[tid] = norm_entry(tid);
    int span;
    const int s0 = stage_table(bounds, coeffs, ksize, yy0, th, in_h, span_cap, s_coef, s_min, s_cnt, &span);

    const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)((int64_t)n_frames * in_h * WB);
    const uintptr_t a0 = lo + (uintptr_t)((n * in_h + s0) * WB + cb0);   // the strip's first byte in the first staged row
    for (int idx = tid; idx < span * PD; idx += 256) {
        const int r = idx / PD, d = idx - r * PD;
        const uintptr_t a = a0 + (uintptr_t)r * WB;
        const int off = (int)(a & 3);
        if (4 * d < off + cbn)
            reinterpret_cast<uint32_t*>(s_src + r * PITCH)[d] = load_dword_inside(a - off + 4 * (uintptr_t)d, lo, hi);
    }
    __syncthreads();
    // byte column j of staged row r: s_src[r * PITCH + ((a0 + r * WB) & 3) + j] (the misalignment differs from row to row when
    // WB is no multiple of 4).  The four outputs of a lane lie in ONE output row, so they share the taps: every coefficient
    // and row base is read once for four bytes.  Columns are clamped into the strip; the caller drops the dead ones.
    auto out_quad = [&](int i, int j0, int js, uint32_t* v) {
        const int32_t* k = s_coef + i * ksize;
        const int mn = s_min[i], cnt = s_cnt[i];
        int col[4], acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            col[e] = clampi(j0 + e * js, 0, cbn - 1);
            acc[e] = 1 << 21;
        }
        const uint8_t* p = s_src + mn * PITCH;
        int off = (int)((a0 + (uintptr_t)mn * WB) & 3);
        for (int x = 0; x < cnt; ++x) {
            const int kx = k[x];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += __mul24((int)p[off + col[e]], kx);
            p += PITCH;
            off = (off + WB) & 3;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (uint32_t)clampi(acc[e] >> 22, 0, 255);
    };
    if (!FUSED) {
        constexpr int ND = (CB + 3 + 3) >> 2;
        for (int idx = tid; idx < th * ND; idx += 256) {
            const int i = idx / ND, d = idx - i * ND;
            uint8_t* g = dst + (n * out_h + yy0 + i) * WB + cb0;
            const int aoff = (int)((uintptr_t)g & 3);
            const int j0 = 4 * d - aoff;
            if (j0 >= cbn) continue;
            uint32_t b[4];
            out_quad(i, j0, 1, b);
            if (j0 >= 0 && j0 + 4 <= cbn) {
                *reinterpret_cast<uint32_t*>(g + j0) = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j0 + e >= 0 && j0 + e < cbn) g[j0 + e] = (uint8_t)b[e];
            }
        }
    } else {
        constexpr int NQ = CB / 12;                 // quads of pixels in a strip
        const int px0 = ct * (CB / 3);              // first pixel of the strip, relative to the window
        const int npx = cbn / 3;
        for (int idx = tid; idx < th * 3 * NQ; idx += 256) {
            const int q = idx % NQ, c = (idx / NQ) % 3, i = idx / (3 * NQ);
            if (4 * q >= npx) continue;
            uint32_t b[4];
            out_quad(i, 12 * q + c, 3, b);
            float f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = s_lut[b[e]];
            float* g = dst_f32 + ((n * 3 + c) * h + (yy0 - y0 + i)) * w + px0 + 4 * q;
            if (4 * q + 4 <= npx && ((uintptr_t)g & 15) == 0) {
                *reinterpret_cast<f32x4*>(g) = f32x4{f[0], f[1], f[2], f[3]};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < npx) g[e] = f[e];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// crop + HWC -> planar + normalise: (N, H, W, 3) u8 -> (N, 3, h, w) fp32
// ---------------------------------------------------------------------------------------------------------------------
constexpr int NORM_PX = 256;                     // pixels of a row piece
constexpr int NORM_PITCH = NORM_PX * 3 + 4;

__global__ __launch_bounds__(256) void u8_to_chw_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                             int n_frames, int H, int W, int y0, int x0, int h, int w) {
    __shared__ float s_lut[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_row[NORM_PITCH];
    const int tid = threadIdx.x;
    s_lut[tid] = norm_entry(tid);
    const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)((int64_t)n_frames * H * W * 3);
    const int p0 = blockIdx.x * NORM_PX;
    const int npx = min(NORM_PX, w - p0);
    const int64_t rows = (int64_t)n_frames * h;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const int64_t n = row / h;
        const int y = (int)(row - n * h);
        const uintptr_t a = lo + (uintptr_t)((((n * H + y0 + y) * W) + x0 + p0) * 3);
        const int off = (int)(a & 3);
        __syncthreads();                          // the previous row's readers are done (first trip: the table is written)
        if (4 * tid < off + npx * 3) reinterpret_cast<uint32_t*>(s_row)[tid] = load_dword_inside(a - off + 4 * (uintptr_t)tid, lo, hi);
        __syncthreads();
        if (tid < 3 * (NORM_PX / 4)) {
            const int q = tid % (NORM_PX / 4), c = tid / (NORM_PX / 4);
            if (4 * q < npx) {
                float f[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) f[e] = 4 * q + e < npx ? s_lut[s_row[off + (4 * q + e) * 3 + c]] : 0.0f;
                float* g = dst + ((n * 3 + c) * h + y) * w + p0 + 4 * q;
                if (4 * q + 4 <= npx && ((uintptr_t)g & 15) == 0) {
                    *reinterpret_cast<f32x4*>(g) = f32x4{f[0], f[1], f[2], f[3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * q + e < npx) g[e] = f[e];
                }
            }
        }
    }
}
static_assert(NORM_PITCH / 4 <= 256, "one dword per thread stages a row piece");

int check_frames(const char* who, int n_frames, int H, int W) {
    VGPT_REQUIRE(n_frames >= 0, VGPT_ERR_INVALID, "%s: n_frames = %d", who, n_frames);
    VGPT_REQUIRE(H >= 1 && W >= 1, VGPT_ERR_INVALID, "%s: bad size H = %d W = %d", who, H, W);
    VGPT_REQUIRE(H <= DIM_MAX && W <= DIM_MAX, VGPT_ERR_UNSUPPORTED, "%s: H = %d W = %d (sides up to %d are built)", who, H, W,
                 DIM_MAX);
    return VGPT_OK;
}

int check_ksize(const char* who, int ksize) {
    VGPT_REQUIRE(ksize >= 1, VGPT_ERR_INVALID, "%s: ksize = %d", who, ksize);
    VGPT_REQUIRE(ksize <= KSIZE_MAX, VGPT_ERR_UNSUPPORTED, "%s: ksize = %d exceeds %d", who, ksize, KSIZE_MAX);
    return VGPT_OK;
}

int check_window(const char* who, int H, int W, int y0, int x0, int h, int w) {
    VGPT_REQUIRE(y0 >= 0 && x0 >= 0, VGPT_ERR_INVALID, "%s: negative crop offset y0 = %d x0 = %d", who, y0, x0);
    VGPT_REQUIRE(h >= 1 && w >= 1, VGPT_ERR_INVALID, "%s: bad crop size h = %d w = %d", who, h, w);
    VGPT_REQUIRE((int64_t)y0 + h <= H, VGPT_ERR_INVALID, "%s: crop rows y0 = %d h = %d leave the image, H = %d", who, y0, h, H);
    VGPT_REQUIRE((int64_t)x0 + w <= W, VGPT_ERR_INVALID, "%s: crop columns x0 = %d w = %d leave the image, W = %d", who, x0, w, W);
    return VGPT_OK;
}

// the staged span of `tile` consecutive outputs: (tile - 1) * scale + 1 between the first and the last xmin, ksize taps, and
// one more for the truncation of the two ends
int span_bound(int tile, int in_len, int out_len, int ksize) {
    const double sp = ceil((double)(tile - 1) * (double)in_len / (double)out_len) + ksize + 2;
    return sp < (double)in_len ? (int)sp : in_len;
}

int launch_vertical(const char* who, bool fused, const uint8_t* src, uint8_t* dst, float* dst_f32, const int32_t* bounds,
                    const int32_t* coeffs, int ksize, int n_frames, int in_h, int W, int out_h, int y0, int x0, int h, int w,
                    hipStream_t st) {
    const int CB = fused ? VCfg<true>::CB : VCfg<false>::CB, PITCH = CB + 4;
    const int out_rows = fused ? h : out_h;
    int TH = 16, span_cap = 0;
    size_t lds = 0;
    for (;; TH >>= 1) {
        span_cap = span_bound(TH, in_h, out_h, ksize);
        lds = (size_t)TH * (ksize + 2) * 4 + (fused ? 1024 : 0) + (size_t)span_cap * PITCH;
        if (lds <= (size_t)LDS_BUDGET || TH == 1) break;
    }
    VGPT_REQUIRE(lds <= (size_t)LDS_BUDGET, VGPT_ERR_UNSUPPORTED, "%s: ksize = %d needs %zu bytes of LDS", who, ksize, lds);
    const int64_t col_tiles = cdiv(fused ? (int64_t)w * 3 : (int64_t)W * 3, CB), row_tiles = cdiv(out_rows, TH);
    const int64_t wgs = col_tiles * row_tiles * n_frames;
    VGPT_REQUIRE(wgs < (1ll << 31), VGPT_ERR_UNSUPPORTED, "%s: %lld workgroups (n_frames = %d) exceed the grid", who,
                 (long long)wgs, n_frames);
    if (fused)
        resample_v_kernel<true><<<dim3((unsigned)wgs), dim3(256), lds, st>>>(src, dst, dst_f32, bounds, coeffs, ksize, n_frames,
                                                                            in_h, out_h, W, TH, span_cap, y0, x0, h, w,
                                                                            (int)col_tiles, (int)row_tiles);
    else
        resample_v_kernel<false><<<dim3((unsigned)wgs), dim3(256), lds, st>>>(src, dst, dst_f32, bounds, coeffs, ksize, n_frames,
                                                                             in_h, out_h, W, TH, span_cap, y0, x0, h, w,
                                                                             (int)col_tiles, (int)row_tiles);
    VGPT_CHECK_LAUNCH(who);
    return VGPT_OK;
}

}  // namespace

VGPT_EXPORT int vgpt_resample_ksize(int in, int out, int filter) {
    PassGeom g;
    const int rc = pass_geom("vgpt_resample_ksize", in, out, filter, &g);
    return rc != VGPT_OK ? rc : g.ksize;
}

VGPT_EXPORT int vgpt_resample_coeffs(int in, int out, int filter, int32_t* bounds, int32_t* coeffs) {
    VGPT_REQUIRE(bounds && coeffs, VGPT_ERR_INVALID, "vgpt_resample_coeffs: null pointer");
    PassGeom g;
    const int rc = pass_geom("vgpt_resample_coeffs", in, out, filter, &g);
    if (rc != VGPT_OK) return rc;
    double wt[KSIZE_MAX];
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * g.scale;
        int xmin = (int)(center - g.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + g.support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double a = (x + xmin - center + 0.5) * g.ss;
            const double w = filter == VGPT_FILTER_BOX ? filter_box(a) : filter_bicubic(a);
            wt[x] = w;
            ww += w;
        }
        int32_t* k = coeffs + (int64_t)xx * g.ksize;
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) wt[x] /= ww;
            k[x] = wt[x] < 0 ? (int)(-0.5 + wt[x] * (double)(1 << 22)) : (int)(0.5 + wt[x] * (double)(1 << 22));
        }
        for (int x = xmax; x < g.ksize; ++x) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_resample_u8(const void* src, void* dst, const int32_t* bounds, const int32_t* coeffs, int ksize,
                                 int n_frames, int in_h, int in_w, int out_len, int axis, void* stream) {
    const char* who = "vgpt_resample_u8";
    VGPT_REQUIRE(src && dst && bounds && coeffs, VGPT_ERR_INVALID, "%s: null pointer", who);
    VGPT_REQUIRE(axis == 0 || axis == 1, VGPT_ERR_INVALID, "%s: axis = %d (0 = vertical, 1 = horizontal)", who, axis);
    int rc = check_frames(who, n_frames, in_h, in_w);
    if (rc != VGPT_OK) return rc;
    VGPT_REQUIRE(out_len >= 1, VGPT_ERR_INVALID, "%s: out_len = %d", who, out_len);
    VGPT_REQUIRE(out_len <= DIM_MAX, VGPT_ERR_UNSUPPORTED, "%s: out_len = %d (sides up to %d are built)", who, out_len, DIM_MAX);
    rc = check_ksize(who, ksize);
    if (rc != VGPT_OK) return rc;
    VGPT_REQUIRE(src != dst, VGPT_ERR_INVALID, "%s: dst overlaps src", who);
    if (n_frames == 0) return VGPT_OK;
    hipStream_t st = (hipStream_t)stream;
    if (axis == 0)
        return launch_vertical(who, false, (const uint8_t*)src, (uint8_t*)dst, nullptr, bounds, coeffs, ksize, n_frames, in_h,
                               in_w, out_len, 0, 0, out_len, in_w, st);
    const int64_t rows = (int64_t)n_frames * in_h;
    int TW = 64, span_cap = 0, pitch = 0;
    size_t fixed = 0;
    for (;; TW >>= 1) {
        span_cap = span_bound(TW, in_w, out_len, ksize);
        pitch = (span_cap * 3 + 3 + 3) & ~3;
        fixed = (size_t)TW * (ksize + 2) * 4;
        if (fixed + pitch <= (size_t)LDS_BUDGET || TW == 1) break;
    }
    VGPT_REQUIRE(fixed + pitch <= (size_t)LDS_BUDGET, VGPT_ERR_UNSUPPORTED, "%s: ksize = %d needs %zu bytes of LDS", who, ksize,
                 fixed + pitch);
    int64_t RB = ((size_t)LDS_BUDGET - fixed) / pitch;
    RB = RB > 16 ? 16 : RB;
    RB = RB > rows ? rows : RB;
    const int64_t tiles = cdiv(out_len, TW);
    int64_t gy = cdiv(rows, RB);
    const int64_t want = cdiv(4096, tiles);     // enough workgroups to fill the device, few enough to keep the table's reuse
    gy = gy > want ? want : gy;
    resample_h_kernel<<<dim3((unsigned)tiles, (unsigned)gy), dim3(256), fixed + (size_t)RB * pitch, st>>>(
        (const uint8_t*)src, (uint8_t*)dst, bounds, coeffs, ksize, rows, in_w, out_len, TW, (int)RB, span_cap, pitch);
    VGPT_CHECK_LAUNCH(who);
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_u8_to_chw_norm(const void* src, float* dst_f32, int n_frames, int H, int W, int y0, int x0, int h, int w,
                                    void* stream) {
    const char* who = "vgpt_u8_to_chw_norm";
    VGPT_REQUIRE(src && dst_f32, VGPT_ERR_INVALID, "%s: null pointer", who);
    int rc = check_frames(who, n_frames, H, W);
    if (rc != VGPT_OK) return rc;
    rc = check_window(who, H, W, y0, x0, h, w);
    if (rc != VGPT_OK) return rc;
    VGPT_REQUIRE(((uintptr_t)dst_f32 & 3) == 0, VGPT_ERR_INVALID, "%s: dst_f32 must be 4-byte aligned", who);
    if (n_frames == 0) return VGPT_OK;
    const int64_t rows = (int64_t)n_frames * h;
    const int64_t tiles = cdiv(w, NORM_PX);
    int64_t gy = cdiv(8192, tiles);
    gy = gy > rows ? rows : gy;
    u8_to_chw_norm_kernel<<<dim3((unsigned)tiles, (unsigned)gy), dim3(256), 0, (hipStream_t)stream>>>(
        (const uint8_t*)src, dst_f32, n_frames, H, W, y0, x0, h, w);
    VGPT_CHECK_LAUNCH(who);
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_resample_u8_v_chw_norm(const void* src, float* dst_f32, const int32_t* bounds, const int32_t* coeffs,
                                            int ksize, int n_frames, int in_h, int in_w, int out_h, int y0, int x0, int h, int w,
                                            void* stream) {
    const char* who = "vgpt_resample_u8_v_chw_norm";
    VGPT_REQUIRE(src && dst_f32 && bounds && coeffs, VGPT_ERR_INVALID, "%s: null pointer", who);
    int rc = check_frames(who, n_frames, in_h, in_w);
    if (rc != VGPT_OK) return rc;
    VGPT_REQUIRE(out_h >= 1, VGPT_ERR_INVALID, "%s: out_h = %d", who, out_h);
    VGPT_REQUIRE(out_h <= DIM_MAX, VGPT_ERR_UNSUPPORTED, "%s: out_h = %d (sides up to %d are built)", who, out_h, DIM_MAX);
    rc = check_ksize(who, ksize);
    if (rc != VGPT_OK) return rc;
    rc = check_window(who, out_h, in_w, y0, x0, h, w);
    if (rc != VGPT_OK) return rc;
    VGPT_REQUIRE(((uintptr_t)dst_f32 & 3) == 0, VGPT_ERR_INVALID, "%s: dst_f32 must be 4-byte aligned", who);
    if (n_frames == 0) return VGPT_OK;
    return launch_vertical(who, true, (const uint8_t*)src, nullptr, dst_f32, bounds, coeffs, ksize, n_frames, in_h, in_w, out_h,
                           y0, x0, h, w, (hipStream_t)stream);
}
