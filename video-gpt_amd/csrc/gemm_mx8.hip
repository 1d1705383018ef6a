// MX-fp8 GEMMs for the four projections of a decoder layer in the sampler's per-step forward (the `linear_precision = "fp8"`
// inference option): C = A W^T with A and W in OCP e4m3 blocks of 32 along K sharing a power-of-two (E8M0) scale, products
// on the block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16 rate), fp32 accumulation, bf16 out.  Same number
// format as attn_fp8.hip: the block exponent is the smallest e with amax 2^-e <= 448, rounding is round-to-nearest-even, an
// all-zero block has a zero payload.
//
// Operand map of the instruction with e4m3 data (pinned on hardware, see attn_fp8.hip): lane l (r = l & 31, h = l >> 5)
// supplies 32 bytes; bytes 0..15 are k = 16 h + j of row r, bytes 16..31 are k = 32 + 16 h + j.  The E8M0 scale of lane
// (r, h) applies to k = 32 h .. 32 h + 31 of row r.  C/D: column = r (the SECOND operand's row), rows (i&3) + 8 (i>>2) + 4 h
// (the FIRST operand's rows).  The GEMM passes W first and A second, so a lane holds one output row (token) and runs of four
// consecutive output columns.
//
// Record layout (include/vgpt.h, vgpt_mx8_bytes): both operands are stored in the fragment order of that map, in tiles of
// 32 rows x 64 k, so the GEMM stages them into LDS with plain 16-byte LDS-DMA and every fragment is two conflict-free
// ds_read_b128:
//   payload  [row group g = m / 32][k tile kb = k / 64][half p][lane l][16 bytes]   byte j = element (32 g + (l & 31),
//            64 kb + 32 p + 16 (l >> 5) + j)
//   scales   at align256(payload bytes): [g][kb][lane l] = E8M0 byte of row 32 g + (l & 31), 32-block 2 kb + (l >> 5)
// Rows past the matrix's last row (up to the next multiple of 32) and k past K (up to the next multiple of 64) are stored
// as zero payload with scale byte 127.
//
// Kernels:
//   mx8_quant_kernel   (rows, K) bf16 [x gain (K)] -> record; optionally rstd[m] = rsqrt(mean_k x^2 + eps) of the UNSCALED row
//                      (the RMSNorm statistic the consumer GEMM's epilogue applies).  8 rows x 32 threads per workgroup.
//   gemm_mx8_kernel    (the RoPE epilogue: one head of 32 WN columns per wave, WN = head_dim / 32 = 2, 3 or 4)
//                      128-row x (64 WN)-column tiles, four waves as 2 (rows) x 2 (columns), each wave 64 rows x 32 WN columns,
//                      k tiles of 64 double-buffered in LDS (a simple compiler-scheduled loop).  Every output element is the
//                      same fixed sequence of MFMAs over k whatever tile or launch computed it: no split-K, no atomics, so a
//                      row's result does not depend on M or on its position.
#include "common.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// smallest e with amax 2^-e <= 448 = 1.75 2^8, from amax = f 2^E (f in [0.5, 1)) without rounding: 2 f <= 1.75 -> e = E - 9,
// else E - 8; clamped to the E8M0 range.  Returns the E8M0 byte and 2^-e.
__device__ __forceinline__ int mx8_block_scale(float amax, float& inv) {
    int e = 0;
    if (amax > 0.f) {
        int E;
        const float f = frexpf(amax, &E);
        e = f <= 0.875f ? E - 9 : E - 8;
        e = max(-127, min(e, 127));
    }
    inv = __builtin_ldexpf(1.0f, -e);
    return e + 127;
}
__device__ __forceinline__ uint32_t mx8_pack4(float a, float b, float c, float d) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}

struct QuantArgs {
    const bf16* x; const bf16* gain;
    uint8_t* pay; uint8_t* sc;
    float* rstd;
    int64_t ldx;
    int M, K, KB;    // KB = k tiles of 64
    float eps;
};

// workgroup = 8 rows; thread t: row r = t & 7 of them, blocks of 32 c = t >> 3, c + 32, ...  (a wave reads 512 contiguous bytes
// of each of its 8 rows and writes 128 contiguous bytes per record piece)
__global__ __launch_bounds__(256) void mx8_quant_kernel(QuantArgs a) {
    const int tid = threadIdx.x, r = tid & 7, c0 = tid >> 3;
    const int m = blockIdx.x * 8 + r;          // < rows rounded up to 32
    const bool live = m < a.M;
    const int g = m >> 5, rl = m & 31;
    const bf16* xr = a.x + (int64_t)min(m, a.M - 1) * a.ldx;
    float ss = 0.f;
    for (int b = c0; b < 2 * a.KB; b += 32) {
        float x[32];
        float amax = 0.f;
        const bool in = live && b * 32 < a.K;   // K % 32 == 0: a block is wholly in or out
        if (in) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bf16x8 t = *reinterpret_cast<const bf16x8*>(xr + b * 32 + 8 * q);
                bf16x8 gn;
                if (a.gain != nullptr) gn = *reinterpret_cast<const bf16x8*>(a.gain + b * 32 + 8 * q);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = bf2f(t[j]);
                    ss += v * v;
                    x[8 * q + j] = a.gain != nullptr ? v * bf2f(gn[j]) : v;
                    amax = fmaxf(amax, fabsf(x[8 * q + j]));
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) x[j] = 0.f;
        }
        float inv;
        const int s = mx8_block_scale(amax, inv);
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = mx8_pack4(x[4 * q] * inv, x[4 * q + 1] * inv, x[4 * q + 2] * inv, x[4 * q + 3] * inv);
        const int kb = b >> 1, p = b & 1;
        const int64_t rec = ((int64_t)g * a.KB + kb);
        uint8_t* dst = a.pay + rec * 2048 + p * 1024;
        *reinterpret_cast<uint4*>(dst + rl * 16) = make_uint4(w[0], w[1], w[2], w[3]);          // k 32 p + 0..15: lane half 0
        *reinterpret_cast<uint4*>(dst + (32 + rl) * 16) = make_uint4(w[4], w[5], w[6], w[7]);   // k 32 p + 16..31: lane half 1
        a.sc[rec * 64 + p * 32 + rl] = (uint8_t)s;
    }
    if (a.rstd == nullptr) return;
    __shared__ float part[32][8];
    part[c0][r] = ss;
    __syncthreads();
    if (tid < 8 && live) {
        float t = 0.f;
        for (int c = 0; c < 32; ++c) t += part[c][tid];   // fixed order
        a.rstd[m] = rsqrtf(t / (float)a.K + a.eps);
    }
}

enum { MX8_NONE = VGPT_MX8_EPI_NONE, MX8_RESID = VGPT_MX8_EPI_RESID, MX8_ROPE = VGPT_MX8_EPI_ROPE, MX8_GATED = VGPT_MX8_EPI_GATED };

struct GemmArgs {
    const uint8_t* a_pay; const uint8_t* a_sc; const uint8_t* w_pay; const uint8_t* w_sc;
    bf16* C; const bf16* resid; const float* rstd; const float* cos_t; const float* sin_t;
    int M, N, KB, tiles_m;
    int NG;           // column groups of 32 in the OUTPUT's column space (GATED: I / 32)
    int I;            // GATED: the up half starts at weight row I
    int rot_cols;     // ROPE: columns [0, rot_cols) are rotated
    int64_t ldc, ldr;
    int act;
};

// LDS-DMA from inline asm (the compiler must not see LDS being written: it would drain vmcnt(0) before later LDS reads)
__device__ __forceinline__ void dma16(const uint8_t* base, uint32_t off, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(off), "s"(base), "s"(lds_dst)
                 : "memory");
}
__device__ __forceinline__ void dma4(const uint8_t* base, uint32_t off, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(off), "s"(base), "s"(lds_dst)
                 : "memory");
}

template <int WN>
struct Tile {
    static constexpr int A_BYTES = 4 * 2048;               // 4 row groups
    static constexpr int B_BYTES = 2 * WN * 2048;          // 2 WN column groups
    static constexpr int SA_OFF = A_BYTES + B_BYTES;
    static constexpr int SB_OFF = SA_OFF + 256;
    static constexpr int STAGE = SB_OFF + 512;             // B scales: two 256-byte DMA pieces (at most 8 groups)
    static constexpr int N_DMA = 8 + 4 * WN + 1 + 2;
};

template <int MODE, int WN>
__global__ __launch_bounds__(256, 2) void gemm_mx8_kernel(GemmArgs a) {
    using T = Tile<WN>;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x STAGE
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int r = lane & 31, h = lane >> 5;
    const int tm = blockIdx.x % a.tiles_m, tn = blockIdx.x / a.tiles_m;
    const int MG = (a.M + 31) >> 5;
    const uint32_t lds_base =
        __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem);

    // weight row group behind block-local column group c (0 .. 2 WN - 1): GATED pairs the gate groups of a wave with the up
    // groups of the same columns (local j < WN / 2: gate, j >= WN / 2: up), so act(gate) * up is formed in one lane
    auto w_group = [&](int c) {
        const int wv = c / WN, j = c % WN;
        if (MODE == MX8_GATED) {
            const int gg = min(tn * WN + wv * (WN / 2) + (j % (WN / 2)), a.NG - 1);
            return j < WN / 2 ? gg : a.I / 32 + gg;
        }
        return min(tn * 2 * WN + c, a.NG - 1);
    };

    auto stage = [&](int buf, int kb) {
        const uint32_t sbase = lds_base + (uint32_t)(buf * T::STAGE);
        for (int p = wave; p < T::N_DMA; p += 4) {
            if (p < 8) {                                  // A payload: row group p / 2, half p % 2
                const int gq = min(tm * 4 + (p >> 1), MG - 1);
                dma16(a.a_pay, (uint32_t)(((int64_t)gq * a.KB + kb) * 2048 + (p & 1) * 1024 + lane * 16),
                      sbase + (uint32_t)(p * 1024));
            } else if (p < 8 + 4 * WN) {                  // W payload
                const int q = p - 8;
                const int gq = w_group(q >> 1);
                dma16(a.w_pay, (uint32_t)(((int64_t)gq * a.KB + kb) * 2048 + (q & 1) * 1024 + lane * 16),
                      sbase + (uint32_t)(T::A_BYTES + q * 1024));
            } else if (p == 8 + 4 * WN) {                 // A scales: 4 groups x 64 bytes
                const int gq = min(tm * 4 + (lane >> 4), MG - 1);
                dma4(a.a_sc, (uint32_t)(((int64_t)gq * a.KB + kb) * 64 + (lane & 15) * 4), sbase + (uint32_t)T::SA_OFF);
            } else {                                      // W scales: groups 4 s .. 4 s + 3 (past 2 WN: a valid group, unused)
                const int s = p - (9 + 4 * WN);
                const int gq = w_group(min(4 * s + (lane >> 4), 2 * WN - 1));
                dma4(a.w_sc, (uint32_t)(((int64_t)gq * a.KB + kb) * 64 + (lane & 15) * 4),
                     sbase + (uint32_t)(T::SB_OFF + s * 256));
            }
        }
    };

    f32x16 acc[2][WN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int t = 0; t < 16; ++t) acc[i][j][t] = 0.f;

    stage(0, 0);
    int buf = 0;
    for (int kb = 0; kb < a.KB; ++kb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // k tile kb landed in `buf` for every wave; every wave is done with the other buffer
        if (kb + 1 < a.KB) stage(buf ^ 1, kb + 1);
        const char* t = smem + buf * T::STAGE;
        v8i af[2], bfr[WN];
        int sa[2], sb[WN];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ag = 2 * wm + i;
            const v4i x0 = *reinterpret_cast<const v4i*>(t + ag * 2048 + lane * 16);
            const v4i x1 = *reinterpret_cast<const v4i*>(t + ag * 2048 + 1024 + lane * 16);
            af[i] = v8i{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
            sa[i] = (int)(uint8_t)t[T::SA_OFF + ag * 64 + lane];
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int bg = wn * WN + j;
            const v4i x0 = *reinterpret_cast<const v4i*>(t + T::A_BYTES + bg * 2048 + lane * 16);
            const v4i x1 = *reinterpret_cast<const v4i*>(t + T::A_BYTES + bg * 2048 + 1024 + lane * 16);
            bfr[j] = v8i{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
            sb[j] = (int)(uint8_t)t[T::SB_OFF + bg * 64 + lane];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(bfr[j], af[i], acc[i][j], 0, 0, 0, sb[j], 0, sa[i]);
        buf ^= 1;
    }

    // ---- epilogue: lane (r, h) of accumulator [i][j] holds row m = 32 (4 tm + 2 wm + i) + r, columns
    //      32 (column group) + 8 g4 + 4 h + u in element 4 g4 + u ----
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = (tm * 4 + 2 * wm + i) * 32 + r;
        if (m >= a.M) continue;
        const float rs = (MODE == MX8_ROPE || MODE == MX8_GATED) && a.rstd != nullptr ? a.rstd[m] : 1.f;
        bf16* crow = a.C + (int64_t)m * a.ldc;
        if constexpr (MODE == MX8_NONE || MODE == MX8_RESID) {
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const int cg = tn * 2 * WN + wn * WN + j;
                if (cg >= a.NG) continue;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int n = cg * 32 + 8 * g4 + 4 * h;
                    float v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = acc[i][j][4 * g4 + u];
                    if constexpr (MODE == MX8_RESID) {
                        const bf16x4 rb = *reinterpret_cast<const bf16x4*>(a.resid + (int64_t)m * a.ldr + n);
#pragma unroll
                        for (int u = 0; u < 4; ++u) v[u] += bf2f(rb[u]);
                    }
                    bf16x4 o;
#pragma unroll
                    for (int u = 0; u < 4; ++u) o[u] = f2bf(v[u]);
                    *reinterpret_cast<bf16x4*>(crow + n) = o;
                }
            }
        } else if constexpr (MODE == MX8_ROPE) {
            // the wave's WN column groups are one head of 32 WN columns: column d and its partner d +- 16 WN sit in the same lane
            static_assert(WN >= 2 && WN <= 4, "RoPE tiles hold one head of 64, 96 or 128 columns per wave");
            const int cg0 = (tn * 2 + wn) * WN;
            if (cg0 >= a.NG) continue;
            const bool rot = cg0 * 32 < a.rot_cols;
            float own[WN][16];
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) own[j][e] = bf2f(f2bf(acc[i][j][e] * rs));
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int d = 32 * j + 8 * g4 + 4 * h;
                    bf16x4 o;
                    if constexpr (WN != 3) {
                        // heads of 64 / 128: the partner d +- 16 WN is column group j +- WN / 2, same g4, same element
                        if (rot) {
                            constexpr int HALF = 16 * WN;
                            const bool upper = j >= WN / 2;
                            const int pj = upper ? j - WN / 2 : j + WN / 2;
                            const int dd = upper ? d - HALF : d;
                            const f32x4 cs = *reinterpret_cast<const f32x4*>(a.cos_t + (int64_t)m * HALF + dd);
                            const f32x4 sn = *reinterpret_cast<const f32x4*>(a.sin_t + (int64_t)m * HALF + dd);
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const float x = own[j][4 * g4 + u], other = own[pj][4 * g4 + u];
                                o[u] = f2bf(upper ? x * cs[u] + other * sn[u] : x * cs[u] - other * sn[u]);
                            }
                        } else {
#pragma unroll
                            for (int u = 0; u < 4; ++u) o[u] = f2bf(own[j][4 * g4 + u]);
                        }
                    } else if (rot) {
                        const bool upper = d >= 48;
                        // partner of d: d + 48 = group j + 1, g4 + 2 (or j + 2, g4 - 2); d - 48 the inverse
                        const int pj = upper ? (g4 >= 2 ? j - 1 : j - 2) : (g4 < 2 ? j + 1 : j + 2);
                        const int pg = upper ? (g4 >= 2 ? g4 - 2 : g4 + 2) : (g4 < 2 ? g4 + 2 : g4 - 2);
                        const int dd = upper ? d - 48 : d;
                        const f32x4 cs = *reinterpret_cast<const f32x4*>(a.cos_t + (int64_t)m * 48 + dd);
                        const f32x4 sn = *reinterpret_cast<const f32x4*>(a.sin_t + (int64_t)m * 48 + dd);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            float other = 0.f;
#pragma unroll
                            for (int jj = 0; jj < 3; ++jj)
#pragma unroll
                                for (int gg = 0; gg < 4; ++gg)
                                    if (jj == pj && gg == pg) other = own[jj][4 * gg + u];
                            const float x = own[j][4 * g4 + u];
                            o[u] = f2bf(upper ? x * cs[u] + other * sn[u] : x * cs[u] - other * sn[u]);
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u) o[u] = f2bf(own[j][4 * g4 + u]);
                    }
                    *reinterpret_cast<bf16x4*>(crow + cg0 * 32 + d) = o;
                }
        } else {   // MX8_GATED: out (M, I) = act(gate) * up from the bf16-rounded gate / up values
#pragma unroll
            for (int j = 0; j < WN / 2; ++j) {
                const int gg = tn * WN + wn * (WN / 2) + j;
                if (gg >= a.NG) continue;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    bf16x4 o;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float gt = bf2f(f2bf(acc[i][j][4 * g4 + u] * rs));
                        const float up = bf2f(f2bf(acc[i][j + WN / 2][4 * g4 + u] * rs));
                        o[u] = f2bf(act_apply(gt, a.act) * up);
                    }
                    *reinterpret_cast<bf16x4*>(crow + gg * 32 + 8 * g4 + 4 * h) = o;
                }
            }
        }
    }
}

template <int MODE, int WN>
int launch_gemm(const GemmArgs& g0, int n_groups_per_tile, hipStream_t stream, const char* name = "vgpt_gemm_mx8") {
    GemmArgs g = g0;
    const int tiles_n = (int)cdiv(g.NG, n_groups_per_tile);
    g.tiles_m = (int)cdiv(g.M, 128);
    const int64_t grid = (int64_t)g.tiles_m * tiles_n;
    VGPT_REQUIRE(grid < (1ll << 31), VGPT_ERR_UNSUPPORTED, "%s: problem too large", name);
    hipLaunchKernelGGL((gemm_mx8_kernel<MODE, WN>), dim3((unsigned)grid), dim3(256), 2 * Tile<WN>::STAGE, stream, g);
    VGPT_CHECK_LAUNCH(name);
    return VGPT_OK;
}

}  // namespace

VGPT_EXPORT int64_t vgpt_mx8_bytes(int64_t rows, int64_t K) {
    if (rows <= 0 || K <= 0 || K % 32 != 0) return -1;
    const int64_t recs = cdiv(rows, 32) * cdiv(K, 64);
    return align256(recs * 2048) + recs * 64;
}

static int mx8_quant(const char* name, const void* x, int64_t ldx, const void* gain, void* out, float* rstd_out, int64_t rows,
                     int64_t K, float eps, void* stream) {
    VGPT_REQUIRE(x && out, VGPT_ERR_INVALID, "%s: null pointer", name);
    VGPT_REQUIRE(rows > 0 && K > 0 && K % 32 == 0, VGPT_ERR_INVALID, "%s: rows > 0 and K a positive multiple of 32 (got %lld, %lld)",
                 name, (long long)rows, (long long)K);
    VGPT_REQUIRE(ldx >= K && ldx % 8 == 0, VGPT_ERR_UNSUPPORTED, "%s: ldx must be a multiple of 8, >= K", name);
    VGPT_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)gain) & 15) == 0, VGPT_ERR_UNSUPPORTED,
                 "%s: x, gain and out must be 16-byte aligned", name);
    VGPT_REQUIRE(rows < (1 << 26) && vgpt_mx8_bytes(rows, K) < (1ll << 32), VGPT_ERR_UNSUPPORTED, "%s: problem too large", name);
    const int64_t MG = cdiv(rows, 32), KB = cdiv(K, 64);
    QuantArgs a;
    a.x = (const bf16*)x; a.gain = (const bf16*)gain;
    a.pay = (uint8_t*)out; a.sc = a.pay + align256(MG * KB * 2048);
    a.rstd = rstd_out; a.ldx = ldx; a.M = (int)rows; a.K = (int)K; a.KB = (int)KB; a.eps = eps;
    hipLaunchKernelGGL(mx8_quant_kernel, dim3((unsigned)(MG * 4)), dim3(256), 0, (hipStream_t)stream, a);
    VGPT_CHECK_LAUNCH(name);
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_mx8_quant_rows(const void* x, int64_t ldx, void* out, float* rstd_out, int64_t rows, int64_t K, float eps,
                                    void* stream) {
    return mx8_quant("vgpt_mx8_quant_rows", x, ldx, nullptr, out, rstd_out, rows, K, eps, stream);
}

VGPT_EXPORT int vgpt_mx8_quant_weight(const void* W, const void* gain, void* out, int64_t N, int64_t K, void* stream) {
    return mx8_quant("vgpt_mx8_quant_weight", W, K, gain, out, nullptr, N, K, 0.f, stream);
}

VGPT_EXPORT int vgpt_gemm_mx8(const void* A8, const void* W8, void* C, const void* resid, const float* rstd, const float* cos_t,
                              const float* sin_t, int64_t M, int64_t N, int64_t K, int64_t ldc, int64_t ldr, int epilogue,
                              int n_rot_heads, int head_dim, int act, void* stream) {
    VGPT_REQUIRE(A8 && W8 && C, VGPT_ERR_INVALID, "vgpt_gemm_mx8: null pointer");
    VGPT_REQUIRE(M > 0 && N > 0 && K > 0 && K % 32 == 0, VGPT_ERR_INVALID,
                 "vgpt_gemm_mx8: M, N > 0 and K a positive multiple of 32 (got %lld, %lld, %lld)", (long long)M, (long long)N,
                 (long long)K);
    VGPT_REQUIRE(epilogue >= VGPT_MX8_EPI_NONE && epilogue <= VGPT_MX8_EPI_GATED, VGPT_ERR_INVALID, "vgpt_gemm_mx8: unknown epilogue %d",
                 epilogue);
    VGPT_REQUIRE(N % 32 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_gemm_mx8: N must be a multiple of 32");
    VGPT_REQUIRE(M < (1 << 26) && vgpt_mx8_bytes(M, K) < (1ll << 32) && vgpt_mx8_bytes(N, K) < (1ll << 32), VGPT_ERR_UNSUPPORTED,
                 "vgpt_gemm_mx8: problem too large");
    VGPT_REQUIRE((((uintptr_t)A8 | (uintptr_t)W8) & 255) == 0 && ((uintptr_t)C & 7) == 0 && ldc % 4 == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_gemm_mx8: records 256-byte aligned, C 8-byte aligned with ldc a multiple of 4");
    const int64_t out_cols = epilogue == VGPT_MX8_EPI_GATED ? N / 2 : N;
    VGPT_REQUIRE(ldc >= out_cols, VGPT_ERR_INVALID, "vgpt_gemm_mx8: ldc < output columns");
    GemmArgs g{};
    const int64_t KB = cdiv(K, 64);
    g.a_pay = (const uint8_t*)A8; g.a_sc = g.a_pay + align256(cdiv(M, 32) * KB * 2048);
    g.w_pay = (const uint8_t*)W8; g.w_sc = g.w_pay + align256(cdiv(N, 32) * KB * 2048);
    g.C = (bf16*)C; g.resid = (const bf16*)resid; g.rstd = rstd; g.cos_t = cos_t; g.sin_t = sin_t;
    g.M = (int)M; g.N = (int)N; g.KB = (int)KB; g.NG = (int)(N / 32); g.I = 0; g.rot_cols = 0;
    g.ldc = ldc; g.ldr = ldr; g.act = act;
    const hipStream_t s = (hipStream_t)stream;
    switch (epilogue) {
        case VGPT_MX8_EPI_NONE: return launch_gemm<MX8_NONE, 2>(g, 4, s);
        case VGPT_MX8_EPI_RESID:
            VGPT_REQUIRE(resid != nullptr, VGPT_ERR_INVALID, "vgpt_gemm_mx8: null pointer (resid)");
            VGPT_REQUIRE(ldr >= N && ldr % 4 == 0 && ((uintptr_t)resid & 7) == 0, VGPT_ERR_UNSUPPORTED,
                         "vgpt_gemm_mx8: resid 8-byte aligned with ldr >= N a multiple of 4");
            return launch_gemm<MX8_RESID, 2>(g, 4, s);
        case VGPT_MX8_EPI_ROPE:
            VGPT_REQUIRE(rstd && cos_t && sin_t, VGPT_ERR_INVALID, "vgpt_gemm_mx8: null pointer (rstd / cos / sin)");
            VGPT_REQUIRE(head_dim == 96 && N % 96 == 0 && n_rot_heads >= 0 && (int64_t)n_rot_heads * 96 <= N, VGPT_ERR_UNSUPPORTED,
                         "vgpt_gemm_mx8: the RoPE epilogue takes head_dim 96, N a multiple of 96");
            VGPT_REQUIRE((((uintptr_t)cos_t | (uintptr_t)sin_t) & 15) == 0, VGPT_ERR_UNSUPPORTED,
                         "vgpt_gemm_mx8: cos / sin 16-byte aligned");
            g.rot_cols = n_rot_heads * 96;
            return launch_gemm<MX8_ROPE, 3>(g, 6, s);
        default:
            VGPT_REQUIRE(rstd != nullptr, VGPT_ERR_INVALID, "vgpt_gemm_mx8: null pointer (rstd)");
            VGPT_REQUIRE(N % 64 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_gemm_mx8: the gated epilogue takes N = 2 I with I a multiple of 32");
            VGPT_REQUIRE(act >= VGPT_ACT_SILU && act <= VGPT_ACT_NONE, VGPT_ERR_INVALID, "vgpt_gemm_mx8: unknown activation");
            g.I = (int)(N / 2); g.NG = (int)(N / 64);
            return launch_gemm<MX8_GATED, 4>(g, 4, s);
    }
}

// vgpt_gemm_mx8 whose RoPE epilogue takes heads of 64, 96 or 128 columns (one head per wave: WN = head_dim / 32); head_dim 96
// launches the instantiation vgpt_gemm_mx8 launches, the other epilogues are vgpt_gemm_mx8 itself
VGPT_EXPORT int vgpt_gemm_mx8_hd(const void* A8, const void* W8, void* C, const void* resid, const float* rstd, const float* cos_t,
                                 const float* sin_t, int64_t M, int64_t N, int64_t K, int64_t ldc, int64_t ldr, int epilogue,
                                 int n_rot_heads, int head_dim, int act, void* stream) {
    const char* name = "vgpt_gemm_mx8_hd";
    VGPT_REQUIRE(epilogue >= VGPT_MX8_EPI_NONE && epilogue <= VGPT_MX8_EPI_GATED, VGPT_ERR_INVALID, "%s: unknown epilogue %d", name,
                 epilogue);
    if (epilogue != VGPT_MX8_EPI_ROPE)
        return vgpt_gemm_mx8(A8, W8, C, resid, rstd, cos_t, sin_t, M, N, K, ldc, ldr, epilogue, n_rot_heads, head_dim, act, stream);
    VGPT_REQUIRE(A8 && W8 && C, VGPT_ERR_INVALID, "%s: null pointer", name);
    VGPT_REQUIRE(M > 0 && N > 0 && K > 0 && K % 32 == 0, VGPT_ERR_INVALID,
                 "%s: M, N > 0 and K a positive multiple of 32 (got %lld, %lld, %lld)", name, (long long)M, (long long)N, (long long)K);
    VGPT_REQUIRE(N % 32 == 0, VGPT_ERR_UNSUPPORTED, "%s: N must be a multiple of 32 (got %lld)", name, (long long)N);
    VGPT_REQUIRE(M < (1 << 26) && vgpt_mx8_bytes(M, K) < (1ll << 32) && vgpt_mx8_bytes(N, K) < (1ll << 32), VGPT_ERR_UNSUPPORTED,
                 "%s: problem too large (M %lld, N %lld, K %lld)", name, (long long)M, (long long)N, (long long)K);
    VGPT_REQUIRE((((uintptr_t)A8 | (uintptr_t)W8) & 255) == 0 && ((uintptr_t)C & 7) == 0 && ldc % 4 == 0, VGPT_ERR_UNSUPPORTED,
                 "%s: records 256-byte aligned, C 8-byte aligned with ldc a multiple of 4 (got A8 %p, W8 %p, C %p, ldc %lld)", name, A8,
                 W8, C, (long long)ldc);
    VGPT_REQUIRE(ldc >= N, VGPT_ERR_INVALID, "%s: ldc %lld < output columns %lld", name, (long long)ldc, (long long)N);
    VGPT_REQUIRE(rstd && cos_t && sin_t, VGPT_ERR_INVALID, "%s: null pointer (rstd / cos / sin)", name);
    VGPT_REQUIRE(head_dim == 64 || head_dim == 96 || head_dim == 128, VGPT_ERR_UNSUPPORTED,
                 "%s: the RoPE epilogue takes head_dim 64, 96 or 128 (got %d)", name, head_dim);
    VGPT_REQUIRE(N % head_dim == 0 && n_rot_heads >= 0 && (int64_t)n_rot_heads * head_dim <= N, VGPT_ERR_UNSUPPORTED,
                 "%s: the RoPE epilogue takes N a multiple of head_dim and n_rot_heads * head_dim <= N (got N %lld, head_dim %d, "
                 "n_rot_heads %d)", name, (long long)N, head_dim, n_rot_heads);
    VGPT_REQUIRE((((uintptr_t)cos_t | (uintptr_t)sin_t) & 15) == 0, VGPT_ERR_UNSUPPORTED, "%s: cos / sin 16-byte aligned (got %p, %p)",
                 name, (const void*)cos_t, (const void*)sin_t);
    GemmArgs g{};
    const int64_t KB = cdiv(K, 64);
    g.a_pay = (const uint8_t*)A8; g.a_sc = g.a_pay + align256(cdiv(M, 32) * KB * 2048);
    g.w_pay = (const uint8_t*)W8; g.w_sc = g.w_pay + align256(cdiv(N, 32) * KB * 2048);
    g.C = (bf16*)C; g.resid = nullptr; g.rstd = rstd; g.cos_t = cos_t; g.sin_t = sin_t;
    g.M = (int)M; g.N = (int)N; g.KB = (int)KB; g.NG = (int)(N / 32); g.I = 0; g.rot_cols = n_rot_heads * head_dim;
    g.ldc = ldc; g.ldr = ldr; g.act = act;
    const hipStream_t s = (hipStream_t)stream;
    if (head_dim == 64) return launch_gemm<MX8_ROPE, 2>(g, 4, s, name);
    if (head_dim == 128) return launch_gemm<MX8_ROPE, 4>(g, 8, s, name);
    return launch_gemm<MX8_ROPE, 3>(g, 6, s, name);
}
