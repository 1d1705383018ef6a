// Fused mid-block attention of the VAE (diffusers==0.29.0 AutoencoderKL mid-block `Attention`, one head over the HW
// positions of a frame; reached from LVM/pipeline.py:110-117 encode and :558-590 decode) in exact fp32.
//
//   s[j][i] = scale * sum_c k[c][j] q[c][i]     p[.][i] = softmax_j s[.][i]     o[c][i] = sum_j v[c][j] p[j][i]
//
// One pass with an online softmax: the score matrix lives in the accumulators of two MFMA tiles and never reaches LDS as
// a matrix or HBM at all.  Operands stay in the VAE's own [n][c][pos] layout.
//
// Work split.  A workgroup of four waves owns VGPT_VAE_ATTN_TQ = 64 queries of one image, as two 32-query halves, and walks
// the keys in tiles of VGPT_VAE_ATTN_TK = 32.  With C = 64 M channels:
//   - wave w keeps channels [w C/4, (w+1) C/4) of both Q halves in registers (C/4 per lane) and computes the partial S^T
//     of the key tile over that slice: per half C/8 v_mfma_f32_32x32x2_f32 on one accumulator, A = K^T (lane (i, h)
//     supplies k[c + h][key0 + i]: 32 consecutive positions of one channel, read straight from global memory: they need
//     no re-layout, no other wave reads them, and one K register feeds both halves), B = Q;
//   - the four partials are exchanged through LDS and summed by every wave in the order ((w0 + w1) + w2) + w3, so all
//     four hold the same S^T tiles;
//   - every wave runs the softmax update on them (scale, tail mask to -inf, running maximum, exp, running sum);
//   - wave w owns the 32-channel output tiles t = w, w + 4, ... < C/32.  P V: A = V (lane (i, h) supplies
//     v[32 t + i][key]), B = P^T = the S^T accumulator itself: register r of lane (query, h) holds key
//     (r & 3) + 8 (r >> 2) + 4 h, so feeding V in that key order needs no movement of P.  The V rows of a wave's own
//     tiles are staged through LDS (row stride 36 floats): 16-byte global loads and LDS writes when ld % 4 == 0 and the
//     base is 16-byte aligned, scalar loads otherwise; the lane then reads four consecutive keys, four MFMAs' worth of
//     A, with one ds_read_b128.  Keys past HW are staged as zeros.
// Prefetch: K runs through a ring of 8 registers, each refilled 8 channel pairs (16 MFMAs) ahead of its use, across the
// end of a key tile into the next; V of the next key tile is requested one output tile (32 MFMAs) before it is written
// to LDS, behind the P V product of the tile it replaces.  Row addresses are a scalar base plus one 32-bit lane offset.
// Registers at C = 512: 256 VGPRs + 239 AGPRs, no scratch, one wave per SIMD (so does the 136 KiB of LDS: 72 KiB of V
// tiles, two 32-KiB exchange buffers); C <= 128: two waves per SIMD.
// Every query column is computed by the same instruction sequence whichever half and workgroup it falls in.
//
// Rounding points: every product is an fp32 FMA chain (the MFMA's), channels ascending inside a wave's slice, then
// three adds for the four slices; x = s * scale; x - m; v_exp_f32 of (x - m) log2(e) (__expf); l = l * a + sum(p) with
// a = exp(m_old - m_new); o = o * a per key tile; P V is an FMA chain over the keys in the order above; o / l is an
// IEEE division.  No atomics, no workspace: the result is a pure function of the inputs.
#include "common.h"

namespace {

constexpr int TQ = VGPT_VAE_ATTN_TQ, TK = VGPT_VAE_ATTN_TK;
constexpr int QH = TQ / 32;                // 32-query halves of a workgroup's query tile
static_assert(QH == 2 && TK == 32, "the lane maps below are those of 32x32 MFMA tiles");
constexpr int V_LD = TK + 4;               // LDS row stride of a staged V row: 16-byte aligned rows, conflict-free b128
constexpr int V_TILE = 32 * V_LD;          // floats of one staged 32-channel x TK-key tile
constexpr int RED_FLOATS = 4 * QH * 16 * WAVE;  // one S^T partial per wave and half

template <int M>
struct AttnCfg {
    static constexpr int C = 64 * M;
    static constexpr int NK = C / 8;         // S^T MFMAs (two channels each) per wave, half and key tile
    static constexpr int OT = C / 32;        // output tiles of 32 channels
    static constexpr int NT = (OT + 3) / 4;  // output tiles per wave
    static constexpr bool EVEN = OT % 4 == 0;  // every wave owns NT tiles
    static constexpr int V_FLOATS = 4 * NT * V_TILE;
    static constexpr int LDS_BYTES = (V_FLOATS + 2 * RED_FLOATS) * 4;
};

template <int M>
__global__ __launch_bounds__(256) void vae_attn_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, float* __restrict__ o, int64_t HW,
                                                       int64_t ld, int64_t batch_stride, int64_t qtiles, float scale,
                                                       int vec) {
    using Cfg = AttnCfg<M>;
    constexpr int NK = Cfg::NK, NT = Cfg::NT, OT = Cfg::OT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // the wave index as a scalar: everything derived from it (channel slice, tile ownership, row addresses) stays in SGPRs,
    // and a row's address is a scalar base plus one 32-bit lane offset (the host refuses ld >= 2^28)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, h = lane >> 5;
    const int64_t n = blockIdx.x / qtiles, q0 = (blockIdx.x % qtiles) * TQ;
    const int64_t img = n * batch_stride;
    const int64_t ntiles = (HW + TK - 1) / TK;

    float* vbuf = smem + w * (NT * V_TILE);  // this wave's own V tiles
    float* red = smem + Cfg::V_FLOATS;

    // ---- Q slice of this wave, resident: q[c0 + 2m + h][q0 + 32 half + col] (query tail: clamped, never stored) ----
    const int64_t c0 = (int64_t)w * (Cfg::C / 4);
    constexpr int KR = 8;  // K registers: a ring of 8 channel pairs, refilled 8 pairs (16 MFMAs) ahead of their use
    static_assert(NK % KR == 0, "the ring wraps from one key tile into the next");
    float qr[QH][NK], kr[KR];
    const float* kbase = k + img + c0 * ld;
    const float* qbase = q + img + c0 * ld;
    const uint32_t hld = (uint32_t)(h * ld);
#pragma unroll
    for (int x = 0; x < QH; ++x) {
        const uint32_t qoff = hld + (uint32_t)min(q0 + 32 * x + col, HW - 1);
#pragma unroll
        for (int m = 0; m < NK; ++m) qr[x][m] = (qbase + (int64_t)(2 * m) * ld)[qoff];
    }
    uint32_t koff = hld + (uint32_t)min((int64_t)col, HW - 1);
#pragma unroll
    for (int m = 0; m < KR; ++m) kr[m] = (kbase + (int64_t)(2 * m) * ld)[koff];

    // ---- V staging: instruction e of tile u covers rows 8e + (lane >> 3), keys 4 (lane & 7) .. + 3 ----
    const int srow = lane >> 3, skey = (lane & 7) * 4;
    const float* vbase = v + img + (int64_t)(32 * w) * ld;
    const uint32_t voff = (uint32_t)(srow * ld + skey);
    f32x4 vn[4];  // one output tile's worth of V in flight
    auto load_v = [&](int u, int64_t key0) {
        if (Cfg::EVEN || w + 4 * u < OT) {
            const bool whole = vec && key0 + TK <= HW;  // wave-uniform: the whole tile is inside and 16-byte loads apply
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* p = vbase + (int64_t)(128 * u + 8 * e) * ld + key0 + voff;
                if (whole) {
                    vn[e] = *reinterpret_cast<const f32x4*>(p);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) vn[e][i] = key0 + skey + i < HW ? p[i] : 0.f;
                }
            }
        }
    };
    auto stage_v = [&](int u) {
        if (Cfg::EVEN || w + 4 * u < OT) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                *reinterpret_cast<f32x4*>(vbuf + u * V_TILE + (8 * e + srow) * V_LD + skey) = vn[e];
        }
    };
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        load_v(u, 0);
        stage_v(u);
    }

    f32x16 acc[QH][NT];
#pragma unroll
    for (int x = 0; x < QH; ++x)
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][u][r] = 0.f;
    float mrun[QH], lrun[QH];
#pragma unroll
    for (int x = 0; x < QH; ++x) mrun[x] = -INFINITY, lrun[x] = 0.f;

    for (int64_t t = 0; t < ntiles; ++t) {
        const int64_t key0 = t * TK;
        const bool has_next = t + 1 < ntiles;
        if (has_next) load_v(0, key0 + TK);
        const uint32_t knext = hld + (uint32_t)min(key0 + TK + col, HW - 1);

        // ---- partial S^T over this wave's channel slice, both halves on one K register ----
        f32x16 s[QH];
#pragma unroll
        for (int x = 0; x < QH; ++x)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[x][r] = 0.f;
#pragma unroll
        for (int m = 0; m < NK; ++m) {
#pragma unroll
            for (int x = 0; x < QH; ++x) s[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[m % KR], qr[x][m], s[x], 0, 0, 0);
            // refill the slot KR channel pairs ahead: this tile's, then the next tile's (past the last tile the position
            // is clamped: a load of valid memory that nothing uses)
            const int mm = (m + KR) % NK;
            kr[m % KR] = (kbase + (int64_t)(2 * mm) * ld)[m + KR < NK ? koff : knext];
        }

        // ---- sum the four slices in a fixed order (double-buffered: one barrier per key tile) ----
        float* rb = red + (t & 1) * RED_FLOATS;
#pragma unroll
        for (int x = 0; x < QH; ++x)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 part = {s[x][4 * g], s[x][4 * g + 1], s[x][4 * g + 2], s[x][4 * g + 3]};
                *reinterpret_cast<f32x4*>(rb + (((w * QH + x) * 4 + g) * WAVE + lane) * 4) = part;
            }
        __syncthreads();

        float alpha[QH];
#pragma unroll
        for (int x = 0; x < QH; ++x) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 p0 = *reinterpret_cast<const f32x4*>(rb + (((0 * QH + x) * 4 + g) * WAVE + lane) * 4);
                const f32x4 p1 = *reinterpret_cast<const f32x4*>(rb + (((1 * QH + x) * 4 + g) * WAVE + lane) * 4);
                const f32x4 p2 = *reinterpret_cast<const f32x4*>(rb + (((2 * QH + x) * 4 + g) * WAVE + lane) * 4);
                const f32x4 p3 = *reinterpret_cast<const f32x4*>(rb + (((3 * QH + x) * 4 + g) * WAVE + lane) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[x][4 * g + j] = ((p0[j] + p1[j]) + p2[j]) + p3[j];
            }

            // ---- online softmax over the keys of this column (register r: key (r & 3) + 8 (r >> 2) + 4 h) ----
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = (int)(HW - key0 > TK ? TK : HW - key0);  // live keys of this tile
                s[x][r] = (r & 3) + 8 * (r >> 2) + 4 * h < key ? s[x][r] * scale : -INFINITY;
                tmax = fmaxf(tmax, s[x][r]);
            }
            tmax = half_max(tmax);
            const float mnew = fmaxf(mrun[x], tmax);
            const float a_ = __expf(mrun[x] - mnew);
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[x][r] = __expf(s[x][r] - mnew);
                psum += s[x][r];
            }
            psum = half_sum(psum);
            lrun[x] = lrun[x] * a_ + psum;
            mrun[x] = mnew;

            alpha[x] = a_;
            __builtin_amdgcn_sched_barrier(0);  // one half's 16 partial reads and exponentials at a time: register budget
        }

        // ---- O = O * alpha + V P, one output tile at a time; behind each tile its V rows of the next key tile, requested
        //      a tile earlier, are staged and the following tile's are requested ----
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            if (Cfg::EVEN || w + 4 * u < OT) {
#pragma unroll
                for (int x = 0; x < QH; ++x)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[x][u][r] *= alpha[x];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(vbuf + u * V_TILE + col * V_LD + 8 * g + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int x = 0; x < QH; ++x)
                            acc[x][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], s[x][4 * g + j], acc[x][u], 0, 0, 0);
                }
            }
            if (has_next) {
                stage_v(u);
                if (u + 1 < NT) load_v(u + 1, key0 + TK);  // lands under the next tile's MFMAs
            }
            __builtin_amdgcn_sched_barrier(0);  // one output tile at a time
        }
        koff = knext;
    }

    // ---- o = O / l, plain dword stores, query tail guarded ----
#pragma unroll
    for (int x = 0; x < QH; ++x) {
        const int64_t qi = q0 + 32 * x + col;
        if (qi < HW) {
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int t = w + 4 * u;
                if (Cfg::EVEN || t < OT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t ch = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                        o[img + ch * ld + qi] = acc[x][u][r] / lrun[x];
                    }
                }
            }
        }
    }
}

template <int M>
int launch_attn(const float* q, const float* k, const float* v, float* o, int64_t N, int64_t HW, int64_t ld,
                int64_t batch_stride, float scale, int vec, hipStream_t s) {
    using Cfg = AttnCfg<M>;
    hipError_t e = hipFuncSetAttribute((const void*)vae_attn_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       Cfg::LDS_BYTES);
    if (e != hipSuccess) {
        vgpt_set_error("vgpt_vae_attn_fwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
        return VGPT_ERR_HIP;
    }
    const int64_t qtiles = cdiv(HW, TQ);
    hipLaunchKernelGGL(vae_attn_kernel<M>, dim3((unsigned)(N * qtiles)), dim3(256), Cfg::LDS_BYTES, s, q, k, v, o, HW, ld,
                       batch_stride, qtiles, scale, vec);
    VGPT_CHECK_LAUNCH("vgpt_vae_attn_fwd");
    return VGPT_OK;
}

bool overlaps(const float* a, const float* b, int64_t extent) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, n = (uintptr_t)extent * sizeof(float);
    return x < y + n && y < x + n;
}

}  // namespace

VGPT_EXPORT int vgpt_vae_attn_fwd(const float* q, const float* k, const float* v, float* o, int64_t N, int C, int64_t HW,
                                  int64_t ld, int64_t batch_stride, float scale, void* stream) {
    VGPT_REQUIRE(q && k && v && o, VGPT_ERR_INVALID, "vgpt_vae_attn_fwd: null pointer");
    VGPT_REQUIRE(N >= 0, VGPT_ERR_INVALID, "vgpt_vae_attn_fwd: N = %lld < 0", (long long)N);
    VGPT_REQUIRE(HW > 0, VGPT_ERR_INVALID, "vgpt_vae_attn_fwd: HW = %lld <= 0", (long long)HW);
    VGPT_REQUIRE(ld >= HW, VGPT_ERR_INVALID, "vgpt_vae_attn_fwd: ld = %lld < HW = %lld", (long long)ld, (long long)HW);
    VGPT_REQUIRE(scale > 0.f, VGPT_ERR_INVALID, "vgpt_vae_attn_fwd: scale = %g <= 0", (double)scale);
    VGPT_REQUIRE(C >= 64 && C <= VGPT_VAE_ATTN_MAX_C && C % 64 == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_vae_attn_fwd: C = %d (supported: multiples of 64 up to %d)", C, VGPT_VAE_ATTN_MAX_C);
    VGPT_REQUIRE(batch_stride >= (int64_t)C * ld, VGPT_ERR_INVALID, "vgpt_vae_attn_fwd: batch_stride = %lld < C * ld = %lld",
                 (long long)batch_stride, (long long)((int64_t)C * ld));
    if (N == 0) return VGPT_OK;
    const int64_t extent = (N - 1) * batch_stride + (int64_t)(C - 1) * ld + HW;
    VGPT_REQUIRE(!overlaps(o, q, extent) && !overlaps(o, k, extent) && !overlaps(o, v, extent), VGPT_ERR_INVALID,
                 "vgpt_vae_attn_fwd: o = %p overlaps an input (q %p, k %p, v %p, %lld floats each)", (const void*)o,
                 (const void*)q, (const void*)k, (const void*)v, (long long)extent);
    VGPT_REQUIRE(ld < (int64_t)1 << 28, VGPT_ERR_UNSUPPORTED, "vgpt_vae_attn_fwd: ld = %lld, 2^28 or more (32-bit lane offsets)",
                 (long long)ld);
    VGPT_REQUIRE(N * cdiv(HW, TQ) < (int64_t)1 << 31, VGPT_ERR_UNSUPPORTED,
                 "vgpt_vae_attn_fwd: N * ceil(HW / %d) = %lld workgroups, 2^31 or more", TQ, (long long)(N * cdiv(HW, TQ)));
    const int vec = ld % 4 == 0 && batch_stride % 4 == 0 && (uintptr_t)v % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    switch (C / 64) {
        case 1: return launch_attn<1>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
        case 2: return launch_attn<2>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
        case 3: return launch_attn<3>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
        case 4: return launch_attn<4>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
        case 5: return launch_attn<5>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
        case 6: return launch_attn<6>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
        case 7: return launch_attn<7>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
        default: return launch_attn<8>(q, k, v, o, N, HW, ld, batch_stride, scale, vec, s);
    }
}
