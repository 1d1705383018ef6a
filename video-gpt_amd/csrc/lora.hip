// LoRA adapter products (include/vgpt.h, "LoRA adapters"): three bandwidth-bound products with one skinny side, the
// padded rank rp in {16, 32, 48, 64}.  Each streams its big bf16 operand once with 16-byte accesses and does the product on
// mfma_f32_16x16x32_bf16 (fragment maps: A[row = lane & 15][k = 8 (lane >> 4) + j], B[k = 8 (lane >> 4) + j][col = lane & 15],
// D[row = 4 (lane >> 4) + i][col = lane & 15]).  The small operand is staged through LDS in its NATURAL layout, whichever
// orientation the caller stores it in: where the reduction index is the contiguous one a fragment is one 16-byte row read,
// where it is the row index the fragment comes from ds_read_b64_tr_b16 (per 16 lanes a block of 4 rows x 16 columns,
// delivered column-major: lane i gets column i, row q in element q) -- no transposed copy is ever written.
//   vgpt_lora_down   : 32 rows of X per workgroup; the four waves are 2 row tiles x 2 halves of every k chunk, the halves are
//                      added through LDS in a fixed order.  X fragments go from global memory straight to registers.
//   vgpt_lora_up_add : a workgroup owns a column tile (a whole head under RoPE) and walks 256 rows in steps of 64: the MFMA
//                      result goes through an fp32 LDS tile so that Y is read and written in 16-byte row pieces, and a
//                      rotated pair (d, d + hd/2) is met by one thread.
//   vgpt_lora_grad   : the reduction runs over the rows of BOTH operands, so both chunks are staged as they lie in memory
//                      and both fragments are transposed reads.  M is cut into slices (a function of the shape alone); each
//                      slice stores its partial sums and a second kernel adds them in slice order: bit-identical run to run.
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (bf16)0.0f;
    return z;
}

// lane gets img[k0 + 8 (lane >> 4) + j][c0 + (lane & 15)], j = 0..7: an MFMA operand whose reduction index is the image's
// row.  Needs all 64 lanes active and every address inside the image (pad, don't mask).
__device__ __forceinline__ bf16x8 lds_tr_frag(const bf16* img, int pitch, int k0, int c0, int lane) {
    const int g = lane >> 4, li = lane & 15;
    const bf16* p = img + (k0 + 8 * g + (li >> 2)) * pitch + c0 + 4 * (li & 3);
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 4 * pitch));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ bf16x8 lds_row8(const bf16* img, int pitch, int row, int col) {
    return *reinterpret_cast<const bf16x8*>(img + row * pitch + col);
}

__device__ __forceinline__ bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// ---------------------------------------------------------------------------------------------------------------------
// down: U (M, 16 R) = alpha X (M, K; ldx) S;  TR = 0: S is (16 R, K), TR = 1: S is (K, 16 R)
// ---------------------------------------------------------------------------------------------------------------------
template <int R>
struct DownCfg {
    static constexpr int RP = 16 * R;
    static constexpr int KC = R == 4 ? 128 : 256;   // k chunk: two LDS images of it stay below 64 KiB
    static constexpr int NS = KC / 64;              // 32-wide k steps of one wave's half chunk
    static constexpr int UPT = RP * KC / 8 / 256;   // 16-byte units of a chunk per thread
};

template <int R, bool TR>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16* __restrict__ X, int64_t ldx, const bf16* __restrict__ S,
                                                        bf16* __restrict__ U, int M, int K, float alpha) {
    using C = DownCfg<R>;
    constexpr int RP = C::RP, KC = C::KC, NS = C::NS, UPT = C::UPT, KH = KC / 2;
    constexpr int PITCH = TR ? RP + 8 : KC + 8;
    constexpr int IMG = TR ? KC * PITCH : RP * PITCH;
    __shared__ __attribute__((aligned(16))) bf16 simg[2][IMG];
    static_assert(IMG * 2 >= 2 * R * 4 * 64 * 4, "the k-half reduction reuses one image");

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rt = w & 1, kh = w >> 1;
    const int g = lane >> 4, li = lane & 15;
    const int64_t row = (int64_t)blockIdx.x * 32 + rt * 16 + li;
    const bool rv = row < M;
    const bf16* xrow = X + (rv ? row : 0) * ldx;

    f32x4 acc[R];
#pragma unroll
    for (int t = 0; t < R; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    bf16x8 xc[NS], xn[NS], sn[UPT];
    auto load_x = [&](int kbase, bf16x8* dst) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = kbase + kh * KH + 32 * s + 8 * g;
            dst[s] = (rv && k < K) ? ld8(xrow + k) : zero8();
        }
    };
    auto load_s = [&](int kbase) {
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            const int u = tid + 256 * i;
            if (TR) {
                const int kk = u / (RP / 8), c = (u % (RP / 8)) * 8;
                sn[i] = (kbase + kk < K) ? ld8(S + (int64_t)(kbase + kk) * RP + c) : zero8();
            } else {
                const int r = u / (KC / 8), c = (u % (KC / 8)) * 8;
                sn[i] = (kbase + c < K) ? ld8(S + (int64_t)r * K + kbase + c) : zero8();
            }
        }
    };
    auto store_s = [&](bf16* img) {
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            const int u = tid + 256 * i;
            const int r = TR ? u / (RP / 8) : u / (KC / 8);
            const int c = TR ? (u % (RP / 8)) * 8 : (u % (KC / 8)) * 8;
            *reinterpret_cast<bf16x8*>(img + r * PITCH + c) = sn[i];
        }
    };

    const int nchunks = (K + KC - 1) / KC;
    load_s(0);
    load_x(0, xc);
    store_s(simg[0]);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;
        if (more) {
            load_s((c + 1) * KC);
            load_x((c + 1) * KC, xn);
        }
        const bf16* img = simg[c & 1];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int kk = kh * KH + 32 * s;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const bf16x8 b = TR ? lds_tr_frag(img, PITCH, kk, 16 * t, lane) : lds_row8(img, PITCH, 16 * t + li, kk + 8 * g);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[s], b, acc[t], 0, 0, 0);
            }
        }
        if (more) {
            store_s(simg[(c + 1) & 1]);
#pragma unroll
            for (int s = 0; s < NS; ++s) xc[s] = xn[s];
        }
        __syncthreads();
    }
    // the upper k halves hand their sums to the lower ones: (lower + upper), always in that order
    float* red = reinterpret_cast<float*>(&simg[0][0]);
    if (kh == 1) {
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[((rt * R + t) * 4 + i) * 64 + lane] = acc[t][i];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t orow = (int64_t)blockIdx.x * 32 + rt * 16 + 4 * g + i;
                if (orow < M) U[orow * RP + 16 * t + li] = f2bf(alpha * (acc[t][i] + red[((rt * R + t) * 4 + i) * 64 + lane]));
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// up_add: Y (M, N; ldy) = bf16(rope?(float(Y) + alpha U (M, rp) S));  TR = 0: S is (N, rp), TR = 1: S is (rp, N)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int UP_ROWS = 64;        // rows of one pass (4 waves x 16)
constexpr int UP_CT_MAX = 128;     // widest column tile (= largest head_dim under RoPE)
constexpr int UP_ROWS_PER_WG = 256;
constexpr int UP_DP = UP_CT_MAX + 4;

template <bool TR>
__global__ __launch_bounds__(256) void lora_up_add_kernel(bf16* __restrict__ Y, int64_t ldy, const bf16* __restrict__ U,
                                                          const bf16* __restrict__ S, const float* __restrict__ cos_t,
                                                          const float* __restrict__ sin_t, int M, int N, int rp, int CT,
                                                          int n_rot_cols, float alpha) {
    // S tile: TR: [64 ranks (zero from rp on)][CT + 8];  else [CT][rp + 8]
    __shared__ __attribute__((aligned(16))) bf16 simg[UP_CT_MAX * (64 + 8)];
    __shared__ __attribute__((aligned(16))) float delta[UP_ROWS * UP_DP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, li = lane & 15;
    const int n0 = blockIdx.x * CT;
    const int ncols = min(CT, N - n0);
    const int pitch = TR ? CT + 8 : rp + 8;
    const int ntl = CT / 16, ks = (rp + 31) / 32;

    if (TR) {
        const int upr = CT / 8;
        for (int u = tid; u < 64 * upr; u += 256) {
            const int r = u / upr, c = (u % upr) * 8;
            *reinterpret_cast<bf16x8*>(simg + r * pitch + c) = (r < rp && c < ncols) ? ld8(S + (int64_t)r * N + n0 + c) : zero8();
        }
    } else {
        const int upr = rp / 8;
        for (int u = tid; u < CT * upr; u += 256) {
            const int n = u / upr, c = (u % upr) * 8;
            *reinterpret_cast<bf16x8*>(simg + n * pitch + c) = (n < ncols) ? ld8(S + (int64_t)(n0 + n) * rp + c) : zero8();
        }
    }
    __syncthreads();

    const bool rot = cos_t != nullptr && n0 < n_rot_cols;
    const int64_t mbeg = (int64_t)blockIdx.y * UP_ROWS_PER_WG;
    for (int rb = 0; rb < UP_ROWS_PER_WG / UP_ROWS; ++rb) {
        const int64_t m0 = mbeg + rb * UP_ROWS;
        if (m0 >= M) break;
        const int64_t arow = m0 + 16 * w + li;
        bf16x8 a[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = 32 * s + 8 * g;
            a[s] = (arow < M && k < rp) ? ld8(U + arow * rp + k) : zero8();
        }
#pragma unroll
        for (int nt = 0; nt < UP_CT_MAX / 16; ++nt) {
            if (nt < ntl) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (s < ks) {
                        bf16x8 b;
                        if (TR) {
                            b = lds_tr_frag(simg, pitch, 32 * s, 16 * nt, lane);
                        } else {
                            const int k = 32 * s + 8 * g;
                            b = k < rp ? lds_row8(simg, pitch, 16 * nt + li, k) : zero8();
                        }
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], b, acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) delta[(16 * w + 4 * g + i) * UP_DP + 16 * nt + li] = alpha * acc[i];
            }
        }
        __syncthreads();
        if (!rot) {
            const int upr = CT / 8;
            for (int u = tid; u < UP_ROWS * upr; u += 256) {
                const int r = u / upr, c = (u % upr) * 8;
                if (m0 + r < M && c < ncols) {
                    bf16* yp = Y + (m0 + r) * ldy + n0 + c;
                    const bf16x8 y = ld8(yp);
                    const float* d = delta + r * UP_DP + c;
                    bf16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(y[j]) + d[j]);
                    *reinterpret_cast<bf16x8*>(yp) = o;
                }
            }
        } else {
            // a whole head: thread meets columns [c, c + 8) and [c + half, c + half + 8) of one row
            const int half = CT / 2, upr = half / 8;
            for (int u = tid; u < UP_ROWS * upr; u += 256) {
                const int r = u / upr, c = (u % upr) * 8;
                if (m0 + r < M) {
                    bf16* yp = Y + (m0 + r) * ldy + n0 + c;
                    const bf16x8 ylo = ld8(yp), yhi = ld8(yp + half);
                    const float* d = delta + r * UP_DP + c;
                    const float* cp = cos_t + (m0 + r) * half + c;
                    const float* sp = sin_t + (m0 + r) * half + c;
                    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cp), c1 = *reinterpret_cast<const f32x4*>(cp + 4);
                    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1 = *reinterpret_cast<const f32x4*>(sp + 4);
                    bf16x8 olo, ohi;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float cs = j < 4 ? c0[j & 3] : c1[j & 3], sn = j < 4 ? s0[j & 3] : s1[j & 3];
                        const float x0 = bf2f(ylo[j]) + d[j], x1 = bf2f(yhi[j]) + d[half + j];
                        olo[j] = f2bf(x0 * cs - x1 * sn);
                        ohi[j] = f2bf(x1 * cs + x0 * sn);
                    }
                    *reinterpret_cast<bf16x8*>(yp) = olo;
                    *reinterpret_cast<bf16x8*>(yp + half) = ohi;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// grad: G (N, 16 R) fp32 = alpha Y (M, N; ldy)^T U (M, 16 R; ldu), optionally stored (16 R, N)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GR_NT = 128;   // columns of Y per workgroup (two 16-column tiles per wave)
constexpr int GR_MC = 64;    // rows per chunk
constexpr int GR_YP = GR_NT + 8;
constexpr int GR_TARGET_WGS = 1024;

template <int R>
__global__ __launch_bounds__(256) void lora_grad_kernel(const bf16* __restrict__ Y, int64_t ldy, const bf16* __restrict__ U,
                                                        int64_t ldu, float* __restrict__ out, int M, int N,
                                                        int chunks_per_slice, float alpha, int direct, int transposed) {
    constexpr int RP = 16 * R, UP = RP + 8;
    __shared__ __attribute__((aligned(16))) bf16 yimg[GR_MC * GR_YP];
    __shared__ __attribute__((aligned(16))) bf16 uimg[GR_MC * UP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, li = lane & 15;
    const int n0 = blockIdx.x * GR_NT;
    const int64_t mbeg = (int64_t)blockIdx.y * chunks_per_slice * GR_MC;
    const int64_t mend = min((int64_t)M, mbeg + (int64_t)chunks_per_slice * GR_MC);
    const int nchunks = (int)((mend - mbeg + GR_MC - 1) / GR_MC);

    f32x4 acc[2][R];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < R; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    bf16x8 yr[4], ur[2];
    auto load = [&](int c) {
        const int64_t m0 = mbeg + (int64_t)c * GR_MC;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + 256 * i, r = u >> 4, col = (u & 15) * 8;
            yr[i] = (m0 + r < mend && n0 + col < N) ? ld8(Y + (m0 + r) * ldy + n0 + col) : zero8();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + 256 * i;
            if (u < GR_MC * (RP / 8)) {
                const int r = u / (RP / 8), col = (u % (RP / 8)) * 8;
                ur[i] = (m0 + r < mend) ? ld8(U + (m0 + r) * ldu + col) : zero8();
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + 256 * i, r = u >> 4, col = (u & 15) * 8;
            *reinterpret_cast<bf16x8*>(yimg + r * GR_YP + col) = yr[i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + 256 * i;
            if (u < GR_MC * (RP / 8)) {
                const int r = u / (RP / 8), col = (u % (RP / 8)) * 8;
                *reinterpret_cast<bf16x8*>(uimg + r * UP + col) = ur[i];
            }
        }
    };

    if (nchunks > 0) load(0);
    for (int c = 0; c < nchunks; ++c) {
        store();
        __syncthreads();
        if (c + 1 < nchunks) load(c + 1);
#pragma unroll
        for (int s = 0; s < GR_MC / 32; ++s) {
            bf16x8 a[2], b[R];
#pragma unroll
            for (int j = 0; j < 2; ++j) a[j] = lds_tr_frag(yimg, GR_YP, 32 * s, 16 * (2 * w + j), lane);
#pragma unroll
            for (int t = 0; t < R; ++t) b[t] = lds_tr_frag(uimg, UP, 32 * s, 16 * t, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < R; ++t) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[t], acc[j][t], 0, 0, 0);
        }
        __syncthreads();
    }
    // D[row = n][col = r]
    float* part = direct ? out : out + (int64_t)blockIdx.y * N * RP;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + 16 * (2 * w + j) + 4 * g + i, r = 16 * t + li;
                if (n < N) {
                    if (!direct) part[(int64_t)n * RP + r] = acc[j][t][i];
                    else if (transposed) out[(int64_t)r * N + n] = alpha * acc[j][t][i];
                    else out[(int64_t)n * RP + r] = alpha * acc[j][t][i];
                }
            }
}

// G = alpha * (slice 0 + slice 1 + ...), in slice order
__global__ __launch_bounds__(256) void lora_grad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int N,
                                                               int rp, int slices, float alpha, int transposed) {
    const int64_t total = (int64_t)N * rp;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float s = ws[idx];
    for (int k = 1; k < slices; ++k) s += ws[(int64_t)k * total + idx];
    const int n = (int)(idx / rp), r = (int)(idx % rp);
    out[transposed ? (int64_t)r * N + n : idx] = alpha * s;
}

bool bad_rp(int rp) { return rp != 16 && rp != 32 && rp != 48 && rp != 64; }
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// slices of M and 64-row chunks per slice: a function of the shape alone
void grad_plan(int64_t M, int64_t N, int* slices, int* cps) {
    const int64_t chunks = cdiv(M, GR_MC), colblocks = cdiv(N, GR_NT);
    int64_t want = GR_TARGET_WGS / colblocks;
    if (want < 1) want = 1;
    if (want > chunks) want = chunks;
    *cps = (int)cdiv(chunks, want);
    *slices = (int)cdiv(chunks, *cps);
}

}  // namespace

VGPT_EXPORT int vgpt_lora_down(const void* X, const void* S, void* U, int64_t M, int64_t K, int rp, int64_t ldx,
                               int s_is_k_by_rp, float alpha, void* stream) {
    VGPT_REQUIRE(X && S && U, VGPT_ERR_INVALID, "vgpt_lora_down: null pointer");
    VGPT_REQUIRE(M > 0 && K > 0 && M < (1ll << 31) && K < (1ll << 31), VGPT_ERR_INVALID, "vgpt_lora_down: bad size M=%lld K=%lld",
                 (long long)M, (long long)K);
    VGPT_REQUIRE(!bad_rp(rp), VGPT_ERR_UNSUPPORTED, "vgpt_lora_down: padded rank %d not in {16, 32, 48, 64}", rp);
    VGPT_REQUIRE(K % 8 == 0, VGPT_ERR_INVALID, "vgpt_lora_down: K=%lld is not a multiple of 8", (long long)K);
    VGPT_REQUIRE(ldx >= K && ldx % 8 == 0, VGPT_ERR_INVALID, "vgpt_lora_down: ldx=%lld < K=%lld or not a multiple of 8",
                 (long long)ldx, (long long)K);
    VGPT_REQUIRE(!misaligned(X) && !misaligned(S) && !misaligned(U), VGPT_ERR_INVALID,
                 "vgpt_lora_down: operands must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(M, 32)), block(256);
    const bf16 *x = (const bf16*)X, *s = (const bf16*)S;
    bf16* u = (bf16*)U;
#define VGPT_DOWN(R_)                                                                                      \
    case R_:                                                                                               \
        if (s_is_k_by_rp) lora_down_kernel<R_, true><<<grid, block, 0, st>>>(x, ldx, s, u, (int)M, (int)K, alpha); \
        else lora_down_kernel<R_, false><<<grid, block, 0, st>>>(x, ldx, s, u, (int)M, (int)K, alpha);     \
        break;
    switch (rp / 16) {
        VGPT_DOWN(1) VGPT_DOWN(2) VGPT_DOWN(3) VGPT_DOWN(4)
    }
#undef VGPT_DOWN
    VGPT_CHECK_LAUNCH("vgpt_lora_down");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_lora_up_add(void* Y, const void* U, const void* S, const float* cos_t, const float* sin_t, int64_t M,
                                 int64_t N, int rp, int64_t ldy, int s_is_rp_by_n, int n_heads, int n_kv_heads, int head_dim,
                                 float alpha, void* stream) {
    VGPT_REQUIRE(Y && U && S, VGPT_ERR_INVALID, "vgpt_lora_up_add: null pointer");
    VGPT_REQUIRE((cos_t == nullptr) == (sin_t == nullptr), VGPT_ERR_INVALID,
                 "vgpt_lora_up_add: null pointer (cos and sin tables come together)");
    VGPT_REQUIRE(M > 0 && N > 0 && M < (1ll << 31) && N < (1ll << 31), VGPT_ERR_INVALID,
                 "vgpt_lora_up_add: bad size M=%lld N=%lld", (long long)M, (long long)N);
    VGPT_REQUIRE(!bad_rp(rp), VGPT_ERR_UNSUPPORTED, "vgpt_lora_up_add: padded rank %d not in {16, 32, 48, 64}", rp);
    VGPT_REQUIRE(N % 8 == 0, VGPT_ERR_INVALID, "vgpt_lora_up_add: N=%lld is not a multiple of 8", (long long)N);
    VGPT_REQUIRE(ldy >= N && ldy % 8 == 0, VGPT_ERR_INVALID, "vgpt_lora_up_add: ldy=%lld < N=%lld or not a multiple of 8",
                 (long long)ldy, (long long)N);
    VGPT_REQUIRE(!misaligned(Y) && !misaligned(S) && !misaligned(U) && !misaligned(cos_t) && !misaligned(sin_t),
                 VGPT_ERR_INVALID, "vgpt_lora_up_add: operands must be 16-byte aligned");
    int ct = 64, n_rot_cols = 0;
    if (cos_t) {
        VGPT_REQUIRE(n_heads > 0 && n_kv_heads > 0 && head_dim > 0, VGPT_ERR_INVALID, "vgpt_lora_up_add: bad head counts");
        VGPT_REQUIRE(N % head_dim == 0 && (int64_t)(n_heads + 2 * n_kv_heads) * head_dim == N, VGPT_ERR_INVALID,
                     "vgpt_lora_up_add: head_dim=%d does not divide the q/k span: N=%lld is not (%d + 2 * %d) heads",
                     head_dim, (long long)N, n_heads, n_kv_heads);
        VGPT_REQUIRE(head_dim % 16 == 0 && head_dim <= UP_CT_MAX, VGPT_ERR_UNSUPPORTED,
                     "vgpt_lora_up_add: head_dim=%d (a multiple of 16 up to %d is built)", head_dim, UP_CT_MAX);
        ct = head_dim;
        n_rot_cols = (n_heads + n_kv_heads) * head_dim;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t gy = cdiv(M, UP_ROWS_PER_WG);
    VGPT_REQUIRE(gy <= 65535, VGPT_ERR_UNSUPPORTED, "vgpt_lora_up_add: M=%lld too large", (long long)M);
    const dim3 grid((unsigned)cdiv(N, ct), (unsigned)gy), block(256);
    if (s_is_rp_by_n)
        lora_up_add_kernel<true><<<grid, block, 0, st>>>((bf16*)Y, ldy, (const bf16*)U, (const bf16*)S, cos_t, sin_t, (int)M,
                                                         (int)N, rp, ct, n_rot_cols, alpha);
    else
        lora_up_add_kernel<false><<<grid, block, 0, st>>>((bf16*)Y, ldy, (const bf16*)U, (const bf16*)S, cos_t, sin_t, (int)M,
                                                          (int)N, rp, ct, n_rot_cols, alpha);
    VGPT_CHECK_LAUNCH("vgpt_lora_up_add");
    return VGPT_OK;
}

VGPT_EXPORT int64_t vgpt_lora_grad_workspace_bytes(int64_t M, int64_t N, int rp) {
    if (M <= 0 || N <= 0 || bad_rp(rp)) return 0;
    int slices, cps;
    grad_plan(M, N, &slices, &cps);
    return slices > 1 ? (int64_t)slices * N * rp * 4 : 0;
}

VGPT_EXPORT int vgpt_lora_grad(const void* Y, const void* U, float* G, int64_t M, int64_t N, int rp, int64_t ldy, int64_t ldu,
                               int store_transposed, float alpha, void* workspace, int64_t workspace_bytes, void* stream) {
    VGPT_REQUIRE(Y && U && G, VGPT_ERR_INVALID, "vgpt_lora_grad: null pointer");
    VGPT_REQUIRE(M > 0 && N > 0 && M < (1ll << 31) && N < (1ll << 31), VGPT_ERR_INVALID, "vgpt_lora_grad: bad size M=%lld N=%lld",
                 (long long)M, (long long)N);
    VGPT_REQUIRE(!bad_rp(rp), VGPT_ERR_UNSUPPORTED, "vgpt_lora_grad: padded rank %d not in {16, 32, 48, 64}", rp);
    VGPT_REQUIRE(N % 8 == 0, VGPT_ERR_INVALID, "vgpt_lora_grad: N=%lld is not a multiple of 8", (long long)N);
    VGPT_REQUIRE(ldy >= N && ldy % 8 == 0, VGPT_ERR_INVALID, "vgpt_lora_grad: ldy=%lld < N=%lld or not a multiple of 8",
                 (long long)ldy, (long long)N);
    VGPT_REQUIRE(ldu >= rp && ldu % 8 == 0, VGPT_ERR_INVALID, "vgpt_lora_grad: ldu=%lld < rp=%d or not a multiple of 8",
                 (long long)ldu, rp);
    VGPT_REQUIRE(!misaligned(Y) && !misaligned(U) && !misaligned(G), VGPT_ERR_INVALID,
                 "vgpt_lora_grad: operands must be 16-byte aligned");
    int slices, cps;
    grad_plan(M, N, &slices, &cps);
    const int64_t need = slices > 1 ? (int64_t)slices * N * rp * 4 : 0;
    VGPT_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && !misaligned(workspace)), VGPT_ERR_INVALID,
                 "vgpt_lora_grad: workspace of %lld bytes needed (vgpt_lora_grad_workspace_bytes), got %lld", (long long)need,
                 (long long)(workspace ? workspace_bytes : 0));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(N, GR_NT), (unsigned)slices), block(256);
    const int direct = slices == 1;
    float* dst = direct ? G : (float*)workspace;
#define VGPT_GRAD(R_)                                                                                                       \
    case R_:                                                                                                                \
        lora_grad_kernel<R_><<<grid, block, 0, st>>>((const bf16*)Y, ldy, (const bf16*)U, ldu, dst, (int)M, (int)N, cps, alpha, \
                                                     direct, store_transposed);                                             \
        break;
    switch (rp / 16) {
        VGPT_GRAD(1) VGPT_GRAD(2) VGPT_GRAD(3) VGPT_GRAD(4)
    }
#undef VGPT_GRAD
    VGPT_CHECK_LAUNCH("vgpt_lora_grad");
    if (!direct) {
        lora_grad_reduce_kernel<<<dim3((unsigned)cdiv(N * rp, 256)), block, 0, st>>>((const float*)workspace, G, (int)N, rp,
                                                                                     slices, alpha, store_transposed);
        VGPT_CHECK_LAUNCH("vgpt_lora_grad (slice sum)");
    }
    return VGPT_OK;
}
