// Ulysses sequence parallelism inside the sampler engine: the re-layouts around the two all-to-alls of a decoder layer.
//
// pack:   this rank's (rows, (nq + 2 nk) hd) post-RoPE q|k|v rows -> P chunks (P, rows, (nq/P + 2 nk/P) hd); chunk j holds
//         the q, k and v columns of rank j's heads, so ONE all-to-all carries q, k and v together and the received chunks,
//         concatenated in rank order, are the live rows of a fused qkv buffer of nq/P + 2 nk/P heads.
// unpack: the P received attention-output head blocks (P, rows, Dc) -> (rows, P Dc) in head order, the o_proj operand of
//         an unsharded step.
// Both are pure copies of 16-byte vectors: one thread per destination vector, so the stores are fully coalesced and the
// loads walk whole head blocks (hd = 96 -> 12 consecutive vectors).  Bandwidth-bound (kernel table).
//
// The sharded trainer (train.Stage1Trainer, sequence_parallel=True) runs the same two exchanges backwards, so it needs the
// two inverses:
// pack_ctx:        d(ctx) of this rank's rows (rows, P Dc) -> (P, rows, Dc): block i = the columns of rank i's heads.
// unpack_qkv_rope: the P received d(qkv) chunks (P, rows, (nq/P + 2 nk/P) hd) -> (rows, (nq + 2 nk) hd) in
//                  [q heads | k heads | v heads] order; with cos / sin tables the q and k heads are rotated on the way
//                  through (the trainer passes cos and -sin: the inverse rotation of the backward), with the arithmetic of
//                  vgpt_rope_qk_inplace (norm_rope.hip) on the same bf16 values: one thread per (d, d + hd/2) pair of
//                  vectors, fp32, one rounding.  The v columns stay bytes.
#include "common.h"

namespace {

constexpr int SP_BLOCK = 256;
constexpr int64_t SP_MAX_GRID = 8192;

__global__ __launch_bounds__(SP_BLOCK) void sp_pack_qkv_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                             uint32_t rows, uint32_t P, uint32_t qw, uint32_t kw,
                                                             uint32_t nq8, uint32_t w8, uint32_t total) {
    const uint32_t wl = qw + 2 * kw;            // vectors per destination row
    const uint32_t chunk = rows * wl;           // vectors per destination chunk
    for (uint32_t v = blockIdx.x * SP_BLOCK + threadIdx.x; v < total; v += gridDim.x * SP_BLOCK) {
        const uint32_t j = v / chunk;
        const uint32_t rem = v - j * chunk;
        const uint32_t t = rem / wl;
        const uint32_t c = rem - t * wl;
        uint32_t col;
        if (c < qw)
            col = j * qw + c;                                   // q heads of rank j
        else if (c < qw + kw)
            col = nq8 + j * kw + (c - qw);                      // k heads of rank j
        else
            col = nq8 + P * kw + j * kw + (c - qw - kw);        // v heads of rank j
        dst[v] = src[(uint64_t)t * w8 + col];
    }
}

__global__ __launch_bounds__(SP_BLOCK) void sp_unpack_ctx_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                               uint32_t rows, uint32_t dv, uint32_t P, uint32_t total) {
    const uint32_t rw = P * dv;                 // vectors per destination row
    for (uint32_t v = blockIdx.x * SP_BLOCK + threadIdx.x; v < total; v += gridDim.x * SP_BLOCK) {
        const uint32_t t = v / rw;
        const uint32_t c = v - t * rw;
        const uint32_t i = c / dv;
        const uint32_t cc = c - i * dv;
        dst[v] = src[((uint64_t)i * rows + t) * dv + cc];
    }
}

__global__ __launch_bounds__(SP_BLOCK) void sp_pack_ctx_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                             uint32_t rows, uint32_t dv, uint32_t P, uint32_t total) {
    const uint32_t block = rows * dv;           // vectors per destination block
    for (uint32_t v = blockIdx.x * SP_BLOCK + threadIdx.x; v < total; v += gridDim.x * SP_BLOCK) {
        const uint32_t i = v / block;
        const uint32_t rem = v - i * block;
        const uint32_t t = rem / dv;
        const uint32_t c = rem - t * dv;
        dst[v] = src[((uint64_t)t * P + i) * dv + c];
    }
}

// source vector (of the (P, rows, wl) chunks) of destination column `col` (in vectors) of row t
__device__ __forceinline__ uint64_t sp_chunk_index(uint32_t t, uint32_t col, uint32_t rows, uint32_t P, uint32_t qw,
                                                   uint32_t kw, uint32_t nq8) {
    const uint32_t wl = qw + 2 * kw;
    uint32_t j, c;
    if (col < nq8) {                                            // q heads of rank j
        j = col / qw;
        c = col - j * qw;
    } else if (col < nq8 + P * kw) {                            // k heads of rank j
        const uint32_t cc = col - nq8;
        j = cc / kw;
        c = qw + (cc - j * kw);
    } else {                                                    // v heads of rank j
        const uint32_t cc = col - nq8 - P * kw;
        j = cc / kw;
        c = qw + kw + (cc - j * kw);
    }
    return ((uint64_t)j * rows + t) * wl + c;
}

__global__ __launch_bounds__(SP_BLOCK) void sp_unpack_qkv_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                               uint32_t rows, uint32_t P, uint32_t qw, uint32_t kw,
                                                               uint32_t nq8, uint32_t w8, uint32_t total) {
    for (uint32_t v = blockIdx.x * SP_BLOCK + threadIdx.x; v < total; v += gridDim.x * SP_BLOCK) {
        const uint32_t t = v / w8;
        const uint32_t col = v - t * w8;
        dst[v] = src[sp_chunk_index(t, col, rows, P, qw, kw, nq8)];
    }
}

// Work items of a row: (nq + nk) * half8 rotated pairs (two source and two destination vectors each), then the v vectors.
__global__ __launch_bounds__(SP_BLOCK) void sp_unpack_qkv_rope_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                    const float* __restrict__ cos_t,
                                                                    const float* __restrict__ sin_t, uint32_t rows,
                                                                    uint32_t P, uint32_t qw, uint32_t kw, uint32_t nq8,
                                                                    uint32_t w8, uint32_t half8, uint32_t total) {
    const uint32_t rot8 = nq8 + P * kw;         // vectors of the q and k heads of a row
    const uint32_t pairs = rot8 / 2;
    const uint32_t per_row = pairs + P * kw;    // work items per row
    const uint32_t half = half8 * 8;
    for (uint32_t it = blockIdx.x * SP_BLOCK + threadIdx.x; it < total; it += gridDim.x * SP_BLOCK) {
        const uint32_t t = it / per_row;
        const uint32_t r = it - t * per_row;
        if (r >= pairs) {                                       // v: bytes
            const uint32_t col = rot8 + (r - pairs);
            dst[(uint64_t)t * w8 + col] = src[sp_chunk_index(t, col, rows, P, qw, kw, nq8)];
            continue;
        }
        const uint32_t head = r / half8;
        const uint32_t c = r - head * half8;
        const uint32_t col = head * 2 * half8 + c;              // first half of the head; the partner is half8 further
        const uint64_t s1 = sp_chunk_index(t, col, rows, P, qw, kw, nq8);     // both halves lie in the same chunk row
        const uint4 r1 = src[s1], r2 = src[s1 + half8];
        const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(&r1), x2 = *reinterpret_cast<const bf16x8*>(&r2);
        const float* cp = cos_t + (uint64_t)t * half + c * 8;
        const float* sp = sin_t + (uint64_t)t * half + c * 8;
        f32x4 c0 = *reinterpret_cast<const f32x4*>(cp), c1 = *reinterpret_cast<const f32x4*>(cp + 4);
        f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1v = *reinterpret_cast<const f32x4*>(sp + 4);
        bf16x8 o1, o2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float cs = j < 4 ? c0[j & 3] : c1[j & 3];
            const float sn = j < 4 ? s0[j & 3] : s1v[j & 3];
            const float a = bf2f(x1[j]), b = bf2f(x2[j]);
            // vgpt_rope_qk_inplace's expressions, to the letter: q*cos + rotate_half(q)*sin, rotate_half(x) = [-x2 | x1]
            o1[j] = f2bf(a * cs - b * sn);
            o2[j] = f2bf(b * cs + a * sn);
        }
        uint4* d = dst + (uint64_t)t * w8 + col;
        d[0] = *reinterpret_cast<const uint4*>(&o1);
        d[half8] = *reinterpret_cast<const uint4*>(&o2);
    }
}

unsigned sp_grid(int64_t total) { return (unsigned)std::min<int64_t>(cdiv(total, SP_BLOCK), SP_MAX_GRID); }

}  // namespace

VGPT_EXPORT int vgpt_sp_pack_qkv(const void* qkv, void* out, int64_t rows, int n_heads, int n_kv_heads, int head_dim,
                                 int n_ranks, void* stream) {
    VGPT_REQUIRE(qkv && out, VGPT_ERR_INVALID, "vgpt_sp_pack_qkv: null pointer");
    VGPT_REQUIRE(rows >= 0 && n_heads > 0 && n_kv_heads > 0 && head_dim > 0 && n_ranks > 0, VGPT_ERR_INVALID,
                 "vgpt_sp_pack_qkv: bad shape");
    VGPT_REQUIRE(n_heads % n_ranks == 0 && n_kv_heads % n_ranks == 0, VGPT_ERR_INVALID,
                 "vgpt_sp_pack_qkv: n_heads %d and n_kv_heads %d must be multiples of n_ranks %d", n_heads, n_kv_heads,
                 n_ranks);
    VGPT_REQUIRE(head_dim % 8 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_sp_pack_qkv: head_dim must be a multiple of 8");
    VGPT_REQUIRE((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_sp_pack_qkv: pointers must be 16-byte aligned");
    const int64_t w8 = (int64_t)(n_heads + 2 * n_kv_heads) * head_dim / 8;
    const int64_t total = rows * w8;
    VGPT_REQUIRE(total < ((int64_t)1 << 31), VGPT_ERR_UNSUPPORTED, "vgpt_sp_pack_qkv: more than 2^31 vectors");
    if (total == 0) return VGPT_OK;
    const uint32_t qw = (uint32_t)(n_heads / n_ranks * head_dim / 8), kw = (uint32_t)(n_kv_heads / n_ranks * head_dim / 8);
    hipLaunchKernelGGL(sp_pack_qkv_kernel, dim3(sp_grid(total)), dim3(SP_BLOCK), 0, (hipStream_t)stream,
                       (const uint4*)qkv, (uint4*)out, (uint32_t)rows, (uint32_t)n_ranks, qw, kw,
                       (uint32_t)(n_heads * head_dim / 8), (uint32_t)w8, (uint32_t)total);
    VGPT_CHECK_LAUNCH("vgpt_sp_pack_qkv");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sp_unpack_ctx(const void* blocks, void* out, int64_t rows, int64_t block_width, int n_ranks,
                                   void* stream) {
    VGPT_REQUIRE(blocks && out, VGPT_ERR_INVALID, "vgpt_sp_unpack_ctx: null pointer");
    VGPT_REQUIRE(rows >= 0 && block_width > 0 && n_ranks > 0, VGPT_ERR_INVALID, "vgpt_sp_unpack_ctx: bad shape");
    VGPT_REQUIRE(block_width % 8 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_sp_unpack_ctx: block_width must be a multiple of 8");
    VGPT_REQUIRE((((uintptr_t)blocks | (uintptr_t)out) & 15) == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_sp_unpack_ctx: pointers must be 16-byte aligned");
    const int64_t total = rows * n_ranks * (block_width / 8);
    VGPT_REQUIRE(total < ((int64_t)1 << 31), VGPT_ERR_UNSUPPORTED, "vgpt_sp_unpack_ctx: more than 2^31 vectors");
    if (total == 0) return VGPT_OK;
    hipLaunchKernelGGL(sp_unpack_ctx_kernel, dim3(sp_grid(total)), dim3(SP_BLOCK), 0, (hipStream_t)stream,
                       (const uint4*)blocks, (uint4*)out, (uint32_t)rows, (uint32_t)(block_width / 8), (uint32_t)n_ranks,
                       (uint32_t)total);
    VGPT_CHECK_LAUNCH("vgpt_sp_unpack_ctx");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sp_pack_ctx(const void* ctx, void* blocks, int64_t rows, int64_t block_width, int n_ranks,
                                 void* stream) {
    VGPT_REQUIRE(ctx && blocks, VGPT_ERR_INVALID, "vgpt_sp_pack_ctx: null pointer");
    VGPT_REQUIRE(rows >= 0 && block_width > 0 && n_ranks > 0, VGPT_ERR_INVALID, "vgpt_sp_pack_ctx: bad shape");
    VGPT_REQUIRE(block_width % 8 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_sp_pack_ctx: block_width must be a multiple of 8");
    VGPT_REQUIRE((((uintptr_t)ctx | (uintptr_t)blocks) & 15) == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_sp_pack_ctx: pointers must be 16-byte aligned");
    const int64_t total = rows * n_ranks * (block_width / 8);
    VGPT_REQUIRE(total < ((int64_t)1 << 31), VGPT_ERR_UNSUPPORTED, "vgpt_sp_pack_ctx: more than 2^31 vectors");
    if (total == 0) return VGPT_OK;
    hipLaunchKernelGGL(sp_pack_ctx_kernel, dim3(sp_grid(total)), dim3(SP_BLOCK), 0, (hipStream_t)stream,
                       (const uint4*)ctx, (uint4*)blocks, (uint32_t)rows, (uint32_t)(block_width / 8), (uint32_t)n_ranks,
                       (uint32_t)total);
    VGPT_CHECK_LAUNCH("vgpt_sp_pack_ctx");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sp_unpack_qkv_rope(const void* chunks, void* qkv, const float* cos_t, const float* sin_t, int64_t rows,
                                        int n_heads, int n_kv_heads, int head_dim, int n_ranks, void* stream) {
    VGPT_REQUIRE(chunks && qkv, VGPT_ERR_INVALID, "vgpt_sp_unpack_qkv_rope: null pointer");
    VGPT_REQUIRE((cos_t == nullptr) == (sin_t == nullptr), VGPT_ERR_INVALID,
                 "vgpt_sp_unpack_qkv_rope: cos and sin tables come together or not at all");
    VGPT_REQUIRE(rows >= 0 && n_heads > 0 && n_kv_heads > 0 && head_dim > 0 && n_ranks > 0, VGPT_ERR_INVALID,
                 "vgpt_sp_unpack_qkv_rope: bad shape");
    VGPT_REQUIRE(n_heads % n_ranks == 0 && n_kv_heads % n_ranks == 0, VGPT_ERR_INVALID,
                 "vgpt_sp_unpack_qkv_rope: n_heads %d and n_kv_heads %d must be multiples of n_ranks %d", n_heads,
                 n_kv_heads, n_ranks);
    VGPT_REQUIRE(head_dim % 8 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_sp_unpack_qkv_rope: head_dim must be a multiple of 8");
    VGPT_REQUIRE(!cos_t || head_dim % 16 == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_sp_unpack_qkv_rope: head_dim=%d needs head_dim/2 %% 8 == 0 to rotate", head_dim);
    VGPT_REQUIRE((((uintptr_t)chunks | (uintptr_t)qkv | (uintptr_t)cos_t | (uintptr_t)sin_t) & 15) == 0,
                 VGPT_ERR_UNSUPPORTED, "vgpt_sp_unpack_qkv_rope: pointers must be 16-byte aligned");
    const int64_t w8 = (int64_t)(n_heads + 2 * n_kv_heads) * head_dim / 8;
    const int64_t total = rows * w8;
    VGPT_REQUIRE(total < ((int64_t)1 << 31), VGPT_ERR_UNSUPPORTED, "vgpt_sp_unpack_qkv_rope: more than 2^31 vectors");
    if (total == 0) return VGPT_OK;
    const uint32_t qw = (uint32_t)(n_heads / n_ranks * head_dim / 8), kw = (uint32_t)(n_kv_heads / n_ranks * head_dim / 8);
    const uint32_t nq8 = (uint32_t)(n_heads * head_dim / 8);
    if (!cos_t) {
        hipLaunchKernelGGL(sp_unpack_qkv_kernel, dim3(sp_grid(total)), dim3(SP_BLOCK), 0, (hipStream_t)stream,
                           (const uint4*)chunks, (uint4*)qkv, (uint32_t)rows, (uint32_t)n_ranks, qw, kw, nq8, (uint32_t)w8,
                           (uint32_t)total);
    } else {
        const int64_t v8 = (int64_t)n_kv_heads * head_dim / 8;
        const int64_t items = rows * ((w8 - v8) / 2 + v8);
        hipLaunchKernelGGL(sp_unpack_qkv_rope_kernel, dim3(sp_grid(items)), dim3(SP_BLOCK), 0, (hipStream_t)stream,
                           (const uint4*)chunks, (uint4*)qkv, cos_t, sin_t, (uint32_t)rows, (uint32_t)n_ranks, qw, kw, nq8,
                           (uint32_t)w8, (uint32_t)(head_dim / 16), (uint32_t)items);
    }
    VGPT_CHECK_LAUNCH("vgpt_sp_unpack_qkv_rope");
    return VGPT_OK;
}
