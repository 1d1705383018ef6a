// Ulysses sequence parallelism inside the sampler engine: the re-layouts around the two all-to-alls of a decoder layer.
//
// pack:   this rank's (rows, (nq + 2 nk) hd) post-RoPE q|k|v rows -> P chunks (P, rows, (nq/P + 2 nk/P) hd); chunk j holds
//         the q, k and v columns of rank j's heads, so ONE all-to-all carries q, k and v together and the received chunks,
//         concatenated in rank order, are the live rows of a fused qkv buffer of nq/P + 2 nk/P heads.
// unpack: the P received attention-output head blocks (P, rows, Dc) -> (rows, P Dc) in head order, the o_proj operand of
//         an unsharded step.
// Both are pure copies of 16-byte vectors: one thread per destination vector, so the stores are fully coalesced and the
// loads walk whole head blocks (hd = 96 -> 12 consecutive vectors).  Bandwidth-bound (kernel table).
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
