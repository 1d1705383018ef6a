/*
 * vgpt.h — C ABI of libvgpt_hip.so: the MI355X (gfx950) kernels behind the
 * next-clip diffusion hot path of Video-GPT.
 *
 * Every entry point replaces one piece of arithmetic the reference executes
 * through PyTorch ops; the reference site each one stands in for is cited as
 * `path:line` relative to the reference checkout (third-party pins:
 * transformers==4.47.1 Phi3 blocks, diffusers==0.29.0 AutoencoderKL).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless a parameter is named host_*;
 *   - outputs and workspaces are caller-allocated; nothing here allocates,
 *     frees or synchronises, so every call is capturable into a hipGraph;
 *   - `stream` is a hipStream_t passed as void*;
 *   - return 0 on success, <0 on failure (VGPT_ERR_*); the message of the last
 *     failure on the calling thread is returned by vgpt_last_error();
 *   - bf16 tensors are raw 16-bit bfloat16; "row-major" means last dim contiguous.
 */
#ifndef VGPT_H
#define VGPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGPT_OK 0
#define VGPT_ERR_INVALID (-1)     /* bad argument (null pointer, negative size, misaligned) */
#define VGPT_ERR_UNSUPPORTED (-2) /* shape outside what the kernel was built for */
#define VGPT_ERR_HIP (-3)         /* HIP runtime error at launch */

/* activation of the gated MLP (Phi3MLP: down(up * act(gate)); config.hidden_act) */
#define VGPT_ACT_SILU 0
#define VGPT_ACT_GELU 1      /* erf form  */
#define VGPT_ACT_GELU_TANH 2 /* tanh form */
#define VGPT_ACT_NONE 3

/* epilogues of vgpt_gemm_bf16 */
#define VGPT_EPI_NONE 0  /* C = A W^T                       */
#define VGPT_EPI_RESID 1 /* C = A W^T + R   (residual add)  */
#define VGPT_EPI_BIAS 2  /* C = A W^T + bias[n]             */

/* prediction type of the sampler (LVM/scheduler.py:178) */
#define VGPT_PRED_V 0
#define VGPT_PRED_X1 1

const char* vgpt_last_error(void);
/* VGPT_ABI_VERSION of the library that was loaded.  Bumped with EVERY change of an exported signature; a binding written
 * for another value must refuse to call (video-gpt_amd/_lib.py does): with shifted arguments a stale library would read a
 * stream pointer as a scale and fault on the device instead of failing cleanly. */
#define VGPT_ABI_VERSION 8
int vgpt_abi_version(void);

/* ---- transformer block -------------------------------------------------- */

/* Phi3RMSNorm (transformers 4.47.1 modeling_phi3.py Phi3RMSNorm.forward; call
 * sites OmniGen/transformer.py:196-214): y = bf16(bf16(x * rsqrt(mean(x^2)+eps)) * w),
 * fp32 accumulation. x,y: (rows, H) bf16 row-major; w: (H) bf16. H % 8 == 0. */
int vgpt_rmsnorm_fwd(const void* x, const void* w, void* y, int64_t rows, int64_t H, float eps,
                     void* stream);

/* Phi3RotaryEmbedding.forward (cos/sin table): cos/sin[t][i] = scale * f(pos[t] * inv_freq[i]),
 * i < half; rounded to bf16 and stored back as fp32 when round_bf16 != 0 (the
 * reference casts cos/sin to the model dtype, LVM/transform/sdpa_transform.py:52).  scale = 1 for
 * plain RoPE; for rope_scaling "su"/"longrope" checkpoints the caller passes the rescaled inv_freq
 * (short / long factors) and the attention factor as `scale` (HF Phi3LongRoPEScaledRotaryEmbedding). */
int vgpt_rope_table(const int64_t* position_ids, const float* inv_freq, float* cos_out,
                    float* sin_out, int64_t tokens, int half, int round_bf16, float scale, void* stream);

/* apply_rotary_pos_emb on the q and k parts of a fused qkv buffer, in place
 * (LVM/transform/sdpa_transform.py:53). qkv: (tokens, (n_q+2*n_kv)*hd) bf16;
 * cos,sin: (tokens, hd/2) fp32. (hd/2) % 8 == 0. */
int vgpt_rope_qk_inplace(void* qkv, const float* cos_t, const float* sin_t, int64_t tokens,
                         int n_q_heads, int n_kv_heads, int head_dim, void* stream);

/* nn.Linear without bias on MFMA: C[M,N] = A[M,K] W[N,K]^T (+ epilogue), bf16 in,
 * fp32 accumulate, bf16 out. Replaces qkv_proj / o_proj / down_proj
 * (LVM/transform/sdpa_transform.py:39,89; Phi3MLP.down_proj). K % 64 == 0, N % 4 == 0.
 * lda/ldw/ldc/ldr are row strides in elements. `extra` is R (M,N) for EPI_RESID,
 * bias (N) for EPI_BIAS, ignored for EPI_NONE. */
int vgpt_gemm_bf16(const void* A, const void* W, void* C, const void* extra, int64_t M, int64_t N,
                   int64_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int epilogue,
                   void* stream);

/* qkv_proj followed by apply_rotary_pos_emb in one kernel (LVM/transform/sdpa_transform.py:39,52-53): C = A W^T rounded
 * to bf16 (the Linear's output), then columns [0, n_rot_heads * head_dim) -- the q heads followed by the k heads --
 * rotated per token: out[d] = x[d] cos[d] - x[d + hd/2] sin[d], out[d + hd/2] = x[d + hd/2] cos[d] + x[d] sin[d] with
 * cos / sin (M, head_dim / 2) fp32 from vgpt_rope_table (row m = token m of A); the remaining columns (v) are stored
 * unrotated.  Same result as vgpt_gemm_bf16 + vgpt_rope_qk_inplace without writing and re-reading q and k.
 * N % 16 == 0, head_dim % 16 == 0, K % 64 == 0. */
int vgpt_gemm_bf16_rope(const void* A, const void* W, void* C, const float* cos_t, const float* sin_t, int64_t M,
                        int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldc, int n_rot_heads, int head_dim,
                        void* stream);
/* The same product with operands stored transposed, for the backward of the Linear layers without materialising a
 * transpose (the reference gets these from torch.autograd: dX = dY W, dW = dY^T X):
 *   w_transposed: W is stored (K, N) row-major (ldw = its row stride)   -> dX[M,N'] = dY[M,K'] W[K',N']
 *   a_transposed: A is stored (K, M) row-major; needs w_transposed      -> dW[N,K'] = dY^T X with A = dY, W = X
 * Widths of transposed operands must be multiples of 8; K % 64 == 0 unless BOTH operands are transposed (then the
 * rows of a partial last k-tile are zero-filled by the hardware's buffer range check).  A transposed operand must
 * stay below 2 GiB.  With both flags 0 this is vgpt_gemm_bf16. */
int vgpt_gemm_bf16_tr(const void* A, const void* W, void* C, const void* extra, int64_t M, int64_t N, int64_t K,
                      int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int epilogue, int a_transposed,
                      int w_transposed, void* stream);

/* Kernel family of the big NT products behind vgpt_gemm_bf16 / vgpt_gemm_bf16_rope / vgpt_gated_mlp_act_fwd[_keep]:
 * 0 (default) = the four-wave kernel with the hand-scheduled register-staged loop wherever it applies (K a multiple of 64
 * with at least two k-tiles, 128 or more 256-row tiles), 1 = the eight-wave LDS-DMA kernels only.  Same operand contract and
 * epilogues; results differ by the order of the fp32 additions inside a k-tile.  Process-wide, not thread-safe: a test and
 * measurement switch, set before the launches it is meant for.  Returns the previous value; other values change nothing. */
int vgpt_gemm_set_family(int family);
/* The family vgpt_gemm_set_family last set (what decides, among other things, whether vgpt_gemm_norm_workspace_bytes is
 * non-zero); changes nothing. */
int vgpt_gemm_get_family(void);
/* What the last top-level GEMM call (vgpt_gemm_bf16, _tr, _rope, _rope_prenorm, _resid_rstd, vgpt_gated_mlp_act_fwd, _keep,
 * _prenorm) launched, one record of 6 int32 per kernel launch, in launch order:
 *   [0] kernel: 128 = the 128 x 128 kernel; 256 / 192 / 288 = the eight-wave 256 x 256 / 256 x 192 / 256 x 288 kernels;
 *               8 / 6 / 9 = the four-wave kernel with 256- / 192- / 288-wide tiles (its NI)
 *   [1] mode: 0 plain, 1 gated, 2 RoPE      [2] a_transposed      [3] w_transposed
 *   [4] first row of the launch (non-zero: the remainder of a split plan)      [5] its row count
 * Writes at most `cap` records to `out` (out may be null when cap is 0) and returns how many launches there were; a call that
 * was refused, or had M == 0 (every entry point returns OK for it), leaves none.  A read-only record for tests: it decides nothing.  Like the family switch it is
 * process-wide and not thread-safe: read it right after the call it is meant for. */
int vgpt_gemm_last_launches(int32_t* out, int cap);
/* Column order of the four-wave kernel's 256 x 288 tiles under vgpt_gemm_bf16_rope[_prenorm].  Where q, k and v have the same
 * number of 96-wide heads (head_dim == 96, N % 288 == 0, 3 * rope_cols == 2 * N with rope_cols = n_rot_heads * head_dim), column
 * tile t computes q head t, k head t and v head t, so that every tile carries the same share of rotated columns.  Each of
 * the tile's two wave columns (144 slots = 9 sub-tiles of 16) holds: sub-tiles 0-2 q and 3-5 k, pair groups u = 3 * wn + {0, 1, 2}
 * (slots 0..7 of a sub-tile are d = 8u .. 8u + 7, slots 8..15 their partners d + 48), sub-tiles 6-8 the v columns
 * 48 * wn .. 48 * wn + 47 of the head.  Returns the output column (= row of W) behind `slot` (0..287) of tile `tile`
 * (0 .. N / 288 - 1), computed by the function the kernel uses, or -1 where this order does not apply: any other shape (the
 * kernel then keeps three consecutive heads per tile), a tile or slot out of range.  Host code only: no GPU needed, decides
 * nothing.  Added without a version bump: no existing signature changed. */
int64_t vgpt_gemm_rope_grouped_col(int64_t N, int64_t rope_cols, int head_dim, int64_t tile, int slot);

/* RMSNorm folded into the GEMMs around it (a decoder layer's two Phi3RMSNorm calls, OmniGen/transformer.py:196-214 through
 * transformers' Phi3DecoderLayer: hidden = residual + attn(input_layernorm(hidden)); hidden = residual +
 * mlp(post_attention_layernorm(hidden))).  The PRODUCER of a residual stream (o_proj / down_proj + residual) also leaves
 * 1 / rms of every output row behind; the CONSUMER (qkv_proj + RoPE, gate_up + activation) reads the raw residual stream as its
 * A operand and a weight with the norm's gain folded in, and multiplies its fp32 accumulators by the row's 1 / rms before
 * anything else:
 *      norm(x) W^T = rstd(x) . (x (W . diag(gain))^T)
 * -- two launches and one activation round trip less per norm.  Differences from the separate kernel: the gain meets the weight
 * (one bf16 rounding of gain * W) instead of the normalised activation (two roundings), and rstd multiplies an fp32 sum; the
 * model-level tolerances (tests/golden/tolerance_calibration.json) hold unchanged.  Deterministic: every workgroup stores the
 * sum of squares of ITS columns of a row, and the last workgroup to arrive at a 256-row block's counter adds the block's
 * partial sums up in a fixed order (no floating-point atomics).
 *   vgpt_gemm_norm_workspace_bytes(M, N, K): bytes of workspace vgpt_gemm_bf16_resid_rstd needs for this shape, 0 if the shape
 *       is not one it takes (then the caller keeps vgpt_rmsnorm_fwd).  The workspace is 256-byte aligned, ZEROED ONCE by the
 *       caller before its first use (it holds arrival counters that every launch leaves at zero again) and may be shared by
 *       all such launches of one stream;
 *   vgpt_gemm_bf16_resid_rstd: C = A W^T + resid (as vgpt_gemm_bf16 with VGPT_EPI_RESID; C may be resid), and
 *       rstd_out[m] = rsqrt(mean_n C[m, n]^2 + eps) on the rounded values.  M == 0 returns OK and touches nothing.  It always runs the four-wave
 *       kernel, so the strides that kernel cannot address are refused here (ldc, ldr < 2^21; (256 + 8) * lda and (N + 8) * ldw
 *       elements below 2 GiB) where vgpt_gemm_bf16 would take the other family;
 *   vgpt_rms_rstd: the same statistic of a matrix x (M, H) no GEMM here produced;
 *   vgpt_fold_norm_gain: W_out (N, K) = bf16(W[n][k] * gain[k]);
 *   vgpt_gemm_bf16_rope_prenorm / vgpt_gated_mlp_act_fwd_prenorm: vgpt_gemm_bf16_rope / vgpt_gated_mlp_act_fwd on
 *       A = the raw stream, W = the folded weight, row m of the product scaled by rstd[m]. */
int64_t vgpt_gemm_norm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int vgpt_gemm_bf16_resid_rstd(const void* A, const void* W, void* C, const void* resid, float* rstd_out, void* workspace,
                              int64_t workspace_bytes, float eps, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                              int64_t ldc, int64_t ldr, void* stream);
int vgpt_rms_rstd(const void* x, float* rstd_out, int64_t rows, int64_t H, int64_t ldx, float eps, void* stream);
int vgpt_fold_norm_gain(const void* W, const void* gain, void* W_out, int64_t N, int64_t K, void* stream);
int vgpt_gemm_bf16_rope_prenorm(const void* A, const void* W, void* C, const float* cos_t, const float* sin_t, const float* rstd,
                                int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldc, int n_rot_heads,
                                int head_dim, void* stream);
int vgpt_gated_mlp_act_fwd_prenorm(const void* A, const void* W_gate_up, void* out, const float* rstd, int64_t M, int64_t I,
                                   int64_t K, int64_t lda, int64_t ldw, int64_t ldo, int act, void* stream);

/* Phi3MLP first half, fused: out[M,I] = act(A Wg^T) * (A Wu^T) where
 * W_gate_up (2I, K) = [Wg ; Wu] as stored by Phi3MLP.gate_up_proj.
 * K % 64 == 0, I % 64 == 0. */
int vgpt_gated_mlp_act_fwd(const void* A, const void* W_gate_up, void* out, int64_t M, int64_t I,
                           int64_t K, int64_t lda, int64_t ldw, int64_t ldo, int act, void* stream);
/* The same product for the TRAINING forward (LVMTraining.forward through Phi3MLP, LVM/model.py:752-845): additionally stores
 * gate_up_out (M, ld_gu >= 2I) = [A Wg^T | A Wu^T] rounded to bf16 -- gate_up_proj's own output, which the backward reads --
 * and computes out = act(gate) * up FROM those rounded values: bit for bit vgpt_gemm_bf16 followed by vgpt_silu_mul_fwd,
 * without writing and re-reading the (M, 2I) tensor in between. */
int vgpt_gated_mlp_act_fwd_keep(const void* A, const void* W_gate_up, void* out, void* gate_up_out, int64_t M, int64_t I,
                                int64_t K, int64_t lda, int64_t ldw, int64_t ldo, int64_t ld_gu, int act, void* stream);

/* ---- block-masked attention ---------------------------------------------- */

/* (B,L,L) bool/uint8 mask (1 = visible; LVM/processor.py:682-731) -> bit-packed rows
 * bits[b][q][w] (w < W = ceil(L/32)); bit j of word w = mask[b][q][32w+j]; bits past L are 0. */
int vgpt_mask_pack_bool(const uint8_t* mask, uint32_t* bits, int64_t B, int64_t L, void* stream);
/* Same from the additive float mask the reference hands to SDPA
 * (OmniGen/transformer.py:139-145: 0 visible, finfo.min masked). is_f32: 0 bf16, 1 fp32.
 * mask is (B,1,L,L) contiguous. */
int vgpt_mask_pack_additive(const void* mask, int is_f32, uint32_t* bits, int64_t B, int64_t L,
                            void* stream);
/* The same packed rows generated from per-token attributes, without any (B,L,L) tensor: replaces the host mask
 * painters LVM/processor.py:575-616 (stage 1), :618-680 (frame-block training), :682-731 (next-clip inference) — all
 * three follow one rule over token attributes (video-gpt_amd/layout.py).
 * attr: (B, L, 2) int32, 8-byte aligned; per token t of row b
 *   word 0 = low | seq << 24     low (24 bits): thr of a CLEAN token = first query row that sees this key; sub of a NOISY
 *                                token = sub-group inside its clip (0 everywhere in the collator's layouts; the engine
 *                                numbers the time rows of denoise step s with s + 1 in its per-clip pass); seq: sequence
 *                                id (8 bits)
 *   word 1 = kind | oc << 2 | grp << 4   kind 0 PAD, 1 CLEAN, 2 NOISY, 3 GAP; oc = min(offset in frame block, 2);
 *                                        grp = id of the (sequence, clip) a NOISY token belongs to
 * bit(q,k) = kind[q]==PAD  ||  (kind[k]==CLEAN && seq[q]==seq[k] && q >= thr[k])
 *         ||  (kind[k]==NOISY && kind[q]==NOISY && grp[q]==grp[k] && oc[q] >= oc[k] && (sub[k]==0 || sub[k]==sub[q])). */
int vgpt_mask_build_tokens(const int32_t* attr, uint32_t* bits, int64_t B, int64_t L, void* stream);
/* Tile summary: one byte per (b, 128-row q block, 64-key tile): 2 bits per 32-row
 * q sub-block (0 = all masked, 1 = all visible, 2 = mixed).
 * summary: (B, ceil(L/128), ceil(L/64)) uint8. */
int vgpt_mask_tile_summary(const uint32_t* bits, uint8_t* summary, int64_t B, int64_t L,
                           void* stream);
/* Number of query rows with no visible key (the reference would average over all keys
 * there; this library does not support it). count: 1 x int32, zeroed by the callee. */
int vgpt_mask_count_empty_rows(const uint32_t* bits, int32_t* count, int64_t B, int64_t L,
                               void* stream);

/* softmax(q k^T * scale + mask) v with the mask given as bits + tile summary.
 * Replaces module.local_attn (F.scaled_dot_product_attention,
 * LVM/transform/sdpa_transform.py:78-86,152). q,k,v,o are bf16 with element strides
 * (batch, head, seq); the head_dim axis is contiguous. head_dim == 96 or 128... see
 * vgpt_attn_supported(). n_kv_heads must divide n_heads (repeat_kv).
 * variant: 0 = default (hardware transposed LDS reads), 1 = reference-slow path. */
int vgpt_attn_blockmask_fwd(const void* q, const void* k, const void* v, void* o,
                            const uint32_t* bits, const uint8_t* summary, int64_t B, int64_t L,
                            int n_heads, int n_kv_heads, int head_dim, int64_t q_sb, int64_t q_sh,
                            int64_t q_ss, int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb,
                            int64_t v_sh, int64_t v_ss, int64_t o_sb, int64_t o_sh, int64_t o_ss,
                            float scale, int variant, void* stream);
int vgpt_attn_supported(int head_dim);
/* Same, computing only query rows [q_start, L) (q_start % 128 == 0) against ALL L keys: rows before q_start are a
 * cached, step-invariant key/value prefix (condition frames never see the clip being denoised, LVM/processor.py:
 * 682-731, so their K/V need not be recomputed every denoise step as LVM/scheduler.py:174 does).  q, o and the mask
 * are indexed by absolute row.  order: NULL, or the launch order computed by vgpt_attn_qblock_order for the same
 * (summary, q_start): block masks give q blocks very different key counts, and starting the long ones first keeps
 * the launch from ending on a few stragglers (results do not depend on it). */
int vgpt_attn_blockmask_fwd_qrange(const void* q, const void* k, const void* v, void* o, int64_t q_start,
                                   const uint32_t* bits, const uint8_t* summary, const int32_t* order, int64_t B, int64_t L,
                                   int n_heads,
                                   int n_kv_heads, int head_dim, int64_t q_sb, int64_t q_sh, int64_t q_ss, int64_t k_sb,
                                   int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh, int64_t v_ss, int64_t o_sb,
                                   int64_t o_sh, int64_t o_ss, float scale, void* stream);

/* ---- planned forward.  A PLAN describes the query side of one mask:
 *   items         (n_items, 4) int32: {batch, row0, nrows (1..item_rows), 0}; disjoint row ranges, cut wherever the
 *                 caller likes -- at the boundaries of packed sequences, so that no item mixes rows with different key
 *                 sets (an aligned block straddling two sequences would walk the key tiles of both);
 *   item_summary  (n_items, ceil(L/64)) uint16: 2 bits per 32-row slab of the item (0 none / 1 all / 2 mixed);
 *   order         (n_items) int32: items sorted longest first.
 * vgpt_attn_plan_build fills item_summary and order from bits and items; both live in ONE caller-allocated workspace of
 * vgpt_attn_plan_workspace_bytes(L, n_items) bytes: item_summary at its start, order at the next multiple of 256 bytes
 * behind n_items * ceil(L/64) * 2.  vgpt_attn_fwd_plan computes exactly the rows the items cover (same result as
 * vgpt_attn_blockmask_fwd up to the rounding of the online softmax); lse may be NULL.  item_rows = the upper bound of the
 * items' row counts, 128 or 256: 256 (head_dim 96 only) runs workgroups of 8 waves on 256 query rows, so one K / V tile
 * staged in LDS serves twice the rows (half the LDS-DMA instructions per wave and half the L2 -> LDS bytes per FLOP). */
int64_t vgpt_attn_plan_workspace_bytes(int64_t L, int64_t n_items);
int vgpt_attn_plan_build(const uint32_t* bits, int64_t B, int64_t L, const int32_t* items, int64_t n_items,
                         uint16_t* item_summary, int32_t* order, void* stream);
int vgpt_attn_fwd_plan(const void* q, const void* k, const void* v, void* o, float* lse, const uint32_t* bits,
                       const int32_t* items, const uint16_t* item_summary, const int32_t* order, int64_t n_items,
                       int64_t B, int64_t L, int n_heads, int n_kv_heads, int head_dim, int64_t q_sb,
                       int64_t q_sh, int64_t q_ss, int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh,
                       int64_t v_ss, int64_t o_sb, int64_t o_sh, int64_t o_ss, float scale, int item_rows, void* stream);

/* ---- MX-fp8 attention (inference option of the cfg-5 rollout; head_dim 96).  Same operator as
 * vgpt_attn_fwd_plan with Q, K, V and the probabilities rounded to OCP e4m3 in blocks of 32 sharing a power-of-two (E8M0)
 * scale, products on the block-scaled MFMA (2x the bf16 rate), fp32 scores / statistics / accumulator.  Two calls:
 * vgpt_attn_fp8_quantize turns the (RoPE-rotated) q / k / v views into `workspace`
 * (vgpt_attn_fp8_workspace_bytes(B, L, n_heads, n_kv_heads, head_dim) bytes, 256-byte aligned; the softmax scale is
 * folded into Q there; only rows >= row_begin, a multiple of 64, are (re)written: a cached prefix keeps its bytes),
 * vgpt_attn_fwd_plan_fp8 computes the rows of a plan (items / item_summary / order of
 * vgpt_attn_plan_build) from it.  No LSE output: the training path stays bf16.  Replaces the same reference lines as
 * vgpt_attn_blockmask_fwd (LVM/transform/sdpa_transform.py:78-86,152). */
int64_t vgpt_attn_fp8_workspace_bytes(int64_t B, int64_t L, int n_heads, int n_kv_heads, int head_dim);
int vgpt_attn_fp8_quantize(const void* q, const void* k, const void* v, void* workspace, int64_t B, int64_t L,
                           int64_t row_begin, int n_heads, int n_kv_heads, int head_dim, int64_t q_sb, int64_t q_sh,
                           int64_t q_ss, int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                           float scale, void* stream);
int vgpt_attn_fwd_plan_fp8(const void* workspace, void* o, const uint32_t* bits, const int32_t* items,
                           const uint16_t* item_summary, const int32_t* order, int64_t n_items, int64_t B, int64_t L,
                           int n_heads, int n_kv_heads, int head_dim, int64_t o_sb, int64_t o_sh, int64_t o_ss, void* stream);

/* The same three calls for every head dim D of vgpt_attn_fp8_supported() (64, 96, 128).  Same parameters and the same
 * stride, alignment, null and row_begin rules as the three above, which stay the head_dim 96 entries; refusals are
 * prefixed with the _hd name and carry the offending value; vgpt_attn_fp8_workspace_bytes_hd returns -1 on a bad shape
 * or an unsupported head dim.  head_dim 96 runs the kernels of the entries above and produces the same bytes.
 *
 * Workspace layout at head dim D (NB = D / 32 blocks of 32 per row; every part starts 256-byte aligned):
 *   Q8   (B, n_heads, L, D) e4m3: q * scale * log2(e), each block of 32 d divided by its power-of-two scale;
 *   QS   (B, n_heads, L, 4) E8M0 bytes: byte j < NB is the scale of d block j, bytes >= NB are 127 (D = 128: all four
 *        are scales; D = 96: byte 3 is 127; D = 64: bytes 2 and 3 are 127);
 *   KV   (B, n_kv_heads, ceil(L / 64)) records of REC(D) bytes, one per tile of 64 keys (keys >= L: zero payload):
 *          K8  at 0:                  [key 64][D] e4m3, blocks of 32 along d
 *          KS  at 64 D:               [key 64][4] E8M0 bytes, as QS
 *          V8  at 64 D + 256:         [d tile NB][h 2][d 32][32 bytes] e4m3, blocks of the 32 keys of a tile half kb at one d:
 *                                     key 32 kb + kk is byte 16 kb + (kk & 3) + 4 (kk >> 3) of h = (kk >> 2) & 1
 *          VS  at 64 D + 256 + 2048 NB: [d tile NB][key half 2][d 32] E8M0 bytes
 *        REC(D) = 128 D + 256 + 64 NB rounded up to whole KiB (the LDS DMA moves 1-KiB pieces):
 *        9 KiB at D = 64, 13 KiB at D = 96, 17 KiB at D = 128.
 * vgpt_attn_fp8_workspace_bytes_hd = align256(B n_heads L D) + align256(B n_heads L 4) + B n_kv_heads ceil(L / 64) REC(D). */
int vgpt_attn_fp8_supported(int head_dim);
int64_t vgpt_attn_fp8_workspace_bytes_hd(int64_t B, int64_t L, int n_heads, int n_kv_heads, int head_dim);
int vgpt_attn_fp8_quantize_hd(const void* q, const void* k, const void* v, void* workspace, int64_t B, int64_t L,
                              int64_t row_begin, int n_heads, int n_kv_heads, int head_dim, int64_t q_sb, int64_t q_sh,
                              int64_t q_ss, int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh,
                              int64_t v_ss, float scale, void* stream);
int vgpt_attn_fwd_plan_fp8_hd(const void* workspace, void* o, const uint32_t* bits, const int32_t* items,
                              const uint16_t* item_summary, const int32_t* order, int64_t n_items, int64_t B, int64_t L,
                              int n_heads, int n_kv_heads, int head_dim, int64_t o_sb, int64_t o_sh, int64_t o_ss,
                              void* stream);

/* ---- MX-fp8 projections (inference option `linear_precision = "fp8"` of the sampler's per-step forward: qkv_proj, o_proj,
 * gate_up_proj, down_proj of every decoder layer).  Number format as the MX-fp8 attention: OCP e4m3 in blocks of 32
 * consecutive k of a row sharing an E8M0 scale 2^e, e the smallest exponent with amax 2^-e <= 448 (clamped to [-127, 127]),
 * elements rounded to nearest-even, an all-zero block stored as zero payload (scale byte 127).
 *
 * Record of a (rows, K) matrix, vgpt_mx8_bytes(rows, K) bytes (-1: K not a positive multiple of 32), 256-byte aligned:
 *   payload  at 0: MG = ceil(rows / 32) row groups x KB = ceil(K / 64) k tiles of 2048 bytes; byte
 *            ((g * KB + kb) * 2 + p) * 1024 + l * 16 + j  holds element (row 32 g + (l & 31), k 64 kb + 32 p + 16 (l >> 5) + j)
 *            for l in [0, 64), j in [0, 16) -- the operand fragment of lane l of the block-scaled 32x32x64 MFMA;
 *   scales   at align256(MG * KB * 2048): byte (g * KB + kb) * 64 + l = E8M0 exponent + 127 of row 32 g + (l & 31),
 *            k block [64 kb + 32 (l >> 5), +32).
 * Rows >= rows and k >= K (padding up to the group / tile) hold zero payload and scale byte 127.
 *   vgpt_mx8_quant_rows: x (rows, K) bf16, row stride ldx -> record `out`; rstd_out (nullable): rsqrt(mean_k x^2 + eps) of
 *       every row in fp32 (the RMSNorm statistic, as vgpt_rms_rstd) -- the activations in front of a projection;
 *   vgpt_mx8_quant_weight: W (N, K) bf16 row-major, times gain (K) bf16 per column when gain != NULL (multiplied in fp32,
 *       rounded once to e4m3: the RMSNorm gain folded into the weight) -> record `out`;
 *   vgpt_gemm_mx8: C (M, .) bf16 from the records A8 (M, K) and W8 (N, K), fp32 accumulation in a fixed k order per output
 *       element (no split-K, no atomics: a row's result does not depend on M or on the tile that computed it), epilogue
 *         VGPT_MX8_EPI_NONE   C = A W^T;
 *         VGPT_MX8_EPI_RESID  C = A W^T + resid (row stride ldr; C may be resid) -- vgpt_gemm_bf16 with VGPT_EPI_RESID;
 *         VGPT_MX8_EPI_ROPE   row m of A W^T times rstd[m], rounded to bf16, then columns [0, n_rot_heads * head_dim) rotated
 *                             with cos / sin (M, head_dim / 2) fp32 -- vgpt_gemm_bf16_rope_prenorm; head_dim 96, N % 96 == 0;
 *         VGPT_MX8_EPI_GATED  W8 = [Wg ; Wu] (N = 2 I rows): C (M, I) = act(gate) * up with gate / up = row m of the product
 *                             times rstd[m], rounded to bf16 -- vgpt_gated_mlp_act_fwd_prenorm; I % 32 == 0.
 *       K % 32 == 0, N % 32 == 0, ldc % 4 == 0; arguments are checked before any launch. */
#define VGPT_MX8_EPI_NONE 0
#define VGPT_MX8_EPI_RESID 1
#define VGPT_MX8_EPI_ROPE 2
#define VGPT_MX8_EPI_GATED 3
int64_t vgpt_mx8_bytes(int64_t rows, int64_t K);
int vgpt_mx8_quant_rows(const void* x, int64_t ldx, void* out, float* rstd_out, int64_t rows, int64_t K, float eps, void* stream);
int vgpt_mx8_quant_weight(const void* W, const void* gain, void* out, int64_t N, int64_t K, void* stream);
int vgpt_gemm_mx8(const void* A8, const void* W8, void* C, const void* resid, const float* rstd, const float* cos_t,
                  const float* sin_t, int64_t M, int64_t N, int64_t K, int64_t ldc, int64_t ldr, int epilogue, int n_rot_heads,
                  int head_dim, int act, void* stream);
/* vgpt_gemm_mx8 whose VGPT_MX8_EPI_ROPE epilogue takes head_dim 64, 96 or 128 (N % head_dim == 0,
 * n_rot_heads * head_dim <= N, cos / sin (M, head_dim / 2) fp32): one head per wave, so tiles of 128, 192 or 256 columns;
 * the rotate-half partner of column d of a head is d +- head_dim / 2.  Same parameters as vgpt_gemm_mx8, which stays the
 * head_dim 96 entry; head_dim 96 runs its kernel, bit for bit; the other three epilogues are vgpt_gemm_mx8 itself. */
int vgpt_gemm_mx8_hd(const void* A8, const void* W8, void* C, const void* resid, const float* rstd, const float* cos_t,
                     const float* sin_t, int64_t M, int64_t N, int64_t K, int64_t ldc, int64_t ldr, int epilogue,
                     int n_rot_heads, int head_dim, int act, void* stream);

/* order (B, ceil(L/128) - q_start/128) int32 <- the 128-row q blocks [q_start/128, ...) of every batch item, the one
 * with the most non-empty 64-key tiles first (stable). */
int vgpt_attn_qblock_order(const uint8_t* summary, int64_t B, int64_t L, int64_t q_start, int32_t* order, void* stream);

/* Diagnostics: while `buf` (device memory, 4 x uint64 per workgroup) is set, every forward launch with at most
 * `capacity_workgroups` workgroups records {start, end (100 MHz realtime ticks), XCC_ID<<32|HW_ID, work item<<32 |
 * key tiles processed} per workgroup.  buf = NULL switches it off (the default). */
int vgpt_attn_trace(void* buf, int64_t capacity_workgroups);

/* Tile body of the head-dim-96 attention forward (every vgpt_attn_* forward entry above): 1 (default) = the generated,
 * hand-scheduled, software-pipelined bodies (csrc/gen/attn_p2_gen.py), 0 = the compiler-scheduled body.  Outputs and log-sum-exp
 * are bit-identical.  Process-wide, not thread-safe: a test and measurement switch (the environment variable VGPT_ATTN_P2=0
 * sets the initial value, read once).  Returns the previous value; other values change nothing. */
int vgpt_attn_set_hand_scheduled(int on);

/* ---- model glue ---------------------------------------------------------- */

/* embed_tokens gather (LVM/model.py:430-432): out[r] = table[ids[r]]. H % 8 == 0.
 * An id outside [0, vocab) is clamped to the nearest valid row (0 or vocab - 1): no read leaves the table. */
int vgpt_embed_gather(const int64_t* ids, const void* table, void* out, int64_t rows, int64_t H,
                      int64_t vocab, void* stream);

/* PatchEmbedMR + cropped 2-D sincos position embedding, scattered into the token
 * sequence (LVM/model.py:149-154,268-289,299-306,436-453).
 * x: (n_frames, C, h, w) bf16; Wp: (H, C*p*p) bf16; bias: (H) bf16;
 * pos_embed: (pos_max*pos_max, H) bf16; dst_row[f]: first row of frame f in `seq`
 * ((rows,H) bf16). patch p = 2, C*p*p == 16. */
int vgpt_patch_embed_fwd(const void* x, const void* Wp, const void* bias, const void* pos_embed,
                         const int32_t* dst_row, void* seq, int n_frames, int C, int h, int w,
                         int64_t H, int pos_max, void* stream);

/* TimestepEmbedder.timestep_embedding (LVM/model.py:39-58): out[n] = [cos(t f) | sin(t f)]
 * (dim = 2*half) rounded to bf16. freqs: (half) fp32 computed by the host exactly as
 * the reference does. t: (n) fp32. */
int vgpt_timestep_sinusoid(const float* t, const float* freqs, void* out, int n, int half,
                           void* stream);

/* Small-M Linear: out[m][n] = post(sum_k pre(x[m][k]) W[n][k] + bias[n]), M <= 32.
 * pre/post: VGPT_ACT_NONE or VGPT_ACT_SILU. Replaces the TimestepEmbedder MLP
 * (LVM/model.py:32-36) and FinalLayer.adaLN_modulation (LVM/model.py:74-77).
 * out rows may be scattered: row m is written at out + out_row[m]*ldo when out_row != NULL
 * (time tokens scattered into the sequence, LVM/model.py:442-446). K % 8 == 0, ldx % 8 == 0,
 * ldx >= K and ldo >= N (row strides in elements). */
int vgpt_linear_small(const void* x, const void* W, const void* bias, void* out,
                      const int32_t* out_row, int M, int64_t N, int64_t K, int64_t ldx, int64_t ldo,
                      int pre_act, int post_act, void* stream);

/* FinalLayer (LayerNorm no-affine eps + modulate + Linear(H -> p*p*C)) + unpatchify
 * (LVM/model.py:79-83,255-265,478-486). hidden: (rows,H) bf16; src_row[f] first row of
 * frame f; mod: (n_frames, 2H) bf16 = [shift | scale]; Wf: (p*p*C, H) bf16; bf: (p*p*C);
 * out: (n_frames, C, h, w) bf16. p = 2, p*p*C == 16. */
int vgpt_final_layer_fwd(const void* hidden, const int32_t* src_row, const void* mod,
                         const void* Wf, const void* bf, void* out, int n_frames, int C, int h,
                         int w, int64_t H, float eps, void* stream);

/* ---- sampler (LVM/scheduler.py:161-208) ---------------------------------- */

/* timesteps[i] = sigma[*step] for i < n (scheduler.py:169).  sigma holds n_steps + 1 entries; with *step outside
 * [0, n_steps] nothing is written (a graph replayed past the end of the table must not read beyond it). */
int vgpt_sampler_set_timesteps(const float* sigma, const int32_t* step, int n_steps, float* timesteps, int n,
                               void* stream);
/* One Euler step with optional x1->v conversion and image CFG (scheduler.py:178-204).
 * z: (n_frames, elems) fp32 state, z_model: same shape bf16 copy handed to the model,
 * pred: (n_frames, elems) bf16. With use_cfg the first half of the frames is the
 * conditional branch, the second half the unconditional one.  sigma holds n_steps + 1 entries; with *step outside
 * [0, n_steps) the state is left untouched. */
int vgpt_euler_cfg_update(float* z, void* z_model, const void* pred, const float* sigma,
                          const int32_t* step, int n_steps, int n_frames, int64_t elems, int pred_type,
                          int use_cfg, float cfg_scale, void* stream);
/* One update of the sampler state by the chosen ODE solver, on the operands of vgpt_euler_cfg_update (same x1->v
 * conversion on the fp32 state, same CFG on the two halves, both halves moved by the guided velocity v_i).
 * h_i = sigma[i+1] - sigma[i], i = *step unless stated.  v_hist: ((n_frames / (1 + use_cfg)), elems) fp32, the guided
 * velocity of the step; may be null for VGPT_SOLVER_EULER only.
 *   VGPT_SOLVER_EULER, stage 0: vgpt_euler_cfg_update itself (bit for bit).
 *   VGPT_SOLVER_AB2, stage 0: z += h_i (v_i + h_i / (2 h_{i-1}) (v_i - v_hist)) for i >= 1, the Euler step for i = 0;
 *     v_hist = v_i at every step.  No-op for *step outside [0, n_steps).
 *   VGPT_SOLVER_HEUN, stage 0 (predictor): v_hist = v_i, z_model = bf16(z + h_i v_i), z untouched; at *step = n_steps - 1
 *     (sigma[n_steps] = 1: the corrector's x1 conversion would divide by zero) a full Euler step.  No-op outside
 *     [0, n_steps).
 *   VGPT_SOLVER_HEUN, stage 1 (corrector), launched AFTER vgpt_sampler_advance with pred = the model's output on
 *     z_model at sigma[*step]: i = *step - 1, z' = z + h_i v_hist (recomputed in fp32), v' from pred with z' and
 *     sigma[i+1], z += h_i / 2 (v_hist + v'), z_model = bf16(z).  No-op for *step outside [1, n_steps).
 * The step is read from device memory (capturable); a replay past the end of the table touches nothing.
 * VGPT_ERR_INVALID (the offending value in the message): null pointer, unknown solver / stage, stage != 0 for a
 * one-stage solver, odd n_frames with CFG, n_steps <= 0, unknown pred_type. */
#define VGPT_SOLVER_EULER 0
#define VGPT_SOLVER_AB2 1
#define VGPT_SOLVER_HEUN 2
int vgpt_sampler_update(float* z, void* z_model, const void* pred, float* v_hist, const float* sigma,
                        const int32_t* step, int n_steps, int n_frames, int64_t elems, int pred_type, int use_cfg,
                        float cfg_scale, int solver, int stage, void* stream);
/* vgpt_sampler_update with image CFG under a per-step guidance scale: cfg_table (n_steps fp32
 * entries, device memory) in place of cfg_scale, and no use_cfg -- this entry point is CFG by definition (n_frames even:
 * first half conditional, second half unconditional).  The scale of a launch is cfg_table[i] with i the index the launch
 * reads sigma at: *step, and *step - 1 for the Heun corrector, so both model calls of a Heun step use that step's scale.
 * An entry that is EXACTLY 1.0f marks an unguided step: v = v_c, the unconditional half of `pred` is not loaded (a caller
 * may leave it uncomputed), both halves of z / z_model still move by v in the roundings of the guided kernels, and
 * v_hist keeps v.  With one value s != 1 in every entry each launch gives the bits of vgpt_sampler_update(..., use_cfg = 1,
 * cfg_scale = s, ...).  A launch with i outside the table is a no-op.  VGPT_ERR_INVALID as vgpt_sampler_update, and for a
 * null cfg_table and an odd n_frames. */
int vgpt_sampler_update_sched(float* z, void* z_model, const void* pred, float* v_hist, const float* sigma,
                              const float* cfg_table, const int32_t* step, int n_steps, int n_frames, int64_t elems,
                              int pred_type, int solver, int stage, void* stream);
/* The Euler step of vgpt_euler_cfg_update with noise re-injected (the flow-matching counterpart of
 * DDIM's eta).  i = *step, h = sigma[i+1] - sigma[i], v the guided velocity, eta = eta_table[i] (n_steps fp32 entries,
 * device memory):
 *     x0_hat = z - sigma[i] v,   z' = (z + h v) + (1 - sigma[i+1]) ((sqrt(1 - eta^2) - 1) x0_hat + eta eps)
 * eps = the normal of vgpt_sampler_noise_fill at (seed, stream, step i, element e), e the frame-major element index
 * within one noise half: all frames without sharing; with use_cfg = 1 (which implies it) or share_halves = 1 the frames
 * [n/2, n) reuse the numbers of [0, n/2) -- share_halves alone is for callers whose model call combined the CFG halves
 * already, every frame then moving by its own prediction.  rng: int64[2] in DEVICE memory, {seed, stream}, read by the
 * kernel: a captured launch serves a new seed without recapture.
 * With eta_table[i] == 0.0f exactly the launch gives vgpt_euler_cfg_update's bits (with cfg_table:
 * vgpt_sampler_update_sched's, VGPT_SOLVER_EULER), and so does any eta at 1 - sigma[i+1] == 0, the last step.
 * cfg_table: null, or n_steps per-step guidance scales in place of cfg_scale with the semantics of
 * vgpt_sampler_update_sched (an entry of exactly 1.0f: v = v_c, the unconditional half of pred is not loaded); it needs
 * use_cfg = 1.  No history buffer: only the first-order step takes noise.  With *step outside [0, n_steps) nothing is
 * written.  VGPT_ERR_INVALID (the offending value in the message): null pointer, n_steps <= 0, negative n_frames or
 * elems ("bad shape"), odd n_frames with use_cfg or share_halves, unknown pred_type, cfg_table with use_cfg = 0.  Zero
 * sizes return VGPT_OK.  The entries of eta_table are NOT checked (they are device memory): keeping them in [0, 1] is the
 * caller's duty -- outside it sqrt(1 - eta^2) is the square root of a negative number and the state becomes NaN
 * (scheduler.eta_table and StaticDenoiser refuse such a value before it reaches a table). */
int vgpt_sampler_update_sde(float* z, void* z_model, const void* pred, const float* sigma, const float* cfg_table,
                            const float* eta_table, const int64_t* rng, const int32_t* step, int n_steps, int n_frames,
                            int64_t elems, int pred_type, int use_cfg, float cfg_scale, int share_halves, void* stream);
/* out[e] = eps(seed, stream, step_index, e) for e < n: counter-based standard normals.  Philox4x32-10 (Salmon et al.
 * 2011) with key (seed low, seed high) and counter (block low, block high, step_index, stream low), block = e >> 2; its
 * four words w0..w3 give elements 4 block .. 4 block + 3: u1 = ((w0 >> 9) + 0.5) 2^-23, u2 = (w1 >> 8) 2^-24,
 * r = sqrtf(-2 logf(u1)), (r cospif(2 u2), r sinpif(2 u2)), and the same from (w2, w3); |eps| <= sqrt(48 ln 2).
 * rng: int64[2] {seed, stream} in device memory.  VGPT_ERR_INVALID: null pointer, n < 0; n == 0 returns VGPT_OK. */
int vgpt_sampler_noise_fill(float* out, int64_t n, const int64_t* rng, int step_index, void* stream);
/* *step += 1 */
int vgpt_sampler_advance(int32_t* step, void* stream);
/* dst[l][0:slab_bytes] = src[*step][l][0:slab_bytes] for l < n_layers (step clamped to [0, n_steps)); all sizes and
 * strides in bytes, multiples of 16.  The engine keeps the post-RoPE q/k/v rows of the time tokens of every denoise
 * step (they depend on the step only: a time row sees `<|diffusion|>` and time columns, never image columns,
 * LVM/processor.py:682-731) and drops the current step's rows into the per-layer qkv buffer; the reference recomputes
 * them inside every model call (LVM/scheduler.py:174 -> LVM/model.py:446-449).  Reads the step from device memory:
 * capturable. */
int vgpt_sampler_copy_step_rows(const void* src, void* dst, const int32_t* step, int n_steps, int n_layers,
                                int64_t slab_bytes, int64_t src_step_stride_bytes, int64_t src_layer_stride_bytes,
                                int64_t dst_layer_stride_bytes, void* stream);
/* ---- Ulysses sequence parallelism in the sampler engine (the re-layouts around the exchanges of
 *      LVM/transform/sdpa_transform.py:125-156, where four all-to-alls of torch tensors move q, k, v and the
 *      attention output between (B, L/P, heads, d) and (B, L, heads/P, d)) ---- */

/* Split this rank's fused post-RoPE projection rows qkv (rows, (n_heads + 2 n_kv_heads) head_dim) bf16 row-major
 * [q heads | k heads | v heads] into n_ranks chunks out (n_ranks, rows, (n_heads + 2 n_kv_heads) / n_ranks * head_dim):
 * chunk j row t = [q heads j*n_heads/P .. | k heads j*n_kv_heads/P .. | v heads j*n_kv_heads/P ..] of row t, i.e. a fused
 * row of rank j's heads.  One all-to-all of the chunks then carries q, k and v together.  n_heads and n_kv_heads
 * multiples of n_ranks (VGPT_ERR_INVALID otherwise); head_dim % 8 == 0 and 16-byte aligned pointers
 * (VGPT_ERR_UNSUPPORTED otherwise).  rows == 0 is a no-op. */
int vgpt_sp_pack_qkv(const void* qkv, void* out, int64_t rows, int n_heads, int n_kv_heads, int head_dim, int n_ranks,
                     void* stream);
/* Interleave the n_ranks attention-output blocks received back (n_ranks, rows, block_width) bf16 into
 * out (rows, n_ranks * block_width): out[t, i*block_width + c] = blocks[i, t, c] -- the heads of rank i land at their
 * place in head order, the o_proj operand of an unsharded step.  block_width % 8 == 0, 16-byte aligned pointers. */
int vgpt_sp_unpack_ctx(const void* blocks, void* out, int64_t rows, int64_t block_width, int n_ranks, void* stream);
/* The same two exchanges run backwards in the sharded training step (train.Stage1Trainer, sequence_parallel=True): the
 * inverses of the two re-layouts above.
 * vgpt_sp_pack_ctx: blocks[i, t, c] = ctx[t, i*block_width + c] -- ctx (rows, n_ranks * block_width) bf16, blocks
 * (n_ranks, rows, block_width): d(ctx) of this rank's rows, cut by the rank that owns the heads.  Checks as
 * vgpt_sp_unpack_ctx. */
int vgpt_sp_pack_ctx(const void* ctx, void* blocks, int64_t rows, int64_t block_width, int n_ranks, void* stream);
/* Inverse of vgpt_sp_pack_qkv: chunks (n_ranks, rows, (n_heads + 2 n_kv_heads) / n_ranks * head_dim) bf16 -> qkv
 * (rows, (n_heads + 2 n_kv_heads) head_dim) laid out [q heads | k heads | v heads].  cos_t == sin_t == NULL: bytes only.
 * With tables (rows, head_dim/2) fp32 the q and k heads are also rotated on the way through, bit for bit what
 * vgpt_rope_qk_inplace would do to the unpacked rows (same bf16 inputs, fp32 arithmetic, one rounding); the v columns
 * stay bytes.  The trainer passes cos and -sin: the inverse rotation of d(qkv).  Exactly one table NULL, null buffers,
 * bad shapes, heads not multiples of n_ranks: VGPT_ERR_INVALID.  head_dim % 8 != 0 (with tables: head_dim/2 % 8 != 0),
 * pointers (tables included) not 16-byte aligned, 2^31 vectors or more: VGPT_ERR_UNSUPPORTED.  rows == 0 is a no-op. */
int vgpt_sp_unpack_qkv_rope(const void* chunks, void* qkv, const float* cos_t, const float* sin_t, int64_t rows,
                            int n_heads, int n_kv_heads, int head_dim, int n_ranks, void* stream);

/* z_model = bf16(z) */
int vgpt_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);

/* ---- VAE conv stack (diffusers==0.29.0 AutoencoderKL, sdxl-vae layout; fp32 like the reference:
 *      LVM/pipeline.py:110-117 encode, :558-590 decode, LVM/train/train_x1_stage1_noiseinput.py:190) ---- */

/* GroupNorm statistics: stats[(n*groups+g)*2 + {0,1}] = {mean, rsqrt(var+eps)} over (C/groups, HW).
 * x: (N, C, HW) fp32. */
int vgpt_groupnorm_stats(const float* x, float* stats, int64_t N, int C, int HW, int groups, float eps,
                         void* stream);

/* Implicit-GEMM convolution on the fp32 MFMA, NCHW fp32:
 *   y = conv(f(x), w) + bias + resid,  f = optional nearest-x2 upsample, then optional
 *   GroupNorm(gn_stats, gamma, beta)[+SiLU] applied on load (zero padding applied after f).
 * ksize 3 (stride 1 pad 1 | stride 2 with Downsample2D's (0,1,0,1) pad) or 1.  w: (Cout, Cin*k*k) with row
 * stride ldw, or stored transposed (Cin*k*k, Cout) when w_transposed; w_batch_stride != 0 selects a
 * per-image weight matrix (attention products).  bias/resid/gn_* may be NULL (gn_groups = 0). */
int vgpt_conv2d_fwd(const float* x, const float* w, const float* bias, const float* resid,
                    const float* gn_stats, const float* gn_gamma, const float* gn_beta, float* y, int N,
                    int Cin, int Hin, int Win, int Cout, int ksize, int stride, int upsample, int gn_groups,
                    int gn_silu, int w_transposed, int64_t ldw, int64_t w_batch_stride, void* stream);

/* 3x3 stride-1 convolution on the bf16 matrix cores at fp32-class accuracy: every operand is split hi + lo (two bf16)
 * and the three leading product terms are accumulated in fp32 (~16 mantissa bits; the reference's torch/cuDNN default
 * for its fp32 VAE is TF32, 10 bits).  Same prologue (nearest x2 upsample, GroupNorm(+SiLU)) and epilogue (bias,
 * residual) as vgpt_conv2d_fwd.  Weights are pre-split once by vgpt_conv_pack_weights_bx3 into LDS-ready images:
 * w (Cout, Cin, 3, 3) fp32 -> `packed`, vgpt_conv_bx3_packed_bytes(Cout, Cin) bytes (one 48-KiB hi + lo image per
 * 64-channel output tile and 16-channel input chunk, ten tap slots of 16 channels per output channel, copied into LDS by
 * LDS-DMA; the format is private to the two functions below). */
int64_t vgpt_conv_bx3_packed_bytes(int Cout, int Cin);
int vgpt_conv_pack_weights_bx3(const float* w, void* packed, int Cout, int Cin, void* stream);
int vgpt_conv2d_bx3_fwd(const float* x, const void* packed, const float* bias, const float* resid, const float* gn_stats,
                        const float* gn_gamma, const float* gn_beta, float* y, int N, int Cin, int Hin, int Win, int Cout,
                        int upsample, int gn_groups, int gn_silu, void* stream);
/* 1x1 convolution (resnet shortcuts, the mid-block attention's projections; diffusers ResnetBlock2D.conv_shortcut /
 * Attention.to_q..to_out, call sites LVM/pipeline.py:565,578) in the same split-bf16 arithmetic and with the same
 * GroupNorm(+SiLU) prologue / bias + residual epilogue; x (N, Cin, HW), y (N, Cout, HW) fp32, Cin % 32 == 0.
 * w (Cout, Cin) fp32 is pre-split once: vgpt_conv1x1_bx3_packed_bytes(Cout, Cin) bytes. */
int64_t vgpt_conv1x1_bx3_packed_bytes(int Cout, int Cin);
int vgpt_conv1x1_pack_weights_bx3(const float* w, void* packed, int Cout, int Cin, void* stream);
int vgpt_conv1x1_bx3_fwd(const float* x, const void* packed, const float* bias, const float* resid, const float* gn_stats,
                         const float* gn_gamma, const float* gn_beta, float* y, int N, int Cin, int HW, int Cout,
                         int gn_groups, int gn_silu, void* stream);

/* In-place softmax over the KEY axis of S^T (N, keys, queries) with pre-scale (mid-block attention). */
int vgpt_col_softmax(float* s, int N, int keys, int queries, float scale, void* stream);

/* Fused mid-block attention (diffusers' `Attention` of the VAE mid-block, one head over the HW positions of a frame,
 * as reached from LVM/pipeline.py:110-117 encode and :558-590 decode), exact fp32, one pass with an online softmax: the
 * (HW, HW) score matrix is never stored, there is no workspace and there are no atomics.
 *   s[j][i] = scale * sum_c k[c][j] q[c][i]   (j = key, i = query)
 *   p[.][i] = softmax over j
 *   o[c][i] = sum_j v[c][j] p[j][i]
 * Layout: q, k, v, o are fp32 in the VAE's [n][c][pos] layout with one shared pair of strides: element (n, c, p) is at
 * base + n * batch_stride + c * ld + p (a contiguous NCHW activation: ld = HW, batch_stride = C * HW).  V is staged with
 * 16-byte accesses when ld % 4 == 0, batch_stride % 4 == 0 and v is 16-byte aligned, with scalar ones otherwise; both
 * give the same bits.
 * Tiles: a workgroup owns VGPT_VAE_ATTN_TQ queries of one image (two halves of 32) and walks the keys
 * VGPT_VAE_ATTN_TK at a time (N * ceil(HW / TQ) workgroups); key tails are masked to -inf before the maximum, query
 * tails are not stored.
 * Rounding points: both products run on v_mfma_f32_32x32x2_f32, bit for bit fp32 FMA chains.  A score is four chains of
 * C/4 channels (ascending) summed as ((c0 + c1) + c2) + c3, then * scale; per key tile x - m with the running maximum m,
 * exp as v_exp_f32((x - m) * log2 e), l = l * a + sum(p) and o = o * a with a = exp(m_old - m_new), then an FMA chain
 * over the tile's keys; o / l is an IEEE division at the end.  The result is a pure function of the inputs: two launches
 * agree bit for bit, and a batch of N equals N single launches.
 * Refusals: a null pointer, N < 0, HW <= 0, ld < HW, batch_stride < C * ld, scale <= 0 or o overlapping an input:
 * VGPT_ERR_INVALID.  C not a multiple of 64 or above VGPT_VAE_ATTN_MAX_C (or ld >= 2^28, or 2^31 workgroups): VGPT_ERR_UNSUPPORTED;
 * vgpt_last_error() names the value.  N == 0: VGPT_OK, nothing launched.  Capturable: no allocation, no sync. */
#define VGPT_VAE_ATTN_TQ 64
#define VGPT_VAE_ATTN_TK 32
#define VGPT_VAE_ATTN_MAX_C 512
int vgpt_vae_attn_fwd(const float* q, const float* k, const float* v, float* o, int64_t N, int C, int64_t HW,
                      int64_t ld, int64_t batch_stride, float scale, void* stream);

/* DiagonalGaussianDistribution.sample + latent scaling (LVM/pipeline.py:110-115):
 * z = (mean + exp(0.5*clamp(logvar,-30,20)) * noise - shift) * scaling.
 * moments: (N, 2*per_image) = [mean | logvar] per image; noise, z: (N, per_image). */
int vgpt_vae_sample(const float* moments, const float* noise, float* z, int N, int64_t per_image, float shift,
                    float scaling, void* stream);

/* (x*0.5+0.5).clamp(0,1)*255 -> uint8, NCHW -> NHWC (LVM/pipeline.py:585-588). */
int vgpt_vae_postprocess_u8(const float* x, uint8_t* out, int N, int C, int H, int W, void* stream);

/* y = float(x) * mul + add (latent / scaling_factor + shift before decode, LVM/pipeline.py:573-577). */
int vgpt_affine_to_f32(const void* x, int x_is_bf16, float* y, int64_t n, float mul, float add, void* stream);

/* ---- stage-1 pre-training step (LVM/train_helper/loss.py:128-243, LVM/train/train_x1_stage1_noiseinput.py:351-405;
 *      the reference gets these from torch.autograd + DeepSpeed) ---------------------------------------- */

/* Attention forward that also returns the base-2 log-sum-exp of the scaled scores, lse (B, n_heads, L) fp32.
 * order: NULL or the launch order from vgpt_attn_qblock_order(q_start = 0). */
int vgpt_attn_blockmask_fwd_lse(const void* q, const void* k, const void* v, void* o, float* lse,
                                const uint32_t* bits, const uint8_t* summary, const int32_t* order, int64_t B, int64_t L,
                                int n_heads,
                                int n_kv_heads, int head_dim, int64_t q_sb, int64_t q_sh, int64_t q_ss, int64_t k_sb,
                                int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh, int64_t v_ss, int64_t o_sb,
                                int64_t o_sh, int64_t o_ss, float scale, void* stream);
/* Attention backward (head_dim 96): dq, dk, dv from q, k, v, o, dout, lse.  strides: 24 x int64 element strides
 * (batch, head, seq) of q, k, v, o, dout, dq, dk, dv in that order.  delta_ws: (B, n_heads, L) fp32 workspace. */
int vgpt_attn_blockmask_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                            const float* lse, float* delta_ws, void* dq, void* dk, void* dv, const uint32_t* bits,
                            const uint8_t* summary, int64_t B, int64_t L, int n_heads, int n_kv_heads, int head_dim,
                            const int64_t* strides, float scale, void* stream);
/* The same backward for every head dim of vgpt_attn_bwd_supported() (64, 96, 128): torch.autograd through
 * F.scaled_dot_product_attention, LVM/transform/sdpa_transform.py:78-86,152.  Same parameters, stride, alignment and
 * null rules as vgpt_attn_blockmask_bwd (which stays the head_dim 96 entry); refusals name the offending value.
 * head_dim 96 runs the kernels of vgpt_attn_blockmask_bwd, bit for bit. */
int vgpt_attn_blockmask_bwd_hd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                               const float* lse, float* delta_ws, void* dq, void* dk, void* dv, const uint32_t* bits,
                               const uint8_t* summary, int64_t B, int64_t L, int n_heads, int n_kv_heads, int head_dim,
                               const int64_t* strides, float scale, void* stream);
/* 1 if vgpt_attn_blockmask_bwd_hd has kernels for this head dim, else 0. */
int vgpt_attn_bwd_supported(int head_dim);

/* (R, C) bf16 row stride ld_in -> (C, Rp) bf16, columns r >= R zero-filled (operands of the backward NT GEMMs). */
int vgpt_transpose_pad_bf16(const void* in, void* out, int64_t R, int64_t C, int64_t Rp, int64_t ld_in, void* stream);
/* un-fused gated activation: act = f(gate) * up from gate_up (M, 2I); and its backward d(gate_up). */
int vgpt_silu_mul_fwd(const void* gate_up, void* act_out, int64_t M, int64_t I, int act, void* stream);
int vgpt_silu_mul_bwd(const void* gate_up, const void* dact, void* dgate_up, int64_t M, int64_t I, int act, void* stream);
/* y = f(pre);  dx = f'(pre) * dy  (bf16, n elements). */
int vgpt_act_fwd(const void* pre, void* y, int64_t n, int act, void* stream);
int vgpt_act_bwd(const void* pre, const void* dy, void* dx, int64_t n, int act, void* stream);
/* Phi3RMSNorm backward: dx = d(norm)/dx (+ dres if not NULL), dw += sum_rows dy * xhat (fp32, caller zeroes). */
int vgpt_rmsnorm_bwd(const void* x, const void* w, const void* dy, const void* dres, void* dx, float* dw,
                     float* rstd_ws /* rows floats */, int64_t rows, int64_t H, float eps, void* stream);
/* C[m][n] = alpha * sum_k A[m*sa_m + k*sa_k] * B[k*sb_k + n*sb_n] (+ C); *_f32: 0 = bf16, 1 = fp32.  For the
 * small heads (patch embeds, timestep MLPs, adaLN, final Linear) whose backward is not worth an MFMA kernel.
 * splitk_ws (NULL or ws_floats floats): workspace that lets long reductions with few outputs be sliced over the chip
 * (slices are added in a fixed order: deterministic).  vgpt_matmul_generic_workspace_bytes(M, N, K) is the size with which
 * a problem gets all the slices it can use (0: it runs unsliced); a smaller workspace means fewer slices. */
int64_t vgpt_matmul_generic_workspace_bytes(int64_t M, int64_t N, int64_t K);
int vgpt_matmul_generic(const void* A, int a_f32, int64_t sa_m, int64_t sa_k, const void* B, int b_f32, int64_t sb_k,
                        int64_t sb_n, void* C, int c_f32, int64_t sc_m, int64_t sc_n, int64_t M, int64_t N, int64_t K,
                        float alpha, int accumulate, float* splitk_ws, int64_t ws_floats, void* stream);
/* out[c] (+)= sum_r X[r*ld + c]  (bias gradients). */
int vgpt_colsum(const void* X, int x_f32, float* out, int64_t R, int64_t C, int64_t ld, int accumulate, void* stream);
/* xt[f] = t[f]*x1[f] + (1-t[f])*x0[f]  (loss.py:175,186), fp32 in, bf16 out. */
int vgpt_lerp_frames(const float* x1, const float* x0, const float* t, void* out, int n_frames, int64_t elems,
                     void* stream);
/* loss[f] = mean((x1[f]-pred[f])^2) (loss.py:209-218); dpred (optional, bf16) = d(mean_f loss)/dpred. */
int vgpt_mse_frames(const void* pred, const float* x1, float* loss, void* dpred, int n_frames, int64_t elems,
                    void* stream);
/* The same with the mean taken over n_mean >= n_frames terms: the frames' terms are part of a longer loss vector (the
 * input-head terms of input_output_return, loss.py:220-225, appended before .mean()). */
int vgpt_mse_frames_mean(const void* pred, const float* x1, float* loss, void* dpred, int n_frames, int n_mean, int64_t elems,
                         void* stream);
/* FinalLayer split for training: v = LN(x)(1+scale)+shift with xhat / rstd saved; and its backward (dmod fp32
 * (n_frames, 2H) accumulated with atomics — caller zeroes; dhidden rows written at dst_row[f] + t). */
int vgpt_ln_mod_fwd(const void* hidden, const int32_t* src_row, const void* mod, void* v_out, float* xhat_out,
                    float* rstd_out, int n_frames, int ntok, int64_t H, float eps, void* stream);
int vgpt_ln_mod_bwd(const void* dv, const float* xhat, const float* rstd, const void* mod, const int32_t* dst_row,
                    void* dhidden, float* dmod, int n_frames, int ntok, int64_t H, void* stream);
/* embed_tokens backward: dtable[ids[r]] += dseq[r] for rows with keep[r] != 0 (fp32 atomics). */
int vgpt_embed_bwd(const int64_t* ids, const uint8_t* keep, const void* dseq, float* dtable, int64_t rows, int64_t H,
                   int64_t vocab, void* stream);
/* Deterministic twins of the three entry points above that add with float atomics (Stage1Trainer(deterministic=True),
 * DESIGN.md 6d).  Same arguments plus a workspace, no float atomics: every sum is cut into partials whose membership
 * depends on the shape alone (for the embedding: on ids and keep), the partials are written with plain stores and ONE
 * writer per output element adds them in ascending order on top of the caller's value.  Same inputs give the same bits on
 * every launch.  ws must be 16-byte aligned and hold at least what the matching *_workspace_bytes query answers (-1 on a
 * negative argument); its contents need no initialisation and are garbage afterwards.
 *
 * vgpt_rmsnorm_bwd_det: dx and rstd_ws are vgpt_rmsnorm_bwd's, bit for bit (the same row kernel).  dw: the twin's row
 * strips (min(ceil(rows/4), 128) wanted, a function of rows alone) store their sums at ws[strip][H]; a second launch adds
 * the strips 0, 1, ... per column and then dw[c] += total (the caller zeroes dw, or keeps a running sum in it). */
int64_t vgpt_rmsnorm_bwd_det_workspace_bytes(int64_t rows, int64_t H);
int vgpt_rmsnorm_bwd_det(const void* x, const void* w, const void* dy, const void* dres, void* dx, float* dw,
                         float* rstd_ws /* rows floats */, int64_t rows, int64_t H, float eps, float* ws, int64_t ws_floats,
                         void* stream);
/* vgpt_ln_mod_bwd_det: dhidden is vgpt_ln_mod_bwd's, bit for bit.  A wave walks ceil(ntok / 64) tokens of one frame (at
 * most 64 waves per frame, a function of ntok alone) and stores its dshift | dscale sums at ws[f][wave][2H]; a second
 * launch adds the waves 0, 1, ... per frame and column and then dmod[f][c] += total. */
int64_t vgpt_ln_mod_bwd_det_workspace_bytes(int64_t n_frames, int64_t ntok, int64_t H);
int vgpt_ln_mod_bwd_det(const void* dv, const float* xhat, const float* rstd, const void* mod, const int32_t* dst_row,
                        void* dhidden, float* dmod, int n_frames, int ntok, int64_t H, float* ws, int64_t ws_floats,
                        void* stream);
/* vgpt_embed_bwd_det (H % 8 == 0, vocab < 2^31): the kept, in-range rows are ranked by (id, row) with rows^2 integer
 * comparisons; one workgroup per id that occurs and 256 columns adds that id's rows -- eight interleaved row slots, each
 * in ascending row order, then the slots 0..7 -- and the one writer of dtable[id][c] adds the total to the caller's
 * value.  The order depends on (ids, keep, rows, H) only.  Table rows whose id never occurs are neither read nor
 * written.  ws: int32 words. */
int64_t vgpt_embed_bwd_det_workspace_bytes(int64_t rows);
int vgpt_embed_bwd_det(const int64_t* ids, const uint8_t* keep, const void* dseq, float* dtable, int64_t rows, int64_t H,
                       int64_t vocab, int32_t* ws, int64_t ws_ints, void* stream);
/* (n_frames, C, h, w) -> (n_frames*ntok, 16) patch vectors; gradient of unpatchify; row-segment gather. */
int vgpt_patchify(const void* x, void* patches, int n_frames, int C, int h, int w, void* stream);
int vgpt_unpatchify_bwd(const void* dpred, void* dy16, int n_frames, int C, int h, int w, void* stream);
int vgpt_gather_rows(const void* in, const int32_t* row0, void* out, int n_seg, int per, int64_t H, void* stream);
/* *out += sum g^2 (deterministic two-stage reduction: replicas must agree bit for bit);  coef = min(1, max_norm/(sqrt(S)+1e-6)) * extra_scale
 * with S the sum of the n >= 1 values sumsq[0..n-1] (per-rank partial sums of a sharded optimizer, in rank order), added in
 * a fixed order (n == 1: S = sumsq[0]); *norm_out (may be NULL) = sqrt(S); n < 1 or a NULL sumsq / coef: VGPT_ERR_INVALID;
 * AdamW on fp32 master weights (torch.optim.AdamW update; bf16 model copy refreshed; *grad_scale multiplies the gradient). */
int vgpt_sumsq(const void* g, int g_f32, float* out, int64_t n, float* partial_ws /* >= 1024 floats */, void* stream);
int vgpt_clip_coef(const float* sumsq, int n, float* coef, float* norm_out, float max_norm, float extra_scale,
                   void* stream);
int vgpt_adamw_step(float* master, void* param, const void* grad, int grad_f32, float* m, float* v, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale,
                    void* stream);
/* EMA of the weights (train_x1_stage1_noiseinput.py:227-230, 288-290, 406-408; update_ema, LVM/utils.py:27-34) inside the
 * AdamW pass: vgpt_adamw_step with a fourth fp32 stream.  master, param, m and v are updated by the same expressions in the
 * same order (bit-identical to vgpt_adamw_step on the same inputs), and ema[i] = fmaf(d, ema[i], (1 - d) * p_new[i]) with
 * d = ema_decay, 1 - d formed in fp32 on the host and p_new the fp32 master value just computed (not its bf16 rounding):
 * the product (1 - d) * p_new is rounded to fp32, then ONE fused multiply-add, two roundings in all.  d = 0 gives
 * ema = p_new bit for bit, d = 1 leaves a finite ema unchanged (a -0 becomes +0).  36 B/param in one pass (a separate EMA
 * pass behind vgpt_adamw_step: 28 + 12).  Same alignment contract, ema held to the 16-byte rule (VGPT_ERR_UNSUPPORTED);
 * a NULL ema, n < 0, step < 1 or ema_decay outside [0, 1]: VGPT_ERR_INVALID; n == 0: VGPT_OK. */
int vgpt_adamw_ema_step(float* master, void* param, const void* grad, int grad_f32, float* m, float* v, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale,
                        float* ema, float ema_decay, void* stream);
/* Gradient accumulation over micro-steps (--gradient_accumulation_steps, train_x1_stage1_noiseinput.py:121, 353
 * accelerator.accumulate, 393, 406-413): acc is an fp32 accumulator of n elements, grad the gradient bucket (bf16, or fp32
 * when grad_f32 != 0).  mode 0: acc = float(grad) (first micro-step); mode 1: acc += float(grad) (middle micro-steps);
 * mode 2: grad = T(acc + float(grad)) written back in the bucket's own type (bf16: round to nearest even), acc NOT written
 * (last micro-step): the bucket then holds the once-rounded sum of all micro-gradients and the exchange, vgpt_sumsq,
 * vgpt_clip_coef and vgpt_adamw_step run on it unchanged.  Elementwise: deterministic.  acc and an fp32 grad 16-byte
 * aligned, a bf16 grad 8-byte aligned (else VGPT_ERR_UNSUPPORTED); a NULL pointer, n < 0 or another mode:
 * VGPT_ERR_INVALID; n == 0: VGPT_OK. */
int vgpt_grad_accumulate(float* acc, void* grad, int grad_f32, int64_t n, int mode, void* stream);
/* ---- guarded optimizer step: a non-finite or spiking step is dropped on the device (Stage1Trainer(skip_bad_steps=True),
 *      DESIGN.md §6f).  Stands in for the overflow check of the reference's optimizer stack: train_x1_stage1_noiseinput.py
 *      hands AdamW to accelerate's DeepSpeed plugin (:114-125, 393-405; pretrain_stage1_nv.sh:49, stage2_bf16_dp.json), whose
 *      ZeRO stage-2 optimizer checks the reduced gradients for inf / nan and returns from step() without an update
 *      (DeepSpeed runtime/zero/stage_1_and_2.py: check_overflow, has_overflow).  The norm threshold has no counterpart there.
 * vgpt_clip_coef_guarded: vgpt_clip_coef with a verdict.  S, sqrt(S) and the coefficient are formed by the same expressions in
 *   the same order; verdict (2 int32 words in device memory) = {0, 0}: apply, and coef and *norm_out hold vgpt_clip_coef's
 *   bits; {1, 1}: skip, sqrt(S) is NaN or Inf (a non-finite or negative S); {1, 2}: skip, skip_norm > 0 and
 *   sqrt(S) > skip_norm (strictly; skip_norm == 0: no threshold; the caller scales it like max_norm).  A skip writes
 *   coef = +0.0f; *norm_out (may be NULL) receives sqrt(S) either way.  One wave, the record written by one lane.  A NULL
 *   sumsq / coef / verdict, n < 1, a negative or NaN max_norm or skip_norm: VGPT_ERR_INVALID, the value named.
 * vgpt_adamw_step_guarded / vgpt_adamw_ema_step_guarded: vgpt_adamw_step / vgpt_adamw_ema_step behind verdict[0] (device
 *   memory, the record above).  0: every output has the unguarded entry point's bits (one kernel body).  Non-zero: every
 *   wave ends behind that one 4-byte load; nothing else is read, nothing is written -- launch overhead instead of 28 / 36
 *   bytes per parameter.  Same alignment contract (VGPT_ERR_UNSUPPORTED); a NULL pointer, n < 0, step < 1, grad_f32 outside
 *   {0, 1}, ema_decay outside [0, 1]: VGPT_ERR_INVALID, the value named; n == 0: VGPT_OK.
 * vgpt_sumsq_keep: vgpt_sumsq that also stores this buffer's own sum: *total += s; *part = s with s the value vgpt_sumsq adds
 *   (same kernels, same order), so the total keeps its bits and per-bucket gradient norms cost nothing.  n == 0: s = 0.
 *   A NULL pointer, n < 0, g_f32 outside {0, 1}: VGPT_ERR_INVALID.
 * vgpt_count_nonfinite (torch.isnan / torch.isinf per tensor, what DeepSpeed's overflow check does not tell): x is a flat
 *   bf16 (x_f32 = 0) or fp32 (1) buffer of n elements, 16-byte aligned; offsets T + 1 ascending int64 element offsets in
 *   device memory (clamped to [0, n]); counts[2 t] = number of NaN, counts[2 t + 1] = number of +-Inf in
 *   [offsets[t], offsets[t + 1]), int32, cleared by the call.  Segments may be empty and start at any element.  Read off
 *   the bit patterns, integer sums: deterministic.  A diagnostic for after a skip, one pass over the buffer.  A NULL x /
 *   counts / offsets, n < 0, T outside [0, 65535], x_f32 outside {0, 1}: VGPT_ERR_INVALID; T == 0: VGPT_OK. */
int vgpt_clip_coef_guarded(const float* sumsq, int n, float* coef, float* norm_out, float max_norm, float extra_scale,
                           float skip_norm, int32_t* verdict, void* stream);
int vgpt_adamw_step_guarded(float* master, void* param, const void* grad, int grad_f32, float* m, float* v, int64_t n,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                            const float* grad_scale, const int32_t* verdict, void* stream);
int vgpt_adamw_ema_step_guarded(float* master, void* param, const void* grad, int grad_f32, float* m, float* v, int64_t n,
                                float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                const float* grad_scale, float* ema, float ema_decay, const int32_t* verdict, void* stream);
int vgpt_sumsq_keep(const void* g, int g_f32, float* total, float* part, int64_t n, float* partial_ws /* >= 1024 floats */,
                    void* stream);
int vgpt_count_nonfinite(const void* x, int x_f32, int64_t n, const int64_t* offsets, int T, int32_t* counts, void* stream);

/* ---- LoRA adapters (LVM/train/train_x1_stage1_noiseinput.py:204-223, peft LoraConfig on qkv_proj / o_proj; the merge of
 *      LVM/pipeline.py:97-101) ------------------------------------------------------------------------------------------
 * Three products with one skinny side.  Every small operand carries a PADDED rank rp in {16, 32, 48, 64} (anything else:
 * VGPT_ERR_UNSUPPORTED); the caller owns the padding: ranks r..rp-1 of every small operand are zero and stay zero, the
 * kernels read rp-wide vectors unmasked.  bf16 operands, fp32 accumulation; the big operand has a row stride in elements
 * (ld >= width, ld % 8 == 0; widths are multiples of 8; every pointer 16-byte aligned).
 *   vgpt_lora_down: U (M, rp) bf16 = alpha X (M, K; ldx) S, with S stored (rp, K) row-major (s_is_k_by_rp = 0: u = x A^T, A as
 *       peft stores it) or (K, rp) row-major (s_is_k_by_rp = 1: du = dy B).  X is read once.
 *   vgpt_lora_up_add: in place, Y (M, N; ldy) = bf16(rope?(float(Y) + alpha U (M, rp) S)), S stored (N, rp) (s_is_rp_by_n = 0)
 *       or (rp, N) (s_is_rp_by_n = 1); one read and one write of Y.  cos_t / sin_t NULL: no rotation.  Otherwise (M, head_dim / 2)
 *       fp32 tables of vgpt_rope_table and N = (n_heads + 2 n_kv_heads) head_dim: the q and k heads are rotated as in
 *       vgpt_gemm_bf16_rope (pairs d, d + head_dim / 2; on the fp32 sum, one rounding), the v columns are not.  head_dim % 16 == 0,
 *       head_dim <= 128.  Serves y += s u B^T (forward), dx += du A (backward) and the merge W += s B A (Y = W, U = B, S = A).
 *   vgpt_lora_grad: G (N, rp) fp32 = alpha Y (M, N; ldy)^T U (M, rp; ldu), stored (rp, N) when store_transposed != 0
 *       (dB = s dy^T u, dA = du^T x).  The reduction over M is cut into slices, a function of (M, N) alone, that are added in a
 *       fixed order: the result is bit-identical from run to run.  workspace: vgpt_lora_grad_workspace_bytes(M, N, rp) bytes
 *       (0: none needed), 16-byte aligned; a smaller one is VGPT_ERR_INVALID. */
int vgpt_lora_down(const void* X, const void* S, void* U, int64_t M, int64_t K, int rp, int64_t ldx, int s_is_k_by_rp,
                   float alpha, void* stream);
int vgpt_lora_up_add(void* Y, const void* U, const void* S, const float* cos_t, const float* sin_t, int64_t M, int64_t N,
                     int rp, int64_t ldy, int s_is_rp_by_n, int n_heads, int n_kv_heads, int head_dim, float alpha,
                     void* stream);
int64_t vgpt_lora_grad_workspace_bytes(int64_t M, int64_t N, int rp);
int vgpt_lora_grad(const void* Y, const void* U, float* G, int64_t M, int64_t N, int rp, int64_t ldy, int64_t ldu,
                   int store_transposed, float alpha, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- frame preprocessing (LVM/processor.py:31-35, 39-64 crop_arr, 78-86; LVM/utils.py:47-66 center_crop_arr) ----------------
 * Decoded uint8 frames -> the (N, 3, h, w) fp32 tensors in [-1, 1] the VAE encoder reads, without leaving the device:
 * PIL.Image.resize with BOX / BICUBIC, the centre crop, ToTensor + Normalize(0.5, 0.5).  The resampler is Pillow's 8-bit one
 * restated: integer arithmetic on a coefficient table built in double precision, so results are Pillow's bit for bit.
 * Frames are (N, H, W, 3) uint8, contiguous, exactly 3 channels (the ABI has no channel argument); any byte alignment.
 *   One pass along one axis (input length in, output length out, filter support S: BOX 0.5, BICUBIC 2 with a = -0.5):
 *       scale = in / out, fs = max(scale, 1), sup = S fs, ksize = 2 (int)ceil(sup) + 1, ss = 1 / fs; for output xx:
 *       center = (xx + 0.5) scale, xmin = max((int)(center - sup + 0.5), 0), xmax = min((int)(center + sup + 0.5), in) - xmin,
 *       w[x] = f((x + xmin - center + 0.5) ss) for x < xmax, normalised by their sum (added in index order) when it is not 0,
 *       k[x] = (int)(w[x] 2^22 +- 0.5) truncated toward zero (the sign of w[x] picks +-), k[xmax..ksize-1] = 0;
 *       out byte = clamp((2^21 + sum_x src[xmin + x] k[x]) >> 22, 0, 255), arithmetic shift on a signed 32-bit sum.
 *   A resize is the horizontal pass if the width changes, then the vertical pass if the height changes, on the uint8 result
 *   of the first; a pass whose length does not change is NOT run (the caller skips it).
 *   vgpt_resample_ksize: host only.  ksize of a pass; sizes < 1 or an unknown filter: VGPT_ERR_INVALID; ksize >
 *       VGPT_RESAMPLE_MAX_KSIZE: VGPT_ERR_UNSUPPORTED (129 admits a BICUBIC ratio of 32; crop_arr never exceeds 9).
 *   vgpt_resample_coeffs: host only, writes HOST memory: bounds[2 xx] = xmin, bounds[2 xx + 1] = xmax (2 out words) and
 *       coeffs (out, ksize).  Same refusals; a NULL pointer: VGPT_ERR_INVALID.
 *   vgpt_resample_u8: one pass over DEVICE pointers, bounds / coeffs being device copies of the table above for
 *       (in_w, out_len) when axis = 1 (horizontal: dst is (N, in_h, out_len, 3)) or (in_h, out_len) when axis = 0 (vertical:
 *       dst is (N, out_len, in_w, 3)).  Table entries are clamped to the image, so a wrong table gives wrong pixels only.
 *       NULL pointer, another axis, n_frames < 0, a side or ksize < 1, dst == src: VGPT_ERR_INVALID; ksize >
 *       VGPT_RESAMPLE_MAX_KSIZE or a side > 2^24: VGPT_ERR_UNSUPPORTED; n_frames == 0: VGPT_OK.
 *   vgpt_u8_to_chw_norm: dst_f32 (N, 3, h, w)[n][c][y][x] = norm(src[n][y0 + y][x0 + x][c]) with norm(b) =
 *       (fp32(b) / 255.0f - 0.5f) / 0.5f, both divisions correctly rounded (ToTensor + Normalize on the CPU).  A window
 *       with a negative offset, a side < 1 or an end past H / W: VGPT_ERR_INVALID, naming the values.
 *   vgpt_resample_u8_v_chw_norm: the vertical pass (in_h -> out_h) writing the window (y0, x0, h, w) of its (out_h, in_w)
 *       result as normalised planar fp32: bit for bit vgpt_resample_u8(axis 0) followed by vgpt_u8_to_chw_norm, without the
 *       uint8 image in between and without the rows and columns the crop drops. */
#define VGPT_FILTER_BOX 0
#define VGPT_FILTER_BICUBIC 1
#define VGPT_RESAMPLE_MAX_KSIZE 129
int vgpt_resample_ksize(int in, int out, int filter);
int vgpt_resample_coeffs(int in, int out, int filter, int32_t* bounds /* 2*out: xmin, xmax */, int32_t* coeffs /* out*ksize */);
int vgpt_resample_u8(const void* src, void* dst, const int32_t* bounds, const int32_t* coeffs, int ksize, int n_frames,
                     int in_h, int in_w, int out_len, int axis, void* stream);
int vgpt_u8_to_chw_norm(const void* src, float* dst_f32, int n_frames, int H, int W, int y0, int x0, int h, int w,
                        void* stream);
int vgpt_resample_u8_v_chw_norm(const void* src, float* dst_f32, const int32_t* bounds, const int32_t* coeffs, int ksize,
                                int n_frames, int in_h, int in_w, int out_h, int y0, int x0, int h, int w, void* stream);

/* ---- hipGraph helpers (sampler loop under graph capture) ----------------- */
int vgpt_graph_begin_capture(void* stream);
int vgpt_graph_end_capture(void* stream, void** graph_exec_out);
int vgpt_graph_launch(void* graph_exec, void* stream);
int vgpt_graph_destroy(void* graph_exec);

/* ---- box calibration (bench.py `calibration`; never on the product path) -- */
/* 256 workgroups x 8 waves of nothing but mfma_f32_16x16x32_bf16 on random register operands: the rate the matrix pipes
 * hold at the clock this device grants under load (scripts/probes/mfma_shape_rate.hip is the stand-alone form);
 * vgpt_calib_mfma_flops(iters) = the FLOPs one such launch executes.  vgpt_calib_copy: 16-byte-per-lane streaming copy
 * of n_bytes (n_bytes read + n_bytes written): the HBM rate.  The caller times the launches with events on `stream`. */
int vgpt_calib_mfma(float* out, int iters, void* stream);
double vgpt_calib_mfma_flops(int iters);
int vgpt_calib_copy(const void* src, void* dst, int64_t n_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VGPT_H */
