// Model-glue kernels around the transformer: token-embedding gather, patch embedding with the
// cropped 2-D sincos position table, timestep embedding, small-M Linear, final adaLN layer with
// unpatchify, and the Euler / CFG sampler update with its second-order, scheduled-guidance and
// stochastic forms (the last makes its noise from a counter, so a replayed graph draws fresh
// numbers). All HBM- or latency-bound; written so the whole denoise step is a fixed sequence of
// launches that can be captured into one hipGraph.
//
// Reference: LVM/model.py:22-83 (modulate, TimestepEmbedder, FinalLayer), :138-154 (PatchEmbedMR),
// :255-327 (unpatchify, cropped_pos_embed, patch_multiple_resolutions), :399-501 (frame_block_forward),
// LVM/scheduler.py:161-208 (Euler loop, x1->v, CFG).
#include "common.h"

namespace {

// ---- embed_tokens gather -------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_gather_kernel(const int64_t* __restrict__ ids,
                                                           const bf16* __restrict__ table,
                                                           bf16* __restrict__ out, int64_t rows,
                                                           int H, int64_t vocab) {
    const int cpr = H >> 3;
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int c = (int)(i % cpr);
        int64_t id = ids[row];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        *reinterpret_cast<bf16x8*>(out + row * H + c * 8) =
            *reinterpret_cast<const bf16x8*>(table + id * H + c * 8);
    }
}

// ---- patch embed: Conv2d(C -> H, k=2, s=2) == 16-wide dot per (token, channel) ---------------
// grid.x = token tiles of 16 tokens, grid.y = frames; each thread owns 4 output channels for
// every token of the tile (weights stay in registers across the 16 tokens).
__global__ __launch_bounds__(256) void patch_embed_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ Wp, const bf16* __restrict__ bias,
    const bf16* __restrict__ pos, const int32_t* __restrict__ dst_row, bf16* __restrict__ seq,
    int C, int h, int w, int H, int pos_max) {
    __shared__ float patch[16][16];
    const int f = blockIdx.y;
    const int h2 = h >> 1, w2 = w >> 1;
    const int ntok = h2 * w2;
    const int t0 = blockIdx.x * 16;
    // stage the 16 patches (16 values each): thread -> (token, element)
    {
        const int tl = threadIdx.x >> 4, e = threadIdx.x & 15;
        const int t = t0 + tl;
        float v = 0.f;
        if (t < ntok) {
            const int ci = e >> 2, p = (e >> 1) & 1, q = e & 1;  // weight layout (H, C, 2, 2)
            const int i = t / w2, j = t % w2;
            v = bf2f(x[(((int64_t)f * C + ci) * h + 2 * i + p) * w + 2 * j + q]);
        }
        patch[tl][e] = v;
    }
    __syncthreads();
    const int top = (pos_max - h2) / 2, left = (pos_max - w2) / 2;
    const int64_t row0 = dst_row[f];
    for (int c0 = threadIdx.x * 4; c0 < H; c0 += 256 * 4) {
        float wreg[4][16];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const bf16x8 lo = *reinterpret_cast<const bf16x8*>(Wp + (int64_t)(c0 + cc) * 16);
            const bf16x8 hi = *reinterpret_cast<const bf16x8*>(Wp + (int64_t)(c0 + cc) * 16 + 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                wreg[cc][e] = bf2f(lo[e]);
                wreg[cc][8 + e] = bf2f(hi[e]);
            }
        }
        const bf16x4 bv = *reinterpret_cast<const bf16x4*>(bias + c0);
        for (int tl = 0; tl < 16; ++tl) {
            const int t = t0 + tl;
            if (t >= ntok) break;
            const int i = t / w2, j = t % w2;
            const bf16x4 pv = *reinterpret_cast<const bf16x4*>(
                pos + ((int64_t)(top + i) * pos_max + left + j) * H + c0);
            bf16x4 o;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                float acc = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc += wreg[cc][e] * patch[tl][e];
                o[cc] = f2bf(acc + bf2f(bv[cc]) + bf2f(pv[cc]));
            }
            *reinterpret_cast<bf16x4*>(seq + (row0 + t) * H + c0) = o;
        }
    }
}

// ---- timestep sinusoid ------------------------------------------------------------------------
__global__ void timestep_sinusoid_kernel(const float* __restrict__ t, const float* __restrict__ freqs,
                                         bf16* __restrict__ out, int n, int half) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * half) return;
    const int m = idx / half, i = idx % half;
    const float arg = t[m] * freqs[i];
    out[(int64_t)m * 2 * half + i] = f2bf(cosf(arg));
    out[(int64_t)m * 2 * half + half + i] = f2bf(sinf(arg));
}

// ---- small-M Linear: one wave per output column, W row streamed once ---------------------------
template <int MT>
__global__ __launch_bounds__(256) void linear_small_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ W, const bf16* __restrict__ bias,
    bf16* __restrict__ out, const int32_t* __restrict__ out_row, int M, int N, int K, int64_t ldx,
    int64_t ldo, int pre_act, int post_act) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int n = blockIdx.x * 4 + wave; n < N; n += gridDim.x * 4) {
        float acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = 0.f;
        const bf16* wr = W + (int64_t)n * K;
        for (int k = lane * 8; k < K; k += 512) {
            const bf16x8 wv = *reinterpret_cast<const bf16x8*>(wr + k);
            float wf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) wf[j] = bf2f(wv[j]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (m < M) {
                    const bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + (int64_t)m * ldx + k);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float xf = bf2f(xv[j]);
                        if (pre_act != VGPT_ACT_NONE) xf = bf2f(f2bf(act_apply(xf, pre_act)));
                        acc[m] += wf[j] * xf;
                    }
                }
            }
        }
        const float bn = bias ? bf2f(bias[n]) : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                float v = wave_sum(acc[m]) + bn;
                v = act_apply(v, post_act);
                if (lane == 0) {
                    const int64_t r = out_row ? (int64_t)out_row[m] : (int64_t)m;
                    out[r * ldo + n] = f2bf(v);
                }
            }
        }
    }
}

// ---- final layer: LayerNorm(no affine) + modulate + Linear(H -> 16) + unpatchify ---------------
// one wave per token; NCH = 512-element slabs cached in registers
template <int NCH>
__global__ __launch_bounds__(256) void final_layer_kernel(
    const bf16* __restrict__ hidden, const int32_t* __restrict__ src_row, const bf16* __restrict__ mod,
    const bf16* __restrict__ Wf, const bf16* __restrict__ bfin, bf16* __restrict__ out, int C, int h,
    int w, int H, float eps) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int f = blockIdx.y;
    const int h2 = h >> 1, w2 = w >> 1;
    const int ntok = h2 * w2;
    const int t = blockIdx.x * 4 + wave;
    if (t >= ntok) return;
    const bf16* xr = hidden + ((int64_t)src_row[f] + t) * H;
    const bf16* shift = mod + (int64_t)f * 2 * H;
    const bf16* scale = shift + H;
    float v[NCH][8];
    float s1 = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int off = (c * 64 + lane) * 8;
        if (off < H) {
            const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xr + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[c][j] = bf2f(xv[j]);
                s1 += v[c][j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c][j] = 0.f;
        }
    }
    const float mean = wave_sum(s1) / (float)H;
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int off = (c * 64 + lane) * 8;
        if (off < H) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[c][j] - mean;
                s2 += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(s2) / (float)H + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int off = (c * 64 + lane) * 8;
        if (off < H) {
            const bf16x8 sh = *reinterpret_cast<const bf16x8*>(shift + off);
            const bf16x8 sc = *reinterpret_cast<const bf16x8*>(scale + off);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                v[c][j] = (v[c][j] - mean) * rstd * (1.0f + bf2f(sc[j])) + bf2f(sh[j]);
        }
    }
    // 16 outputs: y[o] = sum_k v[k] Wf[o][k] + b[o]
    float y = 0.f;  // lane o (< 16) keeps output o
    for (int o = 0; o < 16; ++o) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int off = (c * 64 + lane) * 8;
            if (off < H) {
                const bf16x8 wv = *reinterpret_cast<const bf16x8*>(Wf + (int64_t)o * H + off);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc += v[c][j] * bf2f(wv[j]);
            }
        }
        acc = wave_sum(acc);
        if (lane == o) y = acc + bf2f(bfin[o]);
    }
    if (lane < 16) {
        // unpatchify: out[f][c][2i+p][2j+q] = y[(p*2+q)*C + c]
        const int c = lane % C, pq = lane / C;
        const int p = pq >> 1, q = pq & 1;
        const int i = t / w2, j = t % w2;
        out[(((int64_t)f * C + c) * h + 2 * i + p) * w + 2 * j + q] = f2bf(y);
    }
}

// ---- sampler -----------------------------------------------------------------------------------
// `n_steps` = entries of the sigma table - 1: a replay past the end of the table (step >= n_steps) is a no-op instead of
// an out-of-bounds read of sigma[step + 1]
__global__ void set_timesteps_kernel(const float* sigma, const int32_t* step, float* ts, int n, int n_steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int st = *step;
    if (i < n && st >= 0 && st <= n_steps) ts[i] = sigma[st];
}

__global__ __launch_bounds__(256) void euler_cfg_kernel(float* __restrict__ z, bf16* __restrict__ zm,
                                                        const bf16* __restrict__ pred,
                                                        const float* __restrict__ sigma,
                                                        const int32_t* __restrict__ step, int n_steps, int n_frames,
                                                        int64_t elems, int pred_type, int use_cfg,
                                                        float cfg_scale) {
    const int st = *step;
    if (st < 0 || st >= n_steps) return;   // past the sigma table: leave the state untouched
    const float sg = sigma[st], sg_next = sigma[st + 1];
    const float dt = sg_next - sg;
    const float inv = 1.0f / (1.0f - sg);
    const int half = use_cfg ? n_frames / 2 : n_frames;
    const int64_t total = (int64_t)half * elems;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        float zc = z[i];
        float vc = bf2f(pred[i]);
        if (pred_type == VGPT_PRED_X1) vc = (vc - zc) * inv;
        if (use_cfg) {
            const int64_t iu = i + total;
            float zu = z[iu];
            float vu = bf2f(pred[iu]);
            if (pred_type == VGPT_PRED_X1) vu = (vu - zu) * inv;
            vc = vu + cfg_scale * (vc - vu);
            zu += dt * vc;
            z[iu] = zu;
            zm[iu] = f2bf(zu);
        }
        zc += dt * vc;
        z[i] = zc;
        zm[i] = f2bf(zc);
    }
}

// Second-order updates on the same state.  `vh` keeps the guided velocity of the step, one fp32 per element
// of one CFG half.  MODE 0: ab2 (z += h_i (v_i + h_i / (2 h_{i-1}) (v_i - v_{i-1})), step 0 = Euler, vh written every step).
// MODE 1: Heun predictor (vh = v_i, zm = bf16(z + h_i v_i), z untouched; at the last step, where sigma[i+1] = 1 and the
// corrector's x1 conversion would divide by zero, a full Euler step).  MODE 2: Heun corrector, launched after the step
// counter moved on: i = *step - 1, z' = z + h_i vh recomputed in fp32, v' from `pred` at sigma[i+1], z += h_i/2 (v_i + v').
// Where an update degenerates to Euler (ab2's step 0, ab2 on an unchanged velocity, Heun's last step) it must give
// euler_cfg_kernel's bits, and which a * b + c the compiler fuses there is its choice per kernel.  So contraction is off in
// this kernel and every rounding is spelled out, in the sequence euler_cfg_kernel compiles to for gfx950: CFG combination
// fused, the conditional half z + rn(h v) in two roundings, the unconditional half fma(h, v, z)
// (tests/test_solver_kernels_gpu.py::test_euler_identities_bit_for_bit holds the two kernels together).
template <int MODE>
__global__ __launch_bounds__(256) void solver_update_kernel(float* __restrict__ z, bf16* __restrict__ zm,
                                                            const bf16* __restrict__ pred, float* __restrict__ vh,
                                                            const float* __restrict__ sigma,
                                                            const int32_t* __restrict__ step, int n_steps, int n_frames,
                                                            int64_t elems, int pred_type, int use_cfg, float cfg_scale) {
#pragma clang fp contract(off)
    const int st = *step;
    // the corrector reads sigma[st - 1], sigma[st]; the others sigma[st], sigma[st + 1] (and ab2 sigma[st - 1] for st >= 1)
    if (MODE == 2 ? (st < 1 || st >= n_steps) : (st < 0 || st >= n_steps)) return;
    const int s0 = MODE == 2 ? st - 1 : st;
    const float sg = sigma[s0], sg_next = sigma[s0 + 1];
    const float dt = sg_next - sg;
    const float inv = 1.0f / (1.0f - (MODE == 2 ? sg_next : sg));   // x1 -> v at the sigma the prediction was made at
    const bool two_step = MODE == 0 && st >= 1;
    const float ratio = two_step ? 0.5f * dt / (sg - sigma[st - 1]) : 0.f;
    const bool euler_tail = MODE == 1 && st == n_steps - 1;
    const int half = use_cfg ? n_frames / 2 : n_frames;
    const int64_t total = (int64_t)half * elems;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t iu = i + total;
        float zc = z[i], zu = use_cfg ? z[iu] : 0.f;
        float v0 = 0.f;
        float zpc = zc, zpu = zu;   // the state the prediction was made from
        if (MODE == 2) {
            v0 = vh[i];
            zpc = __builtin_fmaf(dt, v0, zc);   // as the predictor computed it before rounding it to bf16
            zpu = __builtin_fmaf(dt, v0, zu);
        }
        float vc = bf2f(pred[i]);
        if (pred_type == VGPT_PRED_X1) vc = (vc - zpc) * inv;
        if (use_cfg) {
            float vu = bf2f(pred[iu]);
            if (pred_type == VGPT_PRED_X1) vu = (vu - zpu) * inv;
            vc = __builtin_fmaf(cfg_scale, vc - vu, vu);
        }
        if (MODE == 0) {
            float ve = vc;
            if (two_step) ve = __builtin_fmaf(ratio, vc - vh[i], vc);
            vh[i] = vc;
            zc = zc + dt * ve;
            zu = __builtin_fmaf(dt, ve, zu);
        } else if (MODE == 1) {
            if (!euler_tail) {
                vh[i] = vc;
                zm[i] = f2bf(__builtin_fmaf(dt, vc, zc));
                if (use_cfg) zm[iu] = f2bf(__builtin_fmaf(dt, vc, zu));
                continue;
            }
            zc = zc + dt * vc;
            zu = __builtin_fmaf(dt, vc, zu);
        } else {
            const float hh = 0.5f * dt, vs = v0 + vc;
            zc = __builtin_fmaf(hh, vs, zc);
            zu = __builtin_fmaf(hh, vs, zu);
        }
        z[i] = zc;
        zm[i] = f2bf(zc);
        if (use_cfg) {
            z[iu] = zu;
            zm[iu] = f2bf(zu);
        }
    }
}

// solver_update_kernel under a per-step guidance scale: CFG always, the scale of the launch is
// cfg_table[i] with i the index the launch reads sigma at (the corrector: *step - 1, the scale its predictor used).  MODE
// 0 / 1 / 2 as above, MODE 3: Euler, in the roundings euler_cfg_kernel compiles to (the comment above).  An entry that is
// exactly 1.0f is an unguided step: v = v_c, and the unconditional half of `pred` is NOT loaded -- the engine did not
// compute it (engine.py: skip_unguided_branch) and what lies there is stale.  Both halves of z still move by v, each in
// its own rounding, and vh keeps v.  With any other entry every statement is solver_update_kernel's with use_cfg = 1, so
// a table of one value s != 1 gives that kernel's bits with cfg_scale = s.
template <int MODE>
__global__ __launch_bounds__(256) void solver_update_sched_kernel(float* __restrict__ z, bf16* __restrict__ zm,
                                                                  const bf16* __restrict__ pred, float* __restrict__ vh,
                                                                  const float* __restrict__ sigma,
                                                                  const float* __restrict__ cfg_table,
                                                                  const int32_t* __restrict__ step, int n_steps,
                                                                  int n_frames, int64_t elems, int pred_type) {
#pragma clang fp contract(off)
    const int st = *step;
    if (MODE == 2 ? (st < 1 || st >= n_steps) : (st < 0 || st >= n_steps)) return;   // past either table: a no-op
    const int s0 = MODE == 2 ? st - 1 : st;
    const float sg = sigma[s0], sg_next = sigma[s0 + 1];
    const float cfg_scale = cfg_table[s0];
    const bool guided = cfg_scale != 1.0f;
    const float dt = sg_next - sg;
    const float inv = 1.0f / (1.0f - (MODE == 2 ? sg_next : sg));
    const bool two_step = MODE == 0 && st >= 1;
    const float ratio = two_step ? 0.5f * dt / (sg - sigma[st - 1]) : 0.f;
    const bool euler_tail = MODE == 1 && st == n_steps - 1;
    const int64_t total = (int64_t)(n_frames / 2) * elems;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t iu = i + total;
        float zc = z[i], zu = z[iu];
        float v0 = 0.f;
        float zpc = zc, zpu = zu;   // the state the prediction was made from
        if (MODE == 2) {
            v0 = vh[i];
            zpc = __builtin_fmaf(dt, v0, zc);
            zpu = __builtin_fmaf(dt, v0, zu);
        }
        float vc = bf2f(pred[i]);
        if (pred_type == VGPT_PRED_X1) vc = (vc - zpc) * inv;
        if (guided) {
            float vu = bf2f(pred[iu]);
            if (pred_type == VGPT_PRED_X1) vu = (vu - zpu) * inv;
            vc = __builtin_fmaf(cfg_scale, vc - vu, vu);
        }
        if (MODE == 0) {
            float ve = vc;
            if (two_step) ve = __builtin_fmaf(ratio, vc - vh[i], vc);
            vh[i] = vc;
            zc = zc + dt * ve;
            zu = __builtin_fmaf(dt, ve, zu);
        } else if (MODE == 1) {
            if (!euler_tail) {
                vh[i] = vc;
                zm[i] = f2bf(__builtin_fmaf(dt, vc, zc));
                zm[iu] = f2bf(__builtin_fmaf(dt, vc, zu));
                continue;
            }
            zc = zc + dt * vc;
            zu = __builtin_fmaf(dt, vc, zu);
        } else if (MODE == 2) {
            const float hh = 0.5f * dt, vs = v0 + vc;
            zc = __builtin_fmaf(hh, vs, zc);
            zu = __builtin_fmaf(hh, vs, zu);
        } else {
            zc = zc + dt * vc;
            zu = __builtin_fmaf(dt, vc, zu);
        }
        z[i] = zc;
        zm[i] = f2bf(zc);
        z[iu] = zu;
        zm[iu] = f2bf(zu);
    }
}

// ---- stochastic Euler step ----------------------------------------------------
// Counter-based noise: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11: multipliers,
// Weyl key increments and round function of Random123).  Key = the seed's two words, counter = (block low, block high,
// step index, stream low word), block = e >> 2 with e the element index inside one CFG half.  One call yields the four
// normals of elements 4 block .. 4 block + 3 by Box-Muller on (w0, w1) and (w2, w3): a function of (seed, stream, step,
// element) alone, so a captured step replays fresh numbers every step and every launch shape gives the same ones.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// u1 = ((w >> 9) + 0.5) 2^-23 in (0, 1) and u2 = (w >> 8) 2^-24 in [0, 1) are exact in fp32; r = sqrtf(-2 logf(u1));
// (r cospif(2 u2), r sinpif(2 u2)).  The accurate logf / sincospif; every product is one rounding.
__device__ __forceinline__ void sde_normals(const int64_t* __restrict__ rng, int64_t block, int step, float (&eps)[4]) {
#pragma clang fp contract(off)
    const uint64_t seed = (uint64_t)rng[0];
    uint32_t w[4];
    philox4x32_10((uint32_t)block, (uint32_t)((uint64_t)block >> 32), (uint32_t)step, (uint32_t)(uint64_t)rng[1],
                  (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = ((float)(w[2 * p] >> 9) + 0.5f) * 0x1p-23f;
        const float u2 = (float)(w[2 * p + 1] >> 8) * 0x1p-24f;
        const float r = sqrtf(-2.0f * logf(u1));
        float s, c;
        sincospif(2.0f * u2, &s, &c);
        eps[2 * p] = r * c;
        eps[2 * p + 1] = r * s;
    }
}

__global__ __launch_bounds__(256) void noise_fill_kernel(float* __restrict__ out, int64_t n,
                                                         const int64_t* __restrict__ rng, int step) {
    const int64_t blocks = (n + 3) >> 2;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += (int64_t)gridDim.x * blockDim.x) {
        float eps[4];
        sde_normals(rng, b, step, eps);
        const int64_t e = b << 2;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (e + l < n) out[e + l] = eps[l];
    }
}

// The Euler step with noise re-injected, eta = eta_table[*step]:
//   x0_hat = z - sigma_i v,   z' = (z + h v) + (1 - sigma_{i+1}) ((sqrt(1 - eta^2) - 1) x0_hat + eta eps)
// The Euler part is statement for statement euler_cfg_kernel's in the roundings it compiles to (the comment above
// solver_update_kernel), with a guidance table solver_update_sched_kernel<3>'s; with eta == 0.0f exactly, or at the last
// step (1 - sigma_{i+1} == 0), nothing else is computed and those kernels' bits come out.  The noise term of one state
// element, every rounding spelled out: x0 = fma(-sigma_i, v, z); t = fma(eta, eps, rn(ca x0)), ca = rn(sqrtf(rn(1 -
// rn(eta eta))) - 1); z' = fma(g, t, z_euler), g = rn(1 - sigma_{i+1}).  Each thread owns one Philox block: four
// consecutive elements e of one CFG half, and every frame that shares the half's noise (`paired`: the unconditional half
// under CFG, frames [n/2, n) under share_halves) gets the same eps at the same e.  VEC: 16-byte z and 8-byte bf16
// accesses, for a half size that is a multiple of 4 on pointers aligned that far; otherwise element by element, the tail
// thread using the lanes it owns.  Both forms run the same statements per element.
template <bool VEC>
__global__ __launch_bounds__(256) void sde_update_kernel(float* __restrict__ z, bf16* __restrict__ zm,
                                                         const bf16* __restrict__ pred,
                                                         const float* __restrict__ sigma,
                                                         const float* __restrict__ cfg_table,
                                                         const float* __restrict__ eta_table,
                                                         const int64_t* __restrict__ rng,
                                                         const int32_t* __restrict__ step, int n_steps, int n_frames,
                                                         int64_t elems, int pred_type, int use_cfg, float cfg_scale,
                                                         int share_halves) {
#pragma clang fp contract(off)
    const int st = *step;
    if (st < 0 || st >= n_steps) return;   // past the tables: leave everything untouched
    const float sg = sigma[st], sg_next = sigma[st + 1];
    const float eta = eta_table[st];
    if (cfg_table) cfg_scale = cfg_table[st];
    const bool guided = use_cfg && !(cfg_table && cfg_scale == 1.0f);   // an entry of exactly 1: v = v_c, pred[iu] not loaded
    const float dt = sg_next - sg;
    const float inv = 1.0f / (1.0f - sg);
    const float g = 1.0f - sg_next;
    const bool noisy = eta != 0.0f && g != 0.0f;
    const float ca = sqrtf(1.0f - eta * eta) - 1.0f;
    const bool paired = use_cfg || share_halves;
    const int64_t total = (int64_t)(paired ? n_frames / 2 : n_frames) * elems;
    const int64_t blocks = (total + 3) >> 2;
    const bool x1 = pred_type == VGPT_PRED_X1;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = b << 2, eu = e + total;
        const int cnt = VEC ? 4 : (int)(total - e < 4 ? total - e : 4);
        float eps[4] = {0.f, 0.f, 0.f, 0.f};
        if (noisy) sde_normals(rng, b, st, eps);
        float zc[4] = {}, zu[4] = {}, pc[4] = {}, pu[4] = {};
        if (VEC) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(z + e);
            const bf16x4 p = *reinterpret_cast<const bf16x4*>(pred + e);
#pragma unroll
            for (int l = 0; l < 4; ++l) { zc[l] = a[l]; pc[l] = bf2f(p[l]); }
            if (paired) {
                const f32x4 c = *reinterpret_cast<const f32x4*>(z + eu);
#pragma unroll
                for (int l = 0; l < 4; ++l) zu[l] = c[l];
            }
            if (guided || !use_cfg) {
                if (paired) {
                    const bf16x4 q = *reinterpret_cast<const bf16x4*>(pred + eu);
#pragma unroll
                    for (int l = 0; l < 4; ++l) pu[l] = bf2f(q[l]);
                }
            }
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                if (l >= cnt) continue;
                zc[l] = z[e + l];
                pc[l] = bf2f(pred[e + l]);
                if (paired) {
                    zu[l] = z[eu + l];
                    if (guided || !use_cfg) pu[l] = bf2f(pred[eu + l]);
                }
            }
        }
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (l >= cnt) continue;
            float vc = pc[l];
            if (x1) vc = (vc - zc[l]) * inv;
            float vs = vc;   // the velocity of the paired frame: the guided one under CFG, its own prediction's otherwise
            if (use_cfg) {
                if (guided) {
                    float vu = pu[l];
                    if (x1) vu = (vu - zu[l]) * inv;
                    vc = __builtin_fmaf(cfg_scale, vc - vu, vu);
                }
                vs = vc;
            } else if (paired) {
                vs = pu[l];
                if (x1) vs = (vs - zu[l]) * inv;
            }
            float zn = zc[l] + dt * vc;
            if (noisy) zn = __builtin_fmaf(g, __builtin_fmaf(eta, eps[l], ca * __builtin_fmaf(-sg, vc, zc[l])), zn);
            zc[l] = zn;
            if (paired) {
                // CFG: the unconditional half moves by fma(h, v, z), as in euler_cfg_kernel; frames that only share
                // the noise are conditional-shaped elements of their own
                float zq = use_cfg ? __builtin_fmaf(dt, vs, zu[l]) : zu[l] + dt * vs;
                if (noisy) zq = __builtin_fmaf(g, __builtin_fmaf(eta, eps[l], ca * __builtin_fmaf(-sg, vs, zu[l])), zq);
                zu[l] = zq;
            }
        }
        if (VEC) {
            f32x4 a;
            bf16x4 p;
#pragma unroll
            for (int l = 0; l < 4; ++l) { a[l] = zc[l]; p[l] = f2bf(zc[l]); }
            *reinterpret_cast<f32x4*>(z + e) = a;
            *reinterpret_cast<bf16x4*>(zm + e) = p;
            if (paired) {
#pragma unroll
                for (int l = 0; l < 4; ++l) { a[l] = zu[l]; p[l] = f2bf(zu[l]); }
                *reinterpret_cast<f32x4*>(z + eu) = a;
                *reinterpret_cast<bf16x4*>(zm + eu) = p;
            }
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                if (l >= cnt) continue;
                z[e + l] = zc[l];
                zm[e + l] = f2bf(zc[l]);
                if (paired) {
                    z[eu + l] = zu[l];
                    zm[eu + l] = f2bf(zu[l]);
                }
            }
        }
    }
}

__global__ void advance_kernel(int32_t* step) { *step += 1; }

__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* __restrict__ src,
                                                            bf16* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = f2bf(src[i]);
}

}  // namespace

VGPT_EXPORT int vgpt_embed_gather(const int64_t* ids, const void* table, void* out, int64_t rows,
                                  int64_t H, int64_t vocab, void* stream) {
    VGPT_REQUIRE(ids && table && out, VGPT_ERR_INVALID, "vgpt_embed_gather: null pointer");
    VGPT_REQUIRE(rows >= 0 && H > 0 && vocab > 0, VGPT_ERR_INVALID, "vgpt_embed_gather: bad shape");
    VGPT_REQUIRE(H % 8 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_embed_gather: H must be a multiple of 8");
    VGPT_REQUIRE(H < (1ll << 31), VGPT_ERR_UNSUPPORTED, "vgpt_embed_gather: H=%lld too large", (long long)H);
    if (rows == 0) return VGPT_OK;
    int grid = (int)std::min<int64_t>(cdiv(rows * (H / 8), 256), (int64_t)1 << 30);
    hipLaunchKernelGGL(embed_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ids,
                       (const bf16*)table, (bf16*)out, rows, (int)H, vocab);
    VGPT_CHECK_LAUNCH("vgpt_embed_gather");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_patch_embed_fwd(const void* x, const void* Wp, const void* bias,
                                     const void* pos_embed, const int32_t* dst_row, void* seq,
                                     int n_frames, int C, int h, int w, int64_t H, int pos_max,
                                     void* stream) {
    VGPT_REQUIRE(x && Wp && bias && pos_embed && dst_row && seq, VGPT_ERR_INVALID,
                 "vgpt_patch_embed_fwd: null pointer");
    VGPT_REQUIRE(n_frames >= 0 && C > 0 && h > 0 && w > 0 && H > 0, VGPT_ERR_INVALID,
                 "vgpt_patch_embed_fwd: bad shape");
    VGPT_REQUIRE(C * 4 == 16 && h % 2 == 0 && w % 2 == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_patch_embed_fwd: needs in_channels=4, patch 2, even latent size");
    VGPT_REQUIRE(H % 4 == 0, VGPT_ERR_UNSUPPORTED, "vgpt_patch_embed_fwd: H must be a multiple of 4");
    VGPT_REQUIRE(H < (1ll << 31), VGPT_ERR_UNSUPPORTED, "vgpt_patch_embed_fwd: H=%lld too large", (long long)H);
    VGPT_REQUIRE(h / 2 <= pos_max && w / 2 <= pos_max, VGPT_ERR_INVALID,
                 "vgpt_patch_embed_fwd: latent larger than pos_embed_max_size");
    if (n_frames == 0) return VGPT_OK;
    const int ntok = (h / 2) * (w / 2);
    hipLaunchKernelGGL(patch_embed_kernel, dim3((unsigned)cdiv(ntok, 16), n_frames), dim3(256), 0,
                       (hipStream_t)stream, (const bf16*)x, (const bf16*)Wp, (const bf16*)bias,
                       (const bf16*)pos_embed, dst_row, (bf16*)seq, C, h, w, (int)H, pos_max);
    VGPT_CHECK_LAUNCH("vgpt_patch_embed_fwd");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_timestep_sinusoid(const float* t, const float* freqs, void* out, int n,
                                       int half, void* stream) {
    VGPT_REQUIRE(t && freqs && out, VGPT_ERR_INVALID, "vgpt_timestep_sinusoid: null pointer");
    VGPT_REQUIRE(n >= 0 && half > 0, VGPT_ERR_INVALID, "vgpt_timestep_sinusoid: bad shape");
    if (n == 0) return VGPT_OK;
    hipLaunchKernelGGL(timestep_sinusoid_kernel, dim3((unsigned)cdiv((int64_t)n * half, 256)),
                       dim3(256), 0, (hipStream_t)stream, t, freqs, (bf16*)out, n, half);
    VGPT_CHECK_LAUNCH("vgpt_timestep_sinusoid");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_linear_small(const void* x, const void* W, const void* bias, void* out,
                                  const int32_t* out_row, int M, int64_t N, int64_t K, int64_t ldx,
                                  int64_t ldo, int pre_act, int post_act, void* stream) {
    VGPT_REQUIRE(x && W && out, VGPT_ERR_INVALID, "vgpt_linear_small: null pointer");
    VGPT_REQUIRE(M >= 0 && N > 0 && K > 0, VGPT_ERR_INVALID, "vgpt_linear_small: bad shape");
    VGPT_REQUIRE(M <= 32, VGPT_ERR_UNSUPPORTED, "vgpt_linear_small: M=%d > 32", M);
    VGPT_REQUIRE(K % 8 == 0 && ldx % 8 == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_linear_small: K and ldx must be multiples of 8");
    VGPT_REQUIRE(N < (1ll << 31) && K < (1ll << 31), VGPT_ERR_UNSUPPORTED,
                 "vgpt_linear_small: dimension too large");
    VGPT_REQUIRE(ldx >= K, VGPT_ERR_INVALID, "vgpt_linear_small: ldx=%lld < K=%lld", (long long)ldx, (long long)K);
    VGPT_REQUIRE(ldo >= N, VGPT_ERR_INVALID, "vgpt_linear_small: ldo=%lld < N=%lld", (long long)ldo, (long long)N);
    if (M == 0) return VGPT_OK;
    int grid = (int)std::min<int64_t>(cdiv(N, 4), 256 * 8);
    hipStream_t s = (hipStream_t)stream;
#define LS_CASE(MT)                                                                               \
    hipLaunchKernelGGL(linear_small_kernel<MT>, dim3(grid), dim3(256), 0, s, (const bf16*)x,       \
                       (const bf16*)W, (const bf16*)bias, (bf16*)out, out_row, M, (int)N, (int)K, \
                       ldx, ldo, pre_act, post_act)
    if (M <= 8) LS_CASE(8);
    else if (M <= 16) LS_CASE(16);
    else LS_CASE(32);
#undef LS_CASE
    VGPT_CHECK_LAUNCH("vgpt_linear_small");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_final_layer_fwd(const void* hidden, const int32_t* src_row, const void* mod,
                                     const void* Wf, const void* bf, void* out, int n_frames, int C,
                                     int h, int w, int64_t H, float eps, void* stream) {
    VGPT_REQUIRE(hidden && src_row && mod && Wf && bf && out, VGPT_ERR_INVALID,
                 "vgpt_final_layer_fwd: null pointer");
    VGPT_REQUIRE(n_frames >= 0 && C > 0 && h > 0 && w > 0 && H > 0, VGPT_ERR_INVALID,
                 "vgpt_final_layer_fwd: bad shape");
    VGPT_REQUIRE(C * 4 == 16 && h % 2 == 0 && w % 2 == 0, VGPT_ERR_UNSUPPORTED,
                 "vgpt_final_layer_fwd: needs out_channels=4, patch 2, even latent size");
    VGPT_REQUIRE(H % 8 == 0 && H <= 8 * 512, VGPT_ERR_UNSUPPORTED,
                 "vgpt_final_layer_fwd: H must be a multiple of 8 and <= 4096");
    if (n_frames == 0) return VGPT_OK;
    const int ntok = (h / 2) * (w / 2);
    dim3 grid((unsigned)cdiv(ntok, 4), n_frames);
    hipStream_t s = (hipStream_t)stream;
#define FL_CASE(N)                                                                              \
    case N:                                                                                     \
        hipLaunchKernelGGL(final_layer_kernel<N>, grid, dim3(256), 0, s, (const bf16*)hidden,   \
                           src_row, (const bf16*)mod, (const bf16*)Wf, (const bf16*)bf,         \
                           (bf16*)out, C, h, w, (int)H, eps);                                   \
        break;
    switch ((int)cdiv(H, 512)) {
        FL_CASE(1) FL_CASE(2) FL_CASE(3) FL_CASE(4) FL_CASE(5) FL_CASE(6) FL_CASE(7) FL_CASE(8)
    }
#undef FL_CASE
    VGPT_CHECK_LAUNCH("vgpt_final_layer_fwd");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sampler_set_timesteps(const float* sigma, const int32_t* step, int n_steps, float* timesteps,
                                           int n, void* stream) {
    VGPT_REQUIRE(sigma && step && timesteps, VGPT_ERR_INVALID,
                 "vgpt_sampler_set_timesteps: null pointer");
    VGPT_REQUIRE(n >= 0 && n_steps > 0, VGPT_ERR_INVALID, "vgpt_sampler_set_timesteps: bad shape");
    if (n == 0) return VGPT_OK;
    hipLaunchKernelGGL(set_timesteps_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64), 0,
                       (hipStream_t)stream, sigma, step, timesteps, n, n_steps);
    VGPT_CHECK_LAUNCH("vgpt_sampler_set_timesteps");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_euler_cfg_update(float* z, void* z_model, const void* pred, const float* sigma,
                                      const int32_t* step, int n_steps, int n_frames, int64_t elems, int pred_type,
                                      int use_cfg, float cfg_scale, void* stream) {
    VGPT_REQUIRE(z && z_model && pred && sigma && step, VGPT_ERR_INVALID,
                 "vgpt_euler_cfg_update: null pointer");
    VGPT_REQUIRE(n_frames >= 0 && elems >= 0 && n_steps > 0, VGPT_ERR_INVALID, "vgpt_euler_cfg_update: bad shape");
    VGPT_REQUIRE(pred_type == VGPT_PRED_V || pred_type == VGPT_PRED_X1, VGPT_ERR_INVALID,
                 "vgpt_euler_cfg_update: unknown prediction type %d", pred_type);
    VGPT_REQUIRE(!use_cfg || n_frames % 2 == 0, VGPT_ERR_INVALID,
                 "vgpt_euler_cfg_update: CFG needs an even number of frames");
    if (n_frames == 0 || elems == 0) return VGPT_OK;
    const int64_t total = (int64_t)(use_cfg ? n_frames / 2 : n_frames) * elems;
    int grid = (int)std::min<int64_t>(cdiv(total, 256), 2048);
    hipLaunchKernelGGL(euler_cfg_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, z,
                       (bf16*)z_model, (const bf16*)pred, sigma, step, n_steps, n_frames, elems, pred_type,
                       use_cfg, cfg_scale);
    VGPT_CHECK_LAUNCH("vgpt_euler_cfg_update");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sampler_update(float* z, void* z_model, const void* pred, float* v_hist, const float* sigma,
                                    const int32_t* step, int n_steps, int n_frames, int64_t elems, int pred_type,
                                    int use_cfg, float cfg_scale, int solver, int stage, void* stream) {
    VGPT_REQUIRE(solver == VGPT_SOLVER_EULER || solver == VGPT_SOLVER_AB2 || solver == VGPT_SOLVER_HEUN, VGPT_ERR_INVALID,
                 "vgpt_sampler_update: unknown solver %d", solver);
    VGPT_REQUIRE(stage == 0 || stage == 1, VGPT_ERR_INVALID, "vgpt_sampler_update: unknown stage %d", stage);
    VGPT_REQUIRE(stage == 0 || solver == VGPT_SOLVER_HEUN, VGPT_ERR_INVALID,
                 "vgpt_sampler_update: stage %d of the one-stage solver %d", stage, solver);
    VGPT_REQUIRE(z && z_model && pred && sigma && step, VGPT_ERR_INVALID,
                 "vgpt_sampler_update: null pointer (z %p, z_model %p, pred %p, sigma %p, step %p)", (void*)z, z_model, pred,
                 (const void*)sigma, (const void*)step);
    VGPT_REQUIRE(v_hist || solver == VGPT_SOLVER_EULER, VGPT_ERR_INVALID,
                 "vgpt_sampler_update: null v_hist with solver %d (only Euler keeps no history)", solver);
    VGPT_REQUIRE(n_steps > 0, VGPT_ERR_INVALID, "vgpt_sampler_update: n_steps %d <= 0", n_steps);
    VGPT_REQUIRE(n_frames >= 0 && elems >= 0, VGPT_ERR_INVALID, "vgpt_sampler_update: bad shape (%d frames of %lld)",
                 n_frames, (long long)elems);
    VGPT_REQUIRE(pred_type == VGPT_PRED_V || pred_type == VGPT_PRED_X1, VGPT_ERR_INVALID,
                 "vgpt_sampler_update: unknown prediction type %d", pred_type);
    VGPT_REQUIRE(!use_cfg || n_frames % 2 == 0, VGPT_ERR_INVALID,
                 "vgpt_sampler_update: CFG needs an even number of frames (got %d)", n_frames);
    if (solver == VGPT_SOLVER_EULER)   // the Euler kernel itself: its bits by construction
        return vgpt_euler_cfg_update(z, z_model, pred, sigma, step, n_steps, n_frames, elems, pred_type, use_cfg, cfg_scale,
                                     stream);
    if (n_frames == 0 || elems == 0) return VGPT_OK;
    const int64_t total = (int64_t)(use_cfg ? n_frames / 2 : n_frames) * elems;
    int grid = (int)std::min<int64_t>(cdiv(total, 256), 2048);
#define SU_LAUNCH(MODE)                                                                                              \
    hipLaunchKernelGGL(solver_update_kernel<MODE>, dim3(grid), dim3(256), 0, (hipStream_t)stream, z, (bf16*)z_model, \
                       (const bf16*)pred, v_hist, sigma, step, n_steps, n_frames, elems, pred_type, use_cfg, cfg_scale)
    if (solver == VGPT_SOLVER_AB2) SU_LAUNCH(0);
    else if (stage == 0) SU_LAUNCH(1);
    else SU_LAUNCH(2);
#undef SU_LAUNCH
    VGPT_CHECK_LAUNCH("vgpt_sampler_update");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sampler_update_sched(float* z, void* z_model, const void* pred, float* v_hist, const float* sigma,
                                          const float* cfg_table, const int32_t* step, int n_steps, int n_frames,
                                          int64_t elems, int pred_type, int solver, int stage, void* stream) {
    VGPT_REQUIRE(solver == VGPT_SOLVER_EULER || solver == VGPT_SOLVER_AB2 || solver == VGPT_SOLVER_HEUN, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sched: unknown solver %d", solver);
    VGPT_REQUIRE(stage == 0 || stage == 1, VGPT_ERR_INVALID, "vgpt_sampler_update_sched: unknown stage %d", stage);
    VGPT_REQUIRE(stage == 0 || solver == VGPT_SOLVER_HEUN, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sched: stage %d of the one-stage solver %d", stage, solver);
    VGPT_REQUIRE(z && z_model && pred && sigma && step, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sched: null pointer (z %p, z_model %p, pred %p, sigma %p, step %p)", (void*)z, z_model,
                 pred, (const void*)sigma, (const void*)step);
    VGPT_REQUIRE(cfg_table, VGPT_ERR_INVALID, "vgpt_sampler_update_sched: null cfg_table (%p)", (const void*)cfg_table);
    VGPT_REQUIRE(v_hist || solver == VGPT_SOLVER_EULER, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sched: null v_hist with solver %d (only Euler keeps no history)", solver);
    VGPT_REQUIRE(n_steps > 0, VGPT_ERR_INVALID, "vgpt_sampler_update_sched: n_steps %d <= 0", n_steps);
    VGPT_REQUIRE(n_frames >= 0 && elems >= 0, VGPT_ERR_INVALID, "vgpt_sampler_update_sched: bad shape (%d frames of %lld)",
                 n_frames, (long long)elems);
    VGPT_REQUIRE(pred_type == VGPT_PRED_V || pred_type == VGPT_PRED_X1, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sched: unknown prediction type %d", pred_type);
    VGPT_REQUIRE(n_frames % 2 == 0, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sched: CFG needs an even number of frames (got %d)", n_frames);
    if (n_frames == 0 || elems == 0) return VGPT_OK;
    const int64_t total = (int64_t)(n_frames / 2) * elems;
    int grid = (int)std::min<int64_t>(cdiv(total, 256), 2048);
#define SUS_LAUNCH(MODE)                                                                                        \
    hipLaunchKernelGGL(solver_update_sched_kernel<MODE>, dim3(grid), dim3(256), 0, (hipStream_t)stream, z,      \
                       (bf16*)z_model, (const bf16*)pred, v_hist, sigma, cfg_table, step, n_steps, n_frames, elems, \
                       pred_type)
    if (solver == VGPT_SOLVER_EULER) SUS_LAUNCH(3);
    else if (solver == VGPT_SOLVER_AB2) SUS_LAUNCH(0);
    else if (stage == 0) SUS_LAUNCH(1);
    else SUS_LAUNCH(2);
#undef SUS_LAUNCH
    VGPT_CHECK_LAUNCH("vgpt_sampler_update_sched");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sampler_update_sde(float* z, void* z_model, const void* pred, const float* sigma,
                                        const float* cfg_table, const float* eta_table, const int64_t* rng,
                                        const int32_t* step, int n_steps, int n_frames, int64_t elems, int pred_type,
                                        int use_cfg, float cfg_scale, int share_halves, void* stream) {
    VGPT_REQUIRE(z && z_model && pred && sigma && eta_table && rng && step, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sde: null pointer (z %p, z_model %p, pred %p, sigma %p, eta_table %p, rng %p, step %p)",
                 (void*)z, z_model, pred, (const void*)sigma, (const void*)eta_table, (const void*)rng, (const void*)step);
    VGPT_REQUIRE(n_steps > 0, VGPT_ERR_INVALID, "vgpt_sampler_update_sde: n_steps %d <= 0", n_steps);
    VGPT_REQUIRE(n_frames >= 0 && elems >= 0, VGPT_ERR_INVALID, "vgpt_sampler_update_sde: bad shape (%d frames of %lld)",
                 n_frames, (long long)elems);
    VGPT_REQUIRE(pred_type == VGPT_PRED_V || pred_type == VGPT_PRED_X1, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sde: unknown prediction type %d", pred_type);
    VGPT_REQUIRE(!cfg_table || use_cfg, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sde: cfg_table %p with use_cfg %d (a guidance table is CFG by definition)",
                 (const void*)cfg_table, use_cfg);
    VGPT_REQUIRE(!(use_cfg || share_halves) || n_frames % 2 == 0, VGPT_ERR_INVALID,
                 "vgpt_sampler_update_sde: use_cfg %d / share_halves %d need an even number of frames (got %d)", use_cfg,
                 share_halves, n_frames);
    if (n_frames == 0 || elems == 0) return VGPT_OK;
    const int64_t total = (int64_t)(use_cfg || share_halves ? n_frames / 2 : n_frames) * elems;
    const int grid = (int)std::min<int64_t>(cdiv(cdiv(total, 4), 256), 2048);
    const bool vec = total % 4 == 0 && (uintptr_t)z % 16 == 0 && (uintptr_t)z_model % 8 == 0 && (uintptr_t)pred % 8 == 0;
#define SDE_LAUNCH(VEC)                                                                                              \
    hipLaunchKernelGGL(sde_update_kernel<VEC>, dim3(grid), dim3(256), 0, (hipStream_t)stream, z, (bf16*)z_model,     \
                       (const bf16*)pred, sigma, cfg_table, eta_table, rng, step, n_steps, n_frames, elems, pred_type, \
                       use_cfg ? 1 : 0, cfg_scale, share_halves ? 1 : 0)
    if (vec) SDE_LAUNCH(true);
    else SDE_LAUNCH(false);
#undef SDE_LAUNCH
    VGPT_CHECK_LAUNCH("vgpt_sampler_update_sde");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sampler_noise_fill(float* out, int64_t n, const int64_t* rng, int step_index, void* stream) {
    VGPT_REQUIRE(out && rng, VGPT_ERR_INVALID, "vgpt_sampler_noise_fill: null pointer (out %p, rng %p)", (void*)out,
                 (const void*)rng);
    VGPT_REQUIRE(n >= 0, VGPT_ERR_INVALID, "vgpt_sampler_noise_fill: n %lld < 0", (long long)n);
    if (n == 0) return VGPT_OK;
    const int grid = (int)std::min<int64_t>(cdiv(cdiv(n, 4), 256), 2048);
    hipLaunchKernelGGL(noise_fill_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, n, rng, step_index);
    VGPT_CHECK_LAUNCH("vgpt_sampler_noise_fill");
    return VGPT_OK;
}

// dst[l][0:slab] = src[*step][l][0:slab] for every layer l, in 16-byte units (the time-token rows of the current step)
__global__ __launch_bounds__(256) void copy_step_slab_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                             const int32_t* __restrict__ step, int n_steps, int64_t slab,
                                                             int64_t src_step_stride, int64_t src_layer_stride,
                                                             int64_t dst_layer_stride, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int s = min(max(*step, 0), n_steps - 1);
    const int64_t l = i / slab, o = i % slab;
    dst[l * dst_layer_stride + o] = src[s * src_step_stride + l * src_layer_stride + o];
}

VGPT_EXPORT int vgpt_sampler_copy_step_rows(const void* src, void* dst, const int32_t* step, int n_steps, int n_layers,
                                            int64_t slab_bytes, int64_t src_step_stride_bytes,
                                            int64_t src_layer_stride_bytes, int64_t dst_layer_stride_bytes, void* stream) {
    VGPT_REQUIRE(src && dst && step, VGPT_ERR_INVALID, "vgpt_sampler_copy_step_rows: null pointer");
    VGPT_REQUIRE(n_steps > 0 && n_layers >= 0 && slab_bytes >= 0, VGPT_ERR_INVALID, "vgpt_sampler_copy_step_rows: bad shape");
    VGPT_REQUIRE(((slab_bytes | src_step_stride_bytes | src_layer_stride_bytes | dst_layer_stride_bytes) & 15) == 0 &&
                     (((uintptr_t)src | (uintptr_t)dst) & 15) == 0,
                 VGPT_ERR_UNSUPPORTED, "vgpt_sampler_copy_step_rows: sizes, strides and pointers must be multiples of 16 bytes");
    const int64_t slab = slab_bytes / 16, total = slab * n_layers;
    if (total == 0) return VGPT_OK;
    hipLaunchKernelGGL(copy_step_slab_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint4*)src, (uint4*)dst, step, n_steps, slab, src_step_stride_bytes / 16,
                       src_layer_stride_bytes / 16, dst_layer_stride_bytes / 16, total);
    VGPT_CHECK_LAUNCH("vgpt_sampler_copy_step_rows");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_sampler_advance(int32_t* step, void* stream) {
    VGPT_REQUIRE(step, VGPT_ERR_INVALID, "vgpt_sampler_advance: null pointer");
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    VGPT_CHECK_LAUNCH("vgpt_sampler_advance");
    return VGPT_OK;
}

VGPT_EXPORT int vgpt_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
    VGPT_REQUIRE(src && dst, VGPT_ERR_INVALID, "vgpt_cast_f32_to_bf16: null pointer");
    VGPT_REQUIRE(n >= 0, VGPT_ERR_INVALID, "vgpt_cast_f32_to_bf16: bad shape");
    if (n == 0) return VGPT_OK;
    int grid = (int)std::min<int64_t>(cdiv(n, 256), 2048);
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src,
                       (bf16*)dst, n);
    VGPT_CHECK_LAUNCH("vgpt_cast_f32_to_bf16");
    return VGPT_OK;
}
