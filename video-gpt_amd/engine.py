"""StaticDenoiser: one next-clip denoise step as a fixed, allocation-free launch sequence, and the
Euler sampling loop over it replayed from a hipGraph.

This is the execution plan behind `LVMScheduler.__call__` when it drives
`LVM.frame_block_forward_with_cfg` (LVM/scheduler.py:161-208 calling LVM/model.py:519-566 once per
step with `past_key_values=None`).  All buffers are allocated once per clip; a step is
  set_timesteps -> sequence assembly (embedding gather, condition patch-embed, time tokens,
  noisy patch-embed) -> 32 x [rmsnorm, qkv GEMM, RoPE, block-masked attention, o_proj GEMM +
  residual, rmsnorm, gate_up GEMM + act*up, down GEMM + residual] -> final norm -> t_embedder /
  adaLN -> final layer + unpatchify -> Euler / x1->v / CFG update -> step counter += 1,
every launch reading the step index and sigma table from device memory, so the captured graph is
identical for every step.
"""
from __future__ import annotations

import os
import weakref
from types import SimpleNamespace
from typing import Optional

import torch

from . import ops
from .layout import TokenLayout
from .ops import BF16, VgptError
from .step_plan import (_hoist_plan, _rows, clip_pass_rows, conditional_live_rows, count_left_pads,  # noqa: F401 (re-exported)
                        pack_left_padded, plan_step_rows, sp_final_layer_owners, sp_shares)


_FOLDED = weakref.WeakKeyDictionary()   # model -> (key, qkv weights, gate_up weights) with the RMSNorm gains folded in


def weight_generation(model) -> int:
    """Counter of the writes to `model`'s parameters that autograd's version counters do not see (bump_weight_generation)."""
    return model.__dict__.get("_vgpt_weight_generation", 0)


def bump_weight_generation(model) -> None:
    """Called by every writer of `model`'s parameters that bypasses autograd-visible ops -- kernels writing through raw
    pointers (Stage1Trainer's AdamW), parameters re-pointed at new storage, checkpoint loads -- so that copies derived from
    the parameters (folded_weights) are refilled before the next sampler call reads them."""
    model.__dict__["_vgpt_weight_generation"] = weight_generation(model) + 1


def folded_weights(model):
    """Per decoder layer: qkv_proj.weight * input_layernorm.weight and gate_up_proj.weight * post_attention_layernorm.weight
    (per input column, rounded to bf16 once: ops.fold_norm_gain) for the per-step forward with folded RMSNorms.  Derived
    copies (5 GB at Phi-3-mini size), allocated once per model and kept at their addresses (a captured graph reads them);
    refilled in place whenever a parameter involved may have changed since: its storage or autograd version moved, or the
    model's weight generation did (writes autograd does not see).  Checking costs 128 pointer / counter reads at 32 layers."""
    layers = model.llm.layers
    ps = [p_ for l in layers for p_ in (l.self_attn.qkv_proj.weight, l.input_layernorm.weight, l.mlp.gate_up_proj.weight,
                                        l.post_attention_layernorm.weight)]
    key = (weight_generation(model), tuple((p_.data_ptr(), p_._version) for p_ in ps))
    hit = _FOLDED.get(model)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    shapes = [(tuple(l.self_attn.qkv_proj.weight.shape), tuple(l.mlp.gate_up_proj.weight.shape)) for l in layers]
    if hit is not None and [(tuple(a.shape), tuple(b.shape)) for a, b in zip(hit[1], hit[2])] == shapes:
        wq, wgu = hit[1], hit[2]
    else:
        wq = [torch.empty_like(l.self_attn.qkv_proj.weight) for l in layers]
        wgu = [torch.empty_like(l.mlp.gate_up_proj.weight) for l in layers]
    for l, a, b in zip(layers, wq, wgu):
        ops.fold_norm_gain(l.self_attn.qkv_proj.weight, l.input_layernorm.weight, out=a)
        ops.fold_norm_gain(l.mlp.gate_up_proj.weight, l.post_attention_layernorm.weight, out=b)
    _FOLDED[model] = (key, wq, wgu)
    return wq, wgu


class StaticDenoiser:
    _hoist_plan = staticmethod(_hoist_plan)   # its home before step_plan.py; callers of the old name keep working

    def __init__(self, model, input_ids, position_ids, attention_mask, input_img_latents, input_image_sizes,
                 denoise_image_sizes, time_emb_inx, n_frames: int, latent_hw, use_img_cfg: bool, img_cfg_scale: float,
                 prediction_type: str = "v", sigma: Optional[torch.Tensor] = None, pack_padding: bool = True,
                 reuse_condition_prefix: bool = False, hoist_special_rows: bool = True,
                 attention_precision: str = "bf16", fuse_norms: Optional[bool] = None, linear_precision: str = "bf16",
                 sequence_parallel: bool = False, sp_group=None, solver: str = "euler", guidance_scales=None,
                 skip_unguided_branch: Optional[bool] = None, eta_table=None):
        # solver: "euler" (default), "ab2" or "heun" (DESIGN.md section 5); an unknown name is refused, naming it, before
        # anything else is looked at
        # eta_table: None, or one eta in [0, 1] per step (scheduler.eta_table): stochastic Euler steps
        # whose noise key is set per clip with set_noise_seed() -- see _set_eta
        self.solver = ops.solver_id(solver)
        model._check_ready()
        # fuse_norms: the two RMSNorms of a decoder layer folded into the GEMMs around them in the per-step forward (ops:
        # linear_resid_ssq -> *_prenorm; include/vgpt.h).  None = on wherever the step's shapes allow it, VGPT_FUSE_NORMS=0
        # switches it off (same-box A/B); the per-clip passes and the generic model path keep the separate kernel.
        if attention_precision not in ("bf16", "fp8"):
            raise VgptError(f"StaticDenoiser: attention_precision must be 'bf16' or 'fp8' (got {attention_precision!r})")
        # "fp8": the per-step attention of the sampler runs on MX-fp8 operands (csrc/attn_fp8.hip; the cfg-5 option of
        # SURVEY.md §8d).  The per-clip passes (prefill, time rows) stay bf16.
        self.attn_fp8 = attention_precision == "fp8"
        if linear_precision not in ("bf16", "fp8"):
            raise VgptError(f"StaticDenoiser: linear_precision must be 'bf16' or 'fp8' (got {linear_precision!r})")
        # "fp8": the four projections of every decoder layer in the per-step forward run as MX-fp8 GEMMs (csrc/gemm_mx8.hip) on
        # activations quantised per step and weights quantised from the live parameters once per clip (per_clip_setup).  The
        # per-clip passes, embeddings, final norm and final layer stay bf16.
        self.lin_fp8 = linear_precision == "fp8"
        # sequence_parallel: under a sequence-parallel group of P > 1 ranks (sequence_parallel.py) every rank holds about 1/P
        # of the live rows and 1/P of the attention heads (Ulysses, LVM/model.py:457-474 + LVM/transform/sdpa_transform.py:
        # 94-159); see the block comment at _sp_plan.  Off, or with one rank: the replicated engine, unchanged.
        from . import sequence_parallel as SPM
        self.sp = None
        if sequence_parallel and SPM.sp_world(sp_group) > 1:
            for opt, val in (("attention_precision", attention_precision), ("linear_precision", linear_precision)):
                if val != "bf16":
                    raise VgptError(f"StaticDenoiser: {opt}={val!r} is not supported with sequence_parallel (the sharded "
                                    "engine runs the bf16 projections and attention only)")
            g = sp_group if sp_group is not None else SPM.get_sequence_parallel_group()
            self.sp = {"group": g, "P": SPM.sp_world(g), "r": SPM.sp_rank(g)}
        # query rows per work item of the per-step bf16 attention: 128 = the four-wave kernel, two workgroups per CU (product).
        # 256 = the eight-wave kernel (one K / V tile staged per 256 rows: half the LDS-DMA instructions per wave and half the
        # L2 -> LDS bytes per FLOP; head dim 96): bit-identical results, measured SLOWER in round 3 -- 159.5 / 160.4 us per
        # layer against 148.3 us at the cfg-2 live rows, same box (a barrier across eight waves per tile costs more than the
        # staging it saves) -- and kept behind VGPT_ATTN_ITEM_ROWS=256 for A/B runs.
        self.attn_item_rows = int(os.environ.get("VGPT_ATTN_ITEM_ROWS", "128"))
        self.model = model
        cfg = model.llm.config
        for opt, on in (("attention_precision", self.attn_fp8), ("linear_precision", self.lin_fp8)):
            if on and cfg.head_dim not in ops.FP8_HEAD_DIMS:   # refused here, before anything is allocated or launched
                raise VgptError(f"StaticDenoiser: {opt}='fp8' needs a head dim of {ops.FP8_HEAD_DIMS} (got head_dim "
                                f"{cfg.head_dim}): the MX-fp8 attention and the qkv + RoPE projection have kernels for those "
                                "widths only")
        self.cfg = cfg
        dev = input_ids.device
        self.dev = dev

        # ---- the row plan (step_plan.py): left pads dropped and the batch packed into one sequence, the step-invariant
        #      condition prefix found and, behind it, the special rows hoisted or an alignment gap inserted ----
        plan = plan_step_rows(input_ids, position_ids, attention_mask, input_image_sizes, denoise_image_sizes, time_emb_inx,
                              pack_padding=pack_padding, reuse_condition_prefix=reuse_condition_prefix,
                              hoist_special_rows=hoist_special_rows)
        B, L, S = plan.B, plan.L, plan.S
        self.B, self.L, self.H = B, L, cfg.hidden_size
        self.packed = plan.packed
        self.S = S              # static prefix length in the (padded) layout == first computed row, multiple of 128
        self.S0 = plan.S0       # rows the prefill computes (== S without hoisting: the alignment rows ride along)
        self.hoist = plan.hoist  # special-row hoisting: step_plan._hoist_plan's dict when active
        self.Ma = B * L - S     # rows computed per step
        self.seg_all, self.seg_live = plan.seg_all, plan.seg_live
        self.nf = n_frames
        self.h, self.w = latent_hw
        self.use_cfg = bool(use_img_cfg)
        self.cfg_scale = float(img_cfg_scale)
        if prediction_type not in ("v", "x1"):
            raise VgptError(f"unknown prediction_type {prediction_type!r}")
        self.pred_type = ops.PRED_X1 if prediction_type == "x1" else ops.PRED_V
        if self.use_cfg and n_frames % 2:
            raise VgptError("CFG needs an even number of latent frames")
        if len(plan.x_rows) != n_frames or len(plan.t_rows) != n_frames:
            raise AssertionError("denoise_image_sizes / time_emb_inx disagree with the number of latents")

        # static inputs
        self.input_ids = plan.input_ids.contiguous()
        self.pm = ops.as_packed_mask(plan.attention_mask, dev)
        self.layout = plan.attention_mask if isinstance(plan.attention_mask, TokenLayout) else None
        self.position_ids = plan.position_ids
        self.rope = model.llm.rope_tables(plan.position_ids)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.cond = None
        if input_img_latents is not None and len(input_img_latents) > 0:
            shapes = {tuple(t.shape[-2:]) for t in input_img_latents}
            if len(shapes) != 1:
                raise VgptError("StaticDenoiser needs condition frames of one resolution")
            self.cond = torch.cat([t.to(BF16) for t in input_img_latents], dim=0).contiguous()
            if len(plan.cond_rows) != self.cond.shape[0]:
                raise AssertionError("input_image_sizes and input_img_latents disagree")
            self.cond_rows = i32(plan.cond_rows)
        self.x_rows, self.t_rows = i32(plan.x_rows), i32(plan.t_rows)
        # ---- the live rows [S, B L): what a step computes, as views every step method reads (`_a`).  Without a reused
        #      prefix they ARE the whole sequence; this is the one place that tells the two cases apart ----
        if S:
            self.x_rows_a = i32([r - S for r in plan.x_rows])
            self.t_rows_a = None if self.hoist else i32([r - S for r in plan.t_rows])   # hoisted: no time row is live
            self.ids_a = self.input_ids[:, S:].contiguous()
            self.rope_a = (self.rope[0][S:].contiguous(), self.rope[1][S:].contiguous())
            self.seg_a = self.seg_live
        else:
            self.x_rows_a, self.t_rows_a, self.ids_a, self.rope_a = self.x_rows, self.t_rows, self.input_ids, self.rope
            self.seg_a = self.seg_all

        self.heads = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        self._alloc_state(sigma)
        self._alloc_workspaces()
        self._set_projection_mode(fuse_norms)
        self._alloc_step_buffers()
        self._set_guidance(guidance_scales, skip_unguided_branch, plan)
        self._set_eta(eta_table, solver)
        self._initial_passes()

    # ---- allocation, once per engine ------------------------------------------------------------------------------------
    def _alloc_state(self, sigma):
        """The sampler state: latents, prediction, velocity history, timesteps, step counter, sigma table."""
        nf, C = self.nf, self.model.in_channels
        e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=self.dev)
        self.z = e(nf, C * self.h * self.w, dt=torch.float32)
        self.z_model = e(nf, C, self.h, self.w)
        self.pred = e(nf, C, self.h, self.w)
        # ab2 / heun: the guided velocity of the step, one CFG half.  Never cleared between clips: step 0 writes it before
        # anything reads it (ab2 reads from step 1 on, the Heun corrector after its own predictor)
        self.v_hist = None if self.solver == ops.SOLVER_EULER else e(nf // (2 if self.use_cfg else 1), C * self.h * self.w,
                                                                     dt=torch.float32)
        self.ts = e(nf, dt=torch.float32)
        self.step = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.sigma = None
        if sigma is not None:
            self.sigma = sigma.to(self.dev, torch.float32).contiguous()
            self.num_steps = self.sigma.numel() - 1

    def _alloc_step_buffers(self):
        """The small buffers of a step around the decoder layers (time token, t_embedder, adaLN modulation), and the slots
        the per-clip passes and the capture fill."""
        nf, H = self.nf, self.H
        e = lambda *s: torch.empty(*s, dtype=BF16, device=self.dev)
        self.temb_sin = e(nf, 256)
        self.tt_h = e(nf, H)
        self.te_h = e(nf, H)
        self.temb = e(nf, H)
        self.mod = e(nf, 2 * H)
        self._drop_graphs()
        self.time_qkv = None   # hoisting: (steps, layers, n_frames, 3H) q/k/v rows of the time tokens of every step
        self.mod_all = None    # (steps, 1, n_frames, 2H) adaLN shift / scale of the final layer for every step (_mod_pass)
        self.steps_taken = 0

    def _drop_graphs(self):
        """Forget every captured step: `graph` (and Heun's Euler-shaped final step, `graph_last`), and under a guidance
        schedule that skips rows the same pair for the steps that run the conditional rows only."""
        self.graph = self.graph_last = self.graph_c = self.graph_c_last = None

    # ---- per-step guidance scale -----------------------------------------------------------------
    def _set_guidance(self, scales, skip, plan):
        """guidance_scales: None (one scale for the clip, `img_cfg_scale`: nothing here changes what is launched), or one
        image-CFG scale per step (scheduler.guidance_table).  The table lives at a stable device address and every update
        launch reads its entry by the device step counter (vgpt_sampler_update_sched); the host keeps unguided[i] =
        (scales[i] == 1.0).  In an unguided step the guided velocity is the conditional one, so with skipping such a step
        runs the conditional rows only (step_plan.conditional_live_rows): Mc rows of the sequence assembly, the decoder
        layers, the attention (its own segments and plan) and the final layer; the unconditional rows of hid / ctx / act /
        pred are neither read nor written.  skip_unguided_branch: None = skip where the layout gives such a range and the
        engine is not sharded; True = the same, refused otherwise; False = never (the kernel still takes v_c on the 1.0
        entries, so False and None differ only in which rows were computed)."""
        self.gtable, self.unguided, self.cr = None, None, None
        if scales is None:
            if skip:
                raise VgptError("StaticDenoiser: skip_unguided_branch=True without guidance_scales (no step is unguided)")
            return
        if not self.use_cfg:
            raise VgptError("StaticDenoiser: guidance_scales with use_img_cfg=False: there is nothing to schedule")
        t = torch.as_tensor(scales, dtype=torch.float32).reshape(-1).cpu()
        if self.sigma is not None and t.numel() != self.num_steps:
            raise VgptError(f"StaticDenoiser: guidance_scales holds {t.numel()} scales, the sigma table has "
                            f"{self.num_steps} steps")
        if not bool(torch.isfinite(t).all()):
            raise VgptError(f"StaticDenoiser: non-finite guidance scale in {t.tolist()}")
        self.gtable = t.to(self.dev).contiguous()
        self.unguided = [v == 1.0 for v in t.tolist()]
        if skip is False:
            return
        why = None
        cr = conditional_live_rows(plan, plan.attention_mask, self.nf)
        if self.sp is not None:
            why = "a sequence-parallel engine cuts its shares over all live rows"
        elif cr is None:
            why = ("the conditional sequence's live rows are no leading range of their own (an unpacked batch, a pre-packed "
                   "mask, or one sequence)")
        elif cr[2] * 2 != self.nf:
            why = f"the first packed sequence holds {cr[2]} of the {self.nf} latent frames, not the conditional half"
        if why is not None:
            if skip:
                raise VgptError(f"StaticDenoiser: skip_unguided_branch=True cannot be honoured: {why}")
            return
        a, e, ncf, seg = cr
        Mc = e - a
        nq, nk, hd = self.heads
        cut = lambda t_: t_[:, :Mc]                       # leading rows of a (1, rows, .) workspace: a contiguous view
        c = SimpleNamespace(Mc=Mc, nf=ncf, seg=seg, hid=cut(self.hid), nrm=cut(self.nrm), ctx=cut(self.ctx), act=cut(self.act),
                            rope=(self.rope_a[0][:Mc], self.rope_a[1][:Mc]), ids=self.ids_a[:, :Mc].contiguous(),
                            x_rows=self.x_rows_a[:ncf], t_rows=None if self.t_rows_a is None else self.t_rows_a[:ncf],
                            n_cond=sum(1 for r in plan.cond_rows if r < e), ws=None, mx=None,
                            # fp8 attention: the rows behind the range that share its last 32-key quantisation block
                            tail=(e, min(self.L, (e + 31) // 32 * 32)))
        if self.fuse is not None:
            # the folded RMSNorms at Mc rows, with a workspace of their own; where the GEMMs have no folded form at that
            # row count (norm_workspace_bytes is 0) the conditional-rows steps keep the separate RMSNorm kernels
            wa = ops.norm_workspace_bytes(Mc, self.H, nq * hd)
            wb = ops.norm_workspace_bytes(Mc, self.H, self.cfg.intermediate_size)
            if wa > 0 and wb > 0:
                c.ws = ops.norm_workspace(max(wa, wb), self.dev)
        if self.mx8 is not None:   # the row quantisers' records at Mc rows; the weights' records are the engine's
            c.mx = {k: ops.Mx8Tensor(Mc, v.K, self.dev) for k, v in self.mx8.items() if k.startswith("a_")}
        if not self.S:
            # one q/k/v buffer, every row rewritten by a full step before it is read.  A conditional-rows step that comes
            # first leaves the rest unwritten, and a key tile that straddles row Mc is loaded whole: masked keys must be
            # finite
            self.qkv.zero_()
        self.cr = c

    # ---- stochastic steps -------------------------------------------------------------------------
    def _set_eta(self, table, solver):
        """eta_table: None (the deterministic sampler: nothing here changes what is launched), or one eta in [0, 1] per step
        (scheduler.eta_table).  The table and the {seed, stream} pair live at stable device addresses; the update launch of
        every step -- eager or captured -- reads its eta by the device step counter and its noise key from `rng`, so one
        engine and its graphs serve every seed (set_noise_seed).  The noise is counter-based: a function of (seed, stream,
        step, element) that every rank of a sharded engine computes alike on its replicated state."""
        self.etable, self.rng = None, None
        if table is None:
            return
        t = torch.as_tensor(table, dtype=torch.float32).reshape(-1).cpu()
        if self.sigma is not None and t.numel() != self.num_steps:
            raise VgptError(f"StaticDenoiser: eta_table holds {t.numel()} entries, the sigma table has {self.num_steps} steps")
        bad = [(i, v) for i, v in enumerate(t.tolist()) if not 0.0 <= v <= 1.0]
        if bad:
            raise VgptError(f"StaticDenoiser: eta={bad[0][1]!r} at step {bad[0][0]} is outside [0, 1]")
        noisy = [(i, v) for i, v in enumerate(t.tolist()) if v != 0.0]
        if noisy and self.solver != ops.SOLVER_EULER:
            raise VgptError(f"StaticDenoiser: solver={solver!r} with eta={noisy[0][1]!r} at step {noisy[0][0]}: only "
                            "solver='euler' takes a non-zero eta")
        if self.solver != ops.SOLVER_EULER:
            return   # an all-zero table under ab2 / heun: their own updates, untouched
        self.etable = t.to(self.dev).contiguous()
        self.rng = torch.zeros(2, dtype=torch.int64, device=self.dev)

    def set_noise_seed(self, seed: int, stream: int = 0):
        """The noise key of the next clip: per clip, next to set_latents.  Writes the device buffer the update kernel reads;
        captured graphs are not touched."""
        if self.rng is None:
            raise VgptError("StaticDenoiser.set_noise_seed: this engine has no eta_table (nothing is stochastic)")
        self.rng.copy_(ops.noise_rng(seed, stream, "cpu"), non_blocking=False)
        return self

    def step_rows(self, index: int) -> int:
        """Live rows step `index` of the table computes: the conditional rows in an unguided step of an engine that skips,
        all of them otherwise."""
        return self.cr.Mc if self._cond(index) else self.Ma

    def _cond(self, index: int) -> bool:
        return self.cr is not None and 0 <= index < len(self.unguided) and self.unguided[index]

    def _alloc_workspaces(self):
        """Activations and q/k/v of the per-step forward: this rank's share of the live rows (sharded), the live rows behind
        a cached prefix with one full-length q/k/v buffer per layer, or every row with one q/k/v buffer."""
        cfg, dev, B, L, H, Ma = self.cfg, self.dev, self.B, self.L, self.H, self.Ma
        nq, nk, hd = self.heads
        I = cfg.intermediate_size
        e = lambda *s: torch.empty(*s, dtype=BF16, device=dev)
        if self.sp is not None:
            if B != 1:
                raise VgptError("StaticDenoiser: sequence_parallel needs one packed sequence (a batch of one, or left-padded "
                                "rows with pack_padding=True)")
            self._sp_plan()
        elif self.S:
            self.hid, self.nrm, self.ctx, self.act = e(1, Ma, H), e(1, Ma, H), e(1, Ma, nq * hd), e(1, Ma, I)
            self.qkv_full = torch.zeros(cfg.num_hidden_layers, L, (nq + 2 * nk) * hd, dtype=BF16, device=dev)
            if self.attn_fp8:
                # one fp8 workspace per layer (51 MB at cfg-2): prefill() quantises the step-invariant rows once, a step
                # only the rows from the first one it writes on (the time rows of a hoisted layout sit below S)
                self.fp8_ws = [ops.attention_fp8_workspace_hd(1, L, nq, nk, hd, dev) for _ in range(cfg.num_hidden_layers)]
                first = (self.S0 + self.hoist["nf"]) if self.hoist else self.S
                self.fp8_from = first // 64 * 64
        else:
            self.hid = e(B, L, H)
            self.nrm = e(B, L, H)
            self.qkv = e(B, L, (nq + 2 * nk) * hd)
            self.ctx = e(B, L, nq * hd)
            self.act = e(B, L, I)

    def _set_projection_mode(self, fuse_norms):
        """How the per-step forward runs a layer's projections: `mx8` (MX-fp8 records), `fuse` (both RMSNorms folded into
        the bf16 GEMMs around them), or neither (separate RMSNorm kernels)."""
        model, dev, H = self.model, self.dev, self.H
        nq, nk, hd = self.heads
        I = self.cfg.intermediate_size
        self.fuse = None
        if fuse_norms is None:
            fuse_norms = os.environ.get("VGPT_FUSE_NORMS", "1") != "0"
        self.mx8 = None
        if self.lin_fp8:
            # the fp8 step folds both RMSNorms itself (row quantiser -> rstd, gain in the quantised weight): no folded bf16
            # copies.  Records at stable addresses (a captured graph reads them), weights refilled by every per_clip_setup()
            Ms = self.Ma
            W3 = (nq + 2 * nk) * hd
            mk = lambda rows, K: ops.Mx8Tensor(rows, K, dev)
            self.mx8 = {"a_hid": mk(Ms, H), "a_ctx": mk(Ms, nq * hd), "a_act": mk(Ms, I),
                        "rstd": torch.empty(Ms, dtype=torch.float32, device=dev),
                        "w": [{"qkv": mk(W3, H), "o": mk(H, nq * hd), "gate_up": mk(2 * I, H), "down": mk(H, I)}
                              for _ in model.llm.layers]}
            self.quantize_weights()
        elif fuse_norms:
            Ms = self.sp["m"] if self.sp else self.Ma
            wa, wb = ops.norm_workspace_bytes(Ms, H, nq * hd), ops.norm_workspace_bytes(Ms, H, I)
            if wa > 0 and wb > 0:
                wq, wgu = folded_weights(model)
                # rstd_in / rstd_post: 1 / rms of the stream in front of a layer's input / post-attention norm
                self.fuse = {"rstd_in": torch.empty(Ms, dtype=torch.float32, device=dev),
                             "rstd_post": torch.empty(Ms, dtype=torch.float32, device=dev),
                             "ws": ops.norm_workspace(max(wa, wb), dev), "wq": wq, "wgu": wgu}

    def _initial_passes(self):
        """The per-clip passes of the first clip (per_clip_setup repeats them for the next one)."""
        if self.sigma is not None:
            self._mod_pass()
        if self.S:
            if self.hoist and self.sigma is not None:
                self._clip_pass()
            else:
                self.prefill()

    # ---- pieces every pass shares ---------------------------------------------------------------------------------------
    def _embed_cond(self, seq2d):
        """The condition frames' patch embeddings into their rows of seq2d (rows, H)."""
        m = self.model
        if self.cond is not None:
            ops.patch_embed(self.cond, m.input_x_embedder.proj.weight, m.input_x_embedder.proj.bias, m.pos_embed[0],
                            self.cond_rows, seq2d, m.pos_embed_max_size)

    def _embed_static(self, hid, n: int):
        """Rows [0, n) of hid (1, >= n, H), all inside the static prefix: token embeddings + the condition frames' patches."""
        ops.embed_gather(self.input_ids[:, :n].contiguous(), self.model.llm.embed_tokens.weight, out=hid[:, :n])
        self._embed_cond(hid.view(-1, self.H))

    def _sigma_mlp(self, emb, sin, outs, tail=None):
        """sigma_0 .. sigma_{T-1}, one row per step (every frame of a step carries the same t, LVM/scheduler.py:169), through
        the timestep embedder `emb`: sinusoid into `sin`, Linear + SiLU into outs[0], Linear into outs[1] and, with `tail`,
        SiLU + that Linear into outs[2].  Same small-M kernels as the per-step path, at most 32 rows per call."""
        T = self.num_steps
        ops.timestep_sinusoid(self.sigma[:T].contiguous(), emb.freqs(self.dev), out=sin)
        chain = [(emb.mlp[0], {"post_act": ops.ACT_SILU}), (emb.mlp[2], {})]
        if tail is not None:
            chain.append((tail, {"pre_act": ops.ACT_SILU}))
        for c in range(0, T, 32):
            src = sin
            for (lin, kw), dst in zip(chain, outs):
                ops.linear_small(src[c:c + 32], lin.weight, lin.bias, out=dst[c:c + 32], **kw)
                src = dst

    def _pass_workspaces(self, M: int):
        """Workspaces of a per-clip pass over M rows: `hid` for every row (the sequence assembly runs on all of them), nrm /
        ctx / act for the rows [a, b) its decoder layers run on -- all M, or this rank's share with the exchange buffers."""
        nq, _, hd = self.heads
        e = lambda *s_: torch.empty(*s_, dtype=BF16, device=self.dev)
        shares, (a, b) = None, (0, M)
        if self.sp is not None:
            shares, _ = sp_shares(M, self.sp["P"])
            a, b = shares[self.sp["r"]]
        ws = SimpleNamespace(shares=shares, a=a, b=b, hid=e(1, M, self.H), nrm=e(1, b - a, self.H), ctx=e(1, b - a, nq * hd),
                             act=e(1, b - a, self.cfg.intermediate_size))
        ws.bufs = self._sp_buffers(M, b - a) if self.sp is not None else None
        return ws

    def _layers(self, hid, nrm, ctx, act, rope, qkv_dst, attention, fz=None, mx=None):
        """The decoder layers over the residual rows `hid` (1, rows, H), in place -- all rows of a pass, or one rank's share:
        norm -> qkv + RoPE -> attention -> o_proj + residual -> norm -> gate_up + act * up -> down + residual.
        nrm / ctx / act: workspaces of the same rows; rope: their (cos, sin) rows.  qkv_dst(li): where layer li's q/k/v rows
        go; attention(li): everything between that GEMM and o_proj, leaving the rows' attention output in `ctx` -- direct on
        the fused buffer, or through the exchanges (_sp_attention).  Projection form: separate RMSNorm kernels on the live
        parameters (the per-clip passes, always); fz (self.fuse): both norms folded into the GEMMs around them; mx
        (self.mx8): the MX-fp8 projections, which fold the norms themselves."""
        layers = self.model.llm.layers
        nq, nk, hd = self.heads
        if fz is not None:
            # the statistics of the first norm: the embedded rows are no GEMM's output.  From here on every residual stream is
            # written by linear_resid_rstd, which leaves the next norm's 1 / rms behind
            ops.rms_rstd(hid, layers[0].input_layernorm.variance_epsilon, out=fz["rstd_in"])
        for li, layer in enumerate(layers):
            at, mlp, ln_in, ln_post = layer.self_attn, layer.mlp, layer.input_layernorm, layer.post_attention_layernorm
            if mx is not None:
                w = mx["w"][li]
                ops.mx8_quantize_rows(hid, mx["a_hid"], mx["rstd"], ln_in.variance_epsilon)
                ops.linear_mx8(mx["a_hid"], w["qkv"], qkv_dst(li), "rope", rstd=mx["rstd"], cos=rope[0], sin=rope[1],
                               n_rot_heads=nq + nk, head_dim=hd)
            elif fz is not None:
                ops.linear_qkv_rope_prenorm(hid, fz["wq"][li], rope[0], rope[1], fz["rstd_in"], nq, nk, hd, out=qkv_dst(li))
            else:
                ops.rmsnorm(hid, ln_in.weight, ln_in.variance_epsilon, out=nrm)
                ops.linear_qkv_rope(nrm, at.qkv_proj.weight, rope[0], rope[1], nq, nk, hd, out=qkv_dst(li))
            attention(li)
            if mx is not None:
                ops.mx8_quantize_rows(ctx, mx["a_ctx"])
                ops.linear_mx8(mx["a_ctx"], w["o"], hid, "resid", residual=hid)
                ops.mx8_quantize_rows(hid, mx["a_hid"], mx["rstd"], ln_post.variance_epsilon)
                ops.linear_mx8(mx["a_hid"], w["gate_up"], act, "gated", rstd=mx["rstd"], act=mlp.act)
                ops.mx8_quantize_rows(act, mx["a_act"])
                ops.linear_mx8(mx["a_act"], w["down"], hid, "resid", residual=hid)
            elif fz is not None:
                ops.linear_resid_rstd(ctx, at.o_proj.weight, hid, fz["rstd_post"], fz["ws"], ln_post.variance_epsilon, out=hid)
                ops.gated_mlp_act_prenorm(hid, fz["wgu"][li], fz["rstd_post"], mlp.act, out=act)
                # the statistic the NEXT layer's input norm reads (its eps; the last layer's goes unused: the final norm is a
                # separate kernel)
                nxt = layers[min(li + 1, len(layers) - 1)].input_layernorm.variance_epsilon
                ops.linear_resid_rstd(act, mlp.down_proj.weight, hid, fz["rstd_in"], fz["ws"], nxt, out=hid)
            else:
                ops.linear(ctx, at.o_proj.weight, residual=hid, out=hid)
                ops.rmsnorm(hid, ln_post.weight, ln_post.variance_epsilon, out=nrm)
                ops.gated_mlp_act(nrm, mlp.gate_up_proj.weight, mlp.act, out=act)
                ops.linear(act, mlp.down_proj.weight, residual=hid, out=hid)

    # ---- the per-clip passes --------------------------------------------------------------------------------------------
    def prefill(self):
        """One forward over the static prefix rows [0, S) ONLY -- they never see a later row (that is what makes them
        step-invariant), so nothing else is needed to produce them -- leaving every layer's (post-RoPE) q/k/v in
        qkv_full[l][:S].  Rows >= S of qkv_full are written by every step (zero until the first one: the buffer is
        zero-initialised so that masked keys are finite).  Sharded: the rows are cut into shares."""
        nq, nk, hd = self.heads
        # with hoisting the step-invariant `<|diffusion|>` rows (right behind the prefix) are computed here as well: they
        # see the prefix and each other, nothing else
        S = self.S0 + (self.hoist["nf"] if self.hoist else 0)
        ws = self._pass_workspaces(S)
        self._embed_static(ws.hid, S)
        seg = ((0, 0, S),)   # includes the pad rows S0..S: no visible key -> zeros, which keeps their K/V finite
        if self.sp is None:
            def attention(li):
                full = self.qkv_full[li].view(1, self.L, -1)
                if self.attn_fp8:   # the sampler steps read the prefix's K / V from the fp8 workspace of this layer
                    ops.attention_fp8_quantize_hd(full, self.fp8_ws[li], nq, nk, hd)
                ops.attention_qkv_range(full, self.pm, nq, nk, hd, 0, ws.ctx, segments=seg)
            qkv_dst = lambda li: self.qkv_full[li][:S]
        else:
            qkv_dst, attention = self._sp_attention(ws.bufs, ws.shares, lambda li: self.qkv_full[li], 0, self.pm, seg, ws.ctx)
        rope = tuple(t_[ws.a:ws.b].contiguous() for t_ in self.rope)
        self._layers(ws.hid[:, ws.a:ws.b], ws.nrm, ws.ctx, ws.act, rope, qkv_dst, attention)
        torch.cuda.current_stream().synchronize()

    def rebind(self, input_img_latents):
        """The NEXT clip on an engine built for an identical sequence (same ids, positions, mask, frame geometry, sigma table:
        the rounds of a rollout once the frame window is full): new condition latents in, everything that depends on them
        recomputed (the per-clip pass), every buffer, the attention plan and the captured graph kept.  Nothing else of the
        previous clip survives: the live rows of qkv_full and of the fp8 workspaces are rewritten by every step before they
        are read, the sampler state by set_latents()."""
        n_new = 0 if input_img_latents is None else len(input_img_latents)
        if (self.cond is None) != (n_new == 0):
            raise VgptError("StaticDenoiser.rebind: the clip has a different number of condition frames")
        if self.cond is not None:
            new = torch.cat([t.to(BF16) for t in input_img_latents], dim=0)
            if tuple(new.shape) != tuple(self.cond.shape):
                raise VgptError("StaticDenoiser.rebind: condition latents of another shape")
            self.cond.copy_(new)
        self.per_clip_setup()
        self.steps_taken = 0
        return self

    def per_clip_setup(self):
        """Everything a clip computes once instead of once per step: the MX-fp8 weights (linear_precision "fp8"), the
        condition prefix and the special rows of every step (one pass, _clip_pass; prefill() alone when the layout cannot be
        hoisted), the final layer's adaLN modulation of every step.  Weights derived from the parameters (the MX-fp8 records,
        the gain-folded bf16 copies) are brought up to date with the live parameters first."""
        self.quantize_weights()
        self.refold_weights()
        if self.S:
            if self.hoist:
                self._clip_pass()
            else:
                self.prefill()
        self._mod_pass()

    def refold_weights(self):
        """Folded RMSNorms: the gain-folded qkv / gate_up copies refilled in place if a parameter they come from may have
        changed since they were folded (folded_weights); nothing to do otherwise."""
        if self.fuse is None:
            return
        wq, wgu = folded_weights(self.model)
        if wq is not self.fuse["wq"] or wgu is not self.fuse["wgu"]:   # re-allocated (other shapes): the graph read the old ones
            self.fuse["wq"], self.fuse["wgu"] = wq, wgu
            self._drop_graphs()

    def quantize_weights(self):
        """linear_precision "fp8": every decoder layer's qkv / o / gate_up / down weights into their MX-fp8 records, from the
        LIVE parameters (and, for qkv and gate_up, the live RMSNorm gains folded in), so a sampler call never runs weights older
        than the call.  No-op otherwise."""
        if self.mx8 is None:
            return
        for layer, w in zip(self.model.llm.layers, self.mx8["w"]):
            at, mlp = layer.self_attn, layer.mlp
            ops.mx8_quantize_weight(at.qkv_proj.weight, layer.input_layernorm.weight, out=w["qkv"])
            ops.mx8_quantize_weight(at.o_proj.weight, out=w["o"])
            ops.mx8_quantize_weight(mlp.gate_up_proj.weight, layer.post_attention_layernorm.weight, out=w["gate_up"])
            ops.mx8_quantize_weight(mlp.down_proj.weight, out=w["down"])

    def set_sigma(self, sigma: torch.Tensor):
        """A new sigma table on a built engine: everything that depends on the step index alone is recomputed."""
        if self.gtable is not None and sigma.numel() - 1 != self.gtable.numel():
            raise VgptError(f"StaticDenoiser.set_sigma: a sigma table of {sigma.numel() - 1} steps on an engine whose "
                            f"guidance table holds {self.gtable.numel()} scales")
        self.sigma = sigma.to(self.dev, torch.float32).contiguous()
        self.num_steps = self.sigma.numel() - 1
        self._mod_pass()
        if self.hoist:
            self._clip_pass()

    def _mod_pass(self):
        """t_embedder MLP + adaLN modulation of the final layer for EVERY step in one pass per clip: they depend on
        sigma_i alone (every frame of a step carries the same t, LVM/scheduler.py:169), while the reference recomputes
        them inside every model call (LVM/model.py:480-486).  A step then copies its row (step index read on the device)."""
        m, H, T = self.model, self.H, self.num_steps
        e = lambda *s_: torch.empty(*s_, dtype=BF16, device=self.dev)
        sin, te_h, temb, mod = e(T, 256), e(T, H), e(T, H), e(T, 2 * H)
        self._sigma_mlp(m.t_embedder, sin, (te_h, temb, mod), tail=m.final_layer.adaLN_modulation[1])
        shape = (T, 1, self.nf, 2 * H)
        if self.mod_all is None or tuple(self.mod_all.shape) != shape:
            self.mod_all = e(*shape)          # a captured graph reads this buffer: re-allocating invalidates it
            self._drop_graphs()
        self.mod_all.copy_(mod.view(T, 1, 1, 2 * H).expand(*shape))

    # ---- special-row hoisting ------------------------------------------------------------------------------------
    def _clip_layout(self):
        """Mask and row counts of the per-clip pass of a hoisted layout (_clip_pass): pm, Sc (the rows the sampler steps read
        from the cache: prefix + `<|diffusion|>` rows), Lp (all rows of the pass).  The time rows of step s carry sub-group
        s + 1 (layout.TokenLayout): they see the prefix, their clip's `<|diffusion|>` columns (sub-group 0) and the time
        columns of their own step only."""
        nf, T = self.hoist["nf"], self.num_steps
        Sc = self.S0 + nf
        idx, sub_tail = clip_pass_rows(self.S0, nf, T)
        lp = self.layout.permute(idx)
        sub = lp.sub.copy()
        sub[0, Sc:] = sub_tail
        return lp.with_subgroups(sub).packed_mask(self.dev), Sc, Sc + T * nf

    def _clip_pass(self):
        """Everything of a hoisted clip that does not depend on the latents, in ONE forward per clip: the condition prefix
        and the `<|diffusion|>` rows (step-invariant; what prefill() computes) and the time rows of EVERY denoise step (a
        function of the step index alone).  The reference recomputes all of them inside every model call
        (LVM/model.py:435-454, LVM/scheduler.py:174).  Sequence of the pass:
            [prefix 0..S0) | nf `<|diffusion|>` rows | step 0's nf time rows | step 1's | ... | step T-1's]
        with the clip's own token attributes (_clip_layout).  One sequence means every layer's weights stream once per clip
        and the GEMMs run S0 + nf + T nf rows (1.9 k at cfg-2 with 53 steps) instead of two passes of about half that.
        Leaves qkv_full[l][:S0 + nf] (post-RoPE q/k/v of the cached rows) and time_qkv[step, l]; sharded, the pass's rows
        are cut into shares and every rank keeps both for its own heads."""
        m, H = self.model, self.H
        nq, nk, hd = self.heads
        nf, T = self.hoist["nf"], self.num_steps
        pm, Sc, Lp = self._clip_layout()
        W = self.qkv_full.shape[-1]                        # q/k/v of all heads, or of this rank's
        e = lambda *s_: torch.empty(*s_, dtype=BF16, device=self.dev)
        ws = self._pass_workspaces(Lp)
        self._embed_static(ws.hid, Sc)                     # rows [0, Sc) as prefill()
        # time_token(sigma_s): one value per step, broadcast to the step's rows
        sin, tt_h, tt_o = e(T, 256), e(T, H), e(T, H)
        self._sigma_mlp(m.time_token, sin, (tt_h, tt_o))
        ws.hid[0, Sc:].view(T, nf, H)[:] = tt_o[:, None, :]
        # cos / sin are ROWS OF THE CLIP'S OWN TABLE (self.rope, built from the full position_ids): a su / longrope
        # checkpoint picks short or long factors from the largest position of the WHOLE sequence (HF 4.47.1
        # Phi3LongRoPEScaledRotaryEmbedding), which a table rebuilt from this pass's rows alone would get wrong whenever
        # only the image rows cross original_max_position_embeddings
        rope = tuple(torch.cat([t_[:Sc], t_[Sc:Sc + nf].repeat(T, 1)])[ws.a:ws.b].contiguous() for t_ in self.rope)
        buf = e(Lp, W)                                     # the pass's fused q/k/v rows, one layer at a time
        shape = (T, self.cfg.num_hidden_layers, nf, W)
        if self.time_qkv is None or tuple(self.time_qkv.shape) != shape:
            self.time_qkv = e(*shape)      # a captured graph reads this buffer: re-allocating invalidates it
            self._drop_graphs()
        seg = ((0, 0, Lp),)

        def keep(li):
            self.qkv_full[li][:Sc].copy_(buf[:Sc])
            self.time_qkv[:, li].copy_(buf[Sc:].view(T, nf, W))
        if self.sp is None:
            def attention(li):
                keep(li)
                if self.attn_fp8:   # the sampler steps read the cached rows' K / V from the fp8 workspace of this layer
                    ops.attention_fp8_quantize_hd(self.qkv_full[li].view(1, self.L, -1), self.fp8_ws[li], nq, nk, hd)
                ops.attention_qkv_range(buf.view(1, Lp, W), pm, nq, nk, hd, 0, ws.ctx, segments=seg)
            qkv_dst = lambda li: buf
        else:   # buf collects the rows of every rank for this rank's heads
            qkv_dst, attention = self._sp_attention(ws.bufs, ws.shares, lambda li: buf, 0, pm, seg, ws.ctx, keep=keep)
        self._layers(ws.hid[:, ws.a:ws.b], ws.nrm, ws.ctx, ws.act, rope, qkv_dst, attention)
        self.time_dst = self.qkv_full[:, Sc:Sc + nf]    # (layers, nf, 3H) view the step copy writes
        torch.cuda.current_stream().synchronize()

    # ---- Ulysses sequence parallelism (sequence_parallel=True under a group of P > 1 ranks) ---------------------------
    # Every pass (a step, prefill, the per-clip pass) cuts its live rows into P contiguous shares (sp_shares); rank r runs
    # the row-local work of its share -- RMSNorm (or the folded form), qkv_proj + RoPE, o_proj + residual, gate_up + act*up,
    # down + residual: _layers on the share -- and the attention of its nq/P query heads (nk/P K/V heads) over ALL rows
    # (_sp_attention).  Per layer:
    #   qkv rows of the share -> sp_pack_qkv -> one all-to-all -> rows of every rank for my heads, straight into the
    #   layer's fused buffer of width (nq/P + 2 nk/P) hd behind the cached rows -> attention -> ctx rows cut by owner ->
    #   second all-to-all -> sp_unpack_ctx -> (share, nq hd) in head order, the operand o_proj reads at P = 1.
    # The sequence assembly (embeddings, time tokens, patch embeddings) is cheap and runs on all live rows on every rank;
    # the share is a view of it.  After the final norm each rank runs the final layer on the frames it owns rows of and
    # one all-gather of the predictions (owner-selected per element) leaves the full `pred` on every rank: the
    # Euler / x1->v / CFG update runs replicated, so z stays bit-identical on all ranks.

    def _sp_plan(self):
        """Buffers of the sharded per-step forward (B == 1)."""
        cfg, H, dev, sp = self.cfg, self.H, self.dev, self.sp
        P, r = sp["P"], sp["r"]
        nq, nk, hd = self.heads
        if nq % P or nk % P:
            raise VgptError(f"StaticDenoiser: sequence_parallel over {P} ranks needs num_attention_heads ({nq}) and "
                            f"num_key_value_heads ({nk}) divisible by {P}")
        S, L = self.S, self.L
        Ml = self.Ma                                          # live rows of a step
        shares, cut = sp_shares(Ml, P)
        a, b = shares[r]
        m = b - a
        Wl = (nq // P + 2 * nk // P) * hd
        e = lambda *s_, dt=BF16: torch.empty(*s_, dtype=dt, device=dev)
        sp.update(shares=shares, cut=cut, a=a, b=b, m=m, Wl=Wl)
        self.hid_all = e(1, Ml, H)                            # sequence assembly of every live row
        self.hid = self.hid_all[:, a:b]                       # this rank's share (a contiguous view)
        self.nrm, self.ctx, self.act = e(1, m, H), e(1, m, nq * hd), e(1, m, cfg.intermediate_size)
        self.nrm_all = torch.zeros(1, Ml, H, dtype=BF16, device=dev)   # final norm: own rows written, the rest stays finite
        # one fused buffer per layer behind a cached prefix (its rows are the layer's); without one every row is rewritten
        # by every layer before it is read, so one buffer serves all layers
        self.qkv_full = torch.zeros(cfg.num_hidden_layers if S else 1, L, Wl, dtype=BF16, device=dev)
        self.sp_bufs = self._sp_buffers(Ml, m)
        # the final layer: frames with a row in this share, and for every element of pred the rank that computed it
        self.sp_frames, owner = sp_final_layer_owners(self.x_rows_a.tolist(), self.h, self.w, shares, r)
        C = self.pred.shape[1]
        self.sp_owner = owner[:, None].expand(-1, C, -1, -1).reshape(1, -1).to(dev)
        self.pred_loc = torch.zeros_like(self.pred)

    def _sp_buffers(self, Mtot: int, m: int):
        """Exchange buffers of a sharded pass over Mtot rows of which this rank runs m."""
        nq, nk, hd = self.heads
        P = self.sp["P"]
        e = lambda *s_: torch.empty(*s_, dtype=BF16, device=self.dev)
        return {"qkv": e(m, (nq + 2 * nk) * hd), "send": e(P, m, self.sp["Wl"]), "ctx_all": e(Mtot, nq // P * hd),
                "ctx_recv": e(P, m, nq // P * hd)}

    def _sp_attention(self, bufs, shares, full_of, q0: int, pm, segments, ctx_out, item_rows=None, keep=None):
        """(qkv_dst, attention) of a sharded pass for _layers: the share's q/k/v rows go to bufs["qkv"], and attention runs
        through the two exchanges.  full_of(li): the layer's (rows, Wl) fused buffer of this rank's heads; the live rows of
        every rank land at [q0, q0 + sum(shares)) in rank order.  keep(li): called once attention has run on them."""
        from . import sequence_parallel as SPM
        P, g, Wl = self.sp["P"], self.sp["group"], self.sp["Wl"]
        nq, nk, hd = self.heads
        sizes = [e_ - a_ for a_, e_ in shares]
        Mtot, dc = sum(sizes), nq // P * hd
        kw = {} if item_rows is None else {"item_rows": item_rows}

        def attention(li):
            full = full_of(li)
            ops.sp_pack_qkv(bufs["qkv"], P, nq, nk, hd, out=bufs["send"])
            SPM.exchange_split(bufs["send"], full[q0:q0 + Mtot], [[n * Wl] * P for n in sizes], g)
            ops.attention_qkv_range(full.view(1, full.shape[0], Wl), pm, nq // P, nk // P, hd, q0, bufs["ctx_all"],
                                    segments=segments, **kw)
            SPM.exchange_split(bufs["ctx_all"], bufs["ctx_recv"], [[n * dc for n in sizes] for _ in range(P)], g)
            ops.sp_unpack_ctx(bufs["ctx_recv"], P, out=ctx_out.view(-1, nq * hd))
            if keep is not None:
                keep(li)
        return (lambda li: bufs["qkv"]), attention

    def set_latents(self, z: torch.Tensor):
        """z: (n_frames, C, h, w) any float dtype; becomes the fp32 sampler state."""
        self.z.copy_(z.reshape(self.nf, -1).to(torch.float32))
        ops.cast_f32_to_bf16(self.z, self.z_model)
        self.step.zero_()
        self.steps_taken = 0

    # ---- one denoise forward: z_model, ts -> pred ----
    def _step_head(self, from_tables: bool, c=None):
        """Sequence assembly of the live rows (all of them, on every rank): token embeddings, condition patches, time tokens
        (or, hoisted, the time rows' q/k/v of this step dropped into qkv_full), noisy patches.  c (self.cr): the conditional
        rows and frames only."""
        m, H, S = self.model, self.H, self.S
        hid = self.hid if self.sp is None else self.hid_all
        seq2d = hid.view(-1, H)
        if c is not None:
            if not self.hoist:
                ops.embed_gather(c.ids, m.llm.embed_tokens.weight, out=c.hid)
            if not S and c.n_cond:
                ops.patch_embed(self.cond[:c.n_cond], m.input_x_embedder.proj.weight, m.input_x_embedder.proj.bias,
                                m.pos_embed[0], self.cond_rows[:c.n_cond], seq2d, m.pos_embed_max_size)
            if not (from_tables and self.hoist):
                ops.timestep_sinusoid(self.ts, m.time_token.freqs(self.dev), out=self.temb_sin)
            if self.hoist:   # (the time rows sit below S, cached rows: every frame's are dropped in, as in a full step)
                if self.time_qkv is None:
                    raise VgptError("StaticDenoiser: set_sigma() must run before the first step")
                ops.sampler_copy_step_rows(self.time_qkv, self.time_dst, self.step)
            else:
                tt = m.time_token.mlp
                ops.linear_small(self.temb_sin[:c.nf], tt[0].weight, tt[0].bias, post_act=ops.ACT_SILU, out=self.tt_h[:c.nf])
                ops.linear_small(self.tt_h[:c.nf], tt[2].weight, tt[2].bias, out=seq2d, out_row=c.t_rows, ldo=H)
            ops.patch_embed(self.z_model[:c.nf], m.x_embedder.proj.weight, m.x_embedder.proj.bias, m.pos_embed[0], c.x_rows,
                            seq2d, m.pos_embed_max_size)
            return
        if not self.hoist:   # a hoisted step's live rows are image rows only: the patch embedding below writes every one
            ops.embed_gather(self.ids_a, m.llm.embed_tokens.weight, out=hid)
        if not S:
            self._embed_cond(seq2d)
        if not (from_tables and self.hoist):
            ops.timestep_sinusoid(self.ts, m.time_token.freqs(self.dev), out=self.temb_sin)
        if self.hoist:
            if self.time_qkv is None:
                raise VgptError("StaticDenoiser: set_sigma() must run before the first step")
            ops.sampler_copy_step_rows(self.time_qkv, self.time_dst, self.step)
        else:
            tt = m.time_token.mlp
            ops.linear_small(self.temb_sin, tt[0].weight, tt[0].bias, post_act=ops.ACT_SILU, out=self.tt_h)
            ops.linear_small(self.tt_h, tt[2].weight, tt[2].bias, out=seq2d, out_row=self.t_rows_a, ldo=H)
        ops.patch_embed(self.z_model, m.x_embedder.proj.weight, m.x_embedder.proj.bias, m.pos_embed[0], self.x_rows_a, seq2d,
                        m.pos_embed_max_size)

    def _step_tail(self, from_tables: bool, c=None):
        """Final norm, the final layer's adaLN modulation (from the per-clip table, or the small MLPs on self.ts), final layer
        + unpatchify into `pred`.  Sharded: each rank runs the final layer on the frames it owns rows of, and one all-gather
        (owner-selected per element) leaves the full `pred` on every rank.  c (self.cr): the conditional rows and frames
        only; the unconditional half of `pred` keeps what it held."""
        m, H, sp = self.model, self.H, self.sp
        hid = self.hid
        if c is not None:
            (f0, f1), nrm_all, nrm, pred, hid = (0, c.nf), c.nrm, c.nrm, self.pred, c.hid
        elif sp is None:
            (f0, f1), nrm_all, nrm, pred = (0, self.nf), self.nrm, self.nrm, self.pred
        else:
            (f0, f1), nrm_all, nrm, pred = self.sp_frames, self.nrm_all, self.nrm_all[:, sp["a"]:sp["b"]], self.pred_loc
        ops.rmsnorm(hid, m.llm.norm.weight, m.llm.norm.variance_epsilon, out=nrm)
        # t_embedder + adaLN modulation: every frame of a step carries the same t (LVM/scheduler.py:169), so one row is
        # computed and broadcast (the small-M kernel re-reads its input rows for every output column)
        if from_tables:
            ops.sampler_copy_step_rows(self.mod_all, self.mod.view(1, self.nf, 2 * H), self.step)
        else:
            te = m.t_embedder.mlp
            ops.linear_small(self.temb_sin[:1], te[0].weight, te[0].bias, post_act=ops.ACT_SILU, out=self.te_h[:1])
            ops.linear_small(self.te_h[:1], te[2].weight, te[2].bias, out=self.temb[:1])
            ada = m.final_layer.adaLN_modulation[1]
            ops.linear_small(self.temb[:1], ada.weight, ada.bias, pre_act=ops.ACT_SILU, out=self.mod[:1])
            if self.nf > 1:
                self.mod[1:].copy_(self.mod[:1].expand(self.nf - 1, -1))
        if f1 > f0:
            ops.final_layer(nrm_all.view(-1, H), self.x_rows_a[f0:f1], self.mod[f0:f1], m.final_layer.linear.weight,
                            m.final_layer.linear.bias, pred[f0:f1])
        if sp is not None:
            from . import sequence_parallel as SPM
            every = SPM.all_gather_flat(self.pred_loc, sp["group"])          # (P, elements of pred)
            torch.gather(every, 0, self.sp_owner, out=self.pred.view(1, -1))

    def forward_step(self, from_tables: bool = False, cond: bool = False):
        """from_tables: the step is sigma[*step] of the table (sampler_step), so everything that depends on the step
        alone comes from the per-clip passes; otherwise `self.ts` may hold any timesteps.  cond: the conditional rows only
        (self.cr; an unguided step of a guidance schedule) -- the same launches on the leading Mc live rows, the first
        sequence's attention segment, the first half of the frames."""
        from_tables = from_tables and self.mod_all is not None
        c = self.cr if cond else None
        if cond and c is None:
            raise VgptError("StaticDenoiser.forward_step: cond=True on an engine that does not skip the unconditional rows")
        self._step_head(from_tables, c)
        nq, nk, hd = self.heads
        S, pm, ctx, rows, seg, rope = self.S, self.pm, self.ctx, self.attn_item_rows, self.seg_a, self.rope_a
        hid, nrm, act, fz, mx, n_live = self.hid, self.nrm, self.act, self.fuse, self.mx8, None
        if c is not None:
            # ctx stays the full buffer for the attention launches (they address it by absolute row and write the rows of
            # `seg` only); the projections read its leading rows
            hid, nrm, act, seg, rope, n_live = c.hid, c.nrm, c.act, c.seg, c.rope, c.Mc
            if fz is not None:
                fz = None if c.ws is None else {**fz, "rstd_in": fz["rstd_in"][:c.Mc], "rstd_post": fz["rstd_post"][:c.Mc],
                                                "ws": c.ws}
            if mx is not None:
                mx = {**mx, **c.mx, "rstd": mx["rstd"][:c.Mc]}
        if self.sp is not None:
            rope = tuple(t_[self.sp["a"]:self.sp["b"]] for t_ in rope)
            # (one fused buffer serves every layer when no prefix is cached: _sp_plan)
            qkv_dst, attention = self._sp_attention(self.sp_bufs, self.sp["shares"],
                                                    lambda li: self.qkv_full[li % len(self.qkv_full)], S, pm, seg, ctx,
                                                    item_rows=rows)
        elif S:
            # this step's q/k/v rows, behind the cached prefix (n_live: the conditional rows only)
            qkv_dst = lambda li: self.qkv_full[li][S:] if n_live is None else self.qkv_full[li][S:S + n_live]

            def attention(li):
                full = self.qkv_full[li].view(1, self.L, -1)
                if self.attn_fp8:
                    # the prefix rows were quantised once by prefill(); a step re-quantises from the first row it writes.
                    # A conditional-rows step (section 5b) leaves the unconditional rows of qkv_full as the last full step
                    # (or the zero fill) left them, and fp8_from on re-quantises those too: stale but finite values that
                    # no conditional row attends to (conditional_live_rows checked it).  They are harmless to the scores,
                    # but V takes one block scale per 32 keys and column: where the range does not end on a multiple of 32
                    # (the prefix-only and no-prefix layouts) its last keys share a scale with the rows behind it, so those
                    # rows of the straddling block are zeroed first and the step's result is a function of the conditional
                    # rows alone.  (A full step has the unconditional keys there instead: in such a layout skipping on and
                    # off agree within the fp8 tolerance, not bit for bit.)
                    if c is not None and c.tail[1] > c.tail[0]:
                        self.qkv_full[li][c.tail[0]:c.tail[1]].zero_()
                    ops.attention_qkv_fp8_hd(full, pm, nq, nk, hd, out=ctx, q_start=S, segments=seg,
                                          workspace=self.fp8_ws[li], quant_from=self.fp8_from)
                else:
                    ops.attention_qkv_range(full, pm, nq, nk, hd, S, ctx, segments=seg, item_rows=rows)
        else:
            qkv_dst = lambda li: self.qkv if n_live is None else self.qkv[:, :n_live]

            def attention(li):
                if self.attn_fp8:
                    if c is not None and c.tail[1] > c.tail[0]:   # as above: the straddling 32-key block of V
                        self.qkv[0, c.tail[0]:c.tail[1]].zero_()
                    ops.attention_qkv_fp8_hd(self.qkv, pm, nq, nk, hd, out=ctx, segments=seg)
                elif seg is not None:
                    ops.attention_qkv_range(self.qkv, pm, nq, nk, hd, 0, ctx, segments=seg, item_rows=rows)
                else:
                    ops.attention_qkv(self.qkv, pm, nq, nk, hd, out=ctx)
        self._layers(hid, nrm, ctx if c is None else c.ctx, act, rope, qkv_dst, attention, fz=fz, mx=mx)
        self._step_tail(from_tables, c)

    def sampler_step(self, last: bool = True, cond: bool = False):
        """LVM/scheduler.py:168-204 for one i: timesteps, model call, x1->v, CFG, update, i += 1.  Euler and ab2: one model
        call and one update kernel.  Heun (`last` False: not the final step of the table): model call, predictor, i += 1,
        model call at sigma[i+1] on bf16(z + h v), corrector -- the step tables are read by *step, so the second call reads
        index i + 1 <= N - 1; the final step (sigma[N] = 1) is the Euler-shaped one."""
        ops.sampler_set_timesteps(self.sigma, self.step, self.ts)
        self.forward_step(from_tables=True, cond=cond)
        if self.etable is not None:
            # stochastic steps (Euler only): one update kernel that reads the step's eta -- and, under a guidance schedule,
            # its scale -- by the step counter, and makes its noise from (seed, stream, step, element)
            ops.sampler_update_sde(self.z, self.z_model, self.pred, self.sigma, self.gtable, self.etable, self.rng, self.step,
                                   self.pred_type, self.use_cfg, self.cfg_scale, share_halves=self.use_cfg)
            ops.sampler_advance(self.step)
            return
        if self.gtable is not None:
            # a guidance schedule: the same steps with the update that reads the step's scale from the table.  cond: an
            # unguided step on the conditional rows only -- both model calls of a Heun step are of the step's kind
            sched = lambda stage: ops.sampler_update_sched(self.z, self.z_model, self.pred, self.v_hist, self.sigma,
                                                           self.gtable, self.step, self.pred_type, self.solver, stage)
            if self.solver == ops.SOLVER_HEUN and not last:
                sched(0)
                ops.sampler_advance(self.step)
                ops.sampler_set_timesteps(self.sigma, self.step, self.ts)
                self.forward_step(from_tables=True, cond=cond)
                sched(1)
                return
            sched(0)
            ops.sampler_advance(self.step)
            return
        upd = (self.z, self.z_model, self.pred, self.v_hist, self.sigma, self.step, self.pred_type, self.use_cfg,
               self.cfg_scale)
        if self.solver == ops.SOLVER_HEUN and not last:
            ops.sampler_update(*upd, ops.SOLVER_HEUN, 0)
            ops.sampler_advance(self.step)
            ops.sampler_set_timesteps(self.sigma, self.step, self.ts)
            self.forward_step(from_tables=True)
            ops.sampler_update(*upd, ops.SOLVER_HEUN, 1)
            return
        if self.solver == ops.SOLVER_AB2:
            ops.sampler_update(*upd, ops.SOLVER_AB2)
        else:
            ops.euler_cfg_update(self.z, self.z_model, self.pred, self.sigma, self.step, self.pred_type, self.use_cfg,
                                 self.cfg_scale)
        ops.sampler_advance(self.step)

    def _step_then_capture(self, restore: bool, last: bool = True, cond: bool = False):
        """One eager step (kernels set their launch attributes on first use, which a capture cannot record), then the capture
        of a step, which records without executing.  restore: the eager step leaves no trace in the sampler state (the
        velocity history included: an ab2 step in the middle of a clip reads what the step before it wrote).  Heun keeps two graphs: the
        two-call step (`graph`) and the Euler-shaped final step (`graph_last`); the other solvers have `graph` alone.  An
        engine that skips the unconditional rows keeps the same pair once more for its conditional-rows steps (`graph_c`,
        `graph_c_last`): one graph per (kind, Heun-last), each captured at the first step of its kind."""
        saved = (self.z.clone(), self.z_model.clone(), self.step.clone()) if restore else None
        hist = self.v_hist.clone() if restore and self.v_hist is not None else None
        self.sampler_step(last, cond)
        torch.cuda.current_stream().synchronize()
        if restore:
            self.z.copy_(saved[0]); self.z_model.copy_(saved[1]); self.step.copy_(saved[2])
            if hist is not None:
                self.v_hist.copy_(hist)
            torch.cuda.current_stream().synchronize()
        setattr(self, self._graph_slot(last, cond), ops.HipGraph().capture(lambda: self.sampler_step(last, cond)))

    def _graph_slot(self, last: bool, cond: bool) -> str:
        return ("graph_c" if cond else "graph") + ("_last" if self._two_graphs() and last else "")

    def _two_graphs(self) -> bool:
        return self.solver == ops.SOLVER_HEUN

    def _is_last(self, index: int) -> bool:
        """Whether step `index` of the table takes the Euler-shaped step: every step of the one-call solvers, Heun's final one."""
        return not self._two_graphs() or index == self.num_steps - 1

    def capture(self):
        """Capture one sampler step into a hipGraph (must run on a non-default stream)."""
        if self.sp is not None:
            raise VgptError("StaticDenoiser.capture: a sequence-parallel engine runs eagerly (its exchanges are not captured)")
        self._step_then_capture(restore=True, last=self._is_last(self.steps_taken), cond=self._cond(self.steps_taken))
        return self

    def run(self, num_steps: Optional[int] = None, use_graph: bool = True):
        n = self.num_steps if num_steps is None else num_steps
        if self.steps_taken + n > self.num_steps:
            raise VgptError(f"StaticDenoiser.run: {n} more steps after {self.steps_taken} exceed the {self.num_steps}-step "
                            "sigma table")
        first = self.steps_taken
        self.steps_taken += n
        use_graph = use_graph and self.sp is None   # sharded engines run eagerly: collectives are not captured (yet)
        for index in range(first, first + n):
            # by the absolute index: run(k) then run(N - k) is run(N), also across a boundary between step kinds
            last, cond = self._is_last(index), self._cond(index)
            if not use_graph:
                self.sampler_step(last, cond)
                continue
            graph = getattr(self, self._graph_slot(last, cond))
            if graph is None:
                self._step_then_capture(restore=False, last=last, cond=cond)   # the eager step counts as a real one
            else:
                graph.replay()
        return self.z
