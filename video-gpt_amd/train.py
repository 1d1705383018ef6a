"""Stage-1 pre-training step on the HIP path: forward with saved activations, per-frame MSE on x1,
explicit backward, gradient all-reduce (RCCL) overlapped with the backward, global-norm clipping and AdamW.

Mirrors the reference's hot loop (LVM/train/train_x1_stage1_noiseinput.py:351-405) and loss
(LVM/train_helper/loss.py:128-243, `training_losses_x1_noise_input`):
    xt = t*x1 + (1-t)*x0 per frame, clean inputs noised with t_in in [input_noise, 1]; pred = model(xt, t, ...);
    loss_i = mean((x1_i - pred_i)^2); loss.mean().backward(); clip_grad_norm_(1.0); AdamW(lr, weight_decay).step()
The reference delegates backward to torch.autograd, the gradient reduction to DeepSpeed ZeRO-2 and the
optimizer to DeepSpeed's bf16 AdamW (fp32 master weights).  Here:
  * every backward pass is a HIP kernel (ops_train.py); the big dX / dW products reuse the MFMA NT GEMM
    through padded transposes, attention has its own dQ / dKdV kernels;
  * data parallelism replicates the model (288 GB HBM holds params + fp32 master + Adam moments, ~60 GB
    at Phi-3-mini size) and all-reduces one flat bf16 gradient bucket per decoder layer (226 MB at full
    size) as soon as that layer's backward has produced it, on RCCL's stream, while the next layer's
    backward runs; the small fp32 gradients go in one last bucket.  dp_sharding="optimizer" (ZeRO stage 1
    on the reference's stage-2 exchange) reduce-scatters those buckets instead, keeps the fp32 master
    weights and moments of this rank's shard only and all-gathers the updated bf16 parameters;
  * clipping uses the norm of the averaged gradient; the 1/world factor and the clip coefficient are
    folded into the AdamW kernel's gradient scale (no separate pass over the gradients);
  * lora_rank=r (train_x1_stage1_noiseinput.py:204-223) freezes the base model and trains rank-r adapters on qkv_proj /
    o_proj through the three products of ops_lora.py: no dW GEMM, no base optimizer state, one small bucket to exchange
    (DESIGN.md §6a);
  * gradient_accumulation_steps=A keeps one fp32 accumulator per gradient bucket and adds every micro-step's bucket to it
    right where the bucket would be exchanged; the last micro-step writes the once-rounded sum back into the bucket and the
    exchange, clip and AdamW run on it unchanged, 1/A folded in where 1/world is.  use_ema=True keeps an fp32 EMA of the
    fp32 master weights, moved inside the AdamW launch (vgpt_adamw_ema_step); DESIGN.md §6b;
  * sequence_parallel=True under a group of P > 1 ranks (LVMTraining_CP, --sequence_parallel_size; LVM/model.py:1101-1107,
    LVM/transform/sdpa_transform.py:94-159, LVM/utils.py:148-174) shares the rows of ONE packed clip between the P ranks:
    the row-local work of forward and backward runs on this rank's share, attention and its backward on this rank's heads
    over all rows, with two exchanges per layer each way; every saved activation is 1/P of the unsharded step's and the
    gradient buckets hold partial sums over the share that the data-parallel exchange adds up.
"""
from __future__ import annotations

import math
import os
import weakref

from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import ops
from . import ops_lora as LO
from . import ops_train as T
from . import sequence_parallel as SPM
from .engine import _rows, bump_weight_generation, count_left_pads, pack_left_padded, sp_shares
from .ops import BF16, VgptError

F32 = torch.float32
DP_SHARDING_MODES = ("none", "optimizer")
LR_SCHEDULERS = ("constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial")
LR_END = 1e-7           # end LR of "polynomial" (get_scheduler passes none: the schedule's own default)
LORA_TARGETS = ("qkv_proj", "o_proj")
# gradients a sequence-parallel rank computes on replicated rows (the heads behind the gathered final norm): identical on
# every rank of the group, so they enter the data-parallel sum from SP rank 0 only
SP_REPLICATED = ("final_layer.", "t_embedder.", "input_final_layer.")


def lora_key(layer: int, module: str, ab: str) -> str:
    """peft's state-dict key of an adapter matrix of this model (get_peft_model_state_dict: adapter name stripped)."""
    return f"base_model.model.llm.layers.{layer}.self_attn.{module}.lora_{ab}.weight"
# dp_sharding="optimizer": every flat bucket is padded to a multiple of world * SHARD_GRANULE elements, so each rank's
# shard starts 512 (bf16) / 1024 (fp32) bytes apart: vgpt_adamw_step's alignment check and vgpt_sumsq's 16-byte loads
SHARD_GRANULE = 256


def shard_partition(n: int, world: int):
    """(padded length, shard length s) of a flat bucket of n elements sharded over `world` ranks: rank r owns
    [r * s, (r + 1) * s) of the zero-padded bucket.  The padded length is the smallest multiple of world * SHARD_GRANULE
    that holds n; at world 1 it is n itself (no padding)."""
    if world < 1 or n < 0:
        raise VgptError(f"shard_partition: bad bucket length {n} or world size {world}")
    if world == 1:
        return n, n
    g = world * SHARD_GRANULE
    padded = -(-n // g) * g
    return padded, padded // world


def lr_factor(name: str, k: int, warmup: int = 0, total: Optional[int] = None, num_cycles: Optional[float] = None,
              power: float = 1.0, base_lr: float = 1.0) -> float:
    """Multiplier of the base LR at scheduler step k (k = 0 for the first optimizer step): the lambdas diffusers'
    get_scheduler(name, num_warmup_steps=warmup, num_training_steps=total, num_cycles=..., power=...) hands LambdaLR
    (train_x1_stage1_noiseinput.py:279-283, 513-521), restated.  Every name but "constant" ramps k / max(1, warmup) while
    k < warmup.  Past it, with progress = (k - warmup) / max(1, total - warmup):
      linear                max(0, (total - k) / max(1, total - warmup))
      cosine                max(0, (1 + cos(2 pi num_cycles progress)) / 2), num_cycles 0.5 by default
      cosine_with_restarts  0 once progress >= 1, else max(0, (1 + cos(pi ((num_cycles progress) mod 1))) / 2), default 1
      polynomial            ((base_lr - LR_END) (1 - (k - warmup) / (total - warmup))^power + LR_END) / base_lr, and
                            LR_END / base_lr once k > total (the only schedule that needs base_lr)
    Pure Python in float64; no GPU, no torch."""
    if name not in LR_SCHEDULERS:
        raise VgptError(f"lr_scheduler {name!r}: built are {LR_SCHEDULERS}")
    k, warmup = int(k), int(warmup)
    if name == "constant":
        return 1.0
    if k < warmup:
        return float(k) / float(max(1, warmup))
    if name == "constant_with_warmup":
        return 1.0
    if total is None:
        raise VgptError(f"lr_scheduler {name!r} needs lr_num_training_steps")
    total = int(total)
    if name == "linear":
        return max(0.0, float(total - k) / float(max(1, total - warmup)))
    progress = float(k - warmup) / float(max(1, total - warmup))
    if name == "cosine":
        cycles = 0.5 if num_cycles is None else float(num_cycles)
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * cycles * 2.0 * progress)))
    if name == "cosine_with_restarts":
        cycles = 1.0 if num_cycles is None else float(num_cycles)
        if progress >= 1.0:
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((cycles * progress) % 1.0))))
    # polynomial
    if not base_lr > LR_END:
        raise VgptError(f"lr_scheduler 'polynomial': the base LR {base_lr} must exceed the end LR {LR_END}")
    if k > total:
        return LR_END / base_lr
    remaining = 1.0 - (k - warmup) / (total - warmup) if total > warmup else 0.0
    return ((base_lr - LR_END) * remaining ** power + LR_END) / base_lr


_TRAINER_OF = weakref.WeakKeyDictionary()   # model -> weakref to the trainer whose optimizer updates it on a stream of its own


def wait_for_pending_update(model) -> None:
    """Readers of `model`'s parameters outside Stage1Trainer.step() -- the sampler (validation clips through LVMPipeline),
    state_dict() -- call this: with `overlap_optimizer` the last AdamW update may still be running on the trainer's own stream,
    with dp_sharding="optimizer" the all-gathers of the updated parameters may still be in flight.
    Makes the CURRENT stream wait for them; nothing to do otherwise."""
    ref = _TRAINER_OF.get(model)
    tr = ref() if ref is not None else None
    if tr is not None:
        tr.finish_optimizer()


def _state_dict_barrier(module, prefix, keep_vars):
    wait_for_pending_update(module)


class Stage1Trainer:
    def __init__(self, model, lr: float = 1e-4, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: Optional[float] = 1.0, input_noise: float = 0.9, pack_padding: bool = True,
                 lr_scheduler: str = "constant", lr_warmup_steps: int = 0, gradient_checkpointing: Optional[bool] = None,
                 forward_only: bool = False, lr_scheduler_steps_per_optimizer_step: int = 1,
                 overlap_optimizer: bool = False, dp_sharding: Optional[str] = None, lora_rank: Optional[int] = None,
                 lora_alpha: Optional[float] = None, lora_target_modules=LORA_TARGETS,
                 gradient_accumulation_steps: int = 1, use_ema: bool = False, ema_decay: float = 0.9999,
                 lr_num_training_steps: Optional[int] = None, lr_num_cycles: Optional[float] = None,
                 lr_power: float = 1.0, sequence_parallel: bool = False, sp_group=None, check_sp_inputs: bool = True,
                 deterministic: bool = False):
        """lr_scheduler / lr_warmup_steps / lr_num_training_steps / lr_num_cycles / lr_power: diffusers' get_scheduler
        (train_x1_stage1_noiseinput.py:279-283, 513-521; the scripts use constant_with_warmup), one of LR_SCHEDULERS: the
        k-th optimizer step (k = 0, 1, ...) runs at lr * lr_factor(name, k * lr_scheduler_steps_per_optimizer_step, ...);
        "constant_with_warmup" is lr * min(1, k * stride / warmup).  "linear", "cosine", "cosine_with_restarts" and
        "polynomial" need lr_num_training_steps (counted like the warm-up, in scheduler steps); lr_num_cycles defaults to
        0.5 (cosine) / 1 (restarts), lr_power to 1.0 with end LR 1e-7: get_scheduler's defaults.
        Stepping convention mirrored (default 1 = the reference's scripts: they pass --deepspeed_plugin
        (pretrain_stage1_nv.sh:49), so `accelerator.prepare` wraps the scheduler in accelerate's DeepSpeedSchedulerWrapper
        whose step() is a no-op and the DeepSpeed engine advances it ONCE per optimizer step whatever the world size;
        num_warmup_steps there is lr_warmup_steps * gradient_accumulation_steps, :279-283, and the scripts use
        accumulation 1.  With gradient_accumulation_steps = A > 1 the schedule here still counts OPTIMIZER steps: micro-steps
        do not advance it.  The reference under DeepSpeed also advances once per optimizer step but passes
        num_warmup_steps = lr_warmup_steps * A, so its warm-up lasts A times as many optimizer steps: pass
        lr_warmup_steps = A * that value to mirror it; no default changes).  Without the DeepSpeed plugin accelerate's AcceleratedScheduler advances the schedule
        `num_processes` times per optimizer step (split_batches=False): pass lr_scheduler_steps_per_optimizer_step =
        world size to mirror that launch instead.  No fixture pins the LR trajectory of the reference's loop (it needs
        deepspeed, absent here): parity of the warm-up length is unpinned.  gradient_checkpointing (default: model.llm.gradient_checkpointing, set by
        `model.llm.gradient_checkpointing_enable()`, train...py:170-171): keep only each decoder layer's input and
        recompute the layer inside the backward (OmniGen/transformer.py:182-192).  forward_only: no gradient / optimizer
        state (loss evaluation through `loss.training_losses_x1_noise_input`).  dp_sharding (default: $VGPT_DP_SHARDING,
        else "none"): "none" replicates the fp32 optimizer state on every rank and all-reduces the gradients; "optimizer"
        shards it (reduce-scatter of the gradient buckets, AdamW on this rank's 1/world of every bucket, all-gather of the
        updated parameters).  Inert at world size 1.  lora_rank = r (1 <= r <= 64; train...py:204-223): the
        base model is frozen and rank-r adapters on lora_target_modules of every decoder layer are the only trained tensors
        (lora_alpha defaults to r; peft's "gaussian" init); no base gradient buckets, masters or moments exist, the adapter
        state is a few MB and is never sharded.
        gradient_accumulation_steps = A (--gradient_accumulation_steps, train...py:121, 353, 393-413): step(update=True)
        counts micro-steps; micro-steps 1 .. A-1 run forward and backward and add every gradient bucket to an fp32
        accumulator of its own (full length also when sharded, allocated on first use, 4 B per parameter) with no
        collective, no clip, no AdamW and no change of step_count or the LR; micro-step A writes bucket = T(acc + bucket)
        (one rounding of the fp32 sum), exchanges it as ever and steps the optimizer.  The factor 1/A goes where 1/world
        goes, into clip_coef: the clip acts on the norm of the MEAN gradient over micro-batches and ranks and AdamW sees the
        mean, as accelerate's loss / A with clipping on sync_gradients only (:393-400).  `grad_norm` holds the norm of the
        SUM over the A micro-batches and the ranks (A * world times the norm of the mean), as it holds the sum over ranks
        at A = 1.  step(update=False) stays a stand-alone backward that overwrites the buckets and touches neither the
        accumulators nor the micro-step counter (legal in the middle of a cycle).
        use_ema / ema_decay (--use_ema, :227-230, 288-290, 406-408, 440-447; update_ema, LVM/utils.py:27-34, decay 0.9999):
        one fp32 EMA buffer per master buffer (this rank's shard when sharded), a copy of the master at construction (the
        reference's update_ema(ema, model, decay=0)), moved inside every AdamW launch: ema = d ema + (1 - d) master_new.
        Deliberate difference: the reference's EMA is a deepcopy of the model in the model's dtype, and under bf16
        parameters an increment of relative size 1 - 0.9999 lies below bf16 resolution, so that EMA barely moves; here the
        EMA is fp32 and follows the fp32 master.  Full fine-tuning only.  ema_state_dict() / ema_weights() read it.
        sequence_parallel / sp_group (--sequence_parallel_size with LVMTraining_CP): Ulysses sequence parallelism through
        forward and backward over `sp_group` (default: sequence_parallel.get_sequence_parallel_group()); on when the flag
        is set and the group has P > 1 ranks, which then must all call step() with the SAME batch, latents and noise
        (sequence_parallel.broadcast_batch; loss.training_losses_x1_noise_input broadcasts its draws).  The world is
        world / P data-parallel replicas of P ranks; the update equals the P = 1 update on the same clips up to summation
        order (unlike the reference, whose decoder gradients come out scaled 1 / P).  check_sp_inputs:
        every sharded step() first all-gathers a 16-byte digest of (input_ids, t, x1.shape) over the group and raises on
        every rank when they differ; False skips that collective.
        deterministic: the three reductions of the step that add with fp32 atomics (RMSNorm gain gradients, the final
        layer's dshift / dscale, the embedding-table gradient) run their fixed-order twins (vgpt_*_det), which makes the
        step a pure function of its inputs: same inputs, build, world size and collective library give the same bits
        (DESIGN.md §6d).  Composes with every other option; nothing to do in a forward-only trainer."""
        model._check_ready()
        if hasattr(model, "release_engines"):
            model.release_engines()          # a sampler engine cached on the model holds GBs the trainer's buffers want
        self.model = model
        self.cfg = model.llm.config
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        if lr_scheduler not in LR_SCHEDULERS:
            raise VgptError(f"lr_scheduler {lr_scheduler!r}: built are {LR_SCHEDULERS}")
        if lr_scheduler not in ("constant", "constant_with_warmup") and lr_num_training_steps is None:
            raise VgptError(f"lr_scheduler {lr_scheduler!r} needs lr_num_training_steps")
        self.lr_scheduler, self.lr_warmup_steps = lr_scheduler, int(lr_warmup_steps)
        self.lr_num_training_steps = None if lr_num_training_steps is None else int(lr_num_training_steps)
        self.lr_num_cycles = None if lr_num_cycles is None else float(lr_num_cycles)
        self.lr_power = float(lr_power)
        A = gradient_accumulation_steps
        if isinstance(A, bool) or not isinstance(A, int) or A < 1:
            raise VgptError(f"gradient_accumulation_steps {A!r}: an integer >= 1 is built")
        self.accum_steps = A
        self._micro = 0              # micro-steps taken in the current accumulation cycle
        self._acc = None             # fp32 accumulators (small | lora, [layer 0 .. nl-1]); allocated on first use
        self.use_ema, self.ema_decay = bool(use_ema), float(ema_decay)
        self.ema_small, self.ema_layers = None, None
        self._ema_swapped = False    # inside ema_weights(): the parameter buffers hold the EMA, not the training weights
        self.last_load = None        # what the last load_checkpoint did with the EMA ({"ema": ...}); None before any load
        if self.use_ema:
            if lora_rank is not None:
                raise VgptError("use_ema with lora_rank: EMA of adapters is not built")
            if forward_only:
                raise VgptError("use_ema with forward_only: there is no optimizer state, EMA of a forward-only trainer is not built")
            if not 0.0 <= self.ema_decay <= 1.0:
                raise VgptError(f"ema_decay {ema_decay!r}: expected 0 <= decay <= 1")
        if int(lr_scheduler_steps_per_optimizer_step) < 1:
            raise VgptError("lr_scheduler_steps_per_optimizer_step must be >= 1")
        self.lr_sched_stride = int(lr_scheduler_steps_per_optimizer_step)
        self.gradient_checkpointing = (bool(getattr(model.llm, "gradient_checkpointing", False))
                                       if gradient_checkpointing is None else bool(gradient_checkpointing))
        self.forward_only = forward_only
        self.deterministic = bool(deterministic)
        self.max_grad_norm = max_grad_norm
        self.input_noise = input_noise
        self.pack_padding = pack_padding
        self.dev = model.llm.norm.weight.device
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        self._sp = self._sp_state(sequence_parallel, sp_group, lora_rank)     # refusals before any collective
        self.check_sp_inputs = bool(check_sp_inputs)
        if lora_rank is not None:
            if isinstance(lora_rank, bool) or int(lora_rank) != lora_rank or not 1 <= int(lora_rank) <= 64:
                raise VgptError(f"lora_rank {lora_rank!r}: an integer rank 1 <= r <= 64 is built")
            bad = [n for n in lora_target_modules if n not in LORA_TARGETS]
            if bad or not lora_target_modules:
                raise VgptError(f"lora_target_modules {tuple(lora_target_modules)!r}: adapters are built for {LORA_TARGETS} only")
            if dp_sharding == "optimizer":
                raise VgptError('dp_sharding="optimizer" with lora_rank: the adapter state is a few MB, there is nothing to shard')
            dp_sharding = "none"             # $VGPT_DP_SHARDING is ignored in this mode
        if dp_sharding is None:
            dp_sharding = os.environ.get("VGPT_DP_SHARDING", "none")
        if dp_sharding not in DP_SHARDING_MODES:
            raise VgptError(f"dp_sharding {dp_sharding!r}: expected one of {DP_SHARDING_MODES}")
        self.dp_sharding = dp_sharding
        self._sharded = dp_sharding == "optimizer" and self.world > 1 and not forward_only
        self._group = dist.group.WORLD if self.world > 1 else None
        self._gathers = None         # (small, [layer 0 .. nl-1]) all-gathers of updated parameters in flight (sharded)
        # AdamW behind the clip coefficient on a stream of its own (see optimizer_step): events of the update of the small
        # bucket and of every layer bucket, waited for where the next forward first reads those parameters
        self.overlap_optimizer = bool(overlap_optimizer) and self.dev.type == "cuda" and not forward_only
        self._opt_stream = torch.cuda.Stream(device=self.dev) if self.overlap_optimizer else None
        if self.overlap_optimizer or self._sharded:
            # parameters are read outside step() too, and may still be updated (overlap_optimizer) or all-gathered (sharded):
            # the sampler asks wait_for_pending_update(model), state_dict() through this hook
            _TRAINER_OF[model] = weakref.ref(self)
            model.register_state_dict_pre_hook(_state_dict_barrier)
        self._opt_events = None      # (small, [layer 0 .. nl-1]) of the update in flight
        self.step_count = 0
        self.skip_allreduce = False   # measurement only (bench.py's exposed-communication leg): ranks stop agreeing when set;
        #                               skips every collective of the step (sharded: reduce-scatter, norm exchange, all-gather)
        # VGPT_DP_OVERLAP=0: all buckets are reduced behind the backward instead of layer by layer under it (for A/B runs on a
        # multi-GPU node: RCCL's kernels share the CUs with the backward's GEMMs while they overlap)
        self.overlap_allreduce = os.environ.get("VGPT_DP_OVERLAP", "1") != "0"
        self.params = {n: p for n, p in model.named_parameters()}
        self._ws = {}
        self.last = {}
        self.grads: Dict[str, torch.Tensor] = {}
        self.lora_rank = None
        self.lora: Dict[str, torch.Tensor] = {}
        if lora_rank is not None:
            self._init_lora(int(lora_rank), lora_alpha, tuple(lora_target_modules))
            return
        if forward_only:
            return
        L = self.cfg.num_hidden_layers
        # ---- gradient storage: one flat bf16 bucket per decoder layer + one fp32 bucket for the rest ----
        self.layer_names = [[f"llm.layers.{i}.self_attn.qkv_proj.weight", f"llm.layers.{i}.self_attn.o_proj.weight",
                             f"llm.layers.{i}.mlp.gate_up_proj.weight", f"llm.layers.{i}.mlp.down_proj.weight"]
                            for i in range(L)]
        self.layer_buckets = []
        self._bucket_numel = []       # unpadded lengths of the layer buckets: the checkpoint layout
        for names in self.layer_names:
            n = sum(self.params[k].numel() for k in names)
            self._bucket_numel.append(n)
            flat = torch.zeros(self._padded(n), dtype=BF16, device=self.dev)
            o = 0
            for k in names:
                sz = self.params[k].numel()
                self.grads[k] = flat[o:o + sz].view(self.params[k].shape)
                o += sz
            self.layer_buckets.append(flat)
        big = {k for names in self.layer_names for k in names}
        small = [k for k in self.params if k not in big]
        n_small = sum(self.params[k].numel() for k in small)
        self._small_numel = n_small
        self.small_bucket = torch.zeros(self._padded(n_small), dtype=F32, device=self.dev)
        o = 0
        for k in small:
            sz = self.params[k].numel()
            self.grads[k] = self.small_bucket[o:o + sz].view(self.params[k].shape)
            o += sz
        if self._sharded:
            self._init_sharded_state(small)
            return
        # ---- optimizer state (fp32 master + moments), flat per bucket so AdamW is one launch per bucket ----
        def flat_params(names):
            return torch.cat([self.params[k].detach().reshape(-1).to(F32) for k in names])
        self.master_layers = [flat_params(names) for names in self.layer_names]
        self.master_small = flat_params(small)
        self.small_names = small
        z = lambda t: torch.zeros_like(t)
        self.m_layers = [z(t) for t in self.master_layers]
        self.v_layers = [z(t) for t in self.master_layers]
        self.m_small, self.v_small = z(self.master_small), z(self.master_small)
        # model parameters become views of flat bf16 buffers so the optimizer writes them in one launch
        self.param_layers = []
        for names in self.layer_names:
            flat = torch.cat([self.params[k].detach().reshape(-1) for k in names]).contiguous()
            o = 0
            for k in names:
                sz = self.params[k].numel()
                self.params[k].data = flat[o:o + sz].view(self.params[k].shape)
                o += sz
            self.param_layers.append(flat)
        flat = torch.cat([self.params[k].detach().reshape(-1) for k in small]).contiguous()
        o = 0
        for k in small:
            sz = self.params[k].numel()
            self.params[k].data = flat[o:o + sz].view(self.params[k].shape)
            o += sz
        self.param_small = flat
        bump_weight_generation(model)     # storage re-pointed; from here on the optimizer writes it through raw pointers
        self._init_scalars()
        self._init_ema()

    # ---- sequence parallelism ------------------------------------------------------------------------------------------
    def _sp_state(self, flag, group, lora_rank):
        """None (off), or {"group", "P", "r"} of the sequence-parallel group this trainer shares its rows with.  Every
        refusal depends on arguments and group sizes alone, so all ranks raise together and no collective is issued."""
        if not flag:
            return None
        if group is None:
            group = SPM.get_sequence_parallel_group()
        if group is None:
            raise VgptError("sequence_parallel=True needs a group: pass sp_group or call "
                            "sequence_parallel.initialize_sequence_parallel_state() first")
        P = dist.get_world_size(group)
        if P < 1:
            raise VgptError("sequence_parallel: this rank is not a member of sp_group")
        if P == 1:
            return None
        if lora_rank is not None:
            raise VgptError("lora_rank with sequence_parallel: adapters under sequence parallelism are not built")
        if self.world % P:
            raise VgptError(f"sequence_parallel: the world size {self.world} is not a multiple of the group size {P}")
        nq, nk = self.cfg.num_attention_heads, self.cfg.num_key_value_heads
        if nq % P or nk % P:
            raise VgptError(f"sequence_parallel over {P} ranks needs num_attention_heads ({nq}) and num_key_value_heads "
                            f"({nk}) divisible by {P}")
        return {"group": group, "P": P, "r": dist.get_rank(group)}

    def _check_sp_batch(self, batch, x1, t):
        """All ranks of the group must train on the same clip and the same noise: one small collective, and every rank
        raises when the digests differ (nobody is left waiting in an exchange)."""
        import hashlib
        h = hashlib.blake2b(digest_size=16)
        h.update(batch["input_ids"].detach().cpu().contiguous().numpy().tobytes())
        h.update(t.detach().to("cpu", F32).contiguous().numpy().tobytes())
        h.update(repr(tuple(x1.shape)).encode())
        mine = torch.frombuffer(bytearray(h.digest()), dtype=torch.uint8).to(self.dev)
        every = SPM.all_gather_flat(mine, self._sp["group"]).cpu()
        if not bool((every == every[0]).all()):
            bad = [i for i in range(every.shape[0]) if not torch.equal(every[i], every[0])]
            raise VgptError(f"Stage1Trainer.step: the ranks of the sequence-parallel group were given different inputs "
                            f"(input_ids, t or x1.shape of group ranks {bad} differ from group rank 0's): broadcast the "
                            "batch and the noise inside the group (sequence_parallel.broadcast_batch)")

    # ---- LoRA mode --------------------------------------------------------------------------------------------------
    def _init_lora(self, r: int, alpha, targets):
        """One flat rp-padded bf16 working buffer for every adapter (layer order; per module lora_A (rp, in) then lora_B
        (out, rp)), with one flat fp32 master, m, v and gradient bucket: AdamW, the clip's sum of squares and the
        data-parallel exchange are one launch each.  The base parameters stay where they are and get no state at all."""
        self.lora_rank, self.lora_rp = r, LO.padded_rank(r)
        self.lora_alpha = float(r if alpha is None else alpha)
        self.lora_scale = self.lora_alpha / r
        self.lora_targets = tuple(n for n in LORA_TARGETS if n in targets)
        rp = self.lora_rp
        slots, o = [], 0            # (layer, module, "A" | "B", offset, padded shape)
        for i, layer in enumerate(self.model.llm.layers):
            for mod in self.lora_targets:
                out_f, in_f = getattr(layer.self_attn, mod).weight.shape
                for ab, shape in (("A", (rp, in_f)), ("B", (out_f, rp))):
                    slots.append((i, mod, ab, o, shape))
                    o += shape[0] * shape[1]
        self._lora_numel = o
        # peft init_lora_weights="gaussian": lora_A ~ N(0, (1/r)^2), lora_B = 0; CPU draws from torch's global generator in
        # layer order; the padded ranks are zero and every kernel and the optimizer keep them exactly zero
        host = torch.zeros(o, dtype=F32)
        for i, mod, ab, off, shape in slots:
            if ab == "A":
                host[off:off + shape[0] * shape[1]].view(shape)[:r].normal_(0.0, 1.0 / r)
        self.lora_param = host.to(BF16).to(self.dev)
        train = not self.forward_only
        if train:
            self.lora_master = host.to(self.dev)
            self.lora_m, self.lora_v = torch.zeros_like(self.lora_master), torch.zeros_like(self.lora_master)
            self.lora_bucket = torch.zeros(o, dtype=F32, device=self.dev)
        self._lora_w, self._lora_g = {}, {}      # (layer, module) -> padded (A, B) views of the working copy / the gradient
        for i, mod, ab, off, shape in slots:
            name = lora_key(i, mod, ab)
            n = shape[0] * shape[1]
            unpad = (lambda t: t[:r]) if ab == "A" else (lambda t: t[:, :r])
            w = self.lora_param[off:off + n].view(shape)
            self._lora_w.setdefault((i, mod), {})[ab] = w
            self.lora[name] = unpad(w)
            if train:
                gr = self.lora_bucket[off:off + n].view(shape)
                self._lora_g.setdefault((i, mod), {})[ab] = gr
                self.grads[name] = unpad(gr)
        if train:
            self._init_scalars()

    def _lora_optimizer_step(self, lr, b1, b2, micro_batches=1):
        """sumsq, clip coefficient and AdamW over the one adapter bucket (the caller has advanced the step counter)."""
        self.sumsq.zero_()
        T.sumsq(self.lora_bucket, self.sumsq)
        w = float(self.world * micro_batches)
        T.clip_coef(self.sumsq, self.coef, self.grad_norm, (self.max_grad_norm or 0.0) * w, 1.0 / w)
        if not self.overlap_optimizer:
            T.adamw_step(self.lora_master, self.lora_param, self.lora_bucket, self.lora_m, self.lora_v, lr, b1, b2, self.eps,
                         self.wd, self.step_count, self.coef)
            return
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        self._opt_stream.wait_event(ready)
        with torch.cuda.stream(self._opt_stream):
            T.adamw_step(self.lora_master, self.lora_param, self.lora_bucket, self.lora_m, self.lora_v, lr, b1, b2, self.eps,
                         self.wd, self.step_count, self.coef)
            ev = torch.cuda.Event()
            ev.record(self._opt_stream)
        self._opt_events = (ev, [ev] * self.cfg.num_hidden_layers)

    def _merge_into(self, model, sign_scale=None):
        """W <- bf16(float(W) + s B A) on every adapted projection of `model`, through lora_up_add (Y = W, U = B, S = A)."""
        s = self.lora_scale if sign_scale is None else sign_scale
        for (i, mod), w in self._lora_w.items():
            LO.lora_up_add(getattr(model.llm.layers[i].self_attn, mod).weight.data, w["B"], w["A"], s_is_rp_by_n=True, alpha=s)

    def merged_weights(self):
        """Context manager for validation sampling mid-training: inside it the model's qkv_proj / o_proj weights carry the
        current adapters (W + s B A); on exit the saved base weights come back bit for bit.  Cached sampler engines refold on
        both edges (weight generation bumped)."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            if self.lora_rank is None:
                raise VgptError("merged_weights: not a LoRA trainer")
            self.finish_optimizer()
            ws = [getattr(self.model.llm.layers[i].self_attn, mod).weight for (i, mod) in self._lora_w]
            saved = [w.detach().clone() for w in ws]
            self._merge_into(self.model)
            bump_weight_generation(self.model)
            try:
                yield self.model
            finally:
                with torch.no_grad():
                    for w, sv_ in zip(ws, saved):
                        w.copy_(sv_)
                bump_weight_generation(self.model)
        return cm()

    def _init_ema(self):
        """update_ema(ema, model, decay=0) (train...py:288-290): the EMA starts as a copy of the fp32 master weights."""
        if self.use_ema:
            self.ema_layers = [t.clone() for t in self.master_layers]
            self.ema_small = self.master_small.clone()

    def _adamw(self, master, param, grad, m_, v_, ema, lr, b1, b2):
        """One AdamW launch over a flat bucket; with an EMA buffer the launch that also moves it (no second pass)."""
        if ema is None:
            T.adamw_step(master, param, grad, m_, v_, lr, b1, b2, self.eps, self.wd, self.step_count, self.coef)
        else:
            T.adamw_ema_step(master, param, grad, m_, v_, lr, b1, b2, self.eps, self.wd, self.step_count, self.coef, ema,
                             self.ema_decay)

    # ---- gradient accumulation ---------------------------------------------------------------------------------------
    def _accum_mode(self, update: bool):
        """None: no accumulation in this call (A == 1, or a stand-alone backward); else vgpt_grad_accumulate's mode of this
        micro-step: 0 first, 1 middle, 2 last (the bucket receives the sum and the optimizer steps)."""
        if not update or self.accum_steps == 1:
            return None
        if self._micro == self.accum_steps - 1:
            return 2
        return 0 if self._micro == 0 else 1

    def _accumulators(self):
        if self._acc is None:
            z = lambda t: torch.empty(t.numel(), dtype=F32, device=self.dev)
            if self.lora_rank is not None:
                self._acc = (z(self.lora_bucket), [])
            else:
                self._acc = (z(self.small_bucket), [z(b) for b in self.layer_buckets])
        return self._acc

    def _init_scalars(self):
        self.sumsq = torch.zeros(1, dtype=F32, device=self.dev)
        self.coef = torch.ones(1, dtype=F32, device=self.dev)

        self.grad_norm = torch.zeros(1, dtype=F32, device=self.dev)

    # ---- dp_sharding="optimizer" -----------------------------------------------------------------------------------
    def _padded(self, n: int) -> int:
        return shard_partition(n, self.world)[0] if self._sharded else n

    def _shard(self, flat: torch.Tensor) -> torch.Tensor:
        """This rank's contiguous slice of a padded flat bucket (the whole bucket when not sharded)."""
        if not self._sharded:
            return flat
        s = flat.numel() // self.world
        return flat[self.rank * s:(self.rank + 1) * s]

    def _init_sharded_state(self, small):
        """Parameters become views into the front of zero-padded flat bf16 buckets (padded like the gradient buckets);
        fp32 master weights and moments exist for this rank's shard of every bucket only, the master shard taken from the
        parameter shard.  No full-length fp32 temporary: at full size it would be the replicated state this mode avoids."""
        def flat_params(names):
            n = sum(self.params[k].numel() for k in names)
            flat = torch.zeros(self._padded(n), dtype=self.params[names[0]].dtype, device=self.dev)
            o = 0
            for k in names:
                sz = self.params[k].numel()
                flat[o:o + sz].copy_(self.params[k].detach().reshape(-1))
                self.params[k].data = flat[o:o + sz].view(self.params[k].shape)
                o += sz
            return flat
        self.param_layers = [flat_params(names) for names in self.layer_names]
        self.param_small = flat_params(small)
        self.small_names = small
        self.master_layers = [self._shard(b).to(F32) for b in self.param_layers]
        self.master_small = self._shard(self.param_small).to(F32)
        z = lambda t: torch.zeros_like(t)
        self.m_layers = [z(t) for t in self.master_layers]
        self.v_layers = [z(t) for t in self.master_layers]
        self.m_small, self.v_small = z(self.master_small), z(self.master_small)
        bump_weight_generation(self.model)
        self._init_scalars()
        self._init_ema()
        self._partials = torch.zeros(self.world, dtype=F32, device=self.dev)   # every rank's sum of squares, rank order

    def _reduce(self, bucket):
        """Asynchronous gradient exchange of one flat bucket: all-reduce (replicated), or a reduce-scatter whose sum lands in
        this rank's own slice of the bucket (sharded).  None when a host-staged transport has already finished it."""
        if self._sharded:
            return SPM.reduce_scatter_flat(bucket, self._group, async_op=True)
        return dist.all_reduce(bucket, async_op=True)

    def _await_params(self, i: int):
        """Makes the current stream wait until the parameters of bucket i (-1: the small bucket, else decoder layer i) are
        updated (overlap_optimizer) and all-gathered (sharded)."""
        if self._opt_events is not None:
            torch.cuda.current_stream().wait_event(self._opt_events[0] if i < 0 else self._opt_events[1][i])
        if self._gathers is not None:
            w = self._gathers[0] if i < 0 else self._gathers[1][i]
            if w is not None:
                w.wait()

    @classmethod
    def for_evaluation(cls, model, deterministic: bool = False):
        """A forward-only trainer cached on the model (no gradient buckets, no optimizer state; `deterministic` is kept on
        a new one and changes nothing: the forward pass has no order-dependent sum)."""
        tr = getattr(model, "_vgpt_eval_trainer", None)
        if tr is None:
            tr = cls(model, forward_only=True, deterministic=deterministic)
            object.__setattr__(model, "_vgpt_eval_trainer", tr)
        return tr

    def current_lr(self) -> float:
        """Learning rate of the NEXT optimizer step (diffusers get_constant_schedule_with_warmup's lambda at
        current_step = optimizer steps taken so far)."""
        k = self.step_count * self.lr_sched_stride
        if self.lr_scheduler in ("constant", "constant_with_warmup"):      # the two first built: their expression, to the bit
            if self.lr_scheduler == "constant_with_warmup" and k < self.lr_warmup_steps:
                return self.lr * k / max(1.0, float(self.lr_warmup_steps))
            return self.lr
        return self.lr * lr_factor(self.lr_scheduler, k, self.lr_warmup_steps, self.lr_num_training_steps,
                                   self.lr_num_cycles, self.lr_power, self.lr)

    # ------------------------------------------------------------------------------------------------
    def _buf(self, name, shape, dtype=BF16):
        t = self._ws.get(name)
        if t is None or t.shape != torch.Size(shape) or t.dtype != dtype:
            t = torch.empty(*shape, dtype=dtype, device=self.dev)
            self._ws[name] = t
        return t

    def _prepare(self, batch):
        cfg = self.cfg
        ids, pos, mask = batch["input_ids"], batch["position_ids"], batch["attention_mask"]
        B, L = ids.shape
        row_of = lambda b, s: b * L + s
        pads = count_left_pads(mask) if self.pack_padding else []
        if self._sp is not None and B > 1 and not any(pads):
            pads = [0] * B               # the shares cut ONE sequence: rows of a batch are laid end to end
        if any(pads) or (self._sp is not None and B > 1):
            ids, pos, mask, offs = pack_left_padded(ids, pos, mask, pads)
            row_of = lambda b, s: offs[b] + s - pads[b]
            B, L = ids.shape
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.dev)
        x_rows = _rows(batch["denoise_image_sizes"], row_of, True)
        t_rows = _rows(batch["time_emb_inx"], row_of, False)
        c_rows = _rows(batch["input_image_sizes"], row_of, True)
        ntok_x = batch_ntok(batch["denoise_image_sizes"])
        keep = torch.ones(B * L, dtype=torch.uint8)
        for r0 in x_rows + c_rows:
            keep[r0:r0 + ntok_x] = 0
        for r0 in t_rows:
            keep[r0] = 0
        c_idx = torch.tensor([r0 + k for r0 in c_rows for k in range(ntok_x)], dtype=torch.int64, device=self.dev) if c_rows else None
        return dict(ids=ids.contiguous(), B=B, L=L, pm=ops.as_packed_mask(mask, self.dev), rope=self.model.llm.rope_tables(pos),
                    x_rows=i32(x_rows), t_rows=i32(t_rows), c_rows=i32(c_rows) if c_rows else None, c_idx=c_idx,
                    keep=keep.to(self.dev), ntok=ntok_x)

    # ------------------------------------------------------------------------------------------------
    def step(self, batch, x1: torch.Tensor, x0: torch.Tensor, t: torch.Tensor, clean: Optional[torch.Tensor],
             x0_in: Optional[torch.Tensor], t_in: Optional[torch.Tensor], update: bool = True, backward: bool = True,
             input_output_return: bool = False):
        """One optimisation step.  x1/x0: (F, C, h, w) fp32 target latents / noise, t: (F,) fp32;
        clean/x0_in/t_in: the clean-frame latents and their noise (loss.py:166-192).  Returns the per-frame losses.
        With gradient_accumulation_steps = A > 1 and update=True this is one MICRO-step: the optimizer steps on every A-th
        call (see __init__)."""
        if update:
            self._refuse_inside_ema_weights("step(update=True)")
        m, cfg = self.model, self.cfg
        sp = self._sp
        if sp is not None and self.check_sp_inputs:
            self._check_sp_batch(batch, x1, t)
        prep = self._prepare(batch)
        # the previous step's update may still be running on its own stream, its all-gathers (sharded) still in flight
        self._await_params(-1)               # embeddings, heads, final norm: read from the start
        B, L, M, H, I = prep["B"], prep["L"], prep["B"] * prep["L"], cfg.hidden_size, cfg.intermediate_size
        nq, nk, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        nl = cfg.num_hidden_layers
        nf, C, h, w = x1.shape
        ntok = prep["ntok"]
        Tn = nf * ntok
        x1 = x1.to(self.dev, F32).contiguous(); x0 = x0.to(self.dev, F32).contiguous()
        t = t.to(self.dev, F32).contiguous()
        # ---------------- forward ----------------
        xt = T.lerp_frames(x1, x0, t, self._buf("xt", (nf, C, h, w)))
        cl = None
        if clean is not None and clean.shape[0] > 0:
            cl = T.lerp_frames(clean.to(self.dev, F32).contiguous(), x0_in.to(self.dev, F32).contiguous(),
                               t_in.to(self.dev, F32).contiguous(), self._buf("cl", tuple(clean.shape)))
        # sequence parallelism: this rank runs rows [r0, r1) of the one packed sequence (Ms of the M rows) through the
        # row-local work and its nq / P heads (Wl fused q|k|v columns, dc context columns) through attention over all rows
        Ms, rope = M, prep["rope"]
        if sp is not None:
            P = sp["P"]
            shares, _ = sp_shares(M, P)
            sizes = [e_ - a_ for a_, e_ in shares]
            r0, r1 = shares[sp["r"]]
            Ms, Wl, dc = r1 - r0, (nq + 2 * nk) // P * hd, nq // P * hd
            rope = tuple(t_.view(-1, hd // 2)[r0:r1] for t_ in prep["rope"])
        hbuf = self._buf("h", (nl + 1, Ms, H))         # layer inputs (h[l]) and the last output
        # the sequence assembly is cheap and runs on all rows on every rank; the share is a copy of its rows
        seq = hbuf[0] if sp is None else self._buf("seq_all", (M, H))
        ops.embed_gather(prep["ids"], m.llm.embed_tokens.weight, out=seq.view(B, L, H))
        pos = m.pos_embed[0]
        if cl is not None:
            ops.patch_embed(cl, m.input_x_embedder.proj.weight, m.input_x_embedder.proj.bias, pos, prep["c_rows"], seq,
                            m.pos_embed_max_size)
        sin = ops.timestep_sinusoid(t, m.time_token.freqs(self.dev))
        tt, te, ada = m.time_token.mlp, m.t_embedder.mlp, m.final_layer.adaLN_modulation[1]
        tt_pre = ops.linear_small(sin, tt[0].weight, tt[0].bias)
        tt_act = T.act_fwd(tt_pre, ops.ACT_SILU)
        ops.linear_small(tt_act, tt[2].weight, tt[2].bias, out=seq, out_row=prep["t_rows"], ldo=H)
        ops.patch_embed(xt, m.x_embedder.proj.weight, m.x_embedder.proj.bias, pos, prep["x_rows"], seq,
                        m.pos_embed_max_size)
        if sp is not None:
            hbuf[0].copy_(seq[r0:r1])
        # saved activations: every layer's (normal) or ONE layer's worth, recomputed per layer in the backward (checkpointing)
        ck = self.gradient_checkpointing
        ns = 1 if ck else nl
        n1 = self._buf("n1", (ns, Ms, H))
        ctx = self._buf("ctx", (ns, Ms, nq * hd)); h2 = self._buf("h2", (ns, Ms, H)); n2 = self._buf("n2", (ns, Ms, H))
        gu = self._buf("gu", (ns, Ms, 2 * I)); act = self._buf("act", (ns, Ms, I))
        if sp is None:
            qkv = self._buf("qkv", (ns, M, (nq + 2 * nk) * hd))
            lse = self._buf("lse", (ns, B, nq, L), F32)
        else:
            # kept per layer: the fused q|k|v rows of EVERY rank for this rank's heads, their context and lse; the share's
            # own q|k|v rows of all heads ("qkv") and the exchange buffers are transient
            qkv = self._buf("qkv", (Ms, (nq + 2 * nk) * hd))
            qkv_h = self._buf("qkv_heads", (ns, M, Wl)); ctx_h = self._buf("ctx_heads", (ns, M, dc))
            lse = self._buf("lse", (ns, 1, nq // P, M), F32)
            send = self._buf("sp_send", (P, Ms, Wl)); ctx_recv = self._buf("sp_ctx_recv", (P, Ms, dc))
            by_sender = [[n * Wl] * P for n in sizes]                     # every rank sends its rows to every rank
            by_owner = [[n * dc for n in sizes] for _ in range(P)]        # every rank sends each rank that rank's rows
        sv = lambda li: 0 if ck else li
        lora = self.lora_rank is not None
        lq, lo = lora and "qkv_proj" in self.lora_targets, lora and "o_proj" in self.lora_targets
        if lora:        # u = x A^T of both adapted projections, saved for the backward like the other activations
            rp, ls = self.lora_rp, self.lora_scale
            u_q = self._buf("u_q", (ns, M, rp)); u_o = self._buf("u_o", (ns, M, rp))

        def layer_forward(li, with_output=True):
            layer = m.llm.layers[li]
            at, mlp, k = layer.self_attn, layer.mlp, sv(li)
            self._await_params(li)           # this layer's parameters are updated (and gathered)
            ops.rmsnorm(hbuf[li], layer.input_layernorm.weight, layer.input_layernorm.variance_epsilon, out=n1[k])
            if lq:      # plain base GEMM, then y += s (x A^T) B^T and the rotation in one pass over y
                aq = self._lora_w[(li, "qkv_proj")]
                ops.linear(n1[k], at.qkv_proj.weight, out=qkv[k])
                LO.lora_down(n1[k], aq["A"], rp, out=u_q[k])
                LO.lora_up_add(qkv[k], u_q[k], aq["B"], alpha=ls, rope=(prep["rope"][0], prep["rope"][1], nq, nk, hd))
            elif sp is None:
                ops.linear_qkv_rope(n1[k], at.qkv_proj.weight, prep["rope"][0], prep["rope"][1], nq, nk, hd, out=qkv[k])
            if sp is None:
                T.attention_qkv_train(qkv[k].view(B, L, -1), prep["pm"], nq, nk, hd, ctx[k].view(B, L, -1), lse[k])
            else:       # engine.StaticDenoiser._sp_attention with the training forward's kernel
                ops.linear_qkv_rope(n1[k], at.qkv_proj.weight, rope[0], rope[1], nq, nk, hd, out=qkv)
                ops.sp_pack_qkv(qkv, P, nq, nk, hd, out=send)
                SPM.exchange_split(send, qkv_h[k], by_sender, sp["group"])
                T.attention_qkv_train(qkv_h[k].view(1, M, Wl), prep["pm"], nq // P, nk // P, hd, ctx_h[k].view(1, M, dc),
                                      lse[k])
                SPM.exchange_split(ctx_h[k], ctx_recv, by_owner, sp["group"])
                ops.sp_unpack_ctx(ctx_recv, P, out=ctx[k])
            ops.linear(ctx[k], at.o_proj.weight, residual=hbuf[li], out=h2[k])
            if lo:
                ao = self._lora_w[(li, "o_proj")]
                LO.lora_down(ctx[k], ao["A"], rp, out=u_o[k])
                LO.lora_up_add(h2[k], u_o[k], ao["B"], alpha=ls)
            ops.rmsnorm(h2[k], layer.post_attention_layernorm.weight, layer.post_attention_layernorm.variance_epsilon,
                        out=n2[k])
            # gate_up_proj + act(gate) * up in one kernel that also keeps the bf16 [gate | up] for the backward: bit for bit
            # ops.linear(n2, W) followed by T.silu_mul_fwd (tests/test_train_gpu.py), without the (M, 2I) round trip
            ops.gated_mlp_act(n2[k], mlp.gate_up_proj.weight, mlp.act, out=act[k], gate_up_out=gu[k])
            if with_output:
                ops.linear(act[k], mlp.down_proj.weight, residual=h2[k], out=hbuf[li + 1])

        for li in range(nl):
            layer_forward(li)
        if sp is None:
            nrm = ops.rmsnorm(hbuf[nl], m.llm.norm.weight, m.llm.norm.variance_epsilon, out=self._buf("nrm", (M, H)))
        else:
            # final norm on the share, then ONE exchange leaves the normed rows of every rank on every rank (Gather.forward,
            # LVM/utils.py:148-161; shares padded to the largest): the heads below, the loss and their backward run
            # replicated, so the loss vector is the same bits on every rank
            pad = self._buf("nrm_pad", (max(sizes), H))
            ops.rmsnorm(hbuf[nl], m.llm.norm.weight, m.llm.norm.variance_epsilon, out=pad[:Ms])
            every = SPM.all_gather_flat(pad, sp["group"], out=self._buf("nrm_every", (P, max(sizes) * H)))
            nrm = self._buf("nrm", (M, H))
            for i, (a_, e_) in enumerate(shares):
                nrm[a_:e_].copy_(every[i].view(-1, H)[:e_ - a_])
        te_pre = ops.linear_small(sin, te[0].weight, te[0].bias)
        te_act = T.act_fwd(te_pre, ops.ACT_SILU)
        temb = ops.linear_small(te_act, te[2].weight, te[2].bias)
        st = T.act_fwd(temb, ops.ACT_SILU)
        mod = ops.linear_small(st, ada.weight, ada.bias)
        v = self._buf("v", (Tn, H)); xhat = self._buf("xhat", (Tn, H), F32); rstd = self._buf("rstd", (Tn,), F32)
        T.ln_mod_fwd(nrm, prep["x_rows"], mod, v, xhat, rstd, ntok)
        fl = m.final_layer.linear
        y16 = ops.linear(v, fl.weight, bias=fl.bias)                       # (Tn, 16)
        p2 = m.patch_size
        pred = y16.view(nf, h // p2, w // p2, p2, p2, C).permute(0, 5, 1, 3, 2, 4).reshape(nf, C, h, w).contiguous()
        loss = torch.empty(nf, dtype=F32, device=self.dev)
        dpred = self._buf("dpred", (nf, C, h, w))
        head = None
        if input_output_return:
            # LVM/model.py:832-841 + loss.py:220-225: the input_final_layer head predicts the CLEAN condition latents from the
            # last hidden state of their rows; its per-frame MSE terms are appended to the loss vector before .mean()
            if cl is None:
                raise VgptError("Stage1Trainer.step: input_output_return needs condition frames")
            head = m.input_final_layer           # AttributeError without init_input_final_layer(), as in the reference
            nfc = clean.shape[0]
            vin = T.gather_rows(nrm, prep["c_rows"], ntok)                   # (nfc * ntok, H)
            yin = ops.linear(vin, head.weight, bias=head.bias)
            pred_in = yin.view(nfc, h // p2, w // p2, p2, p2, C).permute(0, 5, 1, 3, 2, 4).reshape(nfc, C, h, w).contiguous()
            loss_in = torch.empty(nfc, dtype=F32, device=self.dev)
            dpred_in = self._buf("dpred_in", (nfc, C, h, w))
            T.mse_frames(pred_in, clean.to(self.dev, F32).contiguous(), loss_in, dpred_in, n_mean=nf + nfc)
            T.mse_frames(pred, x1, loss, dpred, n_mean=nf + nfc)
            loss = torch.cat([loss, loss_in])
            self.last = dict(pred=pred, loss=loss, xt=xt, pred_in=pred_in)
        else:
            T.mse_frames(pred, x1, loss, dpred)
            self.last = dict(pred=pred, loss=loss, xt=xt)
        if self.forward_only or not backward:
            if update:
                raise VgptError("Stage1Trainer.step: an optimizer step needs the backward pass")
            return loss
        acc_mode = self._accum_mode(update)
        exchange = acc_mode in (None, 2)     # micro-steps before the last issue no collective
        if lora:
            self._lora_backward(locals())
            if update:
                self._finish_micro_step(acc_mode)
            return loss
        # ---------------- backward ----------------
        g = self.grads
        det = self.deterministic     # the fixed-order twins of the three reductions that add with atomics
        self.small_bucket.zero_()
        dy16 = T.unpatchify_bwd(dpred)                                      # (Tn, 16)
        T.matmul(dy16, v, out=g["final_layer.linear.weight"], ta=True)     # dWf = dy16^T v
        T.colsum(dy16, g["final_layer.linear.bias"])
        dv = T.matmul(dy16, fl.weight)                                      # (Tn, H)
        dnrm = self._buf("dnrm", (M, H)); dnrm.zero_()
        dmod = torch.zeros(nf, 2 * H, dtype=F32, device=self.dev)
        T.ln_mod_bwd(dv, xhat, rstd, mod, prep["x_rows"], dnrm, dmod, ntok, deterministic=det)
        if head is not None:
            dyin = T.unpatchify_bwd(dpred_in)                                # (nfc * ntok, 16)
            T.matmul(dyin, vin, out=g["input_final_layer.weight"], ta=True)
            T.colsum(dyin, g["input_final_layer.bias"])
            dnrm.index_copy_(0, prep["c_idx"], T.matmul(dyin, head.weight))  # condition rows: no other gradient reaches them here
        dh = self._buf("dh", (Ms, H)); dh_b = self._buf("dh_b", (Ms, H))
        # sharded: every rank keeps its own rows of dnrm (Gather.backward, LVM/utils.py:163-169): no exchange
        T.rmsnorm_bwd(hbuf[nl], m.llm.norm.weight, dnrm if sp is None else dnrm[r0:r1], dh, g["llm.norm.weight"],
                      m.llm.norm.variance_epsilon, deterministic=det)
        # adaLN + t_embedder
        T.matmul(dmod, st, out=g["final_layer.adaLN_modulation.1.weight"], ta=True)
        T.colsum(dmod, g["final_layer.adaLN_modulation.1.bias"])
        dtemb = T.act_bwd(temb, T.matmul(dmod, ada.weight), ops.ACT_SILU)
        self._mlp_bwd("t_embedder", te, dtemb, te_act, te_pre, sin)
        # decoder layers, last to first
        sw = sa = sb = None   # dX / dW read their operands transposed inside the GEMM (vgpt_gemm_bf16_tr)
        dact = self._buf("dact", (Ms, I)); dgu = self._buf("dgu", (Ms, 2 * I)); dn = self._buf("dn", (Ms, H))
        dctx = self._buf("dctx", (Ms, nq * hd)); dqkv = self._buf("dqkv", (Ms, (nq + 2 * nk) * hd))
        nsin = self._neg_sin(prep)
        if sp is None:
            delta = self._buf("delta", (B, nq, L), F32)
        else:
            delta = self._buf("delta", (1, nq // P, M), F32)
            nsin = nsin.view(-1, hd // 2)[r0:r1]
            dctx_send = self._buf("sp_dctx_send", (P, Ms, dc)); dctx_h = self._buf("dctx_heads", (M, dc))
            dqkv_h = self._buf("dqkv_heads", (M, Wl)); dqkv_recv = self._buf("sp_dqkv_recv", (P, Ms, Wl))
            ctx_by_sender = [[n * dc] * P for n in sizes]
            qkv_by_owner = [[n * Wl for n in sizes] for _ in range(P)]
        handles = []
        for li in range(nl - 1, -1, -1):
            layer = m.llm.layers[li]
            at, mlp = layer.self_attn, layer.mlp
            names = self.layer_names[li]
            if ck:      # same kernels on the same inputs as the forward pass: the recomputed activations are bit-identical
                layer_forward(li, with_output=False)
            k = sv(li)
            T.linear_dw(dh, act[k], sa, sb, g[names[3]])                               # dW_down
            T.linear_dx(dh, mlp.down_proj.weight, sw, out=dact)
            T.silu_mul_bwd(gu[k], dact, dgu, mlp.act)
            T.linear_dw(dgu, n2[k], sa, sb, g[names[2]])                               # dW_gate_up
            T.linear_dx(dgu, mlp.gate_up_proj.weight, sw, out=dn)
            T.rmsnorm_bwd(h2[k], layer.post_attention_layernorm.weight, dn, dh_b,
                          g[f"llm.layers.{li}.post_attention_layernorm.weight"],
                          layer.post_attention_layernorm.variance_epsilon, dres=dh, deterministic=det)   # dh2
            T.linear_dw(dh_b, ctx[k], sa, sb, g[names[1]])                             # dW_o
            T.linear_dx(dh_b, at.o_proj.weight, sw, out=dctx)
            if sp is None:
                T.attention_qkv_bwd(qkv[k].view(B, L, -1), ctx[k].view(B, L, -1), dctx.view(B, L, -1), lse[k], delta,
                                    dqkv.view(B, L, -1), prep["pm"], nq, nk, hd)
                ops.rope_qk_inplace(dqkv, prep["rope"][0], nsin, nq, nk, hd)             # inverse rotation
            else:
                # the forward's two exchanges, mirrored: d(ctx) of my rows goes to the ranks that own the heads, d(qkv) of
                # my heads goes back to the ranks that own the rows, and is rotated back on its way into row order
                ops.sp_pack_ctx(dctx, P, out=dctx_send)
                SPM.exchange_split(dctx_send, dctx_h, ctx_by_sender, sp["group"])
                T.attention_qkv_bwd(qkv_h[k].view(1, M, Wl), ctx_h[k].view(1, M, dc), dctx_h.view(1, M, dc), lse[k], delta,
                                    dqkv_h.view(1, M, Wl), prep["pm"], nq // P, nk // P, hd)
                SPM.exchange_split(dqkv_h, dqkv_recv, qkv_by_owner, sp["group"])
                ops.sp_unpack_qkv_rope(dqkv_recv, P, nq, nk, hd, rope[0], nsin, out=dqkv)
            T.linear_dw(dqkv, n1[k], sa, sb, g[names[0]])                              # dW_qkv
            T.linear_dx(dqkv, at.qkv_proj.weight, sw, out=dn)
            T.rmsnorm_bwd(hbuf[li], layer.input_layernorm.weight, dn, dh,
                          g[f"llm.layers.{li}.input_layernorm.weight"], layer.input_layernorm.variance_epsilon,
                          dres=dh_b, deterministic=det)                                  # dh (layer input)
            if acc_mode is not None:     # right behind this layer's last dW, where its bucket is complete
                T.grad_accumulate(self._accumulators()[1][li], self.layer_buckets[li], acc_mode)
            if exchange and self.world > 1 and not self.skip_allreduce and self.overlap_allreduce:
                handles.append(self._reduce(self.layer_buckets[li]))
        # heads fed by dseq = dh (sharded: zero outside the share, so what follows yields this rank's partial gradients)
        dseq = dh
        if sp is not None:
            dseq = self._buf("dseq", (M, H)); dseq.zero_()
            dseq[r0:r1].copy_(dh)
            if sp["r"] > 0:      # computed on replicated rows: they enter the sum over the ranks from SP rank 0 alone
                for name in g:
                    if name.startswith(SP_REPLICATED):
                        g[name].zero_()
        dtt = T.gather_rows(dseq, prep["t_rows"], 1)
        self._mlp_bwd("time_token", tt, dtt, tt_act, tt_pre, sin)
        self._patch_bwd("x_embedder", T.gather_rows(dseq, prep["x_rows"], ntok), xt)
        if cl is not None:
            self._patch_bwd("input_x_embedder", T.gather_rows(dseq, prep["c_rows"], ntok), cl)
        T.embed_bwd(prep["ids"].view(-1), prep["keep"], dseq, g["llm.embed_tokens.weight"], deterministic=det)
        if acc_mode is not None:
            T.grad_accumulate(self._accumulators()[0], self.small_bucket, acc_mode)
        if exchange and self.world > 1 and not self.skip_allreduce:
            if not self.overlap_allreduce:
                handles += [self._reduce(b) for b in reversed(self.layer_buckets)]
            handles.append(self._reduce(self.small_bucket))
            for hd_ in handles:
                if hd_ is not None:
                    hd_.wait()
        if update:
            self._finish_micro_step(acc_mode)
        return loss

    def _finish_micro_step(self, acc_mode):
        """End of a step(update=True): the optimizer steps unless this was a micro-step before the last of its cycle."""
        if acc_mode is None:
            self.optimizer_step()
        elif acc_mode == 2:
            self._micro = 0
            self.optimizer_step(micro_batches=self.accum_steps)
        else:
            self._micro += 1

    def _lora_backward(self, f):
        """Backward with the base frozen: the dX chain of the full backward without a single dW GEMM, and per adapted
        projection dB = s dy^T u, du = s dy B, dA = du^T x, dx += du A.  Nothing that only feeds frozen parameters is
        computed: no head / adaLN / embedder / embedding gradients, no dx below layer 0's qkv_proj.  `f`: step()'s locals."""
        m, cfg, prep = self.model, self.cfg, f["prep"]
        B, L, M, H, I = f["B"], f["L"], f["M"], f["H"], f["I"]
        nq, nk, hd, nl, ntok, nf = f["nq"], f["nk"], f["hd"], f["nl"], f["ntok"], f["nf"]
        hbuf, n1, qkv, ctx, h2, n2, gu, act, lse = (f[k] for k in ("hbuf", "n1", "qkv", "ctx", "h2", "n2", "gu", "act", "lse"))
        u_q, u_o, sv, ck, rp, ls = f["u_q"], f["u_o"], f["sv"], f["ck"], self.lora_rp, self.lora_scale
        lq, lo = f["lq"], f["lo"]
        det = self.deterministic     # the discarded dgain / dmod sums too: one rule for every path
        dy16 = T.unpatchify_bwd(f["dpred"])                                  # (Tn, 16)
        dv = T.matmul(dy16, f["fl"].weight)                                  # (Tn, H)
        dnrm = self._buf("dnrm", (M, H)); dnrm.zero_()
        dmod = self._buf("dmod_scratch", (nf, 2 * H), F32); dmod.zero_()     # feeds adaLN only: discarded
        T.ln_mod_bwd(dv, f["xhat"], f["rstd"], f["mod"], prep["x_rows"], dnrm, dmod, ntok, deterministic=det)
        if f["head"] is not None:
            dyin = T.unpatchify_bwd(f["dpred_in"])
            dnrm.index_copy_(0, prep["c_idx"], T.matmul(dyin, f["head"].weight))
        dgain = self._buf("dgain_scratch", (H,), F32); dgain.zero_()         # gain gradients of the frozen norms: discarded
        dh = self._buf("dh", (M, H)); dh_b = self._buf("dh_b", (M, H))
        T.rmsnorm_bwd(hbuf[nl], m.llm.norm.weight, dnrm, dh, dgain, m.llm.norm.variance_epsilon, deterministic=det)
        dact = self._buf("dact", (M, I)); dgu = self._buf("dgu", (M, 2 * I)); dn = self._buf("dn", (M, H))
        dctx = self._buf("dctx", (M, nq * hd)); dqkv = self._buf("dqkv", (M, (nq + 2 * nk) * hd))
        delta = self._buf("delta", (B, nq, L), F32)
        du = self._buf("du", (M, rp))
        nsin = self._neg_sin(prep)
        self.lora_bucket.zero_()     # a target module left out keeps zero gradients; every built one is overwritten
        for li in range(nl - 1, -1, -1):
            layer = m.llm.layers[li]
            at, mlp = layer.self_attn, layer.mlp
            if ck:
                f["layer_forward"](li, with_output=False)
            k = sv(li)
            T.linear_dx(dh, mlp.down_proj.weight, None, out=dact)
            T.silu_mul_bwd(gu[k], dact, dgu, mlp.act)
            T.linear_dx(dgu, mlp.gate_up_proj.weight, None, out=dn)
            T.rmsnorm_bwd(h2[k], layer.post_attention_layernorm.weight, dn, dh_b, dgain,
                          layer.post_attention_layernorm.variance_epsilon, dres=dh, deterministic=det)   # dh2
            T.linear_dx(dh_b, at.o_proj.weight, None, out=dctx)
            if lo:
                w, gr = self._lora_w[(li, "o_proj")], self._lora_g[(li, "o_proj")]
                LO.lora_grad(dh_b, u_o[k], gr["B"], alpha=ls)                            # dB = s dy^T u
                LO.lora_down(dh_b, w["B"], rp, s_is_k_by_rp=True, alpha=ls, out=du)      # du = s dy B
                LO.lora_grad(ctx[k], du, gr["A"], transposed=True)                       # dA = du^T x
                LO.lora_up_add(dctx, du, w["A"], s_is_rp_by_n=True)                      # dx += du A
            T.attention_qkv_bwd(qkv[k].view(B, L, -1), ctx[k].view(B, L, -1), dctx.view(B, L, -1), lse[k], delta,
                                dqkv.view(B, L, -1), prep["pm"], nq, nk, hd)
            ops.rope_qk_inplace(dqkv, prep["rope"][0], nsin, nq, nk, hd)                 # inverse rotation
            if lq:
                w, gr = self._lora_w[(li, "qkv_proj")], self._lora_g[(li, "qkv_proj")]
                LO.lora_grad(dqkv, u_q[k], gr["B"], alpha=ls)
                LO.lora_down(dqkv, w["B"], rp, s_is_k_by_rp=True, alpha=ls, out=du)
                LO.lora_grad(n1[k], du, gr["A"], transposed=True)
            if li == 0:
                break                # everything below layer 0's qkv_proj is frozen
            T.linear_dx(dqkv, at.qkv_proj.weight, None, out=dn)
            if lq:
                LO.lora_up_add(dn, du, w["A"], s_is_rp_by_n=True)
            T.rmsnorm_bwd(hbuf[li], layer.input_layernorm.weight, dn, dh, dgain, layer.input_layernorm.variance_epsilon,
                          dres=dh_b, deterministic=det)                                  # dh (layer input)
        if f["acc_mode"] is not None:
            T.grad_accumulate(self._accumulators()[0], self.lora_bucket, f["acc_mode"])
        if f["exchange"] and self.world > 1 and not self.skip_allreduce:
            dist.all_reduce(self.lora_bucket)        # one small exchange per optimizer step

    def _neg_sin(self, prep):
        key = ("nsin", prep["rope"][1].data_ptr())
        if self._ws.get("nsin_key") != key:
            self._ws["nsin"] = (-prep["rope"][1]).contiguous()   # sign flip of a table: data prep, once per layout
            self._ws["nsin_key"] = key
        return self._ws["nsin"]

    def _mlp_bwd(self, prefix, mlp, dout, act_saved, pre_saved, x_in):
        """2-layer MLP (Linear, SiLU, Linear) backward: LVM/model.py:32-36."""
        g = self.grads
        T.matmul(dout, act_saved, out=g[f"{prefix}.mlp.2.weight"], ta=True)
        T.colsum(dout, g[f"{prefix}.mlp.2.bias"])
        dpre = T.act_bwd(pre_saved, T.matmul(dout, mlp[2].weight), ops.ACT_SILU)
        T.matmul(dpre, x_in, out=g[f"{prefix}.mlp.0.weight"], ta=True)
        T.colsum(dpre, g[f"{prefix}.mlp.0.bias"])

    def _patch_bwd(self, prefix, dtok, latents):
        g = self.grads
        patches = T.patchify(latents)
        T.matmul(dtok, patches, out=g[f"{prefix}.proj.weight"].view(-1, 16), ta=True)
        T.colsum(dtok, g[f"{prefix}.proj.bias"])

    # ------------------------------------------------------------------------------------------------
    def optimizer_step(self, micro_batches: int = 1):
        """sumsq, clip coefficient and AdamW on what the gradient buckets hold.  micro_batches: how many micro-batches were
        summed into them (step() passes gradient_accumulation_steps on the last micro-step): 1 / (world * micro_batches)
        is folded into the clip coefficient, so AdamW sees the mean gradient."""
        self._refuse_inside_ema_weights("optimizer_step")
        # an update still running on the optimizer's stream (overlap_optimizer) reads self.coef / self.sumsq and writes the
        # master weights and moments this call is about to touch: wait for it (free in the normal flow, where the forward of
        # the step that produced these gradients already waited for every layer's event)
        self.finish_optimizer()
        # AdamW writes the bf16 parameters through raw pointers (their autograd versions do not move): copies derived from
        # them (engine.folded_weights) are refilled by the next sampler call, which waits for this update first
        bump_weight_generation(self.model)
        lr = self.current_lr()
        self.last_lr = lr
        self.step_count += 1
        if self.lora_rank is not None:
            self._lora_optimizer_step(lr, *self.betas, micro_batches=micro_batches)
            return
        self.sumsq.zero_()
        for b in self.layer_buckets:
            T.sumsq(self._shard(b), self.sumsq)
        T.sumsq(self._shard(self.small_bucket), self.sumsq)
        partials = self.sumsq
        if self._sharded and not self.skip_allreduce:
            # every rank's sum over its reduced shards, in rank order, added on the device in a fixed order by clip_coef:
            # every rank computes the same norm and coefficient
            partials = SPM.all_gather_flat(self.sumsq, self._group, out=self._partials).view(-1)
        w = float(self.world // (self._sp["P"] if self._sp else 1) * micro_batches)     # data-parallel replicas x micro-batches
        # norm of the AVERAGED gradient = norm(sum)/world; coefficient already carries the 1/world factor (and 1/A, when the
        # buckets hold the sum over A micro-batches)
        T.clip_coef(partials, self.coef, self.grad_norm, (self.max_grad_norm or 0.0) * w, 1.0 / w)
        b1, b2 = self.betas
        if self._sharded:
            self._sharded_update(lr, b1, b2)
            return
        ema_l = self.ema_layers if self.use_ema else [None] * len(self.layer_buckets)
        ema_s = self.ema_small if self.use_ema else None
        if not self.overlap_optimizer:
            for i in range(len(self.layer_buckets)):
                self._adamw(self.master_layers[i], self.param_layers[i], self.layer_buckets[i], self.m_layers[i],
                            self.v_layers[i], ema_l[i], lr, b1, b2)
            self._adamw(self.master_small, self.param_small, self.small_bucket, self.m_small, self.v_small, ema_s,
                        lr, b1, b2)
            return
        # The update is a pure HBM stream (28 bytes per parameter) and the next step's forward is matrix work: they run side by
        # side.  Everything below goes to the optimizer's stream behind the clip coefficient; the small bucket (embeddings,
        # heads: read first) and then the layers in forward order, each followed by an event the next forward waits for right
        # where it first reads that layer.  Readers outside step() call finish_optimizer() first.
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(main)
        self._opt_stream.wait_event(ready)
        with torch.cuda.stream(self._opt_stream):
            self._adamw(self.master_small, self.param_small, self.small_bucket, self.m_small, self.v_small, ema_s,
                        lr, b1, b2)
            ev_small = torch.cuda.Event()
            ev_small.record(self._opt_stream)
            evs = []
            for i in range(len(self.layer_buckets)):
                self._adamw(self.master_layers[i], self.param_layers[i], self.layer_buckets[i], self.m_layers[i],
                            self.v_layers[i], ema_l[i], lr, b1, b2)
                e = torch.cuda.Event()
                e.record(self._opt_stream)
                evs.append(e)
        self._opt_events = (ev_small, evs)

    def _sharded_update(self, lr, b1, b2):
        """AdamW on this rank's shard of every bucket, each bucket's bf16 parameters all-gathered in place right behind its
        update: the small bucket first (embeddings and heads are read first), then the layers in forward order.  With
        overlap_optimizer on the optimizer's stream behind the clip coefficient with an event per bucket, as in the
        replicated update; the next forward waits for bucket i's event and gather where it first reads those parameters."""
        ov = self.overlap_optimizer
        if ov:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream())
            self._opt_stream.wait_event(ready)
        ema_l = self.ema_layers if self.use_ema else [None] * len(self.layer_buckets)
        ema_s = self.ema_small if self.use_ema else None
        buckets = [(self.master_small, self.param_small, self.small_bucket, self.m_small, self.v_small, ema_s)]
        buckets += list(zip(self.master_layers, self.param_layers, self.layer_buckets, self.m_layers, self.v_layers, ema_l))
        evs, works = [], []
        with torch.cuda.stream(self._opt_stream if ov else torch.cuda.current_stream()):
            for master, param, grad, m_, v_, ema in buckets:
                self._adamw(master, self._shard(param), self._shard(grad), m_, v_, ema, lr, b1, b2)
                works.append(None if self.skip_allreduce else
                             SPM.all_gather_flat(self._shard(param), self._group, out=param, async_op=True))
                if ov:
                    e = torch.cuda.Event()
                    e.record(self._opt_stream)
                    evs.append(e)
        self._opt_events = (evs[0], evs[1:]) if ov else None
        self._gathers = (works[0], works[1:])

    def finish_optimizer(self):
        """Makes the current stream wait for the update in flight (overlap_optimizer) and for the parameter all-gathers
        still running (dp_sharding="optimizer"): call before reading parameters or optimizer state outside step()
        (checkpoints, evaluation, the end of a timed region)."""
        if self._opt_events is not None:
            torch.cuda.current_stream().wait_event(self._opt_events[1][-1])
            self._opt_events = None
        if self._gathers is not None:
            for w in [self._gathers[0]] + self._gathers[1]:
                if w is not None:
                    w.wait()
            self._gathers = None


    # ---- checkpoints (LVM/train/train_x1_stage1_noiseinput.py:304-334,437-451: accelerate's checkpoint-{step}
    #      directories with auto-resume from the highest step).  Written with safetensors, nothing is unpickled on
    #      load: model.safetensors holds the bf16 state_dict under the reference's keys (loadable by
    #      LVM.from_pretrained), optimizer.safetensors the fp32 master weights and Adam moments per bucket. ----
    def _optimizer_tensors(self):
        """(tensor of this trainer, optimizer.safetensors key, unpadded bucket length) of every optimizer-state tensor; the
        tensor is this rank's shard when sharded, else the whole bucket."""
        pairs = [(self.master_small, "master_small", self._small_numel), (self.m_small, "m_small", self._small_numel),
                 (self.v_small, "v_small", self._small_numel)]
        for i, n in enumerate(self._bucket_numel):
            pairs += [(self.master_layers[i], f"master.{i}", n), (self.m_layers[i], f"m.{i}", n),
                      (self.v_layers[i], f"v.{i}", n)]
        return pairs

    def _ema_tensors(self):
        """_optimizer_tensors' triples of the EMA buffers (none without use_ema): ema_small / ema.{i} beside master.*."""
        if not self.use_ema:
            return []
        return [(self.ema_small, "ema_small", self._small_numel)] + \
               [(self.ema_layers[i], f"ema.{i}", n) for i, n in enumerate(self._bucket_numel)]

    def _schedule_record(self):
        return {"lr_scheduler": self.lr_scheduler, "lr_warmup_steps": self.lr_warmup_steps,
                "lr_num_training_steps": self.lr_num_training_steps, "lr_num_cycles": self.lr_num_cycles,
                "lr_power": self.lr_power, "gradient_accumulation_steps": self.accum_steps}

    # ---- EMA weights -------------------------------------------------------------------------------------------------
    def _ema_flat(self, t):
        """The whole (padded) fp32 EMA bucket of which `t` is this trainer's tensor: gathered when sharded (a collective:
        every rank calls)."""
        return SPM.all_gather_flat(t, self._group).view(-1) if self._sharded else t

    def _ema_buckets(self):
        """(EMA tensor, flat bf16 parameter buffer, parameter names in buffer order) per bucket, the small one first."""
        if not self.use_ema:
            raise VgptError("this trainer keeps no EMA (use_ema=False)")
        return [(self.ema_small, self.param_small, self.small_names)] + \
               list(zip(self.ema_layers, self.param_layers, self.layer_names))

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The EMA weights as a bf16 state dict under the reference's parameter keys (what train...py:440-447 saves from
        ema.state_dict()): every parameter is the fp32 EMA rounded once to bf16; entries of the model's state dict that
        are not trained parameters are copied as they are.  A sharded EMA is gathered (every rank calls)."""
        self.finish_optimizer()
        out = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for ema, _, names in self._ema_buckets():
            full = self._ema_flat(ema)
            o = 0
            for k in names:
                sz = self.params[k].numel()
                if k in out:
                    out[k] = full[o:o + sz].view(self.params[k].shape).to(BF16)
                o += sz
        return out

    def ema_weights(self):
        """Context manager for sampling from the EMA weights mid-training, built like merged_weights(): inside it the
        model's parameters hold bf16(EMA); on exit the training weights come back bit for bit.  The flat param_* buffers
        AdamW writes through raw pointers stay where they are: the values are copied in and out, nothing is re-pointed.
        Cached sampler engines refold on both edges (weight generation bumped).  Sharded: every rank enters together.
        Inside, step(update=True), optimizer_step() and save_checkpoint() raise: they would train on, or save, the EMA
        values as the model's weights, and the exit would then put stale training weights back.  Forward-only and
        stand-alone backward calls (update=False) are allowed: they evaluate the EMA weights.  Not re-entrant."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            buckets = self._ema_buckets()
            if self._ema_swapped:
                raise VgptError("ema_weights: already inside the context")
            self.finish_optimizer()
            saved = [param.detach().clone() for _, param, _ in buckets]
            self._ema_swapped = True
            try:
                with torch.no_grad():
                    for ema, param, _ in buckets:
                        param.copy_(self._ema_flat(ema))     # fp32 -> bf16, round to nearest even
                bump_weight_generation(self.model)
                yield self.model
            finally:
                with torch.no_grad():
                    for (_, param, _), sv_ in zip(buckets, saved):
                        param.copy_(sv_)
                self._ema_swapped = False
                bump_weight_generation(self.model)
        return cm()

    def _refuse_inside_ema_weights(self, what: str):
        if self._ema_swapped:
            raise VgptError(f"{what} inside ema_weights(): the model holds the EMA weights, not the training weights")

    def save_checkpoint(self, results_dir: str, global_step: Optional[int] = None) -> str:
        """Rank 0 writes (replicas are identical under data parallelism; a sharded optimizer state is gathered to it one
        bucket at a time through host memory, in the replicated layout); every rank returns after the files exist.
        With use_ema the optimizer file gains ema_small / ema.{i} and the directory ema.safetensors, the bf16
        ema_state_dict() (train...py:440-447).  In the middle of an accumulation cycle it raises: the accumulators are not
        part of a checkpoint, and the reference saves on cycle boundaries only (:437)."""
        self._refuse_inside_ema_weights("save_checkpoint")
        if self._micro != 0:
            raise VgptError(f"save_checkpoint in the middle of an accumulation cycle (micro-step {self._micro} of "
                            f"{self.accum_steps}): checkpoints are written on optimizer-step boundaries")
        self.finish_optimizer()
        import json
        import os
        from safetensors.torch import save_file
        step = self.step_count if global_step is None else int(global_step)
        path = os.path.join(results_dir, f"checkpoint-{step}")
        distributed = dist.is_available() and dist.is_initialized()
        writer = not distributed or dist.get_rank() == 0
        if self.lora_rank is not None:
            if writer:
                self._save_lora(path, step)
            if distributed:
                dist.barrier()
            return path
        opt = {}
        ema_sd = self.ema_state_dict() if self.use_ema else None     # gathers when sharded: every rank takes part
        for t, key, n in self._optimizer_tensors() + self._ema_tensors():
            if self._sharded:     # every rank takes part; one gathered bucket on the device at a time, then host memory
                full = SPM.all_gather_flat(t, self._group).view(-1)[:n]
                if writer:
                    opt[key] = full.cpu()
                del full
            elif writer:
                opt[key] = t.detach().cpu().contiguous()
        if writer:
            os.makedirs(path, exist_ok=True)
            save_file({k: v.detach().cpu().contiguous() for k, v in self.model.state_dict().items()},
                      os.path.join(path, "model.safetensors"))
            save_file(opt, os.path.join(path, "optimizer.safetensors"))
            if ema_sd is not None:
                save_file({k: v.detach().cpu().contiguous() for k, v in ema_sd.items()}, os.path.join(path, "ema.safetensors"))
            with open(os.path.join(path, "trainer_state.json"), "w") as f:
                json.dump({"step_count": self.step_count, "global_step": step, "lr": self.lr, "weight_decay": self.wd,
                           "betas": list(self.betas), "eps": self.eps, **self._schedule_record(),
                           "use_ema": self.use_ema, "ema_decay": self.ema_decay, "small_names": self.small_names}, f)
        if distributed:
            dist.barrier()
        return path

    def load_checkpoint(self, path: str, restore_hyperparameters: bool = True) -> int:
        """Restores parameters, fp32 master weights, Adam moments, the step counter and (by default) the optimizer
        hyper-parameters and LR schedule; returns the global step.  Everything is validated before anything is copied.
        The optimizer state is stored unpadded and unsharded: a sharded trainer copies its own slice, so checkpoints move
        between dp_sharding modes and world sizes.  Only checkpoints written by this trainer resume (the reference's are accelerate / DeepSpeed `save_state`
        directories, whose optimizer shards are pickles: warm-start from those through LVM.from_pretrained's weight
        loaders instead).  EMA: a checkpoint without EMA tensors loaded into a use_ema trainer starts the EMA as a copy of
        the loaded master weights (recorded in `self.last_load["ema"]` and logged); an EMA checkpoint loaded into a trainer
        without EMA ignores them.  The checkpoint's gradient_accumulation_steps is a record only: resuming with another
        value is allowed, the optimizer state does not depend on it.  An accumulation cycle under way is dropped."""
        self.finish_optimizer()
        import json
        import os
        from safetensors.torch import load_file
        with open(os.path.join(path, "trainer_state.json")) as f:
            st = json.load(f)
        if (self.lora_rank is not None) != ("lora" in st):
            raise VgptError(f"{path}: a LoRA checkpoint resumes a LoRA trainer and a full one a full trainer")
        self._refuse_inside_ema_weights("load_checkpoint")
        if self.lora_rank is not None:
            self._load_lora(path, st)
            self.last_load = {"ema": "none"}
            return self._restore_record(st, restore_hyperparameters)
        if st["small_names"] != self.small_names:
            raise VgptError("checkpoint was written for a different parameter layout")
        opt = load_file(os.path.join(path, "optimizer.safetensors"))
        pairs = self._optimizer_tensors()
        ema_pairs = self._ema_tensors()
        ema_in_file = bool(ema_pairs) and any(k in opt for _, k, _ in ema_pairs)
        if ema_in_file:
            pairs = pairs + ema_pairs                    # validated and copied like the rest
        model_sd = load_file(os.path.join(path, "model.safetensors"))
        own = self.model.state_dict()
        problems = [f"optimizer tensor {k} missing" for _, k, _ in pairs if k not in opt]
        problems += [f"optimizer tensor {k}: shape {tuple(opt[k].shape)} != {(n,)}" for _, k, n in pairs
                     if k in opt and tuple(opt[k].shape) != (n,)]
        problems += [f"model tensor {k} missing" for k in own if k not in model_sd]
        problems += [f"model tensor {k}: shape {tuple(model_sd[k].shape)} != {tuple(v.shape)}" for k, v in own.items()
                     if k in model_sd and model_sd[k].shape != v.shape]
        if problems:
            raise VgptError(f"{path}: checkpoint does not match this trainer: " + "; ".join(problems[:8]))
        for dst, key, _ in pairs:
            if not self._sharded:
                dst.copy_(opt[key])
                continue
            lo = self.rank * dst.numel()                 # this rank's slice; the zero padding past the bucket stays zero
            hi = min(lo + dst.numel(), opt[key].numel())
            dst.zero_()
            if hi > lo:
                dst[:hi - lo].copy_(opt[key][lo:hi])
        self.last_load = {"ema": "none" if not ema_pairs else "restored" if ema_in_file else "initialised from master"}
        if ema_pairs and not ema_in_file:
            import logging
            for ema, master in zip([self.ema_small] + self.ema_layers, [self.master_small] + self.master_layers):
                ema.copy_(master)
            logging.getLogger(__name__).warning("%s holds no EMA tensors: the EMA starts as a copy of the loaded master weights",
                                                path)
        with torch.no_grad():     # parameters are views of the flat bf16 buffers: copy in place, keep the views
            for k, p_ in own.items():
                p_.copy_(model_sd[k])
        bump_weight_generation(self.model)
        return self._restore_record(st, restore_hyperparameters)

    def _restore_record(self, st, restore_hyperparameters: bool) -> int:
        self.step_count = int(st["step_count"])
        self._micro = 0
        if restore_hyperparameters:
            self.lr, self.wd, self.eps = float(st["lr"]), float(st["weight_decay"]), float(st["eps"])
            self.betas = tuple(st["betas"])
            self.lr_scheduler = st.get("lr_scheduler", self.lr_scheduler)
            self.lr_warmup_steps = int(st.get("lr_warmup_steps", self.lr_warmup_steps))
            self.lr_num_training_steps = st.get("lr_num_training_steps", self.lr_num_training_steps)
            self.lr_num_cycles = st.get("lr_num_cycles", self.lr_num_cycles)
            self.lr_power = float(st.get("lr_power", self.lr_power))
        return int(st["global_step"])

    # LoRA mode: peft's adapter directory (adapter_model.safetensors + adapter_config.json; layout written from knowledge of
    # peft's format, parity unpinned: DESIGN.md §6a) next to this trainer's own optimizer.safetensors / trainer_state.json
    def _save_lora(self, path: str, step: int):
        import json
        import os
        from safetensors.torch import save_file
        from .lora import adapter_config
        os.makedirs(path, exist_ok=True)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.lora.items()}, os.path.join(path, "adapter_model.safetensors"))
        with open(os.path.join(path, "adapter_config.json"), "w") as f:
            json.dump(adapter_config(self.lora_rank, self.lora_alpha, self.lora_targets), f, indent=2)
        save_file({"lora_master": self.lora_master.cpu(), "lora_m": self.lora_m.cpu(), "lora_v": self.lora_v.cpu()},
                  os.path.join(path, "optimizer.safetensors"))
        with open(os.path.join(path, "trainer_state.json"), "w") as f:
            json.dump({"step_count": self.step_count, "global_step": step, "lr": self.lr, "weight_decay": self.wd,
                       "betas": list(self.betas), "eps": self.eps, **self._schedule_record(),
                       "lora": {"r": self.lora_rank, "rp": self.lora_rp, "lora_alpha": self.lora_alpha,
                                "target_modules": list(self.lora_targets), "numel": self._lora_numel}}, f)

    def _load_lora(self, path: str, st):
        import os
        from safetensors.torch import load_file
        from .lora import load_adapter
        rec = st["lora"]
        mine = {"r": self.lora_rank, "rp": self.lora_rp, "target_modules": list(self.lora_targets), "numel": self._lora_numel}
        diff = {k: (rec.get(k), v) for k, v in mine.items() if rec.get(k) != v}
        if diff:
            raise VgptError(f"{path}: checkpoint does not match this trainer's adapters (checkpoint, trainer): {diff}")
        cfg, tensors = load_adapter(path)
        opt = load_file(os.path.join(path, "optimizer.safetensors"))
        problems = [f"adapter tensor {k} missing" for k in self.lora if k not in tensors]
        problems += [f"adapter tensor {k}: shape {tuple(tensors[k].shape)} != {tuple(v.shape)}" for k, v in self.lora.items()
                     if k in tensors and tensors[k].shape != v.shape]
        problems += [f"optimizer tensor {k} missing or mis-sized" for k in ("lora_master", "lora_m", "lora_v")
                     if k not in opt or opt[k].numel() != self._lora_numel]
        if problems:
            raise VgptError(f"{path}: checkpoint does not match this trainer: " + "; ".join(problems[:8]))
        for k, v in self.lora.items():
            v.copy_(tensors[k])
        if not self.forward_only:
            self.lora_master.copy_(opt["lora_master"]); self.lora_m.copy_(opt["lora_m"]); self.lora_v.copy_(opt["lora_v"])
        self.lora_alpha = float(cfg["lora_alpha"])
        self.lora_scale = self.lora_alpha / self.lora_rank

    def auto_resume(self, results_dir: str) -> Optional[int]:
        """Load the checkpoint-{N} with the largest N under results_dir, if any (train...stage1.py:304-315)."""
        import glob
        import os
        found = [d for d in glob.glob(os.path.join(results_dir, "checkpoint-*")) if d.rsplit("-", 1)[-1].isdigit()]
        if not found:
            return None
        return self.load_checkpoint(max(found, key=lambda d: int(d.rsplit("-", 1)[-1])))


def batch_ntok(sizes) -> int:
    ns = {e - s for v in sizes.values() for s, e in v}
    if len(ns) != 1:
        raise VgptError("Stage1Trainer needs frames of one resolution")
    return ns.pop()
