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
    gradient buckets hold partial sums over the share that the data-parallel exchange adds up;
  * skip_bad_steps=True drops a step whose gradient norm is not finite (or exceeds skip_grad_norm_above) on the device: the
    clip kernel writes a verdict, the AdamW launches read it and do nothing, the host learns of it one step later
    (what the reference gets from DeepSpeed's overflow check).
"""
from __future__ import annotations

import json
import math
import os
import weakref
from types import SimpleNamespace
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
SKIP_REASONS = {0: None, 1: "nonfinite", 2: "grad_norm"}       # verdict[1] of vgpt_clip_coef_guarded


def check_guard_arguments(skip_bad_steps, skip_grad_norm_above, forward_only: bool = False):
    """Stage1Trainer's refusals of skip_bad_steps / skip_grad_norm_above, on the arguments alone (no model, no device);
    returns the threshold as a float, or None."""
    if skip_grad_norm_above is not None:
        thr = skip_grad_norm_above
        if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not (0.0 < float(thr) < math.inf):
            raise VgptError(f"skip_grad_norm_above {thr!r}: expected a positive finite norm (or None)")
        if not skip_bad_steps:
            raise VgptError(f"skip_grad_norm_above {thr!r} without skip_bad_steps=True: the threshold is part of the guarded "
                            "step")
    if skip_bad_steps and forward_only:
        raise VgptError("skip_bad_steps with forward_only: there is no optimizer step to skip, the guard of a forward-only "
                        "trainer is not built")
    return None if skip_grad_norm_above is None else float(skip_grad_norm_above)


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


class _Bucket:
    """One gradient bucket and everything the optimizer keeps for it.  key: "small", a decoder layer's index, or "lora";
    names: its tensors in buffer order; numel: its unpadded length (the checkpoint layout); grad / param: the flat buffers
    (zero-padded when sharded); master / m / v / ema: fp32 state, this rank's shard when sharded; acc: the fp32
    accumulator of gradient accumulation.  What a mode does not have is None."""
    __slots__ = ("key", "names", "numel", "grad", "param", "master", "m", "v", "ema", "acc")

    def __init__(self, key, names, numel):
        self.key, self.names, self.numel = key, names, numel
        self.grad = self.param = self.master = self.m = self.v = self.ema = self.acc = None


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
                 deterministic: bool = False, skip_bad_steps: bool = False, skip_grad_norm_above: Optional[float] = None):
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
        (DESIGN.md §6d).  Composes with every other option; nothing to do in a forward-only trainer.
        skip_bad_steps / skip_grad_norm_above (the overflow check of the reference's DeepSpeed optimizer,
        which this trainer's own kernels replaced): an optimizer step whose global gradient norm is NaN or Inf -- or, with
        a threshold, whose norm of the MEAN gradient over ranks and micro-batches (the quantity max_grad_norm clips)
        exceeds skip_grad_norm_above -- is dropped on the device and leaves no trace: masters, moments, EMA, parameters,
        step_count, the AdamW bias-correction step and the LR schedule position stay where they were (all three count
        APPLIED steps).  The verdict is taken by the clip kernel from the one sum of squares every rank already agrees on
        bit for bit (no new collective, no extra pass over the gradients) and read by the AdamW launches on the device;
        the host copies it to pinned memory behind an event and looks at it when it issues the next optimizer stage, or
        when step_count, current_lr(), skipped_steps, last_step_skipped, last_skip_reason or save_checkpoint() is
        asked: no device-wide synchronisation inside step().  On good data the guarded run is bit-identical to the
        unguarded one.  bucket_grad_norms() and nonfinite_report() say where a bad step came from.  Refused on a
        forward-only trainer; the threshold is positive, finite and needs skip_bad_steps=True."""
        self.skip_grad_norm_above = check_guard_arguments(skip_bad_steps, skip_grad_norm_above, forward_only)   # before anything is touched
        self.skip_bad_steps = bool(skip_bad_steps)
        self._skipped, self._last_skipped, self._last_reason = 0, False, None
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
        if not forward_only and not T.attention_bwd_supported(self.cfg.head_dim):
            raise VgptError(f"Stage1Trainer: head_dim {self.cfg.head_dim} cannot train: the attention backward is built for "
                            f"head dims 64, 96 and 128 (a forward-only trainer needs no backward)")
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
        self.buckets: List[_Bucket] = []      # update / read order: the small bucket, then layers 0 .. L-1; LoRA: the one
        #                                       adapter bucket; none in a forward-only trainer
        self.lora_rank = None
        self.lora: Dict[str, torch.Tensor] = {}
        if lora_rank is not None:
            self._init_lora(int(lora_rank), lora_alpha, tuple(lora_target_modules))
            return
        if forward_only:
            return
        # ---- one record per gradient bucket: a flat bf16 bucket per decoder layer + one fp32 bucket for the rest ----
        self.layer_names = [[f"llm.layers.{i}.self_attn.qkv_proj.weight", f"llm.layers.{i}.self_attn.o_proj.weight",
                             f"llm.layers.{i}.mlp.gate_up_proj.weight", f"llm.layers.{i}.mlp.down_proj.weight"]
                            for i in range(self.cfg.num_hidden_layers)]
        big = {k for names in self.layer_names for k in names}
        self.small_names = [k for k in self.params if k not in big]
        layers = [self._make_bucket(i, names, BF16) for i, names in enumerate(self.layer_names)]
        self.buckets = [self._make_bucket("small", self.small_names, F32)] + layers     # update / read order
        # ---- optimizer state (fp32 master + moments) and flat parameters per bucket, so AdamW is one launch per bucket.
        #      The order of these allocations is kept as it was: where the buffers come to lie moves the full-size step by
        #      about 1 % (profiles/trainer_refactor_step_time.log).  Sharded, the parameters go first: the master is taken
        #      from this rank's shard of the flat parameters, so no full-length fp32 temporary is made, which at full size
        #      would be the replicated state that mode avoids ----
        order = layers + self.buckets[:1]
        if self._sharded:
            self._flatten_params(order)
        for b in order:
            b.master = (self._shard(b.param).to(F32, copy=True) if self._sharded else
                        torch.cat([self.params[k].detach().reshape(-1).to(F32) for k in b.names]))
        for kind in ("m", "v"):
            for b in layers:
                setattr(b, kind, torch.zeros_like(b.master))
        self.buckets[0].m, self.buckets[0].v = (torch.zeros_like(self.buckets[0].master) for _ in range(2))
        if not self._sharded:
            self._flatten_params(order)
        bump_weight_generation(model)     # storage re-pointed; from here on the optimizer writes it through raw pointers
        self._init_scalars()
        self._init_ema()
        if self._sharded:
            self._partials = torch.zeros(self.world, dtype=F32, device=self.dev)   # every rank's sum of squares, rank order
        # the names the records' tensors go by (bench.py, scripts/, tests): made once, the tensors are never rebound
        small, layers = self.buckets[0], self.buckets[1:]
        self.small_bucket, self.param_small, self.master_small = small.grad, small.param, small.master
        self.m_small, self.v_small, self.ema_small, self._small_numel = small.m, small.v, small.ema, small.numel
        self.layer_buckets, self.param_layers = [b.grad for b in layers], [b.param for b in layers]
        self.master_layers, self.m_layers, self.v_layers = ([getattr(b, k) for b in layers] for k in ("master", "m", "v"))
        self.ema_layers = [b.ema for b in layers] if self.use_ema else None
        self._bucket_numel = [b.numel for b in layers]       # unpadded lengths of the layer buckets: the checkpoint layout

    def _flatten(self, tensors, dtype, fill: bool):
        """One flat buffer, zero-padded to the shard partition when sharded, that holds `tensors` end to end (their values
        when `fill`, else zeros), and the views of it in their shapes."""
        flat = torch.zeros(self._padded(sum(t.numel() for t in tensors)), dtype=dtype, device=self.dev)
        views, o = [], 0
        for t in tensors:
            views.append(flat[o:o + t.numel()].view(t.shape))
            if fill:
                views[-1].copy_(t.detach())
            o += t.numel()
        return flat, views

    def _make_bucket(self, key, names, grad_dtype) -> _Bucket:
        """The record of one bucket and its flat gradient buffer, of which the gradients of `names` become views: the
        exchange and the clip's sum of squares are one launch per bucket."""
        ps = [self.params[k] for k in names]
        b = _Bucket(key, names, sum(p.numel() for p in ps))
        b.grad, views = self._flatten(ps, grad_dtype, fill=False)
        self.grads.update(zip(names, views))
        return b

    def _flatten_params(self, buckets):
        """The model's parameters become views of one flat buffer per bucket, which the optimizer writes in one launch."""
        for b in buckets:
            ps = [self.params[k] for k in b.names]
            b.param, views = self._flatten(ps, ps[0].dtype, fill=True)
            for p, v in zip(ps, views):
                p.data = v

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
            self._lora_sizes = [shape[0] * shape[1] for *_, shape in slots]      # padded slot lengths, the bucket's layout
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
            b = _Bucket("lora", list(self.lora), o)
            b.grad, b.param, b.master, b.m, b.v = self.lora_bucket, self.lora_param, self.lora_master, self.lora_m, self.lora_v
            self.buckets = [b]
            self._init_scalars()

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
            for b in self.buckets[1:] + self.buckets[:1]:      # allocation order kept, like the rest of the state (__init__)
                b.ema = b.master.clone()

    def _adamw(self, master, param, grad, m_, v_, ema, lr, b1, b2):
        """One AdamW launch over a flat bucket; with an EMA buffer the launch that also moves it (no second pass)."""
        if ema is None:
            T.adamw_step(master, param, grad, m_, v_, lr, b1, b2, self.eps, self.wd, self.step_count, self.coef)
        else:
            T.adamw_ema_step(master, param, grad, m_, v_, lr, b1, b2, self.eps, self.wd, self.step_count, self.coef, ema,
                             self.ema_decay)

    def _adamw_guarded(self, master, param, grad, m_, v_, ema, lr, b1, b2):
        """_adamw behind the verdict of this step's clip kernel.  The step number is the host's count as if this step
        applies (_step_count, read without resolving the verdict in flight): a skipped launch never looks at it."""
        if ema is None:
            T.adamw_step_guarded(master, param, grad, m_, v_, lr, b1, b2, self.eps, self.wd, self._step_count, self.coef,
                                 self._verdict)
        else:
            T.adamw_ema_step_guarded(master, param, grad, m_, v_, lr, b1, b2, self.eps, self.wd, self._step_count, self.coef,
                                     ema, self.ema_decay, self._verdict)

    # ---- guarded step: the verdict in flight and what the host knows of it ---------------------------
    _pending = None      # event behind the copy of the last verdict to pinned memory; None: nothing to resolve

    @property
    def step_count(self) -> int:
        """Optimizer steps APPLIED so far (skipped ones do not count): the AdamW bias-correction step and, times
        lr_scheduler_steps_per_optimizer_step, the position of the LR schedule."""
        self._resolve_verdict()
        return self._step_count

    @step_count.setter
    def step_count(self, value):
        self._resolve_verdict()
        self._step_count = value

    def _resolve_verdict(self):
        """Waits for the EVENT behind the last verdict copy (not for the device) and takes a skipped step back out of the
        host's count.  A no-op unless a guarded optimizer stage was issued since the last call."""
        ev = self._pending
        if ev is None:
            return
        self._pending = None
        ev.synchronize()
        skip, reason = (int(x) for x in self._verdict_host.tolist())
        self._last_skipped, self._last_reason = bool(skip), SKIP_REASONS[reason]
        if skip:
            self._step_count -= 1
            self._skipped += 1

    @property
    def skipped_steps(self) -> int:
        """Optimizer steps dropped by the guard since construction (or since the checkpoint this trainer resumed)."""
        self._resolve_verdict()
        return self._skipped

    @property
    def last_step_skipped(self) -> bool:
        self._resolve_verdict()
        return self._last_skipped

    @property
    def last_skip_reason(self) -> Optional[str]:
        """None (the last optimizer step was applied), "nonfinite" or "grad_norm"."""
        self._resolve_verdict()
        return self._last_reason

    def _sumsq_order(self) -> List[_Bucket]:
        """The buckets in the order their sums of squares are added: the layers, then the small bucket."""
        return self.buckets[1:] + self.buckets[:1]

    def bucket_grad_norms(self) -> Dict[object, float]:
        """{bucket key: norm of what this rank's bucket (its shard when sharded) held at the last optimizer stage}, in the
        order the sums are added (layers 0 .. L-1, then "small"; LoRA: "lora").  Each norm is the float64 square root of
        the fp32 sum vgpt_sumsq_keep stored, so float32(norm ** 2) is that sum again and adding those in this order, in
        fp32, gives trainer.sumsq bit for bit.  Needs skip_bad_steps=True (the unguarded step keeps no per-bucket sums)."""
        if not self.skip_bad_steps:
            raise VgptError("bucket_grad_norms: per-bucket sums are kept by the guarded step only (skip_bad_steps=True)")
        parts = self._bucket_sumsq.tolist()
        return {b.key: (math.sqrt(x) if x >= 0.0 else math.nan) for b, x in zip(self._sumsq_order(), parts)}

    def nonfinite_report(self):
        """[(parameter name, number of NaN, number of +-Inf), ...] of what this rank's gradient buckets hold NOW, tensors
        with a non-zero count only (LoRA: the adapter slots, rank padding included), through vgpt_count_nonfinite with the
        buckets' tensor offsets.  A diagnostic for after a skip: one pass over the buckets and a read-back."""
        if not self.buckets:
            raise VgptError("nonfinite_report: a forward-only trainer has no gradient buckets")
        out = []
        for b in self.buckets:
            off = self._ws.get(("nf_off", b.key))
            if off is None:
                sizes = self._lora_sizes if b.key == "lora" else [self.params[k].numel() for k in b.names]
                edges = [0]
                for n in sizes:
                    edges.append(edges[-1] + n)
                off = self._ws[("nf_off", b.key)] = torch.tensor(edges, dtype=torch.int64, device=self.dev)
            counts = T.count_nonfinite(b.grad, off).tolist()
            out += [(k, n_nan, n_inf) for k, (n_nan, n_inf) in zip(b.names, counts) if n_nan or n_inf]
        return out

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
        """Allocates every bucket's fp32 accumulator on first use; `_acc` is (small | lora, [layer 0 .. nl-1]) of them."""
        if self._acc is None:
            for b in self.buckets:
                b.acc = torch.empty(b.grad.numel(), dtype=F32, device=self.dev)
            self._acc = (self.buckets[0].acc, [b.acc for b in self.buckets[1:]])
        return self._acc

    def _init_scalars(self):
        self.sumsq = torch.zeros(1, dtype=F32, device=self.dev)
        self.coef = torch.ones(1, dtype=F32, device=self.dev)
        self.grad_norm = torch.zeros(1, dtype=F32, device=self.dev)
        if self.skip_bad_steps:
            self._verdict = torch.zeros(2, dtype=torch.int32, device=self.dev)         # {skip?, reason}, written by the clip kernel
            self._verdict_host = torch.zeros(2, dtype=torch.int32).pin_memory()
            self._bucket_sumsq = torch.zeros(len(self.buckets), dtype=F32, device=self.dev)   # per bucket, _sumsq_order()

    # ---- dp_sharding="optimizer" -----------------------------------------------------------------------------------
    def _padded(self, n: int) -> int:
        return shard_partition(n, self.world)[0] if self._sharded else n

    def _shard(self, flat: torch.Tensor) -> torch.Tensor:
        """This rank's contiguous slice of a padded flat bucket (the whole bucket when not sharded)."""
        if not self._sharded:
            return flat
        s = flat.numel() // self.world
        return flat[self.rank * s:(self.rank + 1) * s]

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
    def for_evaluation(cls, model, deterministic: bool = False, skip_bad_steps: bool = False,
                       skip_grad_norm_above: Optional[float] = None):
        """A forward-only trainer cached on the model (no gradient buckets, no optimizer state; `deterministic` is kept on
        a new one and changes nothing: the forward pass has no order-dependent sum).  skip_bad_steps /
        skip_grad_norm_above are refused: there is no optimizer step to guard."""
        check_guard_arguments(skip_bad_steps, skip_grad_norm_above, forward_only=True)
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
        if self._sp is not None and self.check_sp_inputs:
            self._check_sp_batch(batch, x1, t)
        f = self._begin_step(batch, x1, x0, t, clean, x0_in, t_in)
        self._assemble_sequence(f)
        self._decoder_forward(f)
        loss = self._heads_and_loss(f, input_output_return)
        if self.forward_only or not backward:
            if update:
                raise VgptError("Stage1Trainer.step: an optimizer step needs the backward pass")
            return loss
        acc_mode = self._accum_mode(update)
        self._exchange(self._backward(f, acc_mode), acc_mode)
        if update:
            self._finish_micro_step(acc_mode)
        return loss

    # ---- the phases of step(), in order.  `f` is the record the forward phases fill and the backward reads: shapes, the
    #      saved activation buffers, the head intermediates and, under sequence parallelism, this rank's share ----
    def _begin_step(self, batch, x1, x0, t, clean, x0_in, t_in):
        """Prepare: row layout of the batch, shapes, the noised latents, and the share of a sequence-parallel rank."""
        cfg, sp = self.cfg, self._sp
        prep = self._prepare(batch)
        # the previous step's update may still be running on its own stream, its all-gathers (sharded) still in flight
        self._await_params(-1)               # embeddings, heads, final norm: read from the start
        f = SimpleNamespace(prep=prep, sp=sp, B=prep["B"], L=prep["L"], M=prep["B"] * prep["L"], H=cfg.hidden_size,
                            I=cfg.intermediate_size, nq=cfg.num_attention_heads, nk=cfg.num_key_value_heads, hd=cfg.head_dim,
                            nl=cfg.num_hidden_layers, ntok=prep["ntok"], ck=self.gradient_checkpointing, clean=clean)
        f.nf, f.C, f.h, f.w = x1.shape
        f.x1 = x1.to(self.dev, F32).contiguous(); x0 = x0.to(self.dev, F32).contiguous()
        f.t = t.to(self.dev, F32).contiguous()
        f.xt = T.lerp_frames(f.x1, x0, f.t, self._buf("xt", tuple(x1.shape)))
        f.cl = None
        if clean is not None and clean.shape[0] > 0:
            f.cl = T.lerp_frames(clean.to(self.dev, F32).contiguous(), x0_in.to(self.dev, F32).contiguous(),
                                 t_in.to(self.dev, F32).contiguous(), self._buf("cl", tuple(clean.shape)))
        # sequence parallelism: this rank runs rows [r0, r1) of the one packed sequence (Ms of the M rows) through the
        # row-local work and its nq / P heads (Wl fused q|k|v columns, dc context columns) through attention over all rows
        f.r0, f.r1, f.Ms, f.rope = 0, f.M, f.M, prep["rope"]
        if sp is not None:
            P = sp["P"]
            f.shares, _ = sp_shares(f.M, P)
            f.sizes = sizes = [e_ - a_ for a_, e_ in f.shares]
            f.r0, f.r1 = f.shares[sp["r"]]
            f.Ms, f.Wl, f.dc = f.r1 - f.r0, (f.nq + 2 * f.nk) // P * f.hd, f.nq // P * f.hd
            f.rope = tuple(t_.view(-1, f.hd // 2)[f.r0:f.r1] for t_ in prep["rope"])
            # split lists of the four exchanges per layer: rows go to the ranks that own the heads and back
            f.by_sender = [[n * f.Wl] * P for n in sizes]                 # every rank sends its rows to every rank
            f.by_owner = [[n * f.dc for n in sizes] for _ in range(P)]    # every rank sends each rank that rank's rows
            f.ctx_by_sender = [[n * f.dc] * P for n in sizes]
            f.qkv_by_owner = [[n * f.Wl for n in sizes] for _ in range(P)]
        f.lq = self.lora_rank is not None and "qkv_proj" in self.lora_targets
        f.lo = self.lora_rank is not None and "o_proj" in self.lora_targets
        return f

    def _assemble_sequence(self, f):
        """The decoder's input rows: token embeddings, condition and noised patches, the time token.  Cheap, so it runs on
        all rows on every rank; a sequence-parallel share is a copy of its rows."""
        m, prep, H = self.model, f.prep, f.H
        f.hbuf = self._buf("h", (f.nl + 1, f.Ms, H))         # layer inputs (h[l]) and the last output
        seq = f.hbuf[0] if f.sp is None else self._buf("seq_all", (f.M, H))
        ops.embed_gather(prep["ids"], m.llm.embed_tokens.weight, out=seq.view(f.B, f.L, H))
        pos = m.pos_embed[0]
        if f.cl is not None:
            ops.patch_embed(f.cl, m.input_x_embedder.proj.weight, m.input_x_embedder.proj.bias, pos, prep["c_rows"], seq,
                            m.pos_embed_max_size)
        f.sin = ops.timestep_sinusoid(f.t, m.time_token.freqs(self.dev))
        tt = m.time_token.mlp
        f.tt_pre = ops.linear_small(f.sin, tt[0].weight, tt[0].bias)
        f.tt_act = T.act_fwd(f.tt_pre, ops.ACT_SILU)
        ops.linear_small(f.tt_act, tt[2].weight, tt[2].bias, out=seq, out_row=prep["t_rows"], ldo=H)
        ops.patch_embed(f.xt, m.x_embedder.proj.weight, m.x_embedder.proj.bias, pos, prep["x_rows"], seq,
                        m.pos_embed_max_size)
        if f.sp is not None:
            f.hbuf[0].copy_(seq[f.r0:f.r1])

    def _decoder_forward(self, f):
        """Every decoder layer, keeping what the backward reads: every layer's activations (normal) or ONE layer's worth,
        recomputed per layer in the backward (checkpointing)."""
        B, L, M, Ms, H, I, nq, nk, hd = f.B, f.L, f.M, f.Ms, f.H, f.I, f.nq, f.nk, f.hd
        ns = 1 if f.ck else f.nl
        f.n1 = self._buf("n1", (ns, Ms, H))
        f.ctx = self._buf("ctx", (ns, Ms, nq * hd)); f.h2 = self._buf("h2", (ns, Ms, H)); f.n2 = self._buf("n2", (ns, Ms, H))
        f.gu = self._buf("gu", (ns, Ms, 2 * I)); f.act = self._buf("act", (ns, Ms, I))
        if f.sp is None:
            f.qkv = self._buf("qkv", (ns, M, (nq + 2 * nk) * hd))
            f.lse = self._buf("lse", (ns, B, nq, L), F32)
        else:
            # kept per layer: the fused q|k|v rows of EVERY rank for this rank's heads, their context and lse; the share's
            # own q|k|v rows of all heads ("qkv") and the exchange buffers are transient
            P = f.sp["P"]
            f.qkv = self._buf("qkv", (Ms, (nq + 2 * nk) * hd))
            f.qkv_h = self._buf("qkv_heads", (ns, M, f.Wl)); f.ctx_h = self._buf("ctx_heads", (ns, M, f.dc))
            f.lse = self._buf("lse", (ns, 1, nq // P, M), F32)
            f.send = self._buf("sp_send", (P, Ms, f.Wl)); f.ctx_recv = self._buf("sp_ctx_recv", (P, Ms, f.dc))
        if self.lora_rank is not None:      # u = x A^T of both adapted projections, saved like the other activations
            f.u_q = self._buf("u_q", (ns, M, self.lora_rp)); f.u_o = self._buf("u_o", (ns, M, self.lora_rp))
        for li in range(f.nl):
            self._layer_forward(f, li)

    def _layer_forward(self, f, li, with_output=True):
        """Decoder layer li; the checkpointing backward calls it again with with_output=False."""
        layer = self.model.llm.layers[li]
        at, mlp, k = layer.self_attn, layer.mlp, 0 if f.ck else li
        self._await_params(li)           # this layer's parameters are updated (and gathered)
        ops.rmsnorm(f.hbuf[li], layer.input_layernorm.weight, layer.input_layernorm.variance_epsilon, out=f.n1[k])
        self._attention_forward(f, li, k)
        ops.linear(f.ctx[k], at.o_proj.weight, residual=f.hbuf[li], out=f.h2[k])
        if f.lo:
            ao = self._lora_w[(li, "o_proj")]
            LO.lora_down(f.ctx[k], ao["A"], self.lora_rp, out=f.u_o[k])
            LO.lora_up_add(f.h2[k], f.u_o[k], ao["B"], alpha=self.lora_scale)
        ops.rmsnorm(f.h2[k], layer.post_attention_layernorm.weight, layer.post_attention_layernorm.variance_epsilon,
                    out=f.n2[k])
        # gate_up_proj + act(gate) * up in one kernel that also keeps the bf16 [gate | up] for the backward: bit for bit
        # ops.linear(n2, W) followed by T.silu_mul_fwd (tests/test_train_gpu.py), without the (M, 2I) round trip
        ops.gated_mlp_act(f.n2[k], mlp.gate_up_proj.weight, mlp.act, out=f.act[k], gate_up_out=f.gu[k])
        if with_output:
            ops.linear(f.act[k], mlp.down_proj.weight, residual=f.h2[k], out=f.hbuf[li + 1])

    def _attention_forward(self, f, li, k):
        """n1[k] -> ctx[k]: qkv_proj + RoPE, (pack, exchange,) attention (, exchange, unpack)."""
        at, sp, pm = self.model.llm.layers[li].self_attn, f.sp, f.prep["pm"]
        B, L, M, nq, nk, hd = f.B, f.L, f.M, f.nq, f.nk, f.hd
        qkv = f.qkv[k] if sp is None else f.qkv
        if f.lq:        # plain base GEMM, then y += s (x A^T) B^T and the rotation in one pass over y
            aq = self._lora_w[(li, "qkv_proj")]
            ops.linear(f.n1[k], at.qkv_proj.weight, out=qkv)
            LO.lora_down(f.n1[k], aq["A"], self.lora_rp, out=f.u_q[k])
            LO.lora_up_add(qkv, f.u_q[k], aq["B"], alpha=self.lora_scale, rope=(f.rope[0], f.rope[1], nq, nk, hd))
        else:
            ops.linear_qkv_rope(f.n1[k], at.qkv_proj.weight, f.rope[0], f.rope[1], nq, nk, hd, out=qkv)
        if sp is None:
            T.attention_qkv_train(qkv.view(B, L, -1), pm, nq, nk, hd, f.ctx[k].view(B, L, -1), f.lse[k])
            return
        # engine.StaticDenoiser._sp_attention with the training forward's kernel
        P = sp["P"]
        ops.sp_pack_qkv(qkv, P, nq, nk, hd, out=f.send)
        SPM.exchange_split(f.send, f.qkv_h[k], f.by_sender, sp["group"])
        T.attention_qkv_train(f.qkv_h[k].view(1, M, f.Wl), pm, nq // P, nk // P, hd, f.ctx_h[k].view(1, M, f.dc), f.lse[k])
        SPM.exchange_split(f.ctx_h[k], f.ctx_recv, f.by_owner, sp["group"])
        ops.sp_unpack_ctx(f.ctx_recv, P, out=f.ctx[k])

    def _attention_backward(self, f, k, dctx, dqkv):
        """_attention_forward's mirror: d(ctx[k]) -> d(qkv_proj's output), rotated back."""
        sp, pm = f.sp, f.prep["pm"]
        B, L, M, nq, nk, hd = f.B, f.L, f.M, f.nq, f.nk, f.hd
        if sp is None:
            T.attention_qkv_bwd(f.qkv[k].view(B, L, -1), f.ctx[k].view(B, L, -1), dctx.view(B, L, -1), f.lse[k], f.delta,
                                dqkv.view(B, L, -1), pm, nq, nk, hd)
            ops.rope_qk_inplace(dqkv, f.rope[0], f.nsin, nq, nk, hd)                     # inverse rotation
            return
        # the forward's two exchanges, mirrored: d(ctx) of my rows goes to the ranks that own the heads, d(qkv) of my heads
        # goes back to the ranks that own the rows, and is rotated back on its way into row order
        P = sp["P"]
        ops.sp_pack_ctx(dctx, P, out=f.dctx_send)
        SPM.exchange_split(f.dctx_send, f.dctx_h, f.ctx_by_sender, sp["group"])
        T.attention_qkv_bwd(f.qkv_h[k].view(1, M, f.Wl), f.ctx_h[k].view(1, M, f.dc), f.dctx_h.view(1, M, f.dc), f.lse[k],
                            f.delta, f.dqkv_h.view(1, M, f.Wl), pm, nq // P, nk // P, hd)
        SPM.exchange_split(f.dqkv_h, f.dqkv_recv, f.qkv_by_owner, sp["group"])
        ops.sp_unpack_qkv_rope(f.dqkv_recv, P, nq, nk, hd, f.rope[0], f.nsin, out=dqkv)

    def _attention_backward_buffers(self, f):
        f.nsin = self._neg_sin(f.prep)
        if f.sp is None:
            f.delta = self._buf("delta", (f.B, f.nq, f.L), F32)
            return
        P, M, Ms = f.sp["P"], f.M, f.Ms
        f.delta = self._buf("delta", (1, f.nq // P, M), F32)
        f.nsin = f.nsin.view(-1, f.hd // 2)[f.r0:f.r1]
        f.dctx_send = self._buf("sp_dctx_send", (P, Ms, f.dc)); f.dctx_h = self._buf("dctx_heads", (M, f.dc))
        f.dqkv_h = self._buf("dqkv_heads", (M, f.Wl)); f.dqkv_recv = self._buf("sp_dqkv_recv", (P, Ms, f.Wl))

    def _heads_and_loss(self, f, input_output_return):
        """Final norm, the adaLN-modulated output head (and the input_final_layer head), the per-frame MSE and d(pred)."""
        m, prep, sp = self.model, f.prep, f.sp
        M, H, nl, nf, C, h, w, ntok = f.M, f.H, f.nl, f.nf, f.C, f.h, f.w, f.ntok
        if sp is None:
            nrm = ops.rmsnorm(f.hbuf[nl], m.llm.norm.weight, m.llm.norm.variance_epsilon, out=self._buf("nrm", (M, H)))
        else:
            # final norm on the share, then ONE exchange leaves the normed rows of every rank on every rank (Gather.forward,
            # LVM/utils.py:148-161; shares padded to the largest): the heads below, the loss and their backward run
            # replicated, so the loss vector is the same bits on every rank
            pad = self._buf("nrm_pad", (max(f.sizes), H))
            ops.rmsnorm(f.hbuf[nl], m.llm.norm.weight, m.llm.norm.variance_epsilon, out=pad[:f.Ms])
            every = SPM.all_gather_flat(pad, sp["group"], out=self._buf("nrm_every", (sp["P"], max(f.sizes) * H)))
            nrm = self._buf("nrm", (M, H))
            for i, (a_, e_) in enumerate(f.shares):
                nrm[a_:e_].copy_(every[i].view(-1, H)[:e_ - a_])
        te, ada = m.t_embedder.mlp, m.final_layer.adaLN_modulation[1]
        f.te_pre = ops.linear_small(f.sin, te[0].weight, te[0].bias)
        f.te_act = T.act_fwd(f.te_pre, ops.ACT_SILU)
        f.temb = ops.linear_small(f.te_act, te[2].weight, te[2].bias)
        f.st = T.act_fwd(f.temb, ops.ACT_SILU)
        f.mod = ops.linear_small(f.st, ada.weight, ada.bias)
        Tn = nf * ntok
        f.v = self._buf("v", (Tn, H)); f.xhat = self._buf("xhat", (Tn, H), F32); f.rstd = self._buf("rstd", (Tn,), F32)
        T.ln_mod_fwd(nrm, prep["x_rows"], f.mod, f.v, f.xhat, f.rstd, ntok)
        fl = m.final_layer.linear
        y16 = ops.linear(f.v, fl.weight, bias=fl.bias)                     # (Tn, 16)
        p2 = m.patch_size
        pred = y16.view(nf, h // p2, w // p2, p2, p2, C).permute(0, 5, 1, 3, 2, 4).reshape(nf, C, h, w).contiguous()
        loss = torch.empty(nf, dtype=F32, device=self.dev)
        f.dpred = self._buf("dpred", (nf, C, h, w))
        f.head = None
        if not input_output_return:
            T.mse_frames(pred, f.x1, loss, f.dpred)
            self.last = dict(pred=pred, loss=loss, xt=f.xt)
            return loss
        # LVM/model.py:832-841 + loss.py:220-225: the input_final_layer head predicts the CLEAN condition latents from the
        # last hidden state of their rows; its per-frame MSE terms are appended to the loss vector before .mean()
        if f.cl is None:
            raise VgptError("Stage1Trainer.step: input_output_return needs condition frames")
        f.head = m.input_final_layer           # AttributeError without init_input_final_layer(), as in the reference
        nfc = f.clean.shape[0]
        f.vin = T.gather_rows(nrm, prep["c_rows"], ntok)                 # (nfc * ntok, H)
        yin = ops.linear(f.vin, f.head.weight, bias=f.head.bias)
        pred_in = yin.view(nfc, h // p2, w // p2, p2, p2, C).permute(0, 5, 1, 3, 2, 4).reshape(nfc, C, h, w).contiguous()
        loss_in = torch.empty(nfc, dtype=F32, device=self.dev)
        f.dpred_in = self._buf("dpred_in", (nfc, C, h, w))
        T.mse_frames(pred_in, f.clean.to(self.dev, F32).contiguous(), loss_in, f.dpred_in, n_mean=nf + nfc)
        T.mse_frames(pred, f.x1, loss, f.dpred, n_mean=nf + nfc)
        loss = torch.cat([loss, loss_in])
        self.last = dict(pred=pred, loss=loss, xt=f.xt, pred_in=pred_in)
        return loss

    def _backward(self, f, acc_mode):
        """The explicit backward.  A full trainer fills every gradient; per decoder layer it accumulates (acc_mode) and
        starts the exchange of that layer's bucket right behind its last dW, and returns the handles of those exchanges.
        With the base frozen (LoRA) it is the same dX chain without a single dW GEMM, and per adapted projection
        dB = s dy^T u, du = s dy B, dA = du^T x, dx += du A; nothing that only feeds frozen parameters is computed: no
        head / adaLN / embedder / embedding gradients, no dx below layer 0's qkv_proj, and the gain gradients of the
        frozen norms go to a scratch vector."""
        m, prep, g, full = self.model, f.prep, self.grads, self.lora_rank is None
        M, Ms, H, I, nq, nk, hd, nl, ntok = f.M, f.Ms, f.H, f.I, f.nq, f.nk, f.hd, f.nl, f.ntok
        rp, ls = (None, None) if full else (self.lora_rp, self.lora_scale)
        det = self.deterministic     # the fixed-order twins of the three reductions that add with atomics;
        #                              the discarded dgain / dmod sums of a LoRA trainer too: one rule for every path
        exchange = acc_mode in (None, 2)     # micro-steps before the last issue no collective
        # small bucket: zeroed for the sums below; adapter bucket: a target module left out keeps zero gradients
        self.buckets[0].grad.zero_()
        dy16 = T.unpatchify_bwd(f.dpred)                                    # (Tn, 16)
        fl, ada = m.final_layer.linear, m.final_layer.adaLN_modulation[1]
        if full:
            T.matmul(dy16, f.v, out=g["final_layer.linear.weight"], ta=True)     # dWf = dy16^T v
            T.colsum(dy16, g["final_layer.linear.bias"])
        dv = T.matmul(dy16, fl.weight)                                      # (Tn, H)
        dnrm = self._buf("dnrm", (M, H)); dnrm.zero_()
        if full:
            dmod = torch.zeros(f.nf, 2 * H, dtype=F32, device=self.dev)
            gain = g.__getitem__
        else:
            dmod = self._buf("dmod_scratch", (f.nf, 2 * H), F32); dmod.zero_()   # feeds adaLN only: discarded
            dgain = self._buf("dgain_scratch", (H,), F32); dgain.zero_()         # gain gradients of the frozen norms: discarded
            gain = lambda name: dgain
        T.ln_mod_bwd(dv, f.xhat, f.rstd, f.mod, prep["x_rows"], dnrm, dmod, ntok, deterministic=det)
        if f.head is not None:
            dyin = T.unpatchify_bwd(f.dpred_in)                              # (nfc * ntok, 16)
            if full:
                T.matmul(dyin, f.vin, out=g["input_final_layer.weight"], ta=True)
                T.colsum(dyin, g["input_final_layer.bias"])
            dnrm.index_copy_(0, prep["c_idx"], T.matmul(dyin, f.head.weight))    # condition rows: no other gradient reaches them here
        dh = self._buf("dh", (Ms, H)); dh_b = self._buf("dh_b", (Ms, H))
        # sharded: every rank keeps its own rows of dnrm (Gather.backward, LVM/utils.py:163-169): no exchange
        T.rmsnorm_bwd(f.hbuf[nl], m.llm.norm.weight, dnrm if f.sp is None else dnrm[f.r0:f.r1], dh, gain("llm.norm.weight"),
                      m.llm.norm.variance_epsilon, deterministic=det)
        if full:        # adaLN + t_embedder
            T.matmul(dmod, f.st, out=g["final_layer.adaLN_modulation.1.weight"], ta=True)
            T.colsum(dmod, g["final_layer.adaLN_modulation.1.bias"])
            dtemb = T.act_bwd(f.temb, T.matmul(dmod, ada.weight), ops.ACT_SILU)
            self._mlp_bwd("t_embedder", m.t_embedder.mlp, dtemb, f.te_act, f.te_pre, f.sin)
        # decoder layers, last to first; dX / dW read their operands transposed inside the GEMM (vgpt_gemm_bf16_tr): no
        # transposed copies are passed
        dact = self._buf("dact", (Ms, I)); dgu = self._buf("dgu", (Ms, 2 * I)); dn = self._buf("dn", (Ms, H))
        dctx = self._buf("dctx", (Ms, nq * hd)); dqkv = self._buf("dqkv", (Ms, (nq + 2 * nk) * hd))
        self._attention_backward_buffers(f)
        if not full:
            du = self._buf("du", (M, rp))
        handles = []
        for li in range(nl - 1, -1, -1):
            layer = m.llm.layers[li]
            at, mlp = layer.self_attn, layer.mlp
            names = self.layer_names[li] if full else None
            if f.ck:    # same kernels on the same inputs as the forward pass: the recomputed activations are bit-identical
                self._layer_forward(f, li, with_output=False)
            k = 0 if f.ck else li
            if full:
                T.linear_dw(dh, f.act[k], None, None, g[names[3]])                      # dW_down
            T.linear_dx(dh, mlp.down_proj.weight, None, out=dact)
            T.silu_mul_bwd(f.gu[k], dact, dgu, mlp.act)
            if full:
                T.linear_dw(dgu, f.n2[k], None, None, g[names[2]])                      # dW_gate_up
            T.linear_dx(dgu, mlp.gate_up_proj.weight, None, out=dn)
            T.rmsnorm_bwd(f.h2[k], layer.post_attention_layernorm.weight, dn, dh_b,
                          gain(f"llm.layers.{li}.post_attention_layernorm.weight"),
                          layer.post_attention_layernorm.variance_epsilon, dres=dh, deterministic=det)   # dh2
            if full:
                T.linear_dw(dh_b, f.ctx[k], None, None, g[names[1]])                    # dW_o
            T.linear_dx(dh_b, at.o_proj.weight, None, out=dctx)
            if f.lo:
                ao, go = self._lora_w[(li, "o_proj")], self._lora_g[(li, "o_proj")]
                LO.lora_grad(dh_b, f.u_o[k], go["B"], alpha=ls)                          # dB = s dy^T u
                LO.lora_down(dh_b, ao["B"], rp, s_is_k_by_rp=True, alpha=ls, out=du)     # du = s dy B
                LO.lora_grad(f.ctx[k], du, go["A"], transposed=True)                     # dA = du^T x
                LO.lora_up_add(dctx, du, ao["A"], s_is_rp_by_n=True)                     # dx += du A
            self._attention_backward(f, k, dctx, dqkv)
            if full:
                T.linear_dw(dqkv, f.n1[k], None, None, g[names[0]])                     # dW_qkv
            if f.lq:
                aq, gq = self._lora_w[(li, "qkv_proj")], self._lora_g[(li, "qkv_proj")]
                LO.lora_grad(dqkv, f.u_q[k], gq["B"], alpha=ls)
                LO.lora_down(dqkv, aq["B"], rp, s_is_k_by_rp=True, alpha=ls, out=du)
                LO.lora_grad(f.n1[k], du, gq["A"], transposed=True)
            if li == 0 and not full:
                return handles       # everything below layer 0's qkv_proj is frozen
            T.linear_dx(dqkv, at.qkv_proj.weight, None, out=dn)
            if f.lq:
                LO.lora_up_add(dn, du, aq["A"], s_is_rp_by_n=True)
            T.rmsnorm_bwd(f.hbuf[li], layer.input_layernorm.weight, dn, dh, gain(f"llm.layers.{li}.input_layernorm.weight"),
                          layer.input_layernorm.variance_epsilon, dres=dh_b, deterministic=det)   # dh (layer input)
            if full:
                b = self.buckets[1 + li]
                if acc_mode is not None:     # right behind this layer's last dW, where its bucket is complete
                    T.grad_accumulate(self._accumulators()[1][li], b.grad, acc_mode)
                if exchange and self.world > 1 and not self.skip_allreduce and self.overlap_allreduce:
                    handles.append(self._reduce(b.grad))
        # heads fed by dseq = dh (sharded: zero outside the share, so what follows yields this rank's partial gradients)
        dseq = dh
        if f.sp is not None:
            dseq = self._buf("dseq", (M, H)); dseq.zero_()
            dseq[f.r0:f.r1].copy_(dh)
            if f.sp["r"] > 0:    # computed on replicated rows: they enter the sum over the ranks from SP rank 0 alone
                for name in g:
                    if name.startswith(SP_REPLICATED):
                        g[name].zero_()
        dtt = T.gather_rows(dseq, prep["t_rows"], 1)
        self._mlp_bwd("time_token", m.time_token.mlp, dtt, f.tt_act, f.tt_pre, f.sin)
        self._patch_bwd("x_embedder", T.gather_rows(dseq, prep["x_rows"], ntok), f.xt)
        if f.cl is not None:
            self._patch_bwd("input_x_embedder", T.gather_rows(dseq, prep["c_rows"], ntok), f.cl)
        T.embed_bwd(prep["ids"].view(-1), prep["keep"], dseq, g["llm.embed_tokens.weight"], deterministic=det)
        return handles

    def _exchange(self, handles, acc_mode):
        """The last bucket of the backward (the small one; LoRA: the one adapter bucket) is complete only now: accumulate
        and exchange it, behind the layer buckets where those did not go layer by layer, and wait for every exchange."""
        last = self.buckets[0]
        if acc_mode is not None:
            T.grad_accumulate(self._accumulators()[0], last.grad, acc_mode)
        if acc_mode in (None, 2) and self.world > 1 and not self.skip_allreduce:
            if self.lora_rank is not None:
                dist.all_reduce(last.grad)       # one small blocking exchange per optimizer step
                return
            if not self.overlap_allreduce:
                handles += [self._reduce(b.grad) for b in reversed(self.buckets[1:])]
            handles.append(self._reduce(last.grad))
            for hd_ in handles:
                if hd_ is not None:
                    hd_.wait()

    def _finish_micro_step(self, acc_mode):
        """End of a step(update=True): the optimizer steps unless this was a micro-step before the last of its cycle."""
        if acc_mode is None:
            self.optimizer_step()
        elif acc_mode == 2:
            self._micro = 0
            self.optimizer_step(micro_batches=self.accum_steps)
        else:
            self._micro += 1

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
        guard = self.skip_bad_steps
        self.sumsq.zero_()
        for i, b in enumerate(self._sumsq_order()):        # layers, then the small bucket: the order of the fp32 sum
            if guard:      # the same adds; the bucket's own sum is kept for bucket_grad_norms()
                T.sumsq_keep(self._shard(b.grad), self.sumsq, self._bucket_sumsq[i:i + 1])
            else:
                T.sumsq(self._shard(b.grad), self.sumsq)
        partials = self.sumsq
        if self._sharded and not self.skip_allreduce:
            # every rank's sum over its reduced shards, in rank order, added on the device in a fixed order by clip_coef:
            # every rank computes the same norm and coefficient
            partials = SPM.all_gather_flat(self.sumsq, self._group, out=self._partials).view(-1)
        w = float(self.world // (self._sp["P"] if self._sp else 1) * micro_batches)     # data-parallel replicas x micro-batches
        # norm of the AVERAGED gradient = norm(sum)/world; coefficient already carries the 1/world factor (and 1/A, when the
        # buckets hold the sum over A micro-batches)
        if guard:
            # the verdict comes from the sum every rank holds with the same bits (replicated and sequence parallel: the
            # reduced buckets; sharded: every rank's partial in rank order), so all ranks skip together without a collective.
            # Its copy to pinned memory and the event behind it are all the host ever waits for, a step from now
            # (_resolve_verdict): the AdamW launches below read the verdict on the device.
            T.clip_coef_guarded(partials, self.coef, self.grad_norm, (self.max_grad_norm or 0.0) * w, 1.0 / w,
                                (self.skip_grad_norm_above or 0.0) * w, self._verdict)
            self._verdict_host.copy_(self._verdict, non_blocking=True)
            self._pending = torch.cuda.Event()
            self._pending.record(torch.cuda.current_stream())
        else:
            T.clip_coef(partials, self.coef, self.grad_norm, (self.max_grad_norm or 0.0) * w, 1.0 / w)
        adamw = self._adamw_guarded if guard else self._adamw
        b1, b2 = self.betas
        # AdamW on this rank's shard of every bucket (the whole bucket when not sharded), sharded: the bucket's bf16 parameters
        # all-gathered in place right behind its update.  The small bucket goes first (embeddings, heads: read first), then
        # the layers in forward order.  overlap_optimizer: the update is a pure HBM stream (28 bytes per parameter) and the
        # next step's forward is matrix work, so they run side by side: everything below goes to the optimizer's stream
        # behind the clip coefficient, each bucket followed by an event the next forward waits for right where it first
        # reads those parameters (_await_params).  Readers outside step() call finish_optimizer() first.
        ov, order = self.overlap_optimizer, self.buckets
        if ov:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream())
            self._opt_stream.wait_event(ready)
        elif not self._sharded:
            order = self.buckets[1:] + self.buckets[:1]      # nobody waits per bucket: the launch order this path always had
        evs, works = [], []
        with torch.cuda.stream(self._opt_stream if ov else torch.cuda.current_stream()):
            for b in order:
                adamw(b.master, self._shard(b.param), self._shard(b.grad), b.m, b.v, b.ema if self.use_ema else None,
                      lr, b1, b2)      # `use_ema` stays the live switch: scripts/accum_ema_step_time.py flips it
                if self._sharded:
                    works.append(None if self.skip_allreduce else
                                 SPM.all_gather_flat(self._shard(b.param), self._group, out=b.param, async_op=True))
                if ov:
                    e = torch.cuda.Event()
                    e.record(self._opt_stream)
                    evs.append(e)
        # (small, [layer 0 .. nl-1]); a LoRA trainer's layers all wait for the one adapter event
        self._opt_events = (evs[0], evs[1:] or [evs[0]] * self.cfg.num_hidden_layers) if ov else None
        if self._sharded:
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
        return [(getattr(b, kind), self._state_key(b, kind), b.numel) for b in self.buckets for kind in ("master", "m", "v")]

    def _ema_tensors(self):
        """_optimizer_tensors' triples of the EMA buffers (none without use_ema): ema_small / ema.{i} beside master.*."""
        return [(b.ema, self._state_key(b, "ema"), b.numel) for b in self.buckets if b.ema is not None]

    @staticmethod
    def _state_key(b: _Bucket, kind: str) -> str:
        """optimizer.safetensors key of bucket b's `kind` tensor: master_small, m.{i}, ema.{i}, lora_master, ..."""
        return f"{kind}_small" if b.key == "small" else f"lora_{kind}" if b.key == "lora" else f"{kind}.{b.key}"

    def _write_trainer_state(self, path: str, step: int, **mode):
        """trainer_state.json of a checkpoint directory; `mode`: the fields only a full / only a LoRA trainer records."""
        with open(os.path.join(path, "trainer_state.json"), "w") as f:
            json.dump({"step_count": self.step_count, "global_step": step, "lr": self.lr, "weight_decay": self.wd,
                       "betas": list(self.betas), "eps": self.eps, "lr_scheduler": self.lr_scheduler,
                       "lr_warmup_steps": self.lr_warmup_steps, "lr_num_training_steps": self.lr_num_training_steps,
                       "lr_num_cycles": self.lr_num_cycles, "lr_power": self.lr_power,
                       "gradient_accumulation_steps": self.accum_steps, **mode,
                       **({"skipped_steps": self.skipped_steps} if self.skip_bad_steps else {})}, f)

    # ---- EMA weights -------------------------------------------------------------------------------------------------
    def _ema_flat(self, t):
        """The whole (padded) fp32 EMA bucket of which `t` is this trainer's tensor: gathered when sharded (a collective:
        every rank calls)."""
        return SPM.all_gather_flat(t, self._group).view(-1) if self._sharded else t

    def _ema_buckets(self):
        """(EMA tensor, flat bf16 parameter buffer, parameter names in buffer order) per bucket, the small one first."""
        if not self.use_ema:
            raise VgptError("this trainer keeps no EMA (use_ema=False)")
        return [(b.ema, b.param, b.names) for b in self.buckets]

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
            self._write_trainer_state(path, step, use_ema=self.use_ema, ema_decay=self.ema_decay, small_names=self.small_names)
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
            for b in self.buckets:
                b.ema.copy_(b.master)
            logging.getLogger(__name__).warning("%s holds no EMA tensors: the EMA starts as a copy of the loaded master weights",
                                                path)
        with torch.no_grad():     # parameters are views of the flat bf16 buffers: copy in place, keep the views
            for k, p_ in own.items():
                p_.copy_(model_sd[k])
        bump_weight_generation(self.model)
        return self._restore_record(st, restore_hyperparameters)

    def _restore_record(self, st, restore_hyperparameters: bool) -> int:
        self.step_count = int(st["step_count"])
        # the guard's record: kept by a guarded trainer, absent from (and ignored by) an unguarded one
        self._skipped = int(st.get("skipped_steps", 0)) if self.skip_bad_steps else 0
        self._last_skipped, self._last_reason = False, None
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
        from safetensors.torch import save_file
        from .lora import adapter_config
        os.makedirs(path, exist_ok=True)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.lora.items()}, os.path.join(path, "adapter_model.safetensors"))
        with open(os.path.join(path, "adapter_config.json"), "w") as f:
            json.dump(adapter_config(self.lora_rank, self.lora_alpha, self.lora_targets), f, indent=2)
        save_file({key: t.cpu() for t, key, _ in self._optimizer_tensors()}, os.path.join(path, "optimizer.safetensors"))
        self._write_trainer_state(path, step, lora={"r": self.lora_rank, "rp": self.lora_rp, "lora_alpha": self.lora_alpha,
                                                    "target_modules": list(self.lora_targets), "numel": self._lora_numel})

    def _load_lora(self, path: str, st):
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
        found = [d for d in glob.glob(os.path.join(results_dir, "checkpoint-*")) if d.rsplit("-", 1)[-1].isdigit()]
        if not found:
            return None
        return self.load_checkpoint(max(found, key=lambda d: int(d.rsplit("-", 1)[-1])))


def batch_ntok(sizes) -> int:
    ns = {e - s for v in sizes.values() for s, e in v}
    if len(ns) != 1:
        raise VgptError("Stage1Trainer needs frames of one resolution")
    return ns.pop()
