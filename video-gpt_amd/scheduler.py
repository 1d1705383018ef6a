"""LVMScheduler: rectified-flow sampler (mirror of LVM/scheduler.py:119-208: first-order Euler, the default), with two
second-order solvers beside it (`solver="ab2"`: two-step Adams-Bashforth, one model call per step; `solver="heun"`:
2 N - 1 model calls for N steps; arithmetic in DESIGN.md section 5), and stochastic Euler steps (`eta` in (0, 1]: the
flow-matching counterpart of DDIM's eta -- fresh counter-based noise re-injected at every step inside the update kernel;
DESIGN.md section 5c).

`__call__(z, func, model_kwargs, ...)` keeps the reference contract:
`func(z, timesteps, past_key_values=None, prediction_type=..., **model_kwargs) -> (pred, cache)`.

Two execution paths, same arithmetic:
  * fast path — `func` is `LVM.frame_block_forward_with_cfg` of this package and the latents are a
    list of equal-shape frames: the whole step (model + x1->v + CFG + Euler) runs from one
    hipGraph captured once per clip (engine.StaticDenoiser);
  * generic path — any other `func`: the model call is the caller's, the x1->v / CFG / Euler update
    is one HIP kernel per step.
The sampler state is kept in fp32 and rounded to the model dtype only where it enters the model
(the reference rounds the state to bf16 after every step; an fp32 state is closer to its fp32 CPU
path).  KV caching is not used, exactly as the reference passes `past_key_values=None` every step
(LVM/scheduler.py:174).
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch

from . import ops
from .ops import BF16, VgptError


def guidance_table(sigma, scale: float, interval=None, schedule=None):
    """The image-CFG scale of every step of the table `sigma` (N + 1 entries, step i runs at sigma[i]) as an fp32 tensor
    (N), or None when neither `interval` nor `schedule` is given: the scalar path, one scale for the clip.

    interval = (lo, hi), in the scheduler's own sigma units (0 = noise, 1 = data): entry i is `scale` where
    lo <= sigma[i] < hi and 1.0 elsewhere (limited-interval guidance, Kynkaanniemi et al. 2024).  schedule: N scales, or a
    callable of sigma[i].  An entry of exactly 1.0 is an unguided step: the guided velocity is the
    conditional one, and the fast path does not compute the unconditional rows at all."""
    if interval is None and schedule is None:
        return None
    if interval is not None and schedule is not None:
        raise VgptError(f"guidance_table: both interval={interval!r} and schedule={schedule!r} given (one of them)")
    sig = [float(s) for s in torch.as_tensor(sigma).reshape(-1).tolist()]
    n = len(sig) - 1
    if n <= 0:
        raise VgptError(f"guidance_table: a sigma table of {len(sig)} entries has no step")
    if interval is not None:
        lo, hi = (float(v) for v in interval)
        if not lo <= hi:   # also refuses a NaN bound
            raise VgptError(f"guidance_table: interval lo={lo!r} > hi={hi!r}")
        vals = [float(scale) if lo <= s < hi else 1.0 for s in sig[:n]]
    elif callable(schedule):
        vals = [float(schedule(s)) for s in sig[:n]]
    else:
        vals = [float(v) for v in (schedule.tolist() if isinstance(schedule, torch.Tensor) else schedule)]
        if len(vals) != n:
            raise VgptError(f"guidance_table: schedule has {len(vals)} entries, num_steps is {n}")
    out = torch.tensor(vals, dtype=torch.float32)
    bad = [(i, v) for i, v in enumerate(out.tolist()) if v != v or v in (float("inf"), float("-inf"))]
    if bad:
        raise VgptError(f"guidance_table: non-finite scale {bad[0][1]!r} at step {bad[0][0]}")
    return out


def eta_table(sigma, eta: float, interval=None):
    """The stochasticity of every step of the table `sigma` (N + 1 entries, step i runs at sigma[i]) as an fp32 tensor (N),
    or None when eta == 0: the deterministic sampler.  Entry i is `eta` where lo <= sigma[i] < hi of `interval` = (lo, hi),
    in the scheduler's own sigma units (0 = noise, 1 = data), and 0 elsewhere; without an interval every step gets `eta`.
    A step with eta_i in (0, 1] replaces that share of the state's noise part by fresh noise:
    z' = (z + h v) + (1 - sigma[i+1]) ((sqrt(1 - eta_i^2) - 1) x0_hat + eta_i eps), x0_hat = z - sigma[i] v."""
    e = float(eta)
    if not 0.0 <= e <= 1.0:   # also refuses a NaN
        raise VgptError(f"eta_table: eta={eta!r} is outside [0, 1]")
    lo = hi = None
    if interval is not None:
        lo, hi = (float(v) for v in interval)
        if not lo <= hi:   # also refuses a NaN bound
            raise VgptError(f"eta_table: interval lo={lo!r} > hi={hi!r}")
    if e == 0.0:
        return None
    sig = [float(s) for s in torch.as_tensor(sigma).reshape(-1).tolist()]
    n = len(sig) - 1
    if n <= 0:
        raise VgptError(f"eta_table: a sigma table of {len(sig)} entries has no step")
    return torch.tensor([e if lo is None or lo <= s < hi else 0.0 for s in sig[:n]], dtype=torch.float32)


def refuse_noisy_solver(who: str, solver: str, table):
    """Only the first-order step takes noise: a multistep history is meaningless across injected noise."""
    if table is None or solver == "euler":
        return
    bad = [(i, v) for i, v in enumerate(torch.as_tensor(table).reshape(-1).tolist()) if v != 0.0]
    if bad:
        raise VgptError(f"{who}: solver={solver!r} with eta={bad[0][1]!r} at step {bad[0][0]}: only solver='euler' takes a "
                        "non-zero eta")


class LVMScheduler:
    def __init__(self, num_steps: int = 50, time_shifting_factor: int = 1, begin_time=None, solver: str = "euler",
                 guidance_interval=None, guidance_schedule=None, eta: float = 0.0, eta_interval=None, noise_seed: int = 0,
                 noise_stream: int = 0):
        ops.solver_id(solver)   # an unknown name is refused here, naming it
        self.solver = solver
        # stochastic steps (eta_table): eta in [0, 1] inside `eta_interval` = (lo, hi) of sigma (every
        # step without one), 0 = the deterministic sampler, bit for bit.  The noise is counter-based, a function of
        # (noise_seed, noise_stream, step, element) computed in the update kernel: seed and stream live in device memory, so
        # a cached engine and its captured graphs serve any of them
        self.eta = eta
        self.eta_interval = eta_interval
        self.noise_seed = noise_seed
        self.noise_stream = noise_stream
        # a per-step image-CFG scale (guidance_table): the clip's img_cfg_scale inside `guidance_interval` = (lo, hi) of
        # sigma and 1.0 outside it, or `guidance_schedule` (num_steps scales, or a callable of sigma_i).  Both None: one
        # scale for the clip, as before.  The fast path skips the unconditional rows in the steps whose scale is exactly 1
        # (skip_unguided_branch: None = wherever the layout allows it, True = or refuse, False = never); the generic path
        # applies the per-step scale and skips nothing -- the model call is the caller's.
        self.guidance_interval = guidance_interval
        self.guidance_schedule = guidance_schedule
        self.skip_unguided_branch = None
        self.num_steps = num_steps
        self.time_shift = time_shifting_factor
        t = torch.linspace(0 if begin_time is None else begin_time, 1, num_steps + 1)
        self.sigma = t / (t + time_shifting_factor - time_shifting_factor * t)
        guidance_table(self.sigma, 1.0, guidance_interval, guidance_schedule)   # a bad schedule is refused here, by value
        refuse_noisy_solver("LVMScheduler", solver, eta_table(self.sigma, eta, eta_interval))   # so is a bad eta
        self.use_graph = True
        self.pack_padding = True
        self.reuse_condition_prefix = True   # compute the step-invariant condition rows once per clip (engine.py)
        self.hoist_special_rows = True       # ... and the <|diffusion|> / time rows of all steps in one pass (needs a TokenLayout mask)
        self.attention_precision = "bf16"    # "fp8": MX-fp8 attention in the sampler steps of the fast path (cfg-5 option)
        self.linear_precision = "bf16"       # "fp8": MX-fp8 qkv / o / gate_up / down projections in the fast path's steps
        self.fuse_norms = None               # None: RMSNorms folded into the GEMMs wherever the step's shapes allow (engine.py); False: never
        # True: under a sequence-parallel group of P > 1 ranks (sequence_parallel.py) the fast path builds the sharded engine
        # (Ulysses: every rank runs ~1/P of the live rows and 1/P of the attention heads: the same StaticDenoiser passes on the
        # rank's share of the rows, attention through StaticDenoiser._sp_attention).
        # Sharded engines run eagerly, whatever use_graph says: capturing the RCCL exchanges into a hipGraph is a separate
        # step.  False (default): every rank runs the whole clip, as before.
        self.sequence_parallel_engine = False
        # keep the engine of a clip on the model and re-use it for the next clip of an identical sequence (the rounds of a
        # rollout once the window is full: LVM/pipeline.py:418-422 re-creates the same prompt every round): buffers, attention
        # plan and the captured graph survive, the per-clip pass is redone on the new condition latents
        self.cache_engines = os.environ.get("VGPT_ENGINE_CACHE", "1") != "0"
        self.last_engine = None
        self.last_engine_reused = False

    # ---- fast path ----
    def _fast_path_engine(self, z, func, model_kwargs, prediction_type):
        from .engine import StaticDenoiser
        from .model import LVM
        owner = getattr(func, "__self__", None)
        if not isinstance(owner, LVM) or getattr(func, "__name__", "") != "frame_block_forward_with_cfg":
            return None
        if not isinstance(z, (list, tuple)) or len({tuple(t.shape) for t in z}) != 1:
            return None
        lat = model_kwargs.get("input_img_latents")
        if lat is not None and len(lat) > 0 and len({tuple(t.shape) for t in lat}) != 1:
            return None
        need = ("input_ids", "input_image_sizes", "attention_mask", "position_ids", "denoise_image_sizes",
                "time_emb_inx", "use_img_cfg", "img_cfg_scale")
        if any(k not in model_kwargs for k in need) or model_kwargs.get("offload_model"):
            return None
        self.last_engine_reused = False
        from .train import wait_for_pending_update
        wait_for_pending_update(owner)      # a trainer's overlapped AdamW update of these parameters may still be in flight
        self._owner_params = list(owner.parameters())
        self._table = self._guidance(model_kwargs)
        self._eta = self._eta_table()
        key = self._engine_key(z, model_kwargs, prediction_type) if self.cache_engines else None
        cache = owner.__dict__.setdefault("_vgpt_engine_cache", {}) if key is not None else None
        if cache is not None and key in cache:
            eng = cache.pop(key)
            cache[key] = eng                     # most recently used last
            self.last_engine_reused = True
            eng = eng.rebind(lat)
            if self._eta is not None:
                eng.set_noise_seed(self.noise_seed, self.noise_stream)
            return eng
        eng = self._build_engine(StaticDenoiser, owner, z, lat, model_kwargs, prediction_type)
        if self._eta is not None:
            eng.set_noise_seed(self.noise_seed, self.noise_stream)
        if cache is not None:
            cache[key] = eng
            while len(cache) > 2:                # a clip's buffers are a few GB at cfg-2: the last two layouts are kept
                cache.pop(next(iter(cache)))
        return eng

    def _guidance(self, model_kwargs):
        """The clip's scale table (guidance_table on this scheduler's sigma and the call's img_cfg_scale), or None."""
        if self.guidance_interval is None and self.guidance_schedule is None:
            return None
        if not model_kwargs.get("use_img_cfg", False):
            raise VgptError(f"LVMScheduler: guidance_interval={self.guidance_interval!r} / guidance_schedule="
                            f"{self.guidance_schedule!r} with use_img_cfg=False: there is nothing to schedule")
        return guidance_table(self.sigma, float(model_kwargs.get("img_cfg_scale", 1.0)), self.guidance_interval,
                              self.guidance_schedule)

    def _eta_table(self):
        """The clip's eta table (eta_table on this scheduler's sigma), or None: the deterministic sampler."""
        table = eta_table(self.sigma, self.eta, self.eta_interval)
        refuse_noisy_solver("LVMScheduler", self.solver, table)
        if table is not None and not bool((table != 0).any()):
            return None   # an interval that covers no step: nothing is stochastic, the old path and its engine
        return table

    def _engine_key(self, z, model_kwargs, prediction_type):
        """Everything a StaticDenoiser is built from except the condition latents' VALUES; None when the mask is not a
        TokenLayout (a dense mask would have to be compared element by element)."""
        from . import sequence_parallel as SPM
        from .layout import TokenLayout
        mask = model_kwargs["attention_mask"]
        if not isinstance(mask, TokenLayout):
            return None
        lat = model_kwargs.get("input_img_latents")
        tb = lambda t: t.detach().cpu().numpy().tobytes()
        return (tb(model_kwargs["input_ids"]), tb(model_kwargs["position_ids"]), mask.attr().tobytes(),
                repr(model_kwargs["input_image_sizes"]), repr(model_kwargs["denoise_image_sizes"]), repr(model_kwargs["time_emb_inx"]),
                len(z), tuple(z[0].shape), None if not lat else (len(lat), tuple(lat[0].shape)),
                bool(model_kwargs["use_img_cfg"]), float(model_kwargs["img_cfg_scale"]), prediction_type, tb(self.sigma),
                self.pack_padding, self.reuse_condition_prefix, self.hoist_special_rows, self.attention_precision,
                self.linear_precision, self.fuse_norms, str(z[0].device), self.solver,
                # two guidance schedules never share an engine: its table, step kinds and graphs are the schedule's
                None if self._table is None else self._table.numpy().tobytes(), self.skip_unguided_branch,
                # nor two eta tables; the noise seed and stream are NOT here: the engine reads them from device memory
                None if self._eta is None else self._eta.numpy().tobytes(),
                # a sharded engine holds this rank's rows and heads of a group of this size
                self.sequence_parallel_engine, SPM.sp_world(), SPM.sp_rank(),
                # the GEMM family decided whether the engine folded the RMSNorms (norm_workspace_bytes is 0 under family 1) and
                # which kernels its graph captured: an engine of another family is not this call's
                ops.gemm_family(),
                # the captured graph holds the parameters' device addresses: parameters moved or re-allocated since
                # (model.to(...), a new state dict assigned tensor by tensor) must not meet a cached graph
                tuple(p_.data_ptr() for p_ in self._owner_params))

    def _build_engine(self, StaticDenoiser, owner, z, lat, model_kwargs, prediction_type):
        return StaticDenoiser(owner, model_kwargs["input_ids"], model_kwargs["position_ids"],
                              model_kwargs["attention_mask"], lat, model_kwargs["input_image_sizes"],
                              model_kwargs["denoise_image_sizes"], model_kwargs["time_emb_inx"], len(z),
                              tuple(z[0].shape[-2:]), model_kwargs["use_img_cfg"], model_kwargs["img_cfg_scale"],
                              prediction_type, sigma=self.sigma, pack_padding=self.pack_padding,
                              reuse_condition_prefix=self.reuse_condition_prefix,
                              hoist_special_rows=self.hoist_special_rows,
                              attention_precision=self.attention_precision, linear_precision=self.linear_precision,
                              fuse_norms=self.fuse_norms, sequence_parallel=self.sequence_parallel_engine,
                              solver=self.solver, guidance_scales=self._table,
                              skip_unguided_branch=self.skip_unguided_branch, eta_table=self._eta)

    def __call__(self, z, func, model_kwargs, use_kv_cache: bool = True, offload_kv_cache: bool = True,
                 prediction_type: str = "v", vae=None, noise_level=None):
        is_list = isinstance(z, (list, tuple))
        frames = list(z) if is_list else [z]
        if not frames[0].is_cuda:
            raise VgptError("LVMScheduler runs on the MI355X HIP path only (latents must be on the GPU)")
        out_dtype = frames[0].dtype
        if noise_level is not None:  # LVM/scheduler.py:162-163 (RNG stays torch's)
            from . import ops_train   # noise_level * f + (1 - noise_level) * randn through the HIP lerp kernel
            mixed = []
            for f in frames:
                t = torch.full((f.shape[0],), float(noise_level), device=f.device, dtype=torch.float32)
                o = torch.empty(f.shape, device=f.device, dtype=torch.bfloat16)
                mixed.append(ops_train.lerp_frames(f.float().contiguous(), torch.randn_like(f).float().contiguous(), t, o)
                             .to(out_dtype))
            frames = mixed

        engine = self._fast_path_engine(frames, func, model_kwargs, prediction_type) if is_list else None
        if engine is None and self.linear_precision != "bf16":
            # the fp8 projections exist in the engine's per-step forward only: no silent bf16 run of another path
            raise VgptError(f"LVMScheduler: linear_precision={self.linear_precision!r} needs the fast path (StaticDenoiser: "
                            "frame_block_forward_with_cfg of this package on a list of equal-shape latents)")
        if engine is None and self.sequence_parallel_engine:
            from . import sequence_parallel as SPM
            if SPM.sp_world() > 1:   # no silent replicated run of the whole clip on every rank
                raise VgptError("LVMScheduler: sequence_parallel_engine=True needs the fast path (StaticDenoiser: "
                                "frame_block_forward_with_cfg of this package on a list of equal-shape latents)")
        if engine is not None:
            self.last_engine = engine
            stream = torch.cuda.current_stream()
            side = None
            if self.use_graph and stream.cuda_stream == 0:  # the legacy default stream cannot be captured
                side = torch.cuda.Stream()
                side.wait_stream(stream)
            with torch.cuda.stream(side) if side is not None else _null():
                engine.set_latents(torch.cat(frames, dim=0))
                zf = engine.run(self.num_steps, use_graph=self.use_graph)
            if side is not None:
                stream.wait_stream(side)
            zf = zf.view(len(frames), *frames[0].shape[1:]).to(out_dtype)
            return [zf[i:i + 1] for i in range(len(frames))]

        # ---- generic path ----
        # the state is a (rows, elems) fp32 matrix: one row per list entry, or per batch item of a tensor z
        # (LVM/scheduler.py:183-204 treats both the same way: x1 -> v, CFG on the two halves, Euler update)
        dev = frames[0].device
        if is_list:
            shapes = [tuple(f.shape) for f in frames]
            if len({f.numel() for f in frames}) != 1:
                raise VgptError("generic sampler path needs latents of one size (mixed resolutions: call per size)")
            n, elems = len(frames), frames[0].numel()
            zf = torch.cat([f.reshape(1, -1) for f in frames], dim=0).to(torch.float32).contiguous()
        else:
            zt = frames[0]
            n, elems = zt.shape[0], zt.numel() // max(zt.shape[0], 1)
            zf = zt.reshape(n, elems).to(torch.float32).contiguous()
        zm = torch.empty(n, elems, dtype=BF16, device=dev)
        ops.cast_f32_to_bf16(zf, zm)
        sigma = self.sigma.to(dev, torch.float32).contiguous()
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        ts = torch.empty(n, dtype=torch.float32, device=dev)
        use_cfg = bool(model_kwargs.get("use_img_cfg", False))
        scale = float(model_kwargs.get("img_cfg_scale", 1.0))
        # for 'v' predictions the CFG combination already happened inside func (LVM/model.py:508-512, 555-562)
        kernel_cfg = use_cfg and prediction_type == "x1"
        if kernel_cfg and n % 2:
            raise VgptError("image CFG needs the conditional and unconditional halves (an even number of latents)")
        pred_type = ops.PRED_X1 if prediction_type == "x1" else ops.PRED_V
        solver = ops.solver_id(self.solver)
        # a guidance schedule on this path: the per-step scale is applied and NO rows are skipped (the model call is the
        # caller's and computes both halves).  x1: the table goes to the update kernel; v: the CFG combination happens
        # inside func, which gets the step's scale as its img_cfg_scale
        table = self._guidance(model_kwargs)
        scales = None if table is None else table.tolist()
        table_dev = table.to(dev) if kernel_cfg and table is not None else None
        # the guided velocity of the step (ab2: of the previous one when it is read), one CFG half
        # stochastic steps: the same update with the step's eta and counter-based noise.  Under CFG both halves get the same
        # noise, also where func combined them itself (v predictions: share_halves)
        eta_tab = self._eta_table()
        if eta_tab is not None:
            eta_dev = eta_tab.to(dev)
            rng = ops.noise_rng(self.noise_seed, self.noise_stream, dev)
            share = use_cfg and n % 2 == 0
        v_hist = None if solver == ops.SOLVER_EULER else torch.empty(n // 2 if kernel_cfg else n, elems, dtype=torch.float32,
                                                                    device=dev)

        def evaluate(i=None):
            ops.sampler_set_timesteps(sigma, step, ts)
            z_in = [zm[i].view(shapes[i]) for i in range(n)] if is_list else zm.view(frames[0].shape)
            mk = model_kwargs if scales is None else {**model_kwargs, "img_cfg_scale": scales[i]}
            pred, _cache = func(z_in, ts, past_key_values=None, prediction_type=prediction_type, **mk)
            if is_list:
                pred = torch.cat([p.reshape(1, -1) for p in pred], dim=0)
            return pred.reshape(n, elems).to(BF16).contiguous()

        def update(pred, stage=0):
            if table_dev is not None:
                ops.sampler_update_sched(zf, zm, pred, v_hist, sigma, table_dev, step, pred_type, solver, stage)
            else:
                ops.sampler_update(zf, zm, pred, v_hist, sigma, step, pred_type, kernel_cfg, scale, solver, stage)

        for i in range(self.num_steps):
            pred = evaluate(i)
            if solver == ops.SOLVER_HEUN and i < self.num_steps - 1:
                # predictor -> the model at sigma[i+1] on bf16(z + h v) -> corrector; the last step (sigma = 1) is Euler's.
                # Both model calls of the step use the step's scale
                update(pred, 0)
                ops.sampler_advance(step)
                update(evaluate(i), 1)
                continue
            if eta_tab is not None:
                ops.sampler_update_sde(zf, zm, pred, sigma, table_dev, eta_dev, rng, step, pred_type, kernel_cfg, scale, share)
            elif solver == ops.SOLVER_AB2 or table_dev is not None:
                update(pred)
            else:
                ops.euler_cfg_update(zf, zm, pred, sigma, step, pred_type, kernel_cfg, scale)
            ops.sampler_advance(step)
        out = zf.to(out_dtype)
        if is_list:
            return [out[i].view(shapes[i]) for i in range(n)]
        return out.view(frames[0].shape)


class _null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False
