#!/usr/bin/env python3
"""Gradient accumulation and EMA weights at cfg-3 full size (bench.py's stage-1 workload: bs 2 x 8 frames at 256^2, 32 layers):
what the two new optimizer-path kernels cost, alone and inside the step.

Kernels, at the lengths the full-size trainer itself reports for one layer bucket (113.2 M parameters, bf16 gradient) and for
the small bucket (138.2 M, fp32 gradient), on buffers of their own, in ALTERNATING order in one process, so every variant
sees the same clocks:
    adamw_step                         28 B/param   the yardstick
    adamw_ema_step                     36 B/param   the fused launch
    adamw_step + ema.lerp_(master)     28 + 12      a separate fp32 EMA pass made with torch: yardstick only, never shipped
    grad_accumulate mode 0 / 1 / 2     bf16 bucket: 6 / 10 / 8 B/param; fp32 bucket: 8 / 12 / 12
Microseconds per launch (median over 5 rounds; a timed window is 100 back-to-back launches, 10 to 80 ms) and algorithmic bytes over that time next to the 8 TB/s HBM peak.  The working
sets (0.7 GB for mode 0 on a layer bucket, 3.2 GB and up for AdamW) are beyond the last-level cache: these are HBM round trips.

Then the stage-1 step on ONE trainer built with use_ema=True, whose `use_ema` and `accum_steps` attributes the probe flips
between steps on optimizer-step boundaries (two full-size trainers would not fit one model: each re-points the parameters to
flat buffers of its own): A = 1 with and without EMA, and A = 2 with and without EMA, where the first micro-step (forward,
backward, accumulate; no optimizer) and the last one (forward, backward, accumulate, clip, AdamW) are timed separately.
overlap_optimizer is off, so the AdamW launches are inside the timed region.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself; the
child stops at the first failing status (any VgptError ends it with a non-zero exit code).  One JSON line per result:
    python3 scripts/accum_ema_step_time.py > profiles/accum_ema_step_time.log
"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 540
ROUNDS, ITERS = 5, 100
WARMUP, STEPS = 2, 5
HBM_PEAK = 8e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, iters=ITERS):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernels(dev, n_layer, n_small):
    import torch
    T = importlib.import_module("video-gpt_amd.ops_train")
    BF, F32 = torch.bfloat16, torch.float32
    for label, n, gdt in (("layer bucket, bf16 gradient", n_layer, BF), ("small bucket, fp32 gradient", n_small, F32)):
        master = torch.randn(n, device=dev)
        m, v, ema, acc = (torch.zeros(n, device=dev) for _ in range(4))
        param = master.to(BF)
        grad = (torch.randn(n, device=dev) * 1e-3).to(gdt)
        coef = torch.ones(1, device=dev)
        hp = (1e-4, 0.9, 0.999, 1e-8, 0.1)
        gb = 2 if gdt == BF else 4
        step = [0]

        def adamw():
            step[0] += 1
            T.adamw_step(master, param, grad, m, v, *hp, step[0], coef)

        def adamw_ema():
            step[0] += 1
            T.adamw_ema_step(master, param, grad, m, v, *hp, step[0], coef, ema, 0.9999)

        def adamw_then_torch_ema():
            adamw()
            ema.lerp_(master, 1.0 - 0.9999)
        cases = [("adamw_step", 26 + gb, adamw), ("adamw_ema_step", 34 + gb, adamw_ema),
                 ("adamw_step + separate torch EMA pass", 26 + gb + 12, adamw_then_torch_ema),
                 ("grad_accumulate mode 0", 4 + gb, lambda: T.grad_accumulate(acc, grad, 0)),
                 ("grad_accumulate mode 1", 8 + gb, lambda: T.grad_accumulate(acc, grad, 1)),
                 ("grad_accumulate mode 2", 4 + 2 * gb, lambda: T.grad_accumulate(acc, grad, 2))]
        us = {name: [] for name, _, _ in cases}
        for name, _, fn in cases:
            for _ in range(3):
                fn()                               # warm-up, and mode 0 before mode 1
        for _ in range(ROUNDS):
            for name, _, fn in cases:
                if name.endswith("mode 2"):        # mode 2 would compound the bucket: give it a zero accumulator
                    acc.zero_()
                us[name].append(timed(fn))
        base = sorted(us["adamw_step"])[ROUNDS // 2]
        for name, bpp, _ in cases:
            med = sorted(us[name])[ROUNDS // 2]
            emit(kernel=name, bucket=label, n=n, bytes_per_param=bpp, us=round(med, 1), us_rounds=[round(x, 1) for x in us[name]],
                 GB_s=round(bpp * n / med * 1e-3, 1), of_8TB_s=round(bpp * n / med * 1e6 / HBM_PEAK, 3),
                 over_adamw_step=round(med / base, 3))
        del master, m, v, ema, acc, param, grad
        torch.cuda.empty_cache()


def steps(dev, tr_out):
    import torch
    import bench
    M = importlib.import_module("video-gpt_amd.model")
    P = importlib.import_module("video-gpt_amd.processor")
    TR = importlib.import_module("video-gpt_amd.train")
    F, hw, bs = 8, (32, 32), 2
    model = bench.build_model(M, bench.full_config(M, 32), dev, seed=0)
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12))
    prompt = "".join(f"<|diffusion|><|image_{i + 1}|><img><|image_{i + 1}|></img>" if i < F - 1 else f"<|diffusion|><|image_{i + 1}|>"
                     for i in range(F))
    rows = [proc.process_multi_modal_prompt_training(prompt, [torch.zeros(3, hw[0] * 8, hw[1] * 8) for _ in range(F)])
            for _ in range(bs)]
    batch = proc.collator.collate_stage1(rows, F)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items() if k not in ("input_pixel_values", "output_images")}
    g = torch.Generator("cpu").manual_seed(100)
    nd, nc = bs * F, bs * (F - 1)
    mk = lambda n: torch.randn(n, 4, *hw, generator=g).to(dev)
    x1, x0, clean, x0i = mk(nd), mk(nd), mk(nc), mk(nc)
    t, ti = torch.rand(nd, generator=g).to(dev), (0.9 + 0.1 * torch.rand(nc, generator=g)).to(dev)
    args = (batch, x1, x0, t, clean, x0i, ti)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    tr = TR.Stage1Trainer(model, lr=1e-4, weight_decay=0.1, max_grad_norm=1.0, use_ema=True)
    with_ema = torch.cuda.memory_allocated(dev) - base
    n_par = sum(t_.numel() for t_ in tr.master_layers) + tr.master_small.numel()
    tr_out.append((tr._bucket_numel[0], tr._small_numel))
    variants = [("A=1", 1, False), ("A=1 +EMA", 1, True), ("A=2", 2, False), ("A=2 +EMA", 2, True)]

    def cycle(A, ema):
        tr.accum_steps, tr.use_ema = A, ema      # probe only: flipped on an optimizer-step boundary
        out = []
        for _ in range(A):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.step(*args)
            b.record()
            torch.cuda.synchronize()
            out.append(round(a.elapsed_time(b), 2))
        return out
    for _ in range(WARMUP):
        for _, A, ema in variants:
            cycle(A, ema)
    acc_bytes = sum(a_.numel() * a_.element_size() for a_ in [tr._acc[0]] + tr._acc[1])
    emit(parameters=n_par, trainer_state_bytes_with_ema=with_ema, ema_bytes=4 * n_par,
         accumulator_bytes_allocated_on_first_use=acc_bytes,
         activations_and_workspace_bytes=torch.cuda.memory_allocated(dev) - base - with_ema - acc_bytes)
    ms = {name: [] for name, _, _ in variants}
    for _ in range(STEPS):
        for name, A, ema in variants:
            ms[name].append(cycle(A, ema))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    summary = {name: [med([c[i] for c in v]) for i in range(len(v[0]))] for name, v in ms.items()}
    emit(step_ms=ms, median_ms_per_micro_step=summary,
         ema_cost_ms=round(summary["A=1 +EMA"][0] - summary["A=1"][0], 2),
         accumulate_cost_ms_last_micro_step=round(summary["A=2"][1] - summary["A=1"][0], 2),
         first_micro_step_minus_full_step_ms=round(summary["A=2"][0] - summary["A=1"][0], 2),
         config="cfg-3: bs 2 x F=8 frames 256^2, 32 layers, one trainer, alternating variants, overlap_optimizer off; per variant "
                "the list holds the micro-steps of one optimizer step in order")


def child():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accum_ema_step_time.py needs a GPU")
    dev = torch.device("cuda:0")
    lengths = []
    steps(dev, lengths)          # first: the bucket lengths come from the trainer; its buffers are freed on return
    torch.cuda.empty_cache()
    kernels(dev, *lengths[0])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"accum_ema_step_time.py: the measurement did not finish within {LIMIT_S} s")
        sys.exit(rc)
