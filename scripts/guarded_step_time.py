#!/usr/bin/env python3
"""What the guarded optimizer step (Stage1Trainer(skip_bad_steps=True)) costs, at full width.

Kernels, on one full-width decoder layer's bucket (4 * 3072^2 + 3 * 3072 * 8192 = 113.2 M parameters, bf16 gradient; a 3.2 GB
working set, beyond the last-level cache), on buffers of their own, the launches ALTERNATING in one process so every variant
sees the same clocks:
    adamw_step                      28 B/param   the yardstick
    adamw_step_guarded, verdict 0   28 B/param   must cost what the yardstick costs: the bar is that its median exceeds the
                                                 yardstick's by no more than the spread between the yardstick's own repeats
    adamw_step_guarded, verdict 1   4 bytes      launch overhead: the waves end behind one load
Microseconds per launch: the median over three repeats, a repeat being a window of 20 back-to-back launches.
Then clip_coef against clip_coef_guarded (one wave each, 200 launches per window; the guarded one is followed in the trainer
by an 8-byte copy to pinned memory and an event, timed here as a third variant).

Then the stage-1 step of bench.py's cfg-3 workload (bs 2 x 8 frames at 256^2) on a reduced-depth full-width model, on ONE
trainer built with the guard whose `skip_bad_steps` attribute the probe flips between steps (after reading step_count, which
resolves the verdict in flight): guard off and on in alternating order.  A report, not a gate.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself; the
child stops at the first failing status.  One JSON line per result:
    python3 scripts/guarded_step_time.py > profiles/guarded_step_time.log
"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 420
REPEATS, ITERS, ITERS_CLIP = 3, 20, 200
LAYERS, WARMUP, STEPS = 4, 2, 7
N_LAYER = 4 * 3072 ** 2 + 3 * 3072 * 8192
HBM_PEAK = 8e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def median(xs):
    return sorted(xs)[len(xs) // 2]


def alternate(cases, iters):
    """{name: [us per launch of every repeat]}; the variants take turns inside every repeat."""
    us = {name: [] for name, _ in cases}
    for _, fn in cases:
        for _ in range(3):
            fn()
    for _ in range(REPEATS):
        for name, fn in cases:
            us[name].append(timed(fn, iters))
    return us


def kernels(dev):
    import torch
    T = importlib.import_module("video-gpt_amd.ops_train")
    n = N_LAYER
    master = torch.randn(n, device=dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    param = master.to(torch.bfloat16)
    grad = (torch.randn(n, device=dev) * 1e-3).to(torch.bfloat16)
    coef = torch.ones(1, device=dev)
    apply_, skip = (torch.tensor([x, x], dtype=torch.int32, device=dev) for x in (0, 1))
    hp = (1e-4, 0.9, 0.999, 1e-8, 0.1)
    step = [0]

    def adamw(verdict):
        def fn():
            step[0] += 1
            if verdict is None:
                T.adamw_step(master, param, grad, m, v, *hp, step[0], coef)
            else:
                T.adamw_step_guarded(master, param, grad, m, v, *hp, step[0], coef, verdict)
        return fn
    cases = [("adamw_step", adamw(None)), ("adamw_step_guarded verdict 0", adamw(apply_)),
             ("adamw_step_guarded verdict 1", adamw(skip))]
    us = alternate(cases, ITERS)
    base = us["adamw_step"]
    spread = max(base) - min(base)
    for name, _ in cases:
        med = median(us[name])
        rec = dict(kernel=name, n=n, us=round(med, 1), us_repeats=[round(x, 1) for x in us[name]],
                   over_adamw_step_us=round(med - median(base), 1))
        if not name.endswith("1"):
            rec.update(GB_s=round(28 * n / med * 1e-3, 1), of_8TB_s=round(28 * n / med * 1e6 / HBM_PEAK, 3))
        emit(**rec)
    excess = median(us["adamw_step_guarded verdict 0"]) - median(base)
    emit(bar="guarded verdict-0 median minus unguarded median <= spread of the three unguarded repeats",
         excess_us=round(excess, 1), unguarded_spread_us=round(spread, 1), met=bool(excess <= spread))
    del master, m, v, param, grad
    torch.cuda.empty_cache()
    # the clip kernels: one wave over `world` partial sums
    for n_part in (1, 8):
        partials = torch.rand(n_part, device=dev) * 50.0
        norm, verdict = torch.zeros(1, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        host = torch.zeros(2, dtype=torch.int32).pin_memory()
        events = []

        def guarded_and_copy():
            T.clip_coef_guarded(partials, coef, norm, 1.0, 1.0, 100.0, verdict)
            host.copy_(verdict, non_blocking=True)
            events.append(torch.cuda.Event())
            events[-1].record()
        us = alternate([("clip_coef", lambda: T.clip_coef(partials, coef, norm, 1.0, 1.0)),
                        ("clip_coef_guarded", lambda: T.clip_coef_guarded(partials, coef, norm, 1.0, 1.0, 100.0, verdict)),
                        ("clip_coef_guarded + verdict copy + event", guarded_and_copy)], ITERS_CLIP)
        for name, xs in us.items():
            emit(kernel=name, partial_sums=n_part, us=round(median(xs), 2), us_repeats=[round(x, 2) for x in xs])


def steps(dev):
    import torch
    import bench
    M = importlib.import_module("video-gpt_amd.model")
    P = importlib.import_module("video-gpt_amd.processor")
    TR = importlib.import_module("video-gpt_amd.train")
    F, hw, bs = 8, (32, 32), 2
    model = bench.build_model(M, bench.full_config(M, LAYERS), dev, seed=0)
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
    tr = TR.Stage1Trainer(model, lr=1e-4, weight_decay=0.1, max_grad_norm=1.0, skip_bad_steps=True, skip_grad_norm_above=1e6)

    def one(guard):
        assert tr.step_count >= 0            # resolves the verdict in flight before the switch is flipped
        tr.skip_bad_steps = guard            # probe only: flipped on an optimizer-step boundary
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.step(*args)
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b), 3)
    for _ in range(WARMUP):
        for guard in (False, True):
            one(guard)
    ms = {False: [], True: []}
    for i in range(STEPS):
        for guard in ((False, True) if i % 2 == 0 else (True, False)):
            ms[guard].append(one(guard))
    emit(step_ms_guard_off=ms[False], step_ms_guard_on=ms[True], median_ms_guard_off=median(ms[False]),
         median_ms_guard_on=median(ms[True]), guard_cost_ms=round(median(ms[True]) - median(ms[False]), 3),
         spread_ms_guard_off=round(max(ms[False]) - min(ms[False]), 3), skipped_steps=tr.skipped_steps, step_count=tr.step_count,
         config=f"cfg-3 at {LAYERS} of 32 layers (full width): bs 2 x F=8 frames 256^2, one trainer, guard off / on alternating, "
                "overlap_optimizer off")


def child():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("guarded_step_time.py needs a GPU")
    dev = torch.device("cuda:0")
    kernels(dev)
    steps(dev)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"guarded_step_time.py: the measurement did not finish within {LIMIT_S} s")
        sys.exit(rc)
