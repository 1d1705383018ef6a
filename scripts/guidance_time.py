#!/usr/bin/env python3
"""What a clip costs under a guidance schedule, on bench.py's default workload: cfg-2 (4 condition + 8
generated 32x32-latent frames, CFG 1.6, x1 prediction, 32 full-width layers), hipGraph engine, prefix reuse and hoisting on,
Euler, N = 50 steps at shift 1.

One process, one model, five engines on it, whose clips ALTERNATE inside every repeat so that every variant sees the same
clocks.  A clip = per_clip_setup() + every step of the table, as bench.py times it:
    parent_full_cfg   the launch sequence and replay loop of the commit before the schedules (set_timesteps -> forward ->
                      vgpt_euler_cfg_update -> advance captured once, replayed N times), restated here on an engine without a
                      table: the yardstick
    full_cfg          StaticDenoiser.run of this tree without a table: the same graph
    interval_skip     guidance_interval = (0.25, 0.75): 25 of the 50 steps guided; the other 25 run the conditional rows only
    interval_noskip   the same table with skip_unguided_branch=False: every step runs every live row
    all_unguided      a table of 1.0: every step runs the conditional rows only
ms per clip (every repeat and the median), and ms per step by kind: inside a clip the steps run in windows of one kind between
device events (for the interval 13 unguided, 25 guided, 12 unguided steps), summed per kind over the repeats.  The box's
calibration (bench.calibrate: MFMA loop, HBM copy, 8192^3 GEMM) is measured before and after, outside the timed windows.  A
report, not a gate: nothing here says anything about sample quality (no trained checkpoint), only about the cost of a step.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself.
    python3 scripts/guidance_time.py > profiles/guidance_time.log
"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 540
REPEATS = 3
N = 50
SCALE = 1.6
# name -> (guidance arguments of scheduler.guidance_table, skip_unguided_branch); None: no table
VARIANTS = (("parent_full_cfg", None, None), ("full_cfg", None, None), ("interval_skip", dict(interval=(0.25, 0.75)), None),
            ("interval_noskip", dict(interval=(0.25, 0.75)), False), ("all_unguided", dict(schedule=[1.0] * N), None))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def windows(kinds):
    """[(first step, number of steps, kind)] of the maximal runs of one kind."""
    out, a = [], 0
    for i in range(1, len(kinds) + 1):
        if i == len(kinds) or kinds[i] != kinds[a]:
            out.append((a, i - a, kinds[a]))
            a = i
    return out


def child():
    import torch
    import bench
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    importlib.import_module("video-gpt_amd")
    M = importlib.import_module("video-gpt_amd.model")
    P = importlib.import_module("video-gpt_amd.processor")
    E = importlib.import_module("video-gpt_amd.engine")
    S = importlib.import_module("video-gpt_amd.scheduler")
    ops = importlib.import_module("video-gpt_amd.ops")
    BF = torch.bfloat16
    C, G, hw = 4, 8, (32, 32)
    model = bench.build_model(M, bench.full_config(M, 32), dev, seed=0)
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12), mask_format="layout")
    prompt = "".join(f"<img><|image_{i + 1}|></img>" if i < C else f"<|diffusion|><|image_{i + 1}|>" for i in range(C + G))
    prompt_ = "".join(f"<|diffusion|><|image_{i + 1}|>" for i in range(G))
    imgs = [torch.zeros(3, hw[0] * 8, hw[1] * 8) for _ in range(C)]
    batch = proc.prompt_condition_frame_block_inference([prompt, prompt_], [imgs, []], height=hw[0] * 8, width=hw[1] * 8,
                                                        use_img_cfg=True, frame_blocks=[C, G])
    g = torch.Generator("cpu").manual_seed(42)
    z = torch.cat([torch.randn(1, 4, *hw, generator=g).to(dev, BF) for _ in range(G)] * 2, dim=0)
    cond = [torch.randn(1, 4, *hw, generator=torch.Generator("cpu").manual_seed(1000 + i)).to(dev, BF) for i in range(C)]
    sigma = S.LVMScheduler(num_steps=N, time_shifting_factor=1).sigma

    stream = torch.cuda.Stream(device=dev)
    emit(box_calibration=bench.calibrate(dev, stream, ops, "before"))
    clips = {}
    with torch.cuda.stream(stream):
        for name, guide, skip in VARIANTS:
            table = None if guide is None else S.guidance_table(sigma, SCALE, **guide)
            eng = E.StaticDenoiser(model, batch["input_ids"].to(dev), batch["position_ids"].to(dev), batch["attention_mask"],
                                   cond, batch["input_image_sizes"], batch["denoise_image_sizes"], batch["time_emb_inx"],
                                   z.shape[0], hw, True, SCALE, "x1", sigma=sigma, reuse_condition_prefix=True,
                                   hoist_special_rows=True, attention_precision="bf16", guidance_scales=table,
                                   skip_unguided_branch=skip)
            rows = [eng.step_rows(i) for i in range(N)]
            unguided = eng.unguided or [False] * N
            # a step's kind as the report names it: what the table says and how many rows it ran
            kinds = [("unguided" if u else "guided") + f"@{r}rows" for u, r in zip(unguided, rows)]
            wins = windows(kinds)
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(wins) + 2)]
            if name == "parent_full_cfg":
                def parent_step(eng=eng):
                    ops.sampler_set_timesteps(eng.sigma, eng.step, eng.ts)
                    eng.forward_step(from_tables=True)
                    ops.euler_cfg_update(eng.z, eng.z_model, eng.pred, eng.sigma, eng.step, eng.pred_type, eng.use_cfg,
                                         eng.cfg_scale)
                    ops.sampler_advance(eng.step)
                eng.set_latents(z)
                parent_step()                       # launch attributes are set on first use, outside the capture
                stream.synchronize()
                graph = ops.HipGraph().capture(parent_step)

                def clip(eng=eng, graph=graph, wins=wins, marks=marks):
                    marks[0].record(stream)
                    eng.set_latents(z)
                    eng.per_clip_setup()
                    marks[1].record(stream)
                    for w, (_, n, _) in enumerate(wins):
                        for _ in range(n):
                            graph.replay()
                        marks[2 + w].record(stream)
            else:
                def clip(eng=eng, wins=wins, marks=marks):
                    marks[0].record(stream)
                    eng.set_latents(z)
                    eng.per_clip_setup()
                    marks[1].record(stream)
                    for w, (_, n, _) in enumerate(wins):
                        eng.run(n, use_graph=True)
                        marks[2 + w].record(stream)
            clip()                                  # captures this tree's graphs (one per step kind); warms up
            stream.synchronize()
            clips[name] = (clip, eng, wins, marks)
        ms = {name: [] for name in clips}
        by_kind = {name: {} for name in clips}
        finals = {}
        for _ in range(REPEATS):
            for name, (clip, eng, wins, marks) in clips.items():
                stream.synchronize()
                clip()
                stream.synchronize()
                ms[name].append(marks[0].elapsed_time(marks[-1]))
                for w, (_, n, kind) in enumerate(wins):
                    t, k = by_kind[name].get(kind, (0.0, 0))
                    by_kind[name][kind] = (t + marks[1 + w].elapsed_time(marks[2 + w]), k + n)
                finals[name] = eng.z.clone()
    base = sorted(ms["parent_full_cfg"])[REPEATS // 2]
    for name, guide, skip in VARIANTS:
        eng = clips[name][1]
        med = sorted(ms[name])[REPEATS // 2]
        emit(variant=name, guidance=None if guide is None else {k: (v if k == "interval" else "1.0 x %d" % N) for k, v in guide.items()},
             skip_unguided_branch=skip, skips=eng.cr is not None, steps=N,
             rows_per_step={k: sum(1 for x in [eng.step_rows(i) for i in range(N)] if x == k)
                            for k in sorted({eng.step_rows(i) for i in range(N)})},
             ms_per_clip=[round(x, 2) for x in ms[name]], ms_per_clip_median=round(med, 2), vs_parent_full_cfg=round(med / base, 4),
             ms_per_step_by_kind={k: round(t / n, 3) for k, (t, n) in by_kind[name].items()},
             finite=bool(torch.isfinite(finals[name]).all().item()))
    emit(check="full_cfg of this tree ends on the parent sequence's bits",
         equal=bool(torch.equal(finals["full_cfg"], finals["parent_full_cfg"])))
    emit(check="interval_skip ends on interval_noskip's bits (at other shapes the bits may follow the GEMM tile choice)",
         equal=bool(torch.equal(finals["interval_skip"], finals["interval_noskip"])))
    emit(box_calibration=bench.calibrate(dev, stream, ops, "after"))
    emit(note="ms per clip = per_clip_setup() + all steps, hipGraph replay; ms per step by kind = windows of one kind between "
              "device events, summed over the repeats; random-init weights: cost only, no sample-quality claim",
         device=torch.cuda.get_device_name(0), repeats=REPEATS)


def main():
    if "--child" in sys.argv:
        return child()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=LIMIT_S).returncode
    except subprocess.TimeoutExpired:
        emit(error=f"the measurement did not finish in {LIMIT_S} s")
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
