#!/usr/bin/env python3
"""What stochastic steps cost, on bench.py's default workload: cfg-2 (4 condition + 8 generated
32x32-latent frames, CFG 1.6, x1 prediction, 32 full-width layers), hipGraph engine, prefix reuse and hoisting on, Euler,
N = 50 steps at shift 1.

One process, one model, three engines on it, whose clips ALTERNATE inside every repeat so that every variant sees the same
clocks.  A clip = per_clip_setup() + every step of the table, as bench.py times it:
    parent_euler   the launch sequence and replay loop of the commit before eta (set_timesteps -> forward ->
                   vgpt_euler_cfg_update -> advance captured once, replayed N times), restated here: the yardstick
    no_eta         StaticDenoiser.run of this tree without an eta table: the same graph
    eta_0.5        eta = 0.5 at every step: vgpt_sampler_update_sde in place of the Euler update
ms per clip (every repeat and the median of 3).  Then the update kernel alone against vgpt_euler_cfg_update on the cfg-2
latents (16 frames of 4 x 32 x 32, CFG): microseconds per launch over a hipGraph of 200 back-to-back launches between
device events, median of 5 windows, and the achieved GB/s on the bytes both move (z read and written in fp32, pred read and
z_model written in bf16: 12 bytes per element).  The box's calibration (bench.calibrate) is measured before and after, outside the timed windows.  A
report, not a gate: nothing here says anything about sample quality (no trained checkpoint).

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself.
    python3 scripts/sde_time.py > profiles/sde_time.log
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
ETA = 0.5
VARIANTS = (("parent_euler", None), ("no_eta", None), (f"eta_{ETA}", ETA))
LAUNCHES, WINDOWS = 200, 5


def emit(**kw):
    print(json.dumps(kw), flush=True)


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
        for name, eta in VARIANTS:
            eng = E.StaticDenoiser(model, batch["input_ids"].to(dev), batch["position_ids"].to(dev), batch["attention_mask"],
                                   cond, batch["input_image_sizes"], batch["denoise_image_sizes"], batch["time_emb_inx"],
                                   z.shape[0], hw, True, SCALE, "x1", sigma=sigma, reuse_condition_prefix=True,
                                   hoist_special_rows=True, attention_precision="bf16",
                                   eta_table=None if eta is None else S.eta_table(sigma, eta))
            if eta is not None:
                eng.set_noise_seed(42, 0)
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            if name == "parent_euler":
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

                def clip(eng=eng, graph=graph, marks=marks):
                    marks[0].record(stream)
                    eng.set_latents(z)
                    eng.per_clip_setup()
                    for _ in range(N):
                        graph.replay()
                    marks[1].record(stream)
            else:
                def clip(eng=eng, marks=marks):
                    marks[0].record(stream)
                    eng.set_latents(z)
                    eng.per_clip_setup()
                    eng.run(N, use_graph=True)
                    marks[1].record(stream)
            clip()                                  # captures this tree's graph; warms up
            stream.synchronize()
            clips[name] = (clip, eng, marks)
        ms = {name: [] for name in clips}
        finals = {}
        for _ in range(REPEATS):
            for name, (clip, eng, marks) in clips.items():
                stream.synchronize()
                clip()
                stream.synchronize()
                ms[name].append(marks[0].elapsed_time(marks[1]))
                finals[name] = eng.z.clone()
        base = sorted(ms["parent_euler"])[REPEATS // 2]
        for name, eta in VARIANTS:
            med = sorted(ms[name])[REPEATS // 2]
            emit(variant=name, eta=eta, steps=N, ms_per_clip=[round(x, 2) for x in ms[name]], ms_per_clip_median=round(med, 2),
                 vs_parent_euler=round(med / base, 4), finite=bool(torch.isfinite(finals[name]).all().item()))
        emit(check="no_eta of this tree ends on the parent sequence's bits",
             equal=bool(torch.equal(finals["no_eta"], finals["parent_euler"])))
        emit(check=f"eta_{ETA} ends somewhere else", equal=bool(torch.equal(finals[f"eta_{ETA}"], finals["parent_euler"])))

        # ---- the update kernel alone, on the engine's own buffers (step 0 is never advanced: every launch does a full step) --
        eng = clips[f"eta_{ETA}"][1]
        elems = eng.z.numel()
        nbytes = 12 * elems
        eng.set_latents(z)
        eng.pred.copy_(z.view_as(eng.pred))
        eng.step.zero_()
        kernels = {
            "euler_cfg_update": lambda: ops.euler_cfg_update(eng.z, eng.z_model, eng.pred, eng.sigma, eng.step, eng.pred_type,
                                                             eng.use_cfg, eng.cfg_scale),
            "sampler_update_sde": lambda: ops.sampler_update_sde(eng.z, eng.z_model, eng.pred, eng.sigma, None, eng.etable,
                                                                 eng.rng, eng.step, eng.pred_type, eng.use_cfg, eng.cfg_scale,
                                                                 True)}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for name, launch in kernels.items():
            us = []
            launch()                                # launch attributes are set on first use, outside the capture
            stream.synchronize()
            graph = ops.HipGraph().capture(lambda: [launch() for _ in range(LAUNCHES)])
            for _ in range(WINDOWS + 1):            # the first window warms up
                eng.set_latents(z)                  # the state stays bounded: every window starts from the same latents
                stream.synchronize()
                a.record(stream)
                graph.replay()
                b.record(stream)
                stream.synchronize()
                us.append(a.elapsed_time(b) * 1e3 / LAUNCHES)
            us = sorted(us[1:])
            med = us[WINDOWS // 2]
            emit(kernel=name, frames=eng.nf, elements=elems, bytes_per_launch=nbytes, us_per_launch=[round(x, 2) for x in us],
                 us_per_launch_median=round(med, 2), achieved_gb_s=round(nbytes / med * 1e-3, 1),
                 how=f"one hipGraph of {LAUNCHES} back-to-back launches between device events")
    emit(box_calibration=bench.calibrate(dev, stream, ops, "after"))
    emit(note="ms per clip = per_clip_setup() + all steps, hipGraph replay; random-init weights: cost only, no sample-quality "
              "claim", device=torch.cuda.get_device_name(0), repeats=REPEATS)


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
