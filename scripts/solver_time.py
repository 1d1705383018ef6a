#!/usr/bin/env python3
"""What a clip costs under each sampler solver, on bench.py's default workload: cfg-2 (4 condition + 8
generated 32x32-latent frames, CFG 1.6, x1 prediction, 32 full-width layers), hipGraph engine, prefix reuse and hoisting on.

One process, one model, four engines on it, whose clips ALTERNATE inside every repeat so that every variant sees the same
clocks.  A clip = per_clip_setup() + every step of the table, as bench.py times it:
    parent_euler N=50   the launch sequence and the replay loop of the commit before the solvers (set_timesteps -> forward ->
                        vgpt_euler_cfg_update -> advance captured once, `for _ in range(N): graph.replay()`), restated here
                        on an Euler engine: the yardstick
    euler N=50          StaticDenoiser.run of this tree, solver "euler": the same graph under the new loop
    ab2 N=50            one model call per step + vgpt_sampler_update (4 more bytes per latent element of traffic)
    heun N=25           49 model calls: 24 two-call graphs + the Euler-shaped final step
ms per clip: every repeat, and the median.  A report, not a gate: nothing here says anything about sample quality (no trained
checkpoint), only about the cost of the model evaluations.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself.
    python3 scripts/solver_time.py > profiles/solver_time.log
"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 420
REPEATS = 3
VARIANTS = (("parent_euler", "euler", 50), ("euler", "euler", 50), ("ab2", "ab2", 50), ("heun", "heun", 25))


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

    stream = torch.cuda.Stream(device=dev)
    clips = {}
    with torch.cuda.stream(stream):
        for name, solver, n in VARIANTS:
            sigma = S.LVMScheduler(num_steps=n, time_shifting_factor=1).sigma
            eng = E.StaticDenoiser(model, batch["input_ids"].to(dev), batch["position_ids"].to(dev), batch["attention_mask"],
                                   cond, batch["input_image_sizes"], batch["denoise_image_sizes"], batch["time_emb_inx"],
                                   z.shape[0], hw, True, 1.6, "x1", sigma=sigma, reuse_condition_prefix=True, solver=solver)
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

                def clip(eng=eng, graph=graph, n=n):
                    eng.set_latents(z)
                    eng.per_clip_setup()
                    for _ in range(n):
                        graph.replay()
            else:
                def clip(eng=eng, n=n):
                    eng.set_latents(z)
                    eng.per_clip_setup()
                    eng.run(n, use_graph=True)
            clip()                                  # captures this tree's graphs; warms up
            stream.synchronize()
            clips[name] = (clip, eng)
        ms = {name: [] for name in clips}
        finals = {}
        for _ in range(REPEATS):
            for name, (clip, eng) in clips.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                a.record(stream)
                clip()
                b.record(stream)
                stream.synchronize()
                ms[name].append(a.elapsed_time(b))
                finals[name] = eng.z.clone()
    base = sorted(ms["parent_euler"])[REPEATS // 2]
    for name, solver, n in VARIANTS:
        med = sorted(ms[name])[REPEATS // 2]
        evals = 2 * n - 1 if solver == "heun" else n
        emit(variant=name, solver=solver, steps=n, model_evaluations=evals, ms_per_clip=[round(x, 2) for x in ms[name]],
             ms_per_clip_median=round(med, 2), ms_per_model_evaluation=round(med / evals, 3),
             vs_parent_euler=round(med / base, 4), finite=bool(torch.isfinite(finals[name]).all().item()))
    emit(check="euler of this tree ends on the parent sequence's bits",
         equal=bool(torch.equal(finals["euler"], finals["parent_euler"])))
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
