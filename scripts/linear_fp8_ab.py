#!/usr/bin/env python3
"""Same-process A/B of the sampler's linear_precision option on bench.py's infer workload (cfg-2: 256^2, C = 4 condition +
G = 8 generated frames, image CFG, 32 full-width decoder layers, bench.full_config / bench.build_model, same batch, noise and
engine options as bench.py's default run: condition-prefix reuse and special-row hoisting on):
for "bf16" and "fp8" in turn, one StaticDenoiser, graph captured, `--warmup` steps, then `--steps` graph replays timed with
HIP events; per_clip_setup() timed alone afterwards (for "fp8" it includes the weight re-quantisation, also timed alone).
Prints one JSON line: ms/step and per_clip_setup_ms per mode, and the rel-L2 between the two modes' sampled latents.

  python scripts/linear_fp8_ab.py [--steps 20] [--warmup 3] [--attn-precision bf16]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

BF = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--attn-precision", default="bf16", choices=["bf16", "fp8"])
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    importlib.import_module("video-gpt_amd")
    M = importlib.import_module("video-gpt_amd.model")
    P = importlib.import_module("video-gpt_amd.processor")
    E = importlib.import_module("video-gpt_amd.engine")
    S = importlib.import_module("video-gpt_amd.scheduler")
    C, G, hw = 4, 8, (32, 32)
    cfg = bench.full_config(M, args.layers)
    model = bench.build_model(M, cfg, device, seed=0)
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12), mask_format="layout")
    prompt = "".join(f"<img><|image_{i + 1}|></img>" if i < C else f"<|diffusion|><|image_{i + 1}|>" for i in range(C + G))
    prompt_ = "".join(f"<|diffusion|><|image_{i + 1}|>" for i in range(G))
    imgs = [torch.zeros(3, hw[0] * 8, hw[1] * 8) for _ in range(C)]
    batch = proc.prompt_condition_frame_block_inference([prompt, prompt_], [imgs, []], height=hw[0] * 8, width=hw[1] * 8,
                                                        use_img_cfg=True, frame_blocks=[C, G])
    g = torch.Generator("cpu").manual_seed(42)
    z = [torch.randn(1, 4, *hw, generator=g).to(device, BF) for _ in range(G)] * 2
    cond = [torch.randn(1, 4, *hw, generator=torch.Generator("cpu").manual_seed(1000 + i)).to(device, BF) for i in range(C)]
    sched = S.LVMScheduler(num_steps=args.warmup + args.steps, time_shifting_factor=1)
    stream = torch.cuda.Stream(device=device)
    res, lat = {"workload": "cfg-2 sampler step, bench.py infer batch", "layers": args.layers, "steps": args.steps,
                "warmup": args.warmup, "attention_precision": args.attn_precision}, {}

    def ev_ms(fn, reps=1):
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record(stream)
        for _ in range(reps):
            fn()
        e_.record(stream)
        stream.synchronize()
        return s_.elapsed_time(e_) / reps

    for mode in ("bf16", "fp8"):
        eng = E.StaticDenoiser(model, batch["input_ids"].to(device), batch["position_ids"].to(device), batch["attention_mask"],
                               cond, batch["input_image_sizes"], batch["denoise_image_sizes"], batch["time_emb_inx"], len(z), hw,
                               True, 1.6, "x1", sigma=sched.sigma, reuse_condition_prefix=True, hoist_special_rows=True,
                               attention_precision=args.attn_precision, linear_precision=mode)
        with torch.cuda.stream(stream):
            eng.set_latents(torch.cat(z, dim=0))
            eng.capture()
            eng.run(args.warmup)
            stream.synchronize()
            ms = ev_ms(lambda: eng.run(args.steps)) / args.steps
            lat[mode] = eng.z.clone()
            setup = ev_ms(eng.per_clip_setup)
            res[mode] = {"ms_per_step": round(ms, 3), "per_clip_setup_ms": round(setup, 2)}
            if mode == "fp8":
                res[mode]["weight_quantisation_ms"] = round(ev_ms(eng.quantize_weights, 3), 3)
        del eng
        torch.cuda.empty_cache()
    res["speedup_fp8_over_bf16"] = round(res["bf16"]["ms_per_step"] / res["fp8"]["ms_per_step"], 3)
    d = lat["fp8"].double() - lat["bf16"].double()
    res["latents_rel_l2_fp8_vs_bf16"] = float(d.norm() / lat["bf16"].double().norm())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
