#!/usr/bin/env python3
"""LoRA fine-tuning against full fine-tuning at cfg-3 full size (bench.py's stage-1 workload: bs 2 x 8 frames at 256^2,
M = 7740 rows, 32 layers), and the three LoRA kernels (csrc/lora.hip) against vgpt_matmul_generic on the same products.

One process: a full-fine-tuning Stage1Trainer and an r = 8 LoRA Stage1Trainer on the same model, both warmed up, then
ALTERNATING steps (full, LoRA, full, ...) each timed with device events, so both see the same clocks.  overlap_optimizer is
off in both: under alternation the full step's AdamW would otherwise run under the LoRA step's forward.  Then every kernel at
the shapes one decoder layer launches it with (K = 3072, N = 9216 / 3072, rp = 16): microseconds per launch, algorithmic
bytes (every operand once; Y of up_add read and written) over that time next to the 8 TB/s HBM peak, and the generic
kernel's time for the same product (for up_add: its accumulate form, which does not rotate).  The buffers of a shape are
reused back to back and fit the last-level cache in part: the fractions of 8 TB/s are upper bounds on a cold round trip.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself; the
child stops at the first failing status (any VgptError ends it with a non-zero exit code).  One JSON line per result:
    python3 scripts/lora_step_time.py > profiles/lora_step_time.log
"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 420
WARMUP, STEPS, ITERS = 2, 5, 20
M_ROWS, H, NQ, NK, HD, RP = 7740, 3072, 32, 32, 96, 16
HBM_PEAK = 8e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, iters=ITERS, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernels(dev):
    import torch
    LO = importlib.import_module("video-gpt_amd.ops_lora")
    T = importlib.import_module("video-gpt_amd.ops_train")
    BF, F32 = torch.bfloat16, torch.float32
    rnd = lambda *s: (torch.randn(*s, device=dev) * 0.1).to(BF)
    for N in (3 * H, H):
        x, y = rnd(M_ROWS, H), rnd(M_ROWS, N)
        a, b, u = rnd(RP, H), rnd(N, RP), rnd(M_ROWS, RP)
        at, bt = a.t().contiguous(), b.t().contiguous()
        uo, gn, gt = torch.empty(M_ROWS, RP, dtype=BF, device=dev), torch.empty(N, RP, dtype=F32, device=dev), \
            torch.empty(RP, N, dtype=F32, device=dev)
        big = M_ROWS * N * 2
        small = N * RP * 2 + M_ROWS * RP * 2
        cases = [
            ("down u = x A^T (K=3072)", M_ROWS * H * 2 + RP * H * 2 + M_ROWS * RP * 2,
             lambda: LO.lora_down(x, a, RP, out=uo), lambda: T.matmul(x, a, out=uo, tb=True)),
            (f"down du = dy B (K={N})", big + small,
             lambda: LO.lora_down(y, b, RP, s_is_k_by_rp=True, out=uo), lambda: T.matmul(y, b, out=uo)),
            (f"up_add y += u B^T (N={N})", 2 * big + small,
             lambda: LO.lora_up_add(y, u, b), lambda: T.matmul(u, b, out=y, tb=True, accumulate=True)),
            (f"up_add dx += du A (N={N})", 2 * big + small,
             lambda: LO.lora_up_add(y, u, bt, s_is_rp_by_n=True), lambda: T.matmul(u, bt, out=y, accumulate=True)),
            (f"grad dB = dy^T u (N={N})", big + M_ROWS * RP * 2 + N * RP * 4,
             lambda: LO.lora_grad(y, u, gn), lambda: T.matmul(y, u, out=gn, ta=True, out_dtype=F32)),
            (f"grad dA = du^T x, stored (rp, N) (N={N})", big + M_ROWS * RP * 2 + N * RP * 4,
             lambda: LO.lora_grad(y, u, gt, transposed=True), lambda: T.matmul(u, y, out=gt, ta=True, out_dtype=F32)),
        ]
        for name, nbytes, new, generic in cases:
            us_new, us_gen = timed(new), timed(generic, iters=5, warmup=1)
            emit(kernel=name, M=M_ROWS, rp=RP, alg_bytes=nbytes, us=round(us_new, 1), TB_s=round(nbytes / us_new * 1e-6, 2),
                 of_8TB_s=round(nbytes / us_new * 1e6 / HBM_PEAK, 3), generic_us=round(us_gen, 1),
                 speedup_vs_generic=round(us_gen / us_new, 1))
        y.zero_()


def steps(dev):
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
    lora = TR.Stage1Trainer(model, lr=1e-4, weight_decay=0.1, max_grad_norm=1.0, lora_rank=8)
    lora_state = torch.cuda.memory_allocated(dev) - base
    full = TR.Stage1Trainer(model, lr=1e-4, weight_decay=0.1, max_grad_norm=1.0)
    full_state = torch.cuda.memory_allocated(dev) - base - lora_state
    emit(persistent_state_bytes={"full (gradient buckets, fp32 masters, moments, flat parameter copies)": full_state,
                                 "lora r=8 (working copy, master, moments, gradient bucket)": lora_state},
         adapter_values_exchanged_per_step=lora.lora_param.numel())
    for _ in range(WARMUP):
        full.step(*args)
        lora.step(*args)
    torch.cuda.synchronize()
    ms = {"full": [], "lora": []}
    for _ in range(STEPS):
        for name, tr in (("full", full), ("lora", lora)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.step(*args)
            b.record()
            torch.cuda.synchronize()
            ms[name].append(round(a.elapsed_time(b), 2))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    emit(step_ms=ms, median_ms=med, lora_over_full=round(med["lora"] / med["full"], 3),
         config="cfg-3: bs 2 x F=8 frames 256^2, 32 layers, r = 8 on qkv_proj + o_proj, alternating steps, overlap_optimizer off")


def child():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lora_step_time.py needs a GPU")
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
            raise SystemExit(f"lora_step_time.py: the measurement did not finish within {LIMIT_S} s")
        sys.exit(rc)
