#!/usr/bin/env python3
"""Sequence-parallel training step (train.Stage1Trainer(sequence_parallel=True)) at the stage-4 shapes of
bench.py's stage4 workload (one 16-frame 512^2 clip, L = 31 806 rows, 32 layers): step time and peak memory with the
clip's rows shared by P = 1 / 2 / 4 / 8 GPUs over RCCL, with gradient checkpointing and (--no-ckpt) without, and the two
re-layout kernels of the backward (csrc/sp_layout.hip: vgpt_sp_pack_ctx, vgpt_sp_unpack_qkv_rope with and without tables)
at the shapes one rank launches them with per layer, GB/s beside vgpt_calib_copy of the same byte count in the same run.

UNMEASURED ON MORE THAN ONE GPU: nobody has run the multi-GPU legs yet; no result of this script is quoted anywhere.

The parent never touches a GPU: every leg is a child process (the P ranks under torch.distributed.run, one process per
GPU) with a time limit of its own, and the parent stops at the first leg that fails.  Every rank of a leg trains on the
same clip and the same noise (one sequence-parallel group = the whole world).  One JSON line per result:
    python3 scripts/sp_train_step_time.py --gpus 8 [--no-ckpt] [--layers 32] > LOG
    python3 scripts/sp_train_step_time.py --gpus 1                  # the kernels and the P = 1 step only
--rehearse-on-one-gpu puts all ranks of a leg on cuda:0 over gloo (exercises the code path; the times mean nothing).
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 900
NQ = NK = 32
HD, H = 96, 3072
F, HW = 16, (64, 64)
HBM_PEAK = 8e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, iters=20, warmup=3):
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


def kernels(rows_total):
    """pack_ctx / unpack_qkv (bytes) / unpack_qkv_rope (tables) on the largest share of P = 2 / 4 / 8, each beside
    vgpt_calib_copy moving the same number of bytes (read + write)."""
    import torch
    ops = importlib.import_module("video-gpt_amd.ops")
    E = importlib.import_module("video-gpt_amd.engine")
    L = importlib.import_module("video-gpt_amd._lib")
    dev, BF = "cuda:0", torch.bfloat16
    W = (NQ + 2 * NK) * HD
    for P in (2, 4, 8):
        shares, _ = E.sp_shares(rows_total, P)
        m = max(b - a for a, b in shares)
        dctx = torch.randn(m, NQ * HD, device=dev).to(BF)
        blocks = torch.empty(P, m, NQ // P * HD, dtype=BF, device=dev)
        chunks = torch.randn(P, m, W // P, device=dev).to(BF)
        dqkv = torch.empty(m, W, dtype=BF, device=dev)
        ang = torch.rand(m, HD // 2, device=dev) * 6.28
        cos, nsin = ang.cos().contiguous(), (-ang.sin()).contiguous()
        tables = 2 * cos.numel() * 4
        for name, fn, nbytes in (
                ("pack_ctx", lambda: ops.sp_pack_ctx(dctx, P, out=blocks), 2 * dctx.numel() * 2),
                ("unpack_qkv", lambda: ops.sp_unpack_qkv_rope(chunks, P, NQ, NK, HD, out=dqkv), 2 * dqkv.numel() * 2),
                ("unpack_qkv_rope", lambda: ops.sp_unpack_qkv_rope(chunks, P, NQ, NK, HD, cos, nsin, out=dqkv),
                 2 * dqkv.numel() * 2 + tables)):
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            sp = torch.cuda.current_stream().cuda_stream
            us = timed(fn)
            us_copy = timed(lambda: L.call("vgpt_calib_copy", src.data_ptr(), dst.data_ptr(), src.numel(), sp))
            emit(kernel=name, P=P, share_rows=m, bytes=nbytes, us=round(us, 2), GB_s=round(nbytes / us * 1e-3, 1),
                 calib_copy_us=round(us_copy, 2), calib_copy_GB_s=round(nbytes / us_copy * 1e-3, 1),
                 of_8TB_s=round(nbytes / us * 1e6 / HBM_PEAK, 3))


def step_leg(args):
    """One (P, checkpointing) leg: this process is one of the P ranks."""
    import torch
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = 0 if args.rehearse_on_one_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    importlib.import_module("video-gpt_amd")
    D = importlib.import_module("video-gpt_amd.dist_utils")
    M = importlib.import_module("video-gpt_amd.model")
    PR = importlib.import_module("video-gpt_amd.processor")
    TR = importlib.import_module("video-gpt_amd.train")
    E = importlib.import_module("video-gpt_amd.engine")
    SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
    B = importlib.import_module("bench")
    D.init_from_env("gloo" if args.rehearse_on_one_gpu else "nccl", device)
    if world > 1:
        SPM.initialize_sequence_parallel_state(world)
    hw = (args.latent, args.latent)
    model = B.build_model(M, B.full_config(M, args.layers), device, seed=0)
    proc = PR.LVMProcessor(PR.SpecialTokenizer(10, 11, 12))
    prompt = "".join(f"<|diffusion|><|image_{i + 1}|><img><|image_{i + 1}|></img>" if i < F - 1
                     else f"<|diffusion|><|image_{i + 1}|>" for i in range(F))
    row = proc.process_multi_modal_prompt_training(prompt, [torch.zeros(3, hw[0] * 8, hw[1] * 8) for _ in range(F)])
    batch = proc.collator.collate_stage1([row], F)
    batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()
             if k not in ("input_pixel_values", "output_images")}
    g = torch.Generator("cpu").manual_seed(100)            # the same clip and noise on every rank of the group
    mk = lambda n: torch.randn(n, 4, *hw, generator=g).to(device)
    x1, x0, clean, x0i = mk(F), mk(F), mk(F - 1), mk(F - 1)
    t = torch.rand(F, generator=g).to(device)
    ti = (0.9 + 0.1 * torch.rand(F - 1, generator=g)).to(device)
    tr = TR.Stage1Trainer(model, lr=1e-4, weight_decay=0.1, max_grad_norm=1.0, gradient_checkpointing=not args.no_ckpt,
                          sequence_parallel=world > 1)
    for _ in range(args.warmup):
        tr.step(batch, x1, x0, t, clean, x0i, ti)
    losses = []

    def run():
        for _ in range(args.steps):
            losses.append(tr.step(batch, x1, x0, t, clean, x0i, ti))
    elapsed = D.timed_region(run, torch.cuda.synchronize, device)
    rows = int(batch["input_ids"].shape[1])
    if rank == 0:
        emit(leg="step", P=world, gradient_checkpointing=not args.no_ckpt, layers=args.layers, rows=rows,
             largest_share=max(b - a for a, b in E.sp_shares(rows, world)[0]), steps=args.steps,
             ms_per_step=round(elapsed / max(args.steps, 1) * 1e3, 2),
             peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), loss_last=float(losses[-1].mean()),
             rehearsal_times_invalid=bool(args.rehearse_on_one_gpu))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=8, help="GPUs of this node: the legs are P = 1, 2, 4, 8 up to this")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--latent", type=int, default=HW[0], help="latent height = width (64: 512^2 frames)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-ckpt", action="store_true", help="also run every leg without gradient checkpointing")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true")
    ap.add_argument("--leg", choices=["step", "kernels"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg == "step":
        return step_leg(args)
    if args.leg == "kernels":
        return kernels((2 * F - 1) * ((args.latent // 2) ** 2 + 2))
    common = ["--layers", str(args.layers), "--latent", str(args.latent), "--steps", str(args.steps), "--warmup",
              str(args.warmup)] + (["--rehearse-on-one-gpu"] if args.rehearse_on_one_gpu else [])
    me = os.path.abspath(__file__)
    legs = [[sys.executable, me, "--leg", "kernels"] + common]
    for P in (1, 2, 4, 8):
        if P > args.gpus:
            break
        for ck in ([True, False] if args.no_ckpt else [True]):
            launch = [sys.executable, me] if P == 1 else \
                [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={P}", "--master-addr",
                 "127.0.0.1", "--master-port", str(free_port()), me]
            legs.append(launch + ["--leg", "step"] + common + ([] if ck else ["--no-ckpt"]))
    for argv in legs:
        rc = subprocess.run(argv, cwd=ROOT, timeout=LIMIT_S).returncode
        if rc != 0:
            raise SystemExit(f"leg {' '.join(argv[1:])} ended with status {rc}: stopping here")


if __name__ == "__main__":
    main()
