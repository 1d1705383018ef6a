"""Developer probe (GPU): MX-fp8 attention against the bf16 kernel at head dims 64, 96 and 128 on the cfg-2 engine layout
(hoisted: 1152-row prefix, 4096 live rows, L = 5248) at the same model width (3072 = 48 x 64 = 32 x 96 = 24 x 128 heads).
Per head dim, in one process and alternating: the bf16 kernel, the fp8 path (quantise from row 0 + attention) and the fp8
attention kernel alone; `--rounds` windows of `--n` launches each between device events, every shape warmed up first; the
median and the spread over the windows are printed.  The FLOP count is the algorithm's (4 x heads x d x visible pairs)."""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
importlib.import_module("video-gpt_amd")
ops = importlib.import_module("video-gpt_amd.ops")
L_ = importlib.import_module("video-gpt_amd._lib")
P = importlib.import_module("video-gpt_amd.processor")
LY = importlib.import_module("video-gpt_amd.layout")
dev, BF = "cuda:0", torch.bfloat16


def window(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    C, G, bl = 4, 8, 258
    lay = LY.TokenLayout.from_plans([(P.plan_inference([C, G])[0], bl, 0), (P.plan_inference([0, G])[0], bl, C * bl)], (C + G) * bl)
    packed, _ = lay.pack()
    S0, nf, N = C * bl, 16, 256
    x_old = [S0 + f * bl + 2 for f in range(G)] + [S0 + G * bl + f * bl + 2 for f in range(G)]
    d_old = [x - 2 for x in x_old]
    t_old = [x - 1 for x in x_old]
    S = (S0 + 2 * nf + 127) // 128 * 128
    perm = list(range(S0)) + d_old + t_old + [-1] * (S - S0 - 2 * nf) + [x + j for x in x_old for j in range(N)]
    pm = packed.permute(np.array(perm)).packed_mask(dev)
    L = len(perm)
    segs = ((0, S, S + 2048), (0, S + 2048, L))
    pairs = int(np.unpackbits(pm.bits[0, S:L].contiguous().view(torch.uint8).cpu().numpy()).sum())
    print(f"cfg-2 layout: L = {L}, live rows [{S}, {L}), {pairs} visible (row, key) pairs; {args.rounds} windows of {args.n} launches")
    for hd in (64, 96, 128):
        nh = 3072 // hd
        hq = nh * hd
        qkv = torch.randn(1, L, 3 * hq, device=dev, generator=torch.Generator(dev).manual_seed(hd)).to(BF)
        a = torch.empty(1, L - S, hq, device=dev, dtype=BF)
        b = torch.empty_like(a)
        ws = ops.attention_fp8_workspace_hd(1, L, nh, nh, hd, dev)
        plan = pm.plan(segs)
        runs = {
            "bf16 kernel": lambda: ops.attention_qkv_range(qkv, pm, nh, nh, hd, S, a, segments=segs),
            "fp8 quantise + attention": lambda: ops.attention_qkv_fp8_hd(qkv, pm, nh, nh, hd, out=b, q_start=S, segments=segs, workspace=ws),
            "fp8 attention kernel alone": lambda: L_.call(
                "vgpt_attn_fwd_plan_fp8_hd", ws.data_ptr(), b.data_ptr() - S * hq * 2, pm.bits.data_ptr(), plan.items.data_ptr(),
                plan.summary.data_ptr(), plan.order.data_ptr(), plan.n_items, 1, L, nh, nh, hd, L * hq, hd, hq, ops._stream()),
        }
        for fn in runs.values():
            window(fn, 10)
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                times[k].append(window(fn, args.n))
        flops = 4 * nh * hd * pairs
        for k, v in times.items():
            med = statistics.median(v)
            print(f"head_dim {hd:3d} ({nh} heads) {k:28s} median {med:7.1f} us  (min {min(v):.1f}, max {max(v):.1f})  "
                  f"{flops / med / 1e6:5.0f} TF/s algorithmic")
        print(f"head_dim {hd:3d} fp8 vs bf16 output: rel-L2 {float((a.float() - b.float()).norm() / a.float().norm()):.3e}")


if __name__ == "__main__":
    main()
