#!/usr/bin/env python3
"""The VAE mid-block attention (video-gpt_amd/vae.py, _Attention.run) with the score matrix materialised (conv2d ->
col_softmax -> conv2d) against the fused kernel (ops.vae_attention, csrc/vae_attn.hip), at C = 512 and
HW = 1024 / 4096 / 16384 positions (frames of 256^2, 512^2, 1024^2), 1 and 8 images.

One process: per shape both implementations are warmed up, then run ALTERNATELY (materialised, fused, materialised, ...),
each run timed with device events, so both see the same clocks; the median of 5 and torch.cuda.max_memory_allocated of each
leg are reported.  "run" is the whole _Attention.run (GroupNorm statistics, q/k/v projections, attention, to_out with the
residual); "core" is the attention alone on the same q, k, v, with its rate in TF/s for 4 HW^2 C flop per image next to the
157.3 TF/s fp32-MFMA peak.  N = 8 at 16384 positions holds 8.6 GB of scores on the materialised leg: it runs last.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself.  One
JSON line per result:
    timeout -k 10 600 python3 scripts/vae_attn_time.py > profiles/vae_attn_time.log
"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 540
C, GROUPS, RUNS = 512, 32, 5
SHAPES = [(1, 32, 32), (8, 32, 32), (1, 64, 64), (8, 64, 64), (1, 128, 128), (8, 128, 128)]
FP32_MFMA_PEAK = 157.3e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def alternate(torch, legs):
    """legs: {name: fn}.  One warm-up each, then RUNS rounds of every leg in turn; per leg the times in ms and the peak
    allocation of its runs."""
    ms, peak = {k: [] for k in legs}, {k: 0 for k in legs}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(RUNS):
        for name, fn in legs.items():
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(round(a.elapsed_time(b), 3))
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated())
    return ms, peak


def child():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vae_attn_time.py needs a GPU")
    ops = importlib.import_module("video-gpt_amd.ops")
    V = importlib.import_module("video-gpt_amd.vae")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    att = V._Attention(C).to(dev, torch.float32).eval()
    scale = 1.0 / C ** 0.5
    med = lambda v: sorted(v)[len(v) // 2]
    with torch.no_grad():
        for N, H, W in SHAPES:
            HW = H * W
            x = torch.randn(N, C, H, W, device=dev)
            q, k, v = (torch.randn(N, C, H, W, device=dev) for _ in range(3))

            def core_materialised():
                st = ops.conv2d(q, k, ksize=1, cout=HW, w_transposed=True, ldw=HW, w_batch_stride=C * HW)
                ops.col_softmax(st.view(N, HW, HW), scale)
                return ops.conv2d(st, v, ksize=1, cout=C, ldw=HW, w_batch_stride=C * HW)

            base = torch.cuda.memory_allocated()
            run_ms, run_peak = alternate(torch, {i: (lambda i=i: att.run(x, GROUPS, 1e-6, "bf16x3", i))
                                                 for i in ("materialised", "fused")})
            core_ms, _ = alternate(torch, {"materialised": core_materialised,
                                           "fused": lambda: ops.vae_attention(q, k, v, scale)})
            flop = 4.0 * HW * HW * C * N
            tf = {i: round(flop / (med(core_ms[i]) * 1e-3) / 1e12, 1) for i in core_ms}
            emit(N=N, C=C, HW=HW, run_ms=run_ms, run_median_ms={i: med(t) for i, t in run_ms.items()},
                 run_peak_MiB_above_inputs={i: round((p - base) / 2 ** 20, 1) for i, p in run_peak.items()},
                 core_ms=core_ms, core_median_ms={i: med(t) for i, t in core_ms.items()}, core_TF_s=tf,
                 fused_core_of_fp32_mfma_peak=round(tf["fused"] * 1e12 / FP32_MFMA_PEAK, 3),
                 fused_over_materialised_run=round(med(run_ms["fused"]) / med(run_ms["materialised"]), 3))
            del x, q, k, v
            torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"vae_attn_time.py: the measurement did not finish within {LIMIT_S} s")
        sys.exit(rc)
