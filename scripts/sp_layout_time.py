#!/usr/bin/env python3
"""Ulysses re-layout kernels of the sharded sampler engine (csrc/sp_layout.hip) at the shapes one rank sees per decoder
layer: pack of the share's (rows, 3 x 3072) q|k|v rows, unpack of the P received (rows, 3072 / P) attention-output
blocks.  Live rows of a step: cfg-2 (bench.py's default workload) 4096; the reference's scripted inference
(320x176, 24 generated frames with CFG: 48 x 220) 10 560.  One JSON line per (config, P, kernel): the share's rows,
bytes moved (read + write), event-timed microseconds per launch and GB/s against the 8 TB/s HBM peak.  Run it under
`rocprofv3 --kernel-trace --stats -- python3 scripts/sp_layout_time.py > LOG` for the kernel-trace durations, then
`python3 scripts/sp_layout_time.py --by-shape <rocprofv3 results.db> LOG OUT.csv` turns the trace into the per-shape table
(median of the 50 timed launches of every shape; no GPU needed).  The launches of a shape reuse the same buffers back to
back and every pair is at most 256 MB, so part of the traffic is served by the last-level cache: the fractions of 8 TB/s
are upper bounds on what a cold HBM round trip reaches.  Single GPU; no collectives."""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, ITERS = 5, 50

NQ = NK = 32
HD = 96
CONFIGS = {"cfg2": 4096, "scripted": 48 * 220}


def timed(fn, iters=ITERS):
    import torch
    for _ in range(WARMUP):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def by_shape(db_path, log_path, out_path):
    """Per-shape medians of the kernel trace, in the launch order main() used (WARMUP + ITERS launches per line)."""
    import sqlite3
    import statistics
    cur = sqlite3.connect(db_path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    nc = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = sorted({(n, s_, e_) for n, s_, e_ in cur.execute(f"select {nc}, start, end from kernels") if "sp_" in n},
                  key=lambda r: r[1])
    lines = [json.loads(l) for l in open(log_path) if l.startswith("{")]
    n = WARMUP + ITERS
    if len(rows) != n * len(lines):
        raise SystemExit(f"{len(rows)} sp_* launches in the trace, expected {n} x {len(lines)}")
    out = ["config,live_rows,P,kernel,share_rows,bytes,calls,median_ns,min_ns,GB_s_at_median,fraction_of_8TB_s,event_timed_us"]
    for i, l in enumerate(lines):
        grp = rows[i * n:(i + 1) * n]
        if not all(("sp_pack" in nm) == (l["kernel"] == "pack") for nm, _, _ in grp):
            raise SystemExit(f"trace order does not match line {i} of {log_path}")
        d = [e_ - s_ for _, s_, e_ in grp[WARMUP:]]
        med = statistics.median(d)
        gbs = l["bytes"] / med
        out.append(f"{l['config']},{l['live_rows']},{l['P']},{l['kernel']},{l['share_rows']},{l['bytes']},{len(d)},"
                   f"{med:.0f},{min(d)},{gbs:.0f},{gbs / 8000:.3f},{l['us']}")
    open(out_path, "w").write("\n".join(out) + "\n")


def main():
    import torch
    ops = importlib.import_module("video-gpt_amd.ops")
    E = importlib.import_module("video-gpt_amd.engine")
    dev = "cuda:0"
    W3 = (NQ + 2 * NK) * HD
    for name, M in CONFIGS.items():
        for P in (2, 4, 8):
            shares, _ = E.sp_shares(M, P)
            m = max(b - a for a, b in shares)
            x = torch.randn(m, W3, device=dev).to(torch.bfloat16)
            packed = torch.empty(P, m, W3 // P, dtype=torch.bfloat16, device=dev)
            blocks = torch.randn(P, m, NQ // P * HD, device=dev).to(torch.bfloat16)
            ctx = torch.empty(m, NQ * HD, dtype=torch.bfloat16, device=dev)
            for kern, fn, nbytes in (
                    ("pack", lambda: ops.sp_pack_qkv(x, P, NQ, NK, HD, out=packed), 2 * x.numel() * 2),
                    ("unpack", lambda: ops.sp_unpack_ctx(blocks, P, out=ctx), 2 * ctx.numel() * 2)):
                us = timed(fn)
                gbs = nbytes / us * 1e-3
                print(json.dumps({"config": name, "live_rows": M, "P": P, "kernel": kern, "share_rows": m, "bytes": nbytes,
                                  "us": round(us, 2), "GB_s": round(gbs, 1), "of_8TB_s": round(gbs / 8000, 3)}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--by-shape":
        by_shape(*sys.argv[2:])
    else:
        main()
