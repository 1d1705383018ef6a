#!/usr/bin/env python3
"""What Stage1Trainer(deterministic=True) costs, at bench.py's stage-1 workload (cfg-3: bs 2 x 8 frames at
256^2, 32 layers): a developer probe, not a test.

Kernels, each deterministic entry point against its atomic twin on the same buffers, in ALTERNATING order in one process
(median of 5 rounds of 50 back-to-back launches, device events):
    rmsnorm_bwd      7740 x 3072 (the packed sequence of the workload), with a residual gradient
    ln_mod_bwd       the workload's noisy frames and tokens per frame (16 x 256) at H = 3072
    embed_bwd        the workload's own ids and keep flags (what Stage1Trainer._prepare makes of the batch), H = 3072
Then the step: ONE trainer whose `deterministic` attribute the probe flips between steps (two full-size trainers do not
fit one model), flag off / on alternating, 2 warm-up rounds and 7 timed ones, each step between device events and ended by
a synchronise; overlap_optimizer off.  The spread of the flag-off step is what the flag's cost is read against.  The box
calibration of bench.py (pure-MFMA loop, 1-GiB copy, 8192^3 GEMM) is taken before and after.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself; the
child stops at the first failing status.  ONE JSON line:
    python3 scripts/deterministic_step_time.py > profiles/deterministic_step_time.log
"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 540
ROUNDS, ITERS = 5, 50
WARMUP, STEPS = 2, 7


def med(xs):
    return sorted(xs)[len(xs) // 2]


def timed(fn, iters=ITERS):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(pair):
    """pair: {"atomic": fn, "deterministic": fn} -> microseconds per launch, median and rounds, and the difference."""
    for fn in pair.values():
        for _ in range(3):
            fn()
    us = {k: [] for k in pair}
    for _ in range(ROUNDS):
        for k, fn in pair.items():
            us[k].append(timed(fn))
    out = {k: {"us": round(med(v), 1), "us_rounds": [round(x, 1) for x in v]} for k, v in us.items()}
    out["deterministic_minus_atomic_us"] = round(med(us["deterministic"]) - med(us["atomic"]), 1)
    return out


def kernels(dev, prep, nf, ntok, H, vocab):
    import torch
    T = importlib.import_module("video-gpt_amd.ops_train")
    BF, F32 = torch.bfloat16, torch.float32
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)   # noqa: E731
    res = {}
    rows = 7740
    x, dy, dres = rnd(rows, H).to(BF), rnd(rows, H).to(BF), rnd(rows, H).to(BF)
    w = (1 + 0.3 * rnd(H)).to(BF)
    dx, dw = torch.empty(rows, H, dtype=BF, device=dev), torch.zeros(H, device=dev)
    res["rmsnorm_bwd"] = dict(rows=rows, H=H, **alternate({
        "atomic": lambda: T.rmsnorm_bwd(x, w, dy, dx, dw, 1e-5, dres=dres),
        "deterministic": lambda: T.rmsnorm_bwd(x, w, dy, dx, dw, 1e-5, dres=dres, deterministic=True)}))
    del x, dy, dres, dx

    n_rows = nf * ntok
    hidden, mod = rnd(n_rows, H).to(BF), (0.5 * rnd(nf, 2 * H)).to(BF)
    rowmap = torch.arange(nf, dtype=torch.int32, device=dev) * ntok
    v = torch.empty(n_rows, H, dtype=BF, device=dev)
    xhat, rstd = torch.empty(n_rows, H, dtype=F32, device=dev), torch.empty(n_rows, dtype=F32, device=dev)
    T.ln_mod_fwd(hidden, rowmap, mod, v, xhat, rstd, ntok)
    dv, dhid, dmod = rnd(n_rows, H).to(BF), torch.empty(n_rows, H, dtype=BF, device=dev), torch.zeros(nf, 2 * H, device=dev)
    res["ln_mod_bwd"] = dict(n_frames=nf, ntok=ntok, H=H, **alternate({
        "atomic": lambda: T.ln_mod_bwd(dv, xhat, rstd, mod, rowmap, dhid, dmod, ntok),
        "deterministic": lambda: T.ln_mod_bwd(dv, xhat, rstd, mod, rowmap, dhid, dmod, ntok, deterministic=True)}))
    del hidden, v, xhat, dv, dhid

    ids, keep = prep["ids"].view(-1), prep["keep"]
    dseq = rnd(ids.numel(), H).to(BF)
    table = torch.zeros(vocab, H, device=dev)
    kept = ids[keep.bool()]
    counts = torch.bincount(kept.clamp(0, vocab - 1), minlength=1)
    res["embed_bwd"] = dict(rows=ids.numel(), H=H, vocab=vocab, kept_rows=int(kept.numel()),
                            distinct_ids=int((counts > 0).sum()), rows_of_the_most_frequent_id=int(counts.max()),
                            **alternate({"atomic": lambda: T.embed_bwd(ids, keep, dseq, table),
                                         "deterministic": lambda: T.embed_bwd(ids, keep, dseq, table, deterministic=True)}))
    return res


def child():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("deterministic_step_time.py needs a GPU")
    import bench
    dev = torch.device("cuda:0")
    M = importlib.import_module("video-gpt_amd.model")
    P = importlib.import_module("video-gpt_amd.processor")
    TR = importlib.import_module("video-gpt_amd.train")
    ops = importlib.import_module("video-gpt_amd.ops")
    cal = [bench.calibrate(dev, torch.cuda.Stream(device=dev), ops, "before")]
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
    mk = lambda n: torch.randn(n, 4, *hw, generator=g).to(dev)   # noqa: E731
    x1, x0, clean, x0i = mk(nd), mk(nd), mk(nc), mk(nc)
    t, ti = torch.rand(nd, generator=g).to(dev), (0.9 + 0.1 * torch.rand(nc, generator=g)).to(dev)
    args = (batch, x1, x0, t, clean, x0i, ti)
    tr = TR.Stage1Trainer(model, lr=1e-4, weight_decay=0.1, max_grad_norm=1.0)

    def step(det):
        tr.deterministic = det       # probe only: read by step() at every backward
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.step(*args)
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b), 3)
    for _ in range(WARMUP):
        for det in (False, True):
            step(det)
    ms = {False: [], True: []}
    for _ in range(STEPS):
        for det in (False, True):
            ms[det].append(step(det))
    off, on = ms[False], ms[True]
    step_res = {"flag_off_ms": off, "flag_on_ms": on, "flag_off_median_ms": med(off), "flag_on_median_ms": med(on),
                "flag_off_spread_ms": round(max(off) - min(off), 3), "flag_on_spread_ms": round(max(on) - min(on), 3),
                "deterministic_cost_ms": round(med(on) - med(off), 3),
                "config": "cfg-3: bs 2 x F=8 frames 256^2, 32 layers, one trainer, flag off / on alternating, overlap_optimizer off"}
    prep = tr._prepare(batch)
    H, vocab = model.llm.embed_tokens.weight.shape[1], model.llm.embed_tokens.weight.shape[0]
    kern = kernels(dev, prep, nd, prep["ntok"], H, vocab)
    del tr
    torch.cuda.empty_cache()
    cal.append(bench.calibrate(dev, torch.cuda.Stream(device=dev), ops, "after"))
    print(json.dumps({"probe": "deterministic_step_time", "step": step_res, "kernels_us_per_launch": kern,
                      "calibration": cal}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"deterministic_step_time.py: the measurement did not finish within {LIMIT_S} s")
        sys.exit(rc)
