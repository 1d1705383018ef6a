"""Measure the tolerance of the MX-fp8 sampler tests at head dims 64 and 128 (tests/test_sampler_fp8_head_dims_gpu.py)
instead of guessing it, the way scripts/calibrate_tolerances.py measures the bf16 ones (2 x the error of a
stock implementation of the same arithmetic on the same inputs).

CPU only; the library is never loaded.  oracle/restate.py's sampler runs on the test's own cases (tests/head_dim_cases.py
CONFIGS[64] / [128]; C = 2, G = 2, 16x16 latents, 3 Euler steps with CFG 1.6, x1 prediction) once in fp32 -- the checker of
the tests -- once with torch's stock CPU bf16 ops (bf16 parameters, activations and sampler state, as
calibrate_tolerances.py runs it: what the engine is everywhere outside the fp8 kernels), and once per precision mode with
those bf16 ops and R.attention / R.mlp replaced in-process by copies whose operands go through a numpy model of the MX-fp8
format (OCP e4m3, blocks of 32 sharing a power-of-two scale, the smallest e with amax 2^-e <= 448, round-to-nearest-even):

  attention    q (times softmax scale x log2 e) and k in blocks of 32 along d, v in blocks of 32 keys; the unnormalised
               probabilities exp(s - max) x 2^8 rounded to e4m3, the row sum taken from the unrounded ones (csrc/attn_fp8.hip);
  projections  F.linear of qkv_proj, o_proj, gate_up_proj, down_proj with activations and weights in blocks of 32 along K
               (csrc/gemm_mx8.hip).

Two quantities per head dim and mode over three seeds, tolerance = 2 x the largest value, written to
tests/golden/tolerance_calibration_fp8_head_dims.json:
  hdD.mode          rel-L2 of the sampled latents of the bf16 + MX-fp8 run against the fp32 run   (the test: engine vs oracle)
  hdD.mode.vs_bf16  rel-L2 of the same run against the stock bf16 run                              (the test: engine vs bf16 engine)
The fp8 run is measured on top of bf16 ops because that is what the tests compare: the fp8 engine is the bf16 engine with
other attention / projection kernels, so its distance to the fp32 oracle holds the bf16 error as well (MX-fp8 attention
alone on an fp32 model is 7e-4 from the oracle, the bf16 engine itself about 1e-2).  R.TINY (head dim 96) is measured the
same way as a control row: the existing tests there use a hand-set 6e-2.

  python scripts/calibrate_fp8_head_dims.py
"""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import restate as R            # noqa: E402
from tests import head_dim_cases as HC     # noqa: E402
from tests import smoke_case as SC         # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "tolerance_calibration_fp8_head_dims.json")
BF = torch.bfloat16
MODES = {"attention": (True, False), "linear": (False, True), "both": (True, True)}
SEEDS = (0, 1, 2)
STEPS, C, G, HW = 3, 2, 2, (16, 16)


def _e4m3_grid():
    v = [(m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7) for e in range(16) for m in range(8)]
    return np.array(v[:127], dtype=np.float64)          # non-negative finite values, ascending (the last code is NaN)


GRID = _e4m3_grid()


def round_e4m3(y):
    """|y| <= 448 -> the nearest e4m3 value, ties to the even mantissa."""
    a = np.abs(y)
    idx = np.clip(np.searchsorted(GRID, a), 1, len(GRID) - 1)
    lo, hi = GRID[idx - 1], GRID[idx]
    pick_hi = (a - lo > hi - a) | ((a - lo == hi - a) & ((idx % 2) == 0))
    return np.where(pick_hi, hi, lo) * np.sign(y)


def mx8(x, dim=-1):
    """x (torch, fp32) with blocks of 32 along `dim` rounded through MX-fp8; a ragged last block is padded with zeros."""
    t = x.detach().double().movedim(dim, -1)
    n = t.shape[-1]
    pad = (-n) % 32
    a = np.pad(t.numpy(), [(0, 0)] * (t.dim() - 1) + [(0, pad)]).reshape(*t.shape[:-1], (n + pad) // 32, 32)
    amax = np.abs(a).max(axis=-1, keepdims=True)
    _, e = np.frexp(amax / 448.0)                      # amax / 448 = m 2^e, m in [0.5, 1): amax 2^-e <= 448
    e = np.where(amax > 0, e, 0).astype(np.float64)
    q = round_e4m3(a * 2.0 ** -e) * 2.0 ** e
    q = torch.from_numpy(q.reshape(*t.shape[:-1], n + pad)[..., :n]).to(x.dtype)
    return q.movedim(-1, dim)


def make_layers(attn8, lin8):
    lin = (lambda x, w: F.linear(mx8(x), mx8(w))) if lin8 else F.linear

    def attention(p, cfg, i, hidden, amask, cos, sin):
        B, L, _ = hidden.shape
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        qkv = lin(hidden, p[f"llm.layers.{i}.self_attn.qkv_proj.weight"])
        q = qkv[..., : nh * hd].view(B, L, nh, hd).transpose(1, 2)
        k = qkv[..., nh * hd: nh * hd + nkv * hd].view(B, L, nkv, hd).transpose(1, 2)
        v = qkv[..., nh * hd + nkv * hd:].view(B, L, nkv, hd).transpose(1, 2)
        q, k = R.apply_rope(q, k, cos, sin)
        if not attn8:
            if nkv != nh:
                k, v = k.repeat_interleave(nh // nkv, dim=1), v.repeat_interleave(nh // nkv, dim=1)
            w = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(hd) + amask
            w = torch.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
            o = torch.matmul(w, v)
        else:
            c = (1 / math.sqrt(hd)) * 1.4426950408889634   # scores, statistics and the accumulator are fp32; o is rounded once
            q, k, v = mx8(q.float() * c) / c, mx8(k.float()), mx8(v.float(), dim=2)
            if nkv != nh:
                k, v = k.repeat_interleave(nh // nkv, dim=1), v.repeat_interleave(nh // nkv, dim=1)
            s = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(hd)
            s = s.masked_fill(amask < 0, float("-inf"))
            mx = s.amax(-1, keepdim=True)
            e = torch.exp(s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
            p8 = torch.from_numpy(round_e4m3(e.double().numpy() * 256.0) / 256.0).to(e.dtype)
            l = e.sum(-1, keepdim=True)                  # a row that sees no key (padding) is zero, as in the kernel
            o = torch.where(l > 0, torch.matmul(p8, v) / l.clamp_min(1e-30), torch.zeros_like(l))
        o = o.to(hidden.dtype).transpose(1, 2).reshape(B, L, nh * hd)
        return lin(o, p[f"llm.layers.{i}.self_attn.o_proj.weight"])

    def mlp(p, cfg, i, x):
        gate, up = lin(x, p[f"llm.layers.{i}.mlp.gate_up_proj.weight"]).chunk(2, dim=-1)
        return lin(up * R._ACT[cfg.hidden_act](gate), p[f"llm.layers.{i}.mlp.down_proj.weight"])
    return attention, mlp


def sample(cfg, seed, layers=None, dt=torch.float32):
    p, batch, z, cond = SC.build_case(cfg, C=C, G=G, hw=HW, seed=seed, use_cfg=True)
    p, z, cond = {k: v.to(dt) for k, v in p.items()}, [t.to(dt) for t in z], [t.to(dt) for t in cond]
    keep = R.attention, R.mlp
    try:
        if layers is not None:
            R.attention, R.mlp = layers
        with torch.no_grad():
            return torch.cat(SC.oracle_sample(cfg, p, batch, z, cond, STEPS, "x1", use_cfg=True)).float()
    finally:
        R.attention, R.mlp = keep


def main():
    torch.manual_seed(0)
    q = {}
    for hd, cfg in ((64, HC.CONFIGS[64]), (128, HC.CONFIGS[128]), (96, R.TINY)):
        assert cfg.head_dim == hd
        refs = {seed: sample(cfg, seed) for seed in SEEDS}
        assert torch.equal(refs[0], sample(cfg, 0, make_layers(False, False)))   # with nothing quantised the copies are the oracle
        b16 = {seed: sample(cfg, seed, dt=BF) for seed in SEEDS}
        print(f"hd{hd}: stock bf16 against fp32 max {max(SC.rel_l2(b16[s_], refs[s_]) for s_ in SEEDS):.3e}", flush=True)
        for mode, (attn8, lin8) in MODES.items():
            runs = {seed: sample(cfg, seed, make_layers(attn8, lin8), dt=BF) for seed in SEEDS}
            for name, other in ((f"hd{hd}.{mode}", refs), (f"hd{hd}.{mode}.vs_bf16", b16)):
                v = [SC.rel_l2(runs[seed], other[seed]) for seed in SEEDS]
                q[name] = {"mx_fp8_rel_l2_max": round(max(v), 6), "mx_fp8_rel_l2_mean": round(sum(v) / len(v), 6),
                           "samples": len(v), "tolerance": round(2 * max(v), 6)}
                print(f"{name:24s} bf16 + MX-fp8 model max {max(v):.3e}  mean {sum(v) / len(v):.3e}  -> tolerance {2 * max(v):.3e}", flush=True)
    doc = {"what": "rel-L2 of oracle/restate.py's sampler (3 Euler steps with CFG 1.6, C = 2, G = 2, 16x16 latents) run with torch's "
                   "stock CPU bf16 ops and the operands of attention and / or of the four decoder-layer projections rounded through "
                   "a numpy model of MX-fp8, against its fp32 self (hdD.mode) and against the stock bf16 run (hdD.mode.vs_bf16), on "
                   "the head-dim 64 and 128 configs of tests/head_dim_cases.py; hd96 (R.TINY) is a control row; tolerance = 2 x the "
                   "largest value over the seeds (SURVEY.md section 8d)",
           "generated_by": "scripts/calibrate_fp8_head_dims.py", "torch": torch.__version__, "seeds": list(SEEDS), "quantities": q}
    json.dump(doc, open(PATH, "w"), indent=1)


if __name__ == "__main__":
    main()
