"""Measure the tolerances of tests/test_guidance_gpu.py's oracle comparisons, by the method of scripts/calibrate_solvers.py
("2x the error of stock bf16 ops on the same inputs"), per solver, prediction type and guidance
schedule.

The case is the tests' (tests/guidance_cases.py: CASE, STEPS, TABLES): 2 condition + 2 generated 16x16 frames, N = 4 steps,
shift 1, the "interval" and "explicit" scale tables.  tests/guidance_cases.py's restatement drives oracle/restate.py's model
twice on the same bf16-representable weights and inputs: once in fp32 (the checker), once with torch's stock CPU bf16 ops
(bf16 parameters, activations and sampler state).  rel-L2(bf16 run, fp32 run) is what stock bf16 ops cost under that solver
and schedule; the tolerance is 2 x the largest value over three seeds, written to
tests/golden/tolerance_calibration_guidance.json and read by tests/guidance_cases.py::tol().  CPU only, under a minute.

  python scripts/calibrate_guidance.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import restate as R          # noqa: E402
from tests import guidance_cases as GC   # noqa: E402
from tests import smoke_case as SC       # noqa: E402

BF = torch.bfloat16
SEEDS = (0, 1, 2)


def measure(solver, pt, name, seed):
    """rel-L2 of the stock-bf16 run against the fp32 run for one quantity and one parameter seed."""
    cfg = R.TINY
    with torch.no_grad():
        p, _, z, cond = SC.build_case(cfg, seed=seed, **GC.CASE)
        pb = {k: v.to(BF) for k, v in p.items()}
        zb, cb = [t.to(BF) for t in z], [t.to(BF) for t in cond]
        f32 = GC.oracle_sample(cfg, p, z, cond, GC.TABLES[name], pt, solver)
        b16 = GC.oracle_sample(cfg, pb, zb, cb, GC.TABLES[name], pt, solver)
    return SC.rel_l2(torch.cat(b16).float(), torch.cat(f32))


def main():
    torch.manual_seed(0)
    q = {}
    for solver in GC.SOLVERS:
        for pt in ("x1", "v"):
            for name in GC.TABLES:
                vals = [measure(solver, pt, name, seed) for seed in SEEDS]
                q[f"{solver}.{pt}.{name}"] = {"stock_bf16_rel_l2_max": round(max(vals), 6),
                                              "stock_bf16_rel_l2_mean": round(sum(vals) / len(vals), 6),
                                              "stock_bf16_rel_l2_seed0": round(vals[0], 6), "samples": len(vals),
                                              "tolerance": round(2 * max(vals), 6)}
    doc = {"what": "rel-L2 of the final latents of tests/guidance_cases.py's solvers under a per-step guidance scale driving "
                   f"oracle/restate.py's tiny model (tests/smoke_case.py::build_case with {GC.CASE}, {GC.STEPS} steps, shift 1, "
                   f"scale tables {GC.TABLES}) with torch's stock CPU bf16 ops against the same in fp32, on the same "
                   f"bf16-representable weights and inputs; tolerance = 2 x the largest value over seeds {list(SEEDS)} "
                   "(SURVEY.md section 8d)",
           "generated_by": "scripts/calibrate_guidance.py", "torch": torch.__version__, "quantities": q}
    json.dump(doc, open(GC.PATH, "w"), indent=1)
    for k, v in q.items():
        print(f"{k:22s} stock bf16 max {v['stock_bf16_rel_l2_max']:.3e}  mean {v['stock_bf16_rel_l2_mean']:.3e}  -> tolerance "
              f"{v['tolerance']:.3e}")


if __name__ == "__main__":
    main()
