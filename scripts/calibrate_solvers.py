"""Measure the tolerances of tests/test_solver_gpu.py's oracle comparisons, by the method of scripts/calibrate_tolerances.py
("2x the error of stock bf16 ops on the same inputs"), per solver and prediction type.

The case is the tests': tests/smoke_case.py::build_case (2 condition + 2 generated 8x8 frames, CFG 1.6), N = 4 steps, shift
1.  tests/solver_cases.py's restatement of the solver drives oracle/restate.py's model twice on the same bf16-representable
weights and inputs: once in fp32 (the checker), once with torch's stock CPU bf16 ops (bf16 parameters, activations and
sampler state).  rel-L2(bf16 run, fp32 run) is what stock bf16 ops cost under that solver; the tolerance is 2 x the largest
value over three seeds, written to tests/golden/tolerance_calibration_solvers.json and read by tests/solver_cases.py::tol().
CPU only, a few seconds.

  python scripts/calibrate_solvers.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import restate as R          # noqa: E402
from tests import smoke_case as SC       # noqa: E402
from tests import solver_cases as SV     # noqa: E402

BF = torch.bfloat16
STEPS = 4
SEEDS = (0, 1, 2)


def main():
    torch.manual_seed(0)
    cfg = R.TINY
    q = {}
    with torch.no_grad():
        for solver in SV.SOLVERS:
            for pt in ("x1", "v"):
                vals = []
                for seed in SEEDS:
                    p, batch, z, cond = SC.build_case(cfg, seed=seed)
                    pb = {k: v.to(BF) for k, v in p.items()}
                    zb, cb = [t.to(BF) for t in z], [t.to(BF) for t in cond]
                    f32 = SV.oracle_sample(cfg, p, batch, z, cond, STEPS, pt, solver)
                    b16 = SV.oracle_sample(cfg, pb, batch, zb, cb, STEPS, pt, solver)
                    vals.append(SC.rel_l2(torch.cat(b16).float(), torch.cat(f32)))
                q[f"{solver}.{pt}"] = {"stock_bf16_rel_l2_max": round(max(vals), 6),
                                       "stock_bf16_rel_l2_mean": round(sum(vals) / len(vals), 6), "samples": len(vals),
                                       "tolerance": round(2 * max(vals), 6)}
    doc = {"what": "rel-L2 of the final latents of tests/solver_cases.py's solvers driving oracle/restate.py's tiny model "
                   f"(tests/smoke_case.py::build_case, CFG 1.6, {STEPS} steps, shift 1) with torch's stock CPU bf16 ops against "
                   "the same in fp32, on the same bf16-representable weights and inputs; tolerance = 2 x the largest value "
                   f"over seeds {list(SEEDS)} (SURVEY.md section 8d)",
           "generated_by": "scripts/calibrate_solvers.py", "torch": torch.__version__, "quantities": q}
    json.dump(doc, open(SV.PATH, "w"), indent=1)
    for k, v in q.items():
        print(f"{k:10s} stock bf16 max {v['stock_bf16_rel_l2_max']:.3e}  mean {v['stock_bf16_rel_l2_mean']:.3e}  -> tolerance "
              f"{v['tolerance']:.3e}")


if __name__ == "__main__":
    main()
