"""Measure the tolerances of tests/test_sde_gpu.py's oracle comparisons, by the method of scripts/calibrate_solvers.py
("2x the error of stock bf16 ops on the same inputs"), per eta and prediction type.

The case is the tests' (tests/sde_cases.py: CASE, STEPS): 2 condition + 2 generated 16x16 frames, N = 4 steps, shift 1, eta
at every step.  tests/sde_cases.py's restatement drives oracle/restate.py's model twice on the same bf16-representable
weights and inputs: once in fp32 (the checker), once with torch's stock CPU bf16 ops (bf16 parameters, activations and
sampler state).  Both runs take the same noise -- the restatement's fp64 normals of (seed, stream 0), rounded to the run's
dtype -- so rel-L2(bf16 run, fp32 run) is what stock bf16 arithmetic costs under that eta, not what another noise draw
would; the tolerance is 2 x the largest value over three seeds, written to tests/golden/tolerance_calibration_sde.json and
read by tests/sde_cases.py::tol().  CPU only, under a minute.

  python scripts/calibrate_sde.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import restate as R       # noqa: E402
from tests import sde_cases as SD     # noqa: E402
from tests import smoke_case as SC    # noqa: E402

BF = torch.bfloat16
SEEDS = (0, 1, 2)


def measure(eta, pt, seed):
    """rel-L2 of the stock-bf16 run against the fp32 run for one quantity and one parameter (and noise) seed."""
    cfg = R.TINY
    table = [eta] * SD.STEPS
    with torch.no_grad():
        p, batch, z, cond = SC.build_case(cfg, seed=seed, **SD.CASE)
        pb = {k: v.to(BF) for k, v in p.items()}
        zb, cb = [t.to(BF) for t in z], [t.to(BF) for t in cond]
        f32 = SD.oracle_sample(cfg, p, batch, z, cond, SD.STEPS, pt, table, seed, 0)
        b16 = SD.oracle_sample(cfg, pb, batch, zb, cb, SD.STEPS, pt, table, seed, 0)
    return SC.rel_l2(torch.cat(b16).float(), torch.cat(f32))


def main():
    torch.manual_seed(0)
    q = {}
    for eta in SD.ETAS:
        for pt in ("x1", "v"):
            vals = [measure(eta, pt, seed) for seed in SEEDS]
            q[f"eta{eta}.{pt}"] = {"stock_bf16_rel_l2_max": round(max(vals), 6),
                                   "stock_bf16_rel_l2_mean": round(sum(vals) / len(vals), 6),
                                   "stock_bf16_rel_l2_seed0": round(vals[0], 6), "samples": len(vals),
                                   "tolerance": round(2 * max(vals), 6)}
    doc = {"what": "rel-L2 of the final latents of tests/sde_cases.py's stochastic Euler sampler driving oracle/restate.py's "
                   f"tiny model (tests/smoke_case.py::build_case with {SD.CASE}, {SD.STEPS} steps, shift 1, CFG scale "
                   f"{SD.SCALE}, eta at every step, the restatement's own fp64 noise of (seed, stream 0) rounded to the run's "
                   "dtype) with torch's stock CPU bf16 ops against the same in fp32, on the same bf16-representable weights, "
                   f"inputs and noise; tolerance = 2 x the largest value over seeds {list(SEEDS)} (SURVEY.md section 8d)",
           "generated_by": "scripts/calibrate_sde.py", "torch": torch.__version__, "quantities": q}
    json.dump(doc, open(SD.PATH, "w"), indent=1)
    for k, v in q.items():
        print(f"{k:12s} stock bf16 max {v['stock_bf16_rel_l2_max']:.3e}  mean {v['stock_bf16_rel_l2_mean']:.3e}  -> tolerance "
              f"{v['tolerance']:.3e}")


if __name__ == "__main__":
    main()
