"""The three sampler solvers restated in plain torch (the checker of tests/test_solver_*.py), beside
oracle/restate.py::scheduler_call, which is the Euler one and stays the checker of the existing tests.

Notation: sigma the scheduler's table, N = len(sigma) - 1, h_i = sigma[i+1] - sigma[i], v_i the velocity of step i (the
prediction, after x1 -> v with the solver's own state and sigma[i], after CFG on the two halves where the solver does it).

  euler  z += h_i v_i
  ab2    step 0 as euler; i >= 1: z += h_i (v_i + h_i / (2 h_{i-1}) (v_i - v_{i-1}))
  heun   i < N - 1: z' = z + h_i v_i, v' = velocity of the model's prediction on z' at sigma[i+1] (converted with z', not
         with what the model was shown), z += h_i / 2 (v_i + v'); i = N - 1 (sigma = 1, x1 -> v singular) as euler

`func(z, timesteps) -> list of predictions` is the contract of R.scheduler_call.  The state keeps the dtype it is given in
(fp64 for the kernel checks, fp32 for the oracle, bf16 for the stock-bf16 calibration); sigma enters as Python floats, so it
never promotes the state.
"""
from __future__ import annotations

import json
import os
from typing import Callable, List, Optional

import torch

SOLVERS = ("euler", "ab2", "heun")
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tolerance_calibration_solvers.json")

_TOL = None


def tol(quantity: str) -> float:
    """2 x the worst rel-L2 of the oracle on stock bf16 ops against its fp32 self under the same solver, measured by
    scripts/calibrate_solvers.py (tests/golden/tolerance_calibration_solvers.json)."""
    global _TOL
    if _TOL is None:
        _TOL = json.load(open(PATH))["quantities"]
    return float(_TOL[quantity]["tolerance"])


def velocity(pred: List[torch.Tensor], z: List[torch.Tensor], s: float, prediction_type: str, guide: bool, scale: float):
    """x1 -> v on the state the prediction was made from, then (guide) CFG: first half conditional, second unconditional,
    both halves get the guided velocity (LVM/scheduler.py:178-200)."""
    v = [(pred[j] - z[j]) / (1.0 - s) for j in range(len(z))] if prediction_type == "x1" else list(pred)
    if guide:
        half = len(v) // 2
        g = [v[half + j] + scale * (v[j] - v[half + j]) for j in range(half)]
        v = g + g
    return v


def solver_call(sigma: torch.Tensor, z: List[torch.Tensor], func: Callable, guide: bool, scale: float,
                prediction_type: str, solver: str, trace: Optional[list] = None):
    """guide: the solver combines the CFG halves itself (the reference does for x1 predictions; for v predictions its
    `func` already returns the guided prediction).  trace: gets a copy of the state after every step."""
    assert solver in SOLVERS, solver
    z = [t.clone() for t in z]
    sig = [float(s) for s in sigma]
    N = len(sig) - 1
    ts = lambda s: torch.zeros(len(z)) + s
    v_prev = None
    for i in range(N):
        s, s_next = sig[i], sig[i + 1]
        h = s_next - s
        v = velocity(list(func(z, ts(sigma[i]))), z, s, prediction_type, guide, scale)
        if solver == "ab2" and i >= 1:
            r = h / (2.0 * (s - sig[i - 1]))
            ve = [v[j] + r * (v[j] - v_prev[j]) for j in range(len(z))]
        elif solver == "heun" and i < N - 1:
            zp = [z[j] + h * v[j] for j in range(len(z))]
            v2 = velocity(list(func(zp, ts(sigma[i + 1]))), zp, s_next, prediction_type, guide, scale)
            ve = [0.5 * (v[j] + v2[j]) for j in range(len(z))]
        else:
            ve = v
        v_prev = v
        z = [z[j] + h * ve[j] for j in range(len(z))]
        if trace is not None:
            trace.append([t.clone() for t in z])
    return z


def model_evaluations(solver: str, num_steps: int) -> int:
    return 2 * num_steps - 1 if solver == "heun" else num_steps


def oracle_func(cfg, p, batch, cond, prediction_type, use_cfg=True, scale=1.6):
    """`func` of the tiny oracle model (tests/smoke_case.py::oracle_sample's)."""
    from oracle import restate as R

    def func(zl, t):
        return R.frame_block_forward_with_cfg(
            p, cfg, zl, t, use_cfg, scale, prediction_type, input_ids=batch["input_ids"], input_img_latents=cond,
            input_image_sizes=batch["input_image_sizes"], attention_mask=batch["attention_mask"],
            position_ids=batch["position_ids"], denoise_image_sizes=batch["denoise_image_sizes"],
            time_emb_inx=batch["time_emb_inx"])
    return func


def oracle_sample(cfg, p, batch, z, cond, steps, prediction_type, solver, use_cfg=True, scale=1.6, shift=1.0):
    """tests/smoke_case.py::oracle_sample under `solver`: CFG in the solver for x1, inside the model call for v."""
    from oracle import restate as R
    return solver_call(R.scheduler_sigma(steps, shift), z, oracle_func(cfg, p, batch, cond, prediction_type, use_cfg, scale),
                       use_cfg and prediction_type == "x1", scale, prediction_type, solver)
