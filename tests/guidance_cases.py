"""The three sampler solvers under a per-step guidance scale, restated in plain torch (the checker of
tests/test_guidance_*.py), on the arithmetic of tests/solver_cases.py.

table[i] is the image-CFG scale of step i.  A guided step is tests/solver_cases.py's step with scale table[i]; both model
calls of a Heun step use the step's scale.  An entry of exactly 1.0 is an unguided step: the guided velocity IS the
conditional one, v = v_c (not v_u + 1.0 (v_c - v_u), which differs from it by a rounding), and both halves of the state
move by it.  A constant table without a 1.0 is solver_cases.solver_call itself.

`func(z, timesteps) -> predictions` as in solver_cases; `func_cond`, when given, is called in the unguided steps with the
conditional half of the state alone and returns that half's predictions (oracle_sample: the oracle model on the conditional
batch only -- what the engine computes when it skips the unconditional rows).  Without it `func` is called with everything
and the unconditional predictions are dropped.
"""
from __future__ import annotations

import json
import os
from typing import Callable, List, Optional

import torch

from tests import solver_cases as SV

SOLVERS = SV.SOLVERS
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tolerance_calibration_guidance.json")

# the model tests' case: tiny model, 2 condition + 2 generated 16x16 frames (the smallest that hoists: prefix 132 >= 128
# rows, 256 live rows, 128 conditional ones), N = 4 steps at shift 1: sigma = 0, 1/4, 1/2, 3/4, 1
CASE = dict(C=2, G=2, hw=(16, 16))
STEPS = 4
SCALE = 1.6
# "interval": steps 1 and 2 guided at the clip's scale, steps 0 and 3 unguided (Heun's Euler-shaped last step among them);
# "explicit": a decaying scale with the unguided steps in the middle, so every solver crosses both kinds of boundary and
# takes its last step guided
SCHEDULES = {"interval": dict(interval=(0.25, 0.75)), "explicit": dict(schedule=[2.0, 1.0, 1.0, 1.25])}
TABLES = {"interval": [1.0, SCALE, SCALE, 1.0], "explicit": [2.0, 1.0, 1.0, 1.25]}

_TOL = None


def tol(quantity: str) -> float:
    """2 x the worst rel-L2 of the oracle on stock bf16 ops against its fp32 self under the same solver and schedule,
    measured by scripts/calibrate_guidance.py (tests/golden/tolerance_calibration_guidance.json)."""
    global _TOL
    if _TOL is None:
        _TOL = json.load(open(PATH))["quantities"]
    return float(_TOL[quantity]["tolerance"])


def velocity(pred: List[torch.Tensor], z: List[torch.Tensor], s: float, prediction_type: str, scale: float,
             cond_only: bool = False):
    """x1 -> v on the state the prediction was made from, then CFG at `scale` over the two halves; scale exactly 1.0: the
    conditional velocity for both.  cond_only: pred and z are the conditional half alone."""
    v = [(pred[j] - z[j]) / (1.0 - s) for j in range(len(pred))] if prediction_type == "x1" else list(pred)
    half = len(v) if cond_only else len(v) // 2
    if scale == 1.0:
        g = v[:half]
    else:
        g = [v[half + j] + scale * (v[j] - v[half + j]) for j in range(half)]
    return g + g


def solver_call(sigma: torch.Tensor, table, z: List[torch.Tensor], func: Callable, prediction_type: str, solver: str,
                func_cond: Optional[Callable] = None, trace: Optional[list] = None):
    """The solver combines the CFG halves itself, at table[i].  trace: gets a copy of the state after every step."""
    assert solver in SOLVERS, solver
    z = [t.clone() for t in z]
    sig = [float(s) for s in sigma]
    tab = [float(torch.tensor(float(s), dtype=torch.float32)) for s in table]   # the fp32 entry the kernel reads
    N = len(sig) - 1
    assert len(tab) == N
    n, half = len(z), len(z) // 2

    def vel(zs, s_at, s_val, scale):
        if scale == 1.0 and func_cond is not None:
            zc = zs[:half]
            return velocity(list(func_cond(zc, torch.zeros(half) + s_at)), zc, s_val, prediction_type, scale, cond_only=True)
        return velocity(list(func(zs, torch.zeros(n) + s_at)), zs, s_val, prediction_type, scale)
    v_prev = None
    for i in range(N):
        s, s_next = sig[i], sig[i + 1]
        h = s_next - s
        v = vel(z, sigma[i], s, tab[i])
        if solver == "ab2" and i >= 1:
            r = h / (2.0 * (s - sig[i - 1]))
            ve = [v[j] + r * (v[j] - v_prev[j]) for j in range(n)]
        elif solver == "heun" and i < N - 1:
            zp = [z[j] + h * v[j] for j in range(n)]
            v2 = vel(zp, sigma[i + 1], s_next, tab[i])
            ve = [0.5 * (v[j] + v2[j]) for j in range(n)]
        else:
            ve = v
        v_prev = v
        z = [z[j] + h * ve[j] for j in range(n)]
        if trace is not None:
            trace.append([t.clone() for t in z])
    return z


def oracle_funcs(cfg, p, cond, prediction_type, C, G, hw):
    """(func, func_cond): the tiny oracle model on the CFG batch without any combination inside the call (the solver
    guides), and on the conditional batch alone."""
    from oracle import restate as R
    N = (hw[0] // 2) * (hw[1] // 2)
    both = R.collate_inference(C, G, N, use_cfg=True, pad_id=cfg.pad_token_id)
    one = R.collate_inference(C, G, N, use_cfg=False, pad_id=cfg.pad_token_id)

    def call(batch, zl, t, use_cfg, scale):
        return R.frame_block_forward_with_cfg(
            p, cfg, zl, t, use_cfg, scale, prediction_type, input_ids=batch["input_ids"], input_img_latents=cond,
            input_image_sizes=batch["input_image_sizes"], attention_mask=batch["attention_mask"],
            position_ids=batch["position_ids"], denoise_image_sizes=batch["denoise_image_sizes"],
            time_emb_inx=batch["time_emb_inx"])
    return (lambda zl, t: call(both, zl, t, False, 1.0)), (lambda zl, t: call(one, zl, t, False, 1.0))


def oracle_sample(cfg, p, z, cond, table, prediction_type, solver, shift=1.0, C=CASE["C"], G=CASE["G"], hw=CASE["hw"]):
    """The oracle under a scale table: guided steps on the CFG batch, unguided steps on the conditional batch ONLY.  The
    solver guides for both prediction types (for v predictions the reference combines inside the model call: the same
    arithmetic on the same two predictions)."""
    from oracle import restate as R
    func, func_cond = oracle_funcs(cfg, p, cond, prediction_type, C, G, hw)
    return solver_call(R.scheduler_sigma(len(table), shift), table, z, func, prediction_type, solver, func_cond=func_cond)
