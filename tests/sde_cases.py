"""The stochastic Euler step restated in numpy / plain torch: the checker of tests/test_sde_*.py.

  x0_hat = z - sigma_i v,   z' = (z + h v) + (1 - sigma_{i+1}) ((sqrt(1 - eta_i^2) - 1) x0_hat + eta_i eps)

h = sigma_{i+1} - sigma_i, v the guided velocity of step i (tests/solver_cases.py's, or tests/guidance_cases.py's under a
scale table), eta_i in [0, 1].  With eta_i == 0, and at the last step (1 - sigma_{i+1} == 0), the step is Euler's and no
noise term is formed.

eps is counter-based: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11;
multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85) keyed by the seed's two 32-bit words, on the
counter (block low, block high, step, stream low word), block = e >> 2, e the element index within one CFG half, frame-major.
The four words w0..w3 of a block give elements 4 block .. 4 block + 3: u1 = ((w0 >> 9) + 0.5) 2^-23, u2 = (w1 >> 8) 2^-24,
r = sqrt(-2 ln u1), (r cos(2 pi u2), r sin(2 pi u2)), and the same from (w2, w3).  Here the map is evaluated in fp64 from the
same integer words the kernel uses; both CFG halves get the same numbers.
"""
from __future__ import annotations

import json
import os
from typing import Callable, List, Optional

import numpy as np
import torch

from tests import guidance_cases as GC
from tests import solver_cases as SV

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tolerance_calibration_sde.json")
CASE = GC.CASE          # the model tests' case: tiny model, 2 condition + 2 generated 16x16 frames
STEPS = GC.STEPS
SCALE = GC.SCALE
ETAS = (0.5, 1.0)
EPS_MAX = float(np.sqrt(48 * np.log(2.0)))   # u1 >= 2^-24: r <= sqrt(2 * 24 ln 2)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

_TOL = None


def tol(quantity: str) -> float:
    """2 x the worst rel-L2 of the oracle on stock bf16 ops against its fp32 self under the same eta and noise, measured by
    scripts/calibrate_sde.py (tests/golden/tolerance_calibration_sde.json)."""
    global _TOL
    if _TOL is None:
        _TOL = json.load(open(PATH))["quantities"]
    return float(_TOL[quantity]["tolerance"])


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------

def philox4x32_10(counter, key) -> np.ndarray:
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> (..., 4) uint32."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def noise_words(seed: int, stream: int, step: int, n: int) -> np.ndarray:
    """The Philox words of elements 0 .. n - 1: ((n + 3) // 4, 4) uint32."""
    seed, stream = int(seed) % (1 << 64), int(stream) % (1 << 64)
    block = np.arange((n + 3) // 4, dtype=np.uint64)
    return philox4x32_10((block & _MASK, block >> _S32, np.uint64(int(step) & 0xFFFFFFFF), np.uint64(stream & 0xFFFFFFFF)),
                         (seed & 0xFFFFFFFF, seed >> 32))


def uniforms(words: np.ndarray):
    """(u1, u2) of the two Box-Muller pairs of every block, fp64 (both are exact in fp32 as well): (blocks, 2) each."""
    w = words.astype(np.uint64)
    u1 = ((w[:, 0::2] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (w[:, 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normals_from_words(words: np.ndarray) -> np.ndarray:
    """Box-Muller in fp64 on the integer words: (blocks, 4) -> blocks * 4 normals, lanes (cos, sin, cos, sin).  The angle is
    reduced exactly (2 u2 is a multiple of 2^-23 in [0, 2)) before pi enters, as sincospi does."""
    u1, u2 = uniforms(words)
    r = np.sqrt(-2.0 * np.log(u1))
    t = 2.0 * u2
    q = np.floor(t * 2.0 + 0.5)                 # the nearest multiple of 1/2: t = q / 2 + f, |f| <= 1/4
    f = (t - q * 0.5) * np.pi
    cf, sf = np.cos(f), np.sin(f)
    qi = q.astype(np.int64) % 4
    c = np.choose(qi, [cf, -sf, -cf, sf])
    s = np.choose(qi, [sf, cf, -sf, -cf])
    return np.stack([r * c, r * s], axis=-1).reshape(-1)   # (blocks, pair, lane) -> block-major, pair, (cos, sin)


def normals(seed: int, stream: int, step: int, n: int) -> np.ndarray:
    """eps(seed, stream, step, e) for e < n, fp64."""
    return normals_from_words(noise_words(seed, stream, step, n))[:n]


# ---- the update ------------------------------------------------------------------------------------------------------------

def sde_update(z, v, s: float, s_next: float, eta: float, eps):
    """One step on one tensor, in the dtype of z (eps is cast to it)."""
    ze = z + (s_next - s) * v
    g = 1.0 - s_next
    if eta == 0.0 or g == 0.0:
        return ze
    x0 = z - s * v
    return ze + g * ((float(np.sqrt(1.0 - eta * eta)) - 1.0) * x0 + eta * eps.to(z.dtype))


def sde_call(sigma, eta_table, z: List[torch.Tensor], func: Callable, prediction_type: str, seed: int, stream: int,
             guide: bool = False, scale: float = 1.0, table=None, share_halves: bool = True, func_cond=None,
             trace: Optional[list] = None, noise: Optional[Callable] = None):
    """The Euler solver of tests/solver_cases.py (table None: `guide` / `scale` as there) or of tests/guidance_cases.py (a
    per-step scale table: the solver guides, `func_cond` as there) with the step's eta.  share_halves (and guiding, which
    implies it): entries [n/2, n) of z get the noise of [0, n/2).  noise(step, n) -> n fp64 values replaces the restatement's
    own (the kernel tests feed the kernel's fill)."""
    z = [t.clone() for t in z]
    sig = [float(s) for s in sigma]
    etas = [0.0] * (len(sig) - 1) if eta_table is None else [float(torch.tensor(float(e), dtype=torch.float32)) for e in eta_table]
    N = len(sig) - 1
    assert len(etas) == N
    n = len(z)
    shared = guide or table is not None or share_halves
    half = n // 2 if shared else n
    per = z[0].numel()
    tab = None if table is None else [float(torch.tensor(float(s), dtype=torch.float32)) for s in table]
    for i in range(N):
        s, s_next = sig[i], sig[i + 1]
        if tab is None:
            v = SV.velocity(list(func(z, torch.zeros(n) + sigma[i])), z, s, prediction_type, guide, scale)
        elif tab[i] == 1.0 and func_cond is not None:
            zc = z[:n // 2]
            v = GC.velocity(list(func_cond(zc, torch.zeros(n // 2) + sigma[i])), zc, s, prediction_type, 1.0, cond_only=True)
        else:
            v = GC.velocity(list(func(z, torch.zeros(n) + sigma[i])), z, s, prediction_type, tab[i])
        if etas[i] != 0.0 and 1.0 - s_next != 0.0:
            e = noise(i, half * per) if noise is not None else normals(seed, stream, i, half * per)
            e = torch.from_numpy(np.asarray(e, dtype=np.float64)).reshape(half, *z[0].shape)
            eps = [e[j % half] for j in range(n)]
        else:
            eps = [None] * n
        z = [sde_update(z[j], v[j], s, s_next, etas[i], eps[j]) for j in range(n)]
        if trace is not None:
            trace.append([t.clone() for t in z])
    return z


def oracle_sample(cfg, p, batch, z, cond, steps, prediction_type, eta_table, seed, stream, guidance=None, use_cfg=True,
                  scale=SCALE, shift=1.0):
    """tests/smoke_case.py::oracle_sample under an eta table.  guidance None: CFG at `scale` in the solver for x1, inside
    the model call for v (tests/solver_cases.py).  guidance = a scale table: tests/guidance_cases.py's oracle (the solver
    guides, unguided steps on the conditional batch only; `batch` is rebuilt from CASE there)."""
    from oracle import restate as R
    sigma = R.scheduler_sigma(steps, shift)
    if guidance is None:
        func = SV.oracle_func(cfg, p, batch, cond, prediction_type, use_cfg, scale)
        return sde_call(sigma, eta_table, z, func, prediction_type, seed, stream, guide=use_cfg and prediction_type == "x1",
                        scale=scale, share_halves=use_cfg)
    func, func_cond = GC.oracle_funcs(cfg, p, cond, prediction_type, CASE["C"], CASE["G"], CASE["hw"])
    return sde_call(sigma, eta_table, z, func, prediction_type, seed, stream, table=guidance, func_cond=func_cond)


# ---- the kernel tests' references: fp64 from the fp32 operands, with the running bound of the fp32 evaluation --------------

PRED_V, PRED_X1 = 0, 1
# (seed, stream) and step indices at which block 0 has an exact Box-Muller angle (2 u2 = quarter / 4 turns of pi in the pair
# `pair`): cospi / sinpi are exactly 0 or +-1 there, so one lane of the pair is exactly 0 and the other exactly +-r.  Any
# other word w1 (w3) gives a non-zero value in that lane: the probe pins the integer word.  Found by a search over the step
# word; tests/test_sde_cabi.py checks the words.
PROBE_KEY = (0x1234, 5)
PROBES = [(4331397, 0, 0), (1764256, 0, 1), (8395136, 0, 2), (5905454, 1, 1)]   # (step, pair, quarter)


def noise_bound(eps64: np.ndarray) -> np.ndarray:
    """|fp32 eps - fp64 eps| at the kernel's rounding points, u1 and u2 being exact: logf within 1 ulp (half of its relative
    error survives the square root), sqrtf correctly rounded (0.5 ulp), sincospif within 1 ulp of a result computed from
    an exactly reduced argument, one rounded product (0.5 ulp); an ulp is at most 2^-23 of the value.  Together
    (0.5 + 0.5 + 1 + 0.5) 2^-23 |eps|, first order."""
    return 2.5 * 2.0 ** -23 * np.abs(eps64) * (1 + 2.0 ** -10)


def model_noise_f32(seed, stream, step, n) -> np.ndarray:
    """numpy float32 at the kernel's rounding points: logf, one product, sqrtf, the trigonometric value rounded once, one
    product."""
    f = np.float32
    u1, u2 = uniforms(noise_words(seed, stream, step, n))
    r = np.sqrt(f(-2.0) * np.log(u1.astype(f)))
    t = 2.0 * u2
    q = np.floor(t * 2.0 + 0.5)
    a = (t - q * 0.5) * np.pi
    cf, sf = np.cos(a), np.sin(a)
    qi = q.astype(np.int64) % 4
    c = np.choose(qi, [cf, -sf, -cf, sf]).astype(f)
    s = np.choose(qi, [sf, cf, -sf, -cf]).astype(f)
    out = np.stack([r * c, r * s], axis=-1).reshape(-1)[:n]
    assert out.dtype == f
    return out


def _hu(x):
    from tests.kernel_guards import half_ulp32
    return half_ulp32(torch.as_tensor(x, dtype=torch.float64))


def sde_reference(z0, pred, sigma, step, pred_type, use_cfg, scale, eta, eps, share=False):
    """One launch in fp64 from the fp32 operands: (z64, bound).  z0 (nf, elems) fp32, pred bf16, sigma fp32 table, scale /
    eta the fp32 values the kernel reads (scale exactly 1.0 with `unguided`-table semantics is passed as scale=None), eps
    (noise rows, elems): the kernel's own fill.  The bound follows the kernel's rounding points with half an fp32 ulp each
    (tests/test_glue_kernels_gpu.py::euler_reference for the Euler part), first order in 2^-24."""
    hu = _hu
    sg, sg_next = sigma[step].double(), sigma[step + 1].double()
    dt = sg_next - sg
    e_dt = hu(dt)
    z, p = z0.double(), pred.double()
    if pred_type == PRED_X1:
        inv = 1 / (1 - sg)
        e_inv = hu(1 - sg) * inv * inv + hu(inv)
        d = p - z
        v = d * inv
        e_v = hu(d) * inv + d.abs() * e_inv + hu(v)
    else:
        v, e_v = p, torch.zeros_like(p)
    nf = z.shape[0]
    if use_cfg:
        half = nf // 2
        if scale is None:                          # an unguided entry: v = v_c for both halves
            v, e_v = torch.cat([v[:half]] * 2), torch.cat([e_v[:half]] * 2)
        else:
            vc, vu, e_vc, e_vu = v[:half], v[half:], e_v[:half], e_v[half:]
            diff = vc - vu
            e_diff = e_vc + e_vu + hu(diff)
            e_prod = abs(scale) * e_diff + hu(scale * diff)
            guided = vu + scale * diff
            e_g = e_vu + e_prod + hu(guided)
            v, e_v = torch.cat([guided, guided]), torch.cat([e_g, e_g])
    ze = z + dt * v
    e_ze = v.abs() * e_dt + abs(dt) * e_v + hu(dt * v) + hu(ze)
    g = 1.0 - sg_next
    eta = float(eta)
    if eta == 0.0 or float(g) == 0.0:
        return ze, e_ze * (1 + 2.0 ** -10)
    rows = nf // 2 if (use_cfg or share) else nf
    e64 = torch.as_tensor(np.asarray(eps, dtype=np.float64)).reshape(rows, -1)
    e64 = torch.cat([e64] * (nf // rows))
    e_g = hu(g)
    e2 = torch.tensor(eta * eta, dtype=torch.float64)
    om = 1.0 - e2
    e_om = hu(e2) + hu(om)
    sq = torch.sqrt(om)
    e_sq = (e_om / (2 * sq) if float(sq) > 0 else torch.sqrt(e_om)) + hu(sq)
    ca = sq - 1.0
    e_ca = e_sq + hu(ca)
    x0 = z - sg * v
    e_x0 = sg * e_v + hu(x0)
    pr = ca * x0
    e_pr = x0.abs() * e_ca + ca.abs() * e_x0 + hu(pr)
    t = eta * e64 + pr
    e_t = e_pr + hu(t)
    out = ze + g * t
    bound = e_ze + t.abs() * e_g + g.abs() * e_t + hu(out)
    return out, bound * (1 + 2.0 ** -10)


def model_sde_f32(z0, pred, sigma, step, pred_type, use_cfg, scale, eta, eps, share=False):
    """numpy float32 at the kernel's rounding points (csrc/glue.hip: sde_update_kernel).  fma(a, b, c) is a * b + c in fp64
    rounded once to fp32 (the double rounding matters only within 2^-29 of a tie)."""
    f = np.float32
    fma = lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f)
    sg, sg_next = f(sigma[step]), f(sigma[step + 1])
    dt, inv, g = f(sg_next - sg), f(f(1.0) / f(f(1.0) - sg)), f(f(1.0) - sg_next)
    z, p = z0.numpy().astype(f), pred.float().numpy()
    nf = z.shape[0]
    half = nf // 2
    v = ((p - z) * inv).astype(f) if pred_type == PRED_X1 else p
    if use_cfg:
        vg = v[:half] if scale is None else fma(f(scale), (v[:half] - v[half:]).astype(f), v[half:])
        zn = np.concatenate([z[:half] + (dt * vg).astype(f), fma(dt, vg, z[half:])]).astype(f)
        v = np.concatenate([vg, vg])
    else:
        zn = (z + (dt * v).astype(f)).astype(f)
    eta = f(eta)
    if eta == 0 or g == 0:
        return torch.from_numpy(zn)
    rows = half if (use_cfg or share) else nf
    e = np.asarray(eps, dtype=f).reshape(rows, -1)
    e = np.concatenate([e] * (nf // rows))
    ca = f(np.sqrt(f(f(1.0) - f(eta * eta))) - f(1.0))
    x0 = fma(-sg, v, z)
    return torch.from_numpy(fma(g, fma(eta, e, (ca * x0).astype(f)), zn))
