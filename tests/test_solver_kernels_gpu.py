"""vgpt_sampler_update (csrc/glue.hip: ab2, Heun predictor / corrector, Euler through the new entry) on the device, alone:
hand-derived exact end states, bit identities with the Euler kernel, a straight-line probe, random predictions against the
fp64 restatement of tests/solver_cases.py, and launches outside the sigma table.  z, z_model, v_hist and pred sit between
NaN guard bands that are checked after every launch."""
import importlib

import pytest
import torch

from oracle import restate as R
from tests import solver_cases as SV
from tests.smoke_case import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
BAND = 64
SOLVERS = ("euler", "ab2", "heun")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("video-gpt_amd.ops")


class Guarded:
    """A tensor in the middle of a NaN-filled allocation."""

    def __init__(self, rows, cols, dtype):
        n = rows * cols
        self.full = torch.full((n + 2 * BAND,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.full[BAND:BAND + n].view(rows, cols)

    def bands_intact(self):
        return bool(torch.isnan(self.full[:BAND]).all() and torch.isnan(self.full[-BAND:]).all())

    def bits(self):
        return self.full.view(torch.int32 if self.full.dtype == torch.float32 else torch.int16).clone()


class State:
    def __init__(self, ops, sigma, z0, use_cfg, pred_type, scale=1.6):
        nf, elems = z0.shape
        self.ops, self.nf, self.elems, self.use_cfg, self.scale = ops, nf, elems, use_cfg, scale
        self.pred_type = ops.PRED_X1 if pred_type == "x1" else ops.PRED_V
        self.z, self.zm, self.pred = Guarded(nf, elems, torch.float32), Guarded(nf, elems, BF), Guarded(nf, elems, BF)
        self.vh = Guarded(nf // 2 if use_cfg else nf, elems, torch.float32)
        self.z.t.copy_(z0)
        self.zm.t.copy_(z0)
        self.pred.t.zero_()
        self.vh.t.fill_(12345.0)          # stale history of "the previous clip": nothing may read it before writing it
        self.sigma = sigma.to(DEV, torch.float32).contiguous()
        self.N = self.sigma.numel() - 1
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)

    def buffers(self):
        return (self.z, self.zm, self.pred, self.vh)

    def update(self, solver, stage=0, history=True):
        o = self.ops
        o.sampler_update(self.z.t, self.zm.t, self.pred.t, self.vh.t if history else None, self.sigma, self.step,
                         self.pred_type, self.use_cfg, self.scale, o.SOLVERS[solver], stage)
        torch.cuda.synchronize()
        for b in self.buffers():
            assert b.bands_intact(), (solver, stage, int(self.step.item()))

    def euler_kernel(self):
        self.ops.euler_cfg_update(self.z.t, self.zm.t, self.pred.t, self.sigma, self.step, self.pred_type, self.use_cfg,
                                  self.scale)

    def solve(self, solver, pred_at):
        """The scheduler's loop with the model replaced by pred_at(index into sigma) -> (nf, elems) predictions.  Heun's final
        step goes through its predictor entry, which is a full Euler step there."""
        for i in range(self.N):
            self.pred.t.copy_(pred_at(i))
            if solver == "heun" and i < self.N - 1:
                self.update("heun", 0)
                self.ops.sampler_advance(self.step)
                self.pred.t.copy_(pred_at(i + 1))
                self.update("heun", 1)
            else:
                self.update(solver, 0, history=solver != "euler")
                self.ops.sampler_advance(self.step)
        assert int(self.step.item()) == self.N
        return self.z.t, self.zm.t


# ---- exact probe ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("N", [8, 16])
@pytest.mark.parametrize("solver", SOLVERS)
def test_exact_end_state_on_a_linear_field(ops, solver, N, use_cfg):
    """v prediction, z0 = 0, sigma_i = i/N, prediction i/N at sigma_i: every value dyadic and exact in bf16 and fp32.  Euler is
    the left Riemann sum (N-1)/(2N).  ab2 and Heun integrate a field linear in sigma exactly (to 1/2) except in their one
    Euler step (ab2's first, Heun's last), which is short by h^2/2 = 1/(2N^2): 63/128 at N = 8, 255/512 at N = 16.  With CFG
    (cond i/N, uncond 0, scale 2) the guided velocity doubles and both halves move by it."""
    nf, elems = 4, 256
    sigma = torch.arange(N + 1, dtype=torch.float32) / N
    st = State(ops, sigma, torch.zeros(nf, elems), use_cfg, "v", scale=2.0)

    def pred_at(i):
        p = torch.full((nf, elems), i / N, dtype=BF, device=DEV)
        if use_cfg:
            p[nf // 2:] = 0
        return p
    z, zm = st.solve(solver, pred_at)
    want = (N - 1) / (2 * N) if solver == "euler" else 0.5 - 1 / (2 * N * N)
    if N == 8 and solver != "euler":
        assert want == 63 / 128
    if N == 16 and solver != "euler":
        assert want == 255 / 512
    want *= 2 if use_cfg else 1
    assert torch.equal(z, torch.full_like(z, want)), (z.flatten()[0].item(), want)
    assert torch.equal(zm, torch.full_like(zm, want))


# ---- Euler identities ----------------------------------------------------------------------------------------------------

def _random_case(nf, elems, n_steps, shift, use_cfg, seed=39):
    g = lambda s: torch.Generator("cpu").manual_seed(s)
    sigma = R.scheduler_sigma(n_steps, shift)
    z0 = torch.randn(nf, elems, generator=g(seed))
    if use_cfg:
        z0[nf // 2:] = z0[: nf // 2]
    preds = [torch.randn(nf, elems, generator=g(seed + 1 + i)).to(BF) for i in range(2 * n_steps)]
    return sigma, z0, preds


def _euler_reference(ops, sigma, z0, preds, use_cfg, pred_type):
    st = State(ops, sigma, z0, use_cfg, pred_type)
    for i in range(st.N):
        st.pred.t.copy_(preds[i])
        st.euler_kernel()
        ops.sampler_advance(st.step)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("pred_type", ["x1", "v"])
@pytest.mark.parametrize("use_cfg", [True, False], ids=["cfg", "nocfg"])
def test_euler_identities_bit_for_bit(ops, pred_type, use_cfg):
    nf, elems = 4, 256
    sigma, z0, preds = _random_case(nf, elems, 5, 3.0, use_cfg)
    ref = _euler_reference(ops, sigma, z0, preds, use_cfg, pred_type)
    same = lambda a, b: torch.equal(a.z.t, b.z.t) and torch.equal(a.zm.t, b.zm.t)
    # solver = euler through the new entry (with and without a history pointer) is vgpt_euler_cfg_update
    for history in (False, True):
        st = State(ops, sigma, z0, use_cfg, pred_type)
        for i in range(st.N):
            st.pred.t.copy_(preds[i])
            st.update("euler", 0, history=history)
            ops.sampler_advance(st.step)
        assert same(st, ref)
        assert torch.equal(st.vh.t, torch.full_like(st.vh.t, 12345.0))     # Euler keeps no history
    # ab2 at step 0, and ab2 / heun at N = 1 (sigma = (0, 1)), are the Euler step
    one = torch.tensor([0.0, 1.0])
    ref1 = _euler_reference(ops, one, z0, preds, use_cfg, pred_type)
    ref0 = _euler_reference(ops, sigma[:2].clone(), z0, preds, use_cfg, pred_type)   # one step of h_0 = sigma[1]
    st = State(ops, sigma, z0, use_cfg, pred_type)
    st.pred.t.copy_(preds[0])
    st.update("ab2")
    assert same(st, ref0)
    for solver in ("ab2", "heun"):
        st = State(ops, one, z0, use_cfg, pred_type)
        st.solve(solver, lambda i: preds[i])
        assert same(st, ref1), solver
    # ab2 on the same velocity at every step is Euler (v prediction: the same prediction is the same velocity)
    if pred_type == "v":
        const = [preds[0]] * 5
        refc = _euler_reference(ops, sigma, z0, const, use_cfg, pred_type)
        st = State(ops, sigma, z0, use_cfg, pred_type)
        st.solve("ab2", lambda i: const[i])
        assert same(st, refc)


# ---- straight line -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_constant_x1_prediction_ends_on_it(ops, solver, use_cfg):
    """x1 prediction, the same x* at every evaluation: the velocity field (x* - z) / (1 - sigma) is the straight line to
    x*, which every solver follows exactly and ends on at sigma = 1."""
    nf, elems = 4, 256
    sigma, z0, preds = _random_case(nf, elems, 5, 3.0, use_cfg, seed=77)
    target = preds[0].clone()
    if use_cfg:
        target[nf // 2:] = target[: nf // 2]
    st = State(ops, sigma, z0, use_cfg, "x1")
    z, zm = st.solve(solver, lambda i: target)
    err = rel_l2(z, target.float())
    print(f"{solver}: rel-L2 to x* {err:.3e}")
    assert err < 1e-5


# ---- random predictions against fp64 -------------------------------------------------------------------------------------

# x1 / v x CFG on / off at (4, 256); once more at (2, 240), which is not a multiple of the 256-thread block
RANDOM_CASES = [(pt, cfg, 4, 256) for pt in ("x1", "v") for cfg in (True, False)] + [("x1", True, 2, 240)]


@pytest.mark.parametrize("pred_type,use_cfg,nf,elems", RANDOM_CASES,
                         ids=[f"{pt}-{'cfg' if c else 'nocfg'}-{n}x{e}" for pt, c, n, e in RANDOM_CASES])
@pytest.mark.parametrize("solver", SOLVERS)
def test_random_predictions_against_fp64(ops, solver, pred_type, use_cfg, nf, elems):
    """Shift 3 (non-uniform steps), N = 5; bounds of tests/test_ops_gpu.py::test_euler_cfg_update: 1e-5 on z, 4e-3 on
    z_model."""
    sigma, z0, preds = _random_case(nf, elems, 5, 3.0, use_cfg)
    st = State(ops, sigma, z0, use_cfg, pred_type)
    it = iter(preds)
    z, zm = st.solve(solver, lambda i: next(it))
    it64 = iter(preds)
    ref = SV.solver_call(sigma, [z0[j].double() for j in range(nf)], lambda zl, t: list(next(it64).double()), use_cfg, 1.6,
                         pred_type, solver)
    ref = torch.stack(ref)
    ez, ezm = rel_l2(z, ref), rel_l2(zm, ref)
    print(f"{solver} {pred_type} cfg={use_cfg} {nf}x{elems}: z {ez:.3e}  z_model {ezm:.3e}")
    assert ez < 1e-5
    assert ezm < 4e-3


# ---- outside the table ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_cfg", [True, False], ids=["cfg", "nocfg"])
def test_launches_outside_the_table_touch_nothing(ops, use_cfg):
    nf, elems = 4, 256
    sigma, z0, preds = _random_case(nf, elems, 5, 3.0, use_cfg)
    st = State(ops, sigma, z0, use_cfg, "x1")
    it = iter(preds)
    st.solve("heun", lambda i: next(it))           # leaves *step = N and live values in every buffer
    st.pred.t.copy_(preds[-1])
    before = [b.bits() for b in st.buffers()]
    untouched = lambda: all(torch.equal(b.bits(), a) for b, a in zip(st.buffers(), before))
    for value in (st.N, st.N + 3, -1):                 # a replay past the end of the table (and a step that never was)
        st.step.fill_(value)
        for solver, stage in (("euler", 0), ("ab2", 0), ("heun", 0), ("heun", 1)):
            st.update(solver, stage)
            assert untouched(), (value, solver, stage)
    st.step.zero_()                                    # a corrector without a predictor step before it
    st.update("heun", 1)
    assert untouched()
