"""vgpt_sampler_update_sched (csrc/glue.hip: the solver updates under a device table of per-step guidance scales) on the
device, alone: a constant table against vgpt_sampler_update bit for bit, unguided entries with NaN where the unconditional
predictions would be, a mixed table against the fp64 restatement of tests/guidance_cases.py, hand-derived exact end states,
and launches outside the table.  z, z_model, v_hist, pred and the table sit in tests/kernel_guards.py allocations whose bands
are checked after every launch."""
import importlib

import pytest
import torch

from oracle import restate as R
from tests import guidance_cases as GC
from tests.kernel_guards import BF, DEV, Guarded, all_intact
from tests.smoke_case import rel_l2

pytestmark = pytest.mark.gpu

SOLVERS = ("euler", "ab2", "heun")
NF = 4
# 256: one block per 256 elements, no tail; 4 * 257: a ragged last block; the last: (NF / 2) * elems is past the 2048 x 256
# threads of the largest grid, so some threads take a second grid-stride trip (and the last one is ragged)
ELEMS = (256, 4 * 257)
ELEMS_SECOND_TRIP = 2048 * 128 + 257
Z_BOUND, ZM_BOUND = 1e-5, 4e-3        # tests/test_ops_gpu.py::test_euler_cfg_update's bounds on the fp32 state and its bf16 copy


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("video-gpt_amd.ops")


class State:
    """The operands of one sampler: z, z_model, pred, v_hist, and (table given) the scale table."""

    def __init__(self, ops, sigma, z0, pred_type, table=None, use_cfg=True, scale=1.6):
        nf, elems = z0.shape
        self.ops, self.nf, self.elems, self.use_cfg, self.scale = ops, nf, elems, use_cfg, scale
        self.pred_type = ops.PRED_X1 if pred_type == "x1" else ops.PRED_V
        self.z, self.zm, self.pred = Guarded(nf, elems, torch.float32), Guarded(nf, elems, BF), Guarded(nf, elems, BF)
        self.vh = Guarded(nf // 2 if use_cfg else nf, elems, torch.float32)
        self.z.t.copy_(z0)
        self.zm.t.copy_(z0)
        self.pred.t.zero_()
        self.vh.t.fill_(12345.0)          # stale history of "the previous clip"
        self.sigma = sigma.to(DEV, torch.float32).contiguous()
        self.N = self.sigma.numel() - 1
        self.table = None if table is None else Guarded.of(torch.tensor(table, dtype=torch.float32))
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)

    def buffers(self):
        return (self.z, self.zm, self.pred, self.vh) + (() if self.table is None else (self.table,))

    def update(self, solver, stage=0):
        o = self.ops
        if self.table is not None:
            o.sampler_update_sched(self.z.t, self.zm.t, self.pred.t, self.vh.t, self.sigma, self.table.t.view(-1), self.step,
                                   self.pred_type, o.SOLVERS[solver], stage)
        else:
            o.sampler_update(self.z.t, self.zm.t, self.pred.t, self.vh.t, self.sigma, self.step, self.pred_type, self.use_cfg,
                             self.scale, o.SOLVERS[solver], stage)
        torch.cuda.synchronize()
        assert all_intact(*self.buffers()), (solver, stage, int(self.step.item()))

    def solve(self, solver, pred_at, after=None):
        """The scheduler's loop with the model replaced by pred_at(step, index into sigma) -> (nf, elems) predictions; Heun's
        final step goes through its predictor entry, a full Euler step there.  after(): called behind every launch."""
        after = after or (lambda: None)
        for i in range(self.N):
            self.pred.t.copy_(pred_at(i, i))
            if solver == "heun" and i < self.N - 1:
                self.update("heun", 0); after()
                self.ops.sampler_advance(self.step)
                self.pred.t.copy_(pred_at(i, i + 1))
                self.update("heun", 1); after()
            else:
                self.update(solver, 0); after()
                self.ops.sampler_advance(self.step)
        assert int(self.step.item()) == self.N
        return self.z.t, self.zm.t


def _random_case(nf, elems, n_steps, shift, seed=39):
    g = lambda s: torch.Generator("cpu").manual_seed(s)
    sigma = R.scheduler_sigma(n_steps, shift)
    z0 = torch.randn(nf, elems, generator=g(seed))
    z0[nf // 2:] = z0[: nf // 2] + 0.125 * torch.randn(nf // 2, elems, generator=g(seed + 100))   # each half moves from its own state
    preds = [torch.randn(nf, elems, generator=g(seed + 1 + i)).to(BF) for i in range(2 * n_steps)]
    return sigma, z0, preds


def _same(a, b):
    return all(torch.equal(x.bits(), y.bits()) for x, y in zip((a.z, a.zm, a.pred, a.vh), (b.z, b.zm, b.pred, b.vh)))


# ---- a constant table is the scalar entry point ---------------------------------------------------------------------------

LAUNCHES = [("euler", 0), ("ab2", 0), ("heun", 0), ("heun", 1)]


@pytest.mark.parametrize("elems", ELEMS)
@pytest.mark.parametrize("pred_type", ["x1", "v"])
@pytest.mark.parametrize("solver,stage", LAUNCHES, ids=[f"{s}{g}" for s, g in LAUNCHES])
def test_constant_table_is_sampler_update_bit_for_bit(ops, solver, stage, pred_type, elems):
    """Every step position -- 0, the middle, N - 1, past the table -- from the same state: z, z_model and v_hist (a live
    history, read by ab2 from step 1 on and by the corrector) equal, bands included."""
    N = 5
    sigma, z0, preds = _random_case(NF, elems, N, 3.0)
    hist = torch.randn(NF // 2, elems, generator=torch.Generator("cpu").manual_seed(5))
    for pos in (0, 2, N - 1, N, N + 2):
        a = State(ops, sigma, z0, pred_type, table=[1.6] * N)
        b = State(ops, sigma, z0, pred_type, scale=1.6)
        for st in (a, b):
            st.pred.t.copy_(preds[pos % len(preds)])
            st.vh.t.copy_(hist)
            st.step.fill_(pos)
            st.update(solver, stage)
        assert _same(a, b), pos
        moved = not torch.equal(a.zm.t.float().cpu(), z0.to(BF).float())
        assert moved == ((1 <= pos < N) if stage == 1 else (pos < N)), pos      # a real update inside the table, none outside


@pytest.mark.parametrize("solver", SOLVERS)
def test_constant_table_whole_clip_and_second_grid_stride_trip(ops, solver):
    """A whole clip at the size where the grid is capped and threads loop, x1, against the scalar entry point."""
    N = 3
    sigma, z0, preds = _random_case(NF, ELEMS_SECOND_TRIP, N, 3.0)
    assert (NF // 2) * ELEMS_SECOND_TRIP > 2048 * 256
    a = State(ops, sigma, z0, "x1", table=[2.25] * N)
    b = State(ops, sigma, z0, "x1", scale=2.25)
    for st in (a, b):
        st.solve(solver, lambda i, k: preds[i + k])
    assert _same(a, b)


# ---- unguided entries ------------------------------------------------------------------------------------------------------

def _poisoned(pred):
    p = pred.clone()
    p[NF // 2:] = float("nan")
    return p


@pytest.mark.parametrize("elems", ELEMS + (ELEMS_SECOND_TRIP,))
@pytest.mark.parametrize("pred_type", ["x1", "v"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_unguided_entries_never_read_the_unconditional_predictions(ops, solver, pred_type, elems):
    """A table of 1.0 with NaN in the unconditional half of `pred` at every launch (both stages of Heun): every output stays
    finite after every launch; the first half is the use_cfg = 0 kernel on the conditional half, bit for bit (z, z_model and
    the history); the second half, moved from its own state by the same velocity, is within the update kernels' bounds of the
    fp64 restatement."""
    N = 5 if elems < ELEMS_SECOND_TRIP else 2
    sigma, z0, preds = _random_case(NF, elems, N, 3.0)
    st = State(ops, sigma, z0, pred_type, table=[1.0] * N)

    def finite():
        for b in (st.z, st.zm) + (() if solver == "euler" else (st.vh,)):
            assert bool(torch.isfinite(b.t).all())
    z, zm = st.solve(solver, lambda i, k: _poisoned(preds[i + k]), after=finite)
    half = NF // 2
    ref = State(ops, sigma, z0[:half], pred_type, use_cfg=False)
    ref.solve(solver, lambda i, k: preds[i + k][:half])
    assert torch.equal(z[:half], ref.z.t) and torch.equal(zm[:half], ref.zm.t)
    assert torch.equal(st.vh.t, ref.vh.t)                                   # (Euler: both still hold the stale history)
    ref64 = torch.stack(GC.solver_call(sigma, [1.0] * N, [z0[j].double() for j in range(NF)],
                                       _replayed(solver, N, lambda i, k: _poisoned(preds[i + k])), pred_type, solver))
    assert bool(torch.isfinite(ref64).all())
    ez, ezm = rel_l2(z[half:], ref64[half:]), rel_l2(zm[half:], ref64[half:])
    print(f"{solver} {pred_type} {elems}: unconditional half z {ez:.3e}  z_model {ezm:.3e}")
    assert ez < Z_BOUND and ezm < ZM_BOUND


def _replayed(solver, N, pred_at):
    """`func` of the fp64 restatement that hands out pred_at(step, index into sigma) in the order the solver evaluates:
    once per step, and for Heun a second time at the next sigma in every step but the last."""
    order = [(i, i + k) for i in range(N) for k in range(2 if solver == "heun" and i < N - 1 else 1)]
    calls = iter(order)
    return lambda zl, t: list(pred_at(*next(calls)).double())


# ---- a mixed table against fp64 --------------------------------------------------------------------------------------------

MIXED = [1.6, 1.0, 1.0, 2.5, 1.0]


@pytest.mark.parametrize("elems", ELEMS)
@pytest.mark.parametrize("pred_type", ["x1", "v"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_mixed_table_against_fp64(ops, solver, pred_type, elems):
    """Shift 3 (non-uniform steps), N = 5, guided and unguided steps on both sides of each other (ab2 reads the history
    across the boundary; Heun's corrector takes the scale of its own step), NaN in the unconditional predictions of the
    unguided steps."""
    N = len(MIXED)
    sigma, z0, preds = _random_case(NF, elems, N, 3.0)
    at = lambda i, k: preds[i + k] if MIXED[i] != 1.0 else _poisoned(preds[i + k])
    st = State(ops, sigma, z0, pred_type, table=MIXED)
    z, zm = st.solve(solver, at)
    z64 = [z0[j].double() for j in range(NF)]
    ref = torch.stack(GC.solver_call(sigma, MIXED, z64, _replayed(solver, N, at), pred_type, solver))
    assert bool(torch.isfinite(ref).all())
    ez, ezm = rel_l2(z, ref), rel_l2(zm, ref)
    print(f"{solver} {pred_type} {elems}: z {ez:.3e}  z_model {ezm:.3e}")
    assert ez < Z_BOUND and ezm < ZM_BOUND
    # and the table matters: the constant-scale restatement of the same predictions is somewhere else
    const = torch.stack(GC.solver_call(sigma, [1.6] * N, z64, _replayed(solver, N, lambda i, k: preds[i + k]), pred_type,
                                       solver))
    assert rel_l2(z, const) > 100 * Z_BOUND


# ---- exact end states ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver,want", [("euler", 17 / 32), ("ab2", 75 / 128), ("heun", 79 / 128)])
def test_exact_end_state_on_a_linear_field(ops, solver, want):
    """v prediction, z0 = 0, N = 8, sigma_i = i/8 (h = 1/8), conditional prediction i/8 at sigma_i, unconditional 0 in the
    guided steps and NaN in the unguided ones, scale 2 in steps 0..3 and 1 (unguided) in steps 4..7: every value is dyadic
    and exact in bf16 and fp32.  With v_i = s_i i/8 = (0, 2, 4, 6, 4, 5, 6, 7) / 8:
      euler  z = h sum v_i = 34/64 = 17/32;
      ab2    z = h (v_0 + sum_{i>=1} (3/2 v_i - 1/2 v_{i-1})) = (1/8) (51/8 - 27/16) = 75/128;
      heun   steps 0..6 add h s_i (i + (i+1)) / 16 -- the corrector's prediction at sigma_{i+1} is guided with the scale of
             step i, also in step 3, whose successor is unguided -- = (2 (1+3+5+7) + 9+11+13) / 128 = 65/128, the Euler-shaped
             last step adds h 7/8 = 14/128: 79/128.
    Both halves of z move by the guided velocity."""
    N, elems = 8, 256
    table = [2.0] * 4 + [1.0] * 4
    sigma = torch.arange(N + 1, dtype=torch.float32) / N
    st = State(ops, sigma, torch.zeros(NF, elems), "v", table=table)

    def pred_at(i, k):
        p = torch.full((NF, elems), k / N, dtype=BF, device=DEV)
        p[NF // 2:] = 0 if table[i] != 1.0 else float("nan")
        return p
    z, zm = st.solve(solver, pred_at)
    assert torch.equal(z, torch.full_like(z, want)), (z.flatten()[0].item(), want)
    assert torch.equal(zm, torch.full_like(zm, want))


# ---- outside the table -----------------------------------------------------------------------------------------------------

def test_launches_outside_the_table_touch_nothing(ops):
    N = len(MIXED)
    sigma, z0, preds = _random_case(NF, 4 * 257, N, 3.0)
    st = State(ops, sigma, z0, "x1", table=MIXED)
    st.solve("heun", lambda i, k: preds[i + k])        # leaves *step = N and live values in every buffer
    st.pred.t.copy_(preds[-1])
    before = [b.bits() for b in st.buffers()]
    untouched = lambda: all(torch.equal(b.bits(), a) for b, a in zip(st.buffers(), before))
    for value in (N, N + 3, -1):                       # a replay past the end of the table (and a step that never was)
        st.step.fill_(value)
        for solver, stage in LAUNCHES:
            st.update(solver, stage)
            assert untouched(), (value, solver, stage)
    st.step.zero_()                                    # a corrector without a predictor step before it
    st.update("heun", 1)
    assert untouched()
