"""vgpt_sampler_noise_fill and vgpt_sampler_update_sde (csrc/glue.hip) element by element against the
restatement of tests/sde_cases.py.  Every operand sits in a kernel_guards.Guarded allocation: NaN (or 0xDEADBEEF) bands in
front and behind, checked after every launch.

  noise_fill   against the fp64 Box-Muller map on the same Philox words, under the bound read from the rounding points
               (sde_cases.noise_bound: logf, sqrtf, sincospif, one product); the integer words pinned at step indices where
               the angle is an exact quarter turn (one lane exactly 0); determinism across launches, streams and shapes.
  update_sde   eta = 0 and the last step: the bits of vgpt_euler_cfg_update / vgpt_sampler_update_sched; an exact probe
               (z = 0, v = 0, eta = 1: z' = fl((1 - sigma') eps)); random predictions against the fp64 update fed the
               kernel's own fill, under the running bound of sde_cases.sde_reference plus half a bf16 ulp for the copy; the
               scalar path and the tail against the vector path's bits; unguided entries; launches outside the table.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import sde_cases as SD
from tests import test_glue_kernels_gpu as GG
from tests.kernel_guards import BF, DEV, Guarded, all_intact, half_ulp

pytestmark = pytest.mark.gpu

F32 = torch.float32
PRED_V, PRED_X1 = SD.PRED_V, SD.PRED_X1
GRID_TRIP = 2048 * 256 * 4          # elements of the capped grid's first trip (2048 blocks of 256 threads, 4 per thread)


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("video-gpt_amd.ops")


def _sync(*bufs):
    torch.cuda.synchronize()
    assert all_intact(*bufs)


def _rng(seed, stream):
    wrap = lambda v: ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)
    return Guarded.of(torch.tensor([wrap(seed), wrap(stream)], dtype=torch.int64))


def _fill(ops, n, seed, stream, step):
    out, rng = Guarded(1, n, F32), _rng(seed, stream)
    ops.sampler_noise_fill(out.t.view(-1), rng.t.view(-1), step)
    _sync(out, rng)
    assert rng.t.view(-1).tolist() == _rng(seed, stream).t.view(-1).tolist()
    return out.t.view(-1).cpu()


# ---- noise_fill ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000, GRID_TRIP + 4 * 256 + 3])
def test_noise_fill_against_the_fp64_restatement(ops, n):
    seed, stream, step = (1 << 40) + 12345, (9 << 32) + 3, 17      # both seed words in use; of the stream the low word only
    got = _fill(ops, n, seed, stream, step).double().numpy()
    want = SD.normals(seed, 3, step, n)
    err, bound = np.abs(got - want), SD.noise_bound(want)
    print(f"MEASURE noise_fill n={n}: worst |err|/bound = {float((err / np.maximum(bound, 1e-300)).max()):.3g}, "
          f"max |eps| = {np.abs(got).max():.3f}")
    assert (err <= bound).all()
    assert np.abs(got).max() <= SD.EPS_MAX


def test_noise_fill_words_are_pinned_where_the_angle_is_exact(ops):
    for step, pair, quarter in SD.PROBES:
        got = _fill(ops, 4, *SD.PROBE_KEY, step).double().numpy()
        want = SD.normals(*SD.PROBE_KEY, step, 4)
        zero, full = 2 * pair + (quarter + 1) % 2, 2 * pair + quarter % 2
        assert want[zero] == 0 and got[zero] == 0, (step, got, want)           # any other w1 >> 8 gives a non-zero value here
        assert abs(got[full] - want[full]) <= SD.noise_bound(want)[full] and np.sign(got[full]) == np.sign(want[full])
        assert (np.abs(got - want) <= SD.noise_bound(want)).all()


def test_noise_fill_is_deterministic(ops):
    n = 4099
    base = _fill(ops, n, 7, 1, 3)
    assert torch.equal(base.view(torch.int32), _fill(ops, n, 7, 1, 3).view(torch.int32))
    assert torch.equal(base[:1000].view(torch.int32), _fill(ops, 1000, 7, 1, 3).view(torch.int32))   # whatever the shape
    # beside a busy stream
    busy, side = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    out, rng = Guarded(1, n, F32), _rng(7, 1)
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        for _ in range(4):
            a = a @ a * 1e-3
    with torch.cuda.stream(side):
        ops.sampler_noise_fill(out.t.view(-1), rng.t.view(-1), 3)
    _sync(out, rng)
    assert torch.equal(out.t.view(-1).cpu().view(torch.int32), base.view(torch.int32))
    for other in ((8, 1, 3), (7, 2, 3), (7, 1, 4), (7 + (1 << 32), 1, 3)):
        assert not torch.equal(_fill(ops, n, *other), base), other


# ---- update_sde ------------------------------------------------------------------------------------------------------------

class State:
    """The operands of one launch.  shift: elements by which z / z_model / pred are moved off their 16-byte alignment (the
    scalar path on a shape the vector path would take)."""

    def __init__(self, z0, pred, sigma, step, eta, seed=5, stream=2, table=None, shift=0):
        nf, elems = z0.shape
        n = nf * elems
        self.nf, self.elems, self.shift = nf, elems, shift
        self.z, self.zm, self.pred = Guarded(1, n + shift, F32), Guarded(1, n + shift, BF), Guarded(1, n + shift, BF)
        for g, v in ((self.z, z0), (self.zm, z0.to(BF)), (self.pred, pred)):
            g.t.view(-1)[shift:].copy_(v.reshape(-1))
            if shift:
                g.t.view(-1)[:shift] = float("nan")
        self.sigma, self.step = Guarded.of(sigma), Guarded.of(torch.tensor([step], dtype=torch.int32))
        n_steps = sigma.numel() - 1
        eta = [eta] * n_steps if not isinstance(eta, (list, tuple)) else eta
        self.eta = Guarded.of(torch.tensor(eta, dtype=F32))
        self.table = None if table is None else Guarded.of(torch.tensor(table, dtype=F32))
        self.rng = _rng(seed, stream)

    def buffers(self):
        return [b for b in (self.z, self.zm, self.pred, self.sigma, self.step, self.eta, self.table, self.rng) if b is not None]

    def _view(self, g):
        return g.t.view(-1)[self.shift:].view(self.nf, self.elems)

    def update(self, ops, pred_type, use_cfg, scale=1.6, share=False):
        ops.sampler_update_sde(self._view(self.z), self._view(self.zm), self._view(self.pred), self.sigma.t.view(-1),
                               None if self.table is None else self.table.t.view(-1), self.eta.t.view(-1), self.rng.t.view(-1),
                               self.step.t.view(-1), pred_type, use_cfg, scale, share)
        _sync(*self.buffers())
        if self.shift:
            assert bool(torch.isnan(self.z.t.view(-1)[:self.shift]).all())
        return self._view(self.z).cpu().clone(), self._view(self.zm).cpu().clone()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("step", [0, 2, 4], ids=["first", "middle", "last"])
@pytest.mark.parametrize("use_cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("pred_type", [PRED_X1, PRED_V], ids=["x1", "v"])
def test_eta_zero_gives_the_euler_kernels_bits(ops, pred_type, use_cfg, step):
    sigma = GG.sampler_sigma()
    for nf, elems in ((4, 250), (4, 251), (2, 5)):              # vector path, scalar path, a tail only
        z0, pred = GG.euler_inputs(nf, elems)
        ref = GG.EulerState(z0, pred, sigma, step)
        ref.update(ops, pred_type, use_cfg, 1.6)
        want = (ref.z.t.cpu(), ref.zm.t.cpu())
        for share in ((False, True) if not use_cfg else (False,)):
            assert _same(State(z0, pred, sigma, step, 0.0).update(ops, pred_type, use_cfg, 1.6, share), want), (nf, elems, share)
        if step == 4:                                           # the last step: 1 - sigma' == 0, any eta is Euler's
            assert _same(State(z0, pred, sigma, step, 1.0).update(ops, pred_type, use_cfg, 1.6), want)
            assert _same(State(z0, pred, sigma, step, 0.3).update(ops, pred_type, use_cfg, 1.6), want)
        if use_cfg:                                             # with a guidance table: vgpt_sampler_update_sched's, Euler
            for table in ([1.6] * 5, [1.0, 2.0, 1.0, 0.5, 1.0]):
                zs, zms, ps = Guarded.of(z0), Guarded(nf, elems, BF), Guarded.of(pred)
                zms.t.copy_(z0)
                sg, tb, st = Guarded.of(sigma), Guarded.of(torch.tensor(table, dtype=F32)), GG._step(step)
                ops.sampler_update_sched(zs.t, zms.t, ps.t, None, sg.t.view(-1), tb.t.view(-1), st.t.view(-1), pred_type)
                GG._sync(zs, zms, ps, sg, tb, st)
                got = State(z0, pred, sigma, step, 0.0, table=table).update(ops, pred_type, True, 99.0)
                assert _same(got, (zs.t.cpu(), zms.t.cpu())), (nf, elems, table)


@pytest.mark.parametrize("nf,elems", [(4, 250), (2, 253), (2, 255)], ids=["h500", "h253-tail1", "h255-tail3"])
def test_exact_probe(ops, nf, elems):
    """z = 0, v = 0, eta = 1 on sigma = 0, 1/4, 1/2, 3/4, 1: ca = -1, x0 = 0, so z' = fl((1 - sigma') eps) in one rounding
    (0.5 and 0.25 are exact), with eps the fill of that step; the last step forms no noise and leaves 0.  Half sizes 500
    (vector path), 253 and 255 (scalar path, a tail thread that owns 1 / 3 lanes of its Philox block)."""
    sigma = torch.linspace(0, 1, 5)
    seed, stream, h = 21, 6, nf // 2
    zero, pred = torch.zeros(nf, elems), torch.zeros(nf, elems).to(BF)
    for step in range(4):
        g = float(1 - sigma[step + 1])
        half = _fill(ops, h * elems, seed, stream, step).view(h, elems)
        whole = _fill(ops, nf * elems, seed, stream, step).view(nf, elems)
        for use_cfg, share in ((True, False), (False, True), (False, False)):
            z, zm = State(zero, pred, sigma, step, 1.0, seed, stream).update(ops, PRED_V, use_cfg, 1.6, share)
            want = whole * g if not (use_cfg or share) else torch.cat([half, half]) * g
            assert torch.equal(z, want), (step, use_cfg, share)
            assert torch.equal(zm, want.to(BF))
            assert torch.equal(z[:h], z[h:]) == (use_cfg or share or step == 3)


@pytest.mark.parametrize("nf,elems", [(4, 128), (4, 500), (2, 1001), (2, 1002), (2, 1003)],
                         ids=["h256", "h1000", "h1001-1mod4", "h1002-2mod4", "h1003-3mod4"])
@pytest.mark.parametrize("eta", [0.3, 1.0])
@pytest.mark.parametrize("pred_type", [PRED_X1, PRED_V], ids=["x1", "v"])
def test_random_predictions_against_fp64(ops, pred_type, eta, nf, elems):
    """A shift-3 sigma table, CFG 1.6, step 2.  Half sizes 256 and 1000 (2 frames per half) take the vector path; half sizes
    1001, 1002 and 1003 (one frame per half) the scalar path, whose last thread owns 1, 2 and 3 lanes of its Philox block.
    The same operands moved one element off their alignment take the scalar path on every shape, and the first 1000 columns
    of a tail shape launched alone take the vector path: the two paths give the same bits wherever both apply."""
    sigma, step, seed, stream = GG.sampler_sigma(), 2, 77, 1
    z0, pred = GG.euler_inputs(nf, elems, seed=131)
    rows = nf // 2
    assert (rows * elems) % 4 == {128: 0, 500: 0, 1001: 1, 1002: 2, 1003: 3}[elems]
    eps = _fill(ops, rows * elems, seed, stream, step).double().numpy()
    got = State(z0, pred, sigma, step, eta, seed, stream).update(ops, pred_type, True, 1.6)
    scale, et = float(torch.tensor(1.6, dtype=F32)), float(torch.tensor(eta, dtype=F32))
    z64, bound = SD.sde_reference(z0, pred, sigma, step, pred_type, True, scale, et, eps)
    err = (got[0].double() - z64).abs()
    print(f"MEASURE update_sde pred{pred_type} eta={eta} half={rows * elems}: worst |err|/bound = {GG._ratio(err, bound):.3g}")
    assert bool((err <= bound).all())
    assert torch.equal(got[1], got[0].to(BF))
    assert bool(((got[1].double() - z64).abs() <= bound + half_ulp(z64)).all())       # the copy: half a bf16 ulp more
    moved = State(z0, pred, sigma, step, eta, seed, stream, shift=1).update(ops, pred_type, True, 1.6)
    assert _same(moved, got)
    if (rows * elems) % 4:
        # one frame per half: element e of the noise is column e, so the leading 1000 columns alone are a vector-path launch
        # of the same elements
        head = State(z0[:, :1000].contiguous(), pred[:, :1000].contiguous(), sigma, step, eta, seed, stream)
        assert _same(head.update(ops, pred_type, True, 1.6), (got[0][:, :1000], got[1][:, :1000]))
    # the Euler step on the same operands is somewhere else
    eu = State(z0, pred, sigma, step, 0.0, seed, stream).update(ops, pred_type, True, 1.6)
    assert float((eu[0] - got[0]).abs().max()) > 1e-2


@pytest.mark.parametrize("nf,elems,share", [(4, 251, False), (4, 251, True), (2, 1003, False), (2, 1003, True), (3, 335, False)],
                         ids=["4x251-own", "4x251-shared", "2x1003-own", "2x1003-shared", "3x335-own"])
@pytest.mark.parametrize("pred_type", [PRED_X1, PRED_V], ids=["x1", "v"])
def test_without_cfg_every_frame_moves_by_its_own_prediction(ops, pred_type, nf, elems, share):
    """Noise sizes 1004 / 502 (4 x 251: own / shared), 2006 / 1003 (2 x 1003) and 1005 (3 x 335: an odd frame count, which
    only an unshared launch takes, and a one-lane tail)."""
    sigma, step, seed, stream = GG.sampler_sigma(), 1, 3, 0
    z0, pred = GG.euler_inputs(nf, elems, seed=151)
    rows = nf // 2 if share else nf
    eps = _fill(ops, rows * elems, seed, stream, step).double().numpy()
    got = State(z0, pred, sigma, step, 0.3, seed, stream).update(ops, pred_type, False, 1.6, share)
    z64, bound = SD.sde_reference(z0, pred, sigma, step, pred_type, False, None, float(torch.tensor(0.3, dtype=F32)), eps, share)
    err = (got[0].double() - z64).abs()
    print(f"MEASURE update_sde nocfg pred{pred_type} share={share}: worst |err|/bound = {GG._ratio(err, bound):.3g}")
    assert bool((err <= bound).all()) and torch.equal(got[1], got[0].to(BF))


@pytest.mark.parametrize("elems", [250, 251])
@pytest.mark.parametrize("pred_type", [PRED_X1, PRED_V], ids=["x1", "v"])
def test_unguided_entry_does_not_load_the_unconditional_predictions(ops, pred_type, elems):
    sigma, step, nf, seed, stream = GG.sampler_sigma(), 2, 4, 13, 4
    z0, pred = GG.euler_inputs(nf, elems, seed=171)
    z0[2:] = z0[:2]                                   # the CFG halves of a clip start from the same latents
    poisoned = pred.clone()
    poisoned[2:] = float("nan")
    table = [1.6, 1.6, 1.0, 1.6, 1.6]
    z, zm = State(z0, poisoned, sigma, step, 0.3, seed, stream, table=table).update(ops, pred_type, True, 99.0)
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(zm.float()).all())
    plain = State(z0[:2].contiguous(), pred[:2].contiguous(), sigma, step, 0.3, seed, stream).update(ops, pred_type, False)
    assert torch.equal(_bits(z[:2]), _bits(plain[0])) and torch.equal(_bits(zm[:2]), _bits(plain[1]))
    # a guided entry of the same table reads them
    z, _ = State(z0, poisoned, sigma, 1, 0.3, seed, stream, table=table).update(ops, pred_type, True, 99.0)
    assert bool(torch.isnan(z).all())


@pytest.mark.parametrize("use_cfg", [False, True], ids=["nocfg", "cfg"])
def test_launches_outside_the_table_touch_nothing(ops, use_cfg):
    sigma = GG.sampler_sigma()
    z0, pred = GG.euler_inputs(4, 251)
    for step in (-1, 5, 6):
        st = State(z0, pred, sigma, step, 1.0, table=[1.6] * 5 if use_cfg else None)
        before = [b.bits() for b in st.buffers()]
        st.update(ops, PRED_X1, use_cfg, 1.6)
        assert all(torch.equal(b.bits(), a) for b, a in zip(st.buffers(), before)), step
