"""A per-step guidance scale through LVMScheduler's two paths, the engine (unguided steps on the conditional rows only,
graphs per step kind, partial runs, the engine cache), the sharded engine and the pipeline, on the
tiny model at C = 2, G = 2, 16x16 latents, N = 4 steps: the smallest case that hoists (prefix 132 >= 128 rows, 256 live
rows, 128 conditional ones).

Against the oracle (tests/guidance_cases.py's restatement driving oracle/restate.py's model, unguided steps on the
conditional batch only) the bound is the measured one of scripts/calibrate_guidance.py.  That comparison cannot see a wrong
table entry (a scale off by 0.6 in one step moves the result by less than the bf16 bar), so
test_engine_follows_the_table_on_its_own_predictions replays the engine's own predictions through the fp64 restatement at
the update kernel's bound, and the sentinel test shows that the rows an unguided step is said to skip are not touched."""
import functools
import importlib
import traceback

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import guidance_cases as GC
from tests import smoke_case as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
STEPS = GC.STEPS
KERNEL_BOUND = 1e-5     # tests/test_ops_gpu.py::test_euler_cfg_update's bound on the fp32 state
MA, MC, G = 256, 128, GC.CASE["G"]
SOLVERS = GC.SOLVERS
PRECISIONS = {"bf16": {}, "attn_fp8": dict(attention_precision="fp8"), "lin_fp8": dict(linear_precision="fp8")}


def _case():
    WU = importlib.import_module("tests.test_weight_updates_gpu")
    c = WU.Case(R.TINY, steps=STEPS, **GC.CASE)
    c.model = SC.build_product_model(R.TINY, c.p, DEV)
    return c


@pytest.fixture(scope="module")
def case():
    return _case()


def _scheduler(solver="euler", schedule=None, cache=False, graph=True, **opts):
    """schedule: a name of GC.SCHEDULES, a dict of LVMScheduler's guidance arguments, or None."""
    S = importlib.import_module("video-gpt_amd.scheduler")
    kw = GC.SCHEDULES[schedule] if isinstance(schedule, str) else (schedule or {})
    kw = {"guidance_" + k: v for k, v in kw.items()}
    sched = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=1, solver=solver, **kw)
    sched.cache_engines, sched.use_graph = cache, graph
    for k, v in opts.items():
        setattr(sched, k, v)
    return sched


def _kwargs(c, layout=True, cond=None):
    kw = SC.model_kwargs(c.batch, c.cond if cond is None else cond, DEV, scale=GC.SCALE)
    if layout:
        kw["attention_mask"] = c.lay
    return kw


def _sample(c, sched, pt="x1", generic=False, z=None, cond=None):
    func = c.model.frame_block_forward_with_cfg
    if generic:
        def func(zl, ts, past_key_values=None, prediction_type="x1", **mk):   # not a bound LVM method -> generic path
            return c.model.frame_block_forward_with_cfg(zl, ts, past_key_values=past_key_values,
                                                        prediction_type=prediction_type, **mk)
    out = torch.cat(sched([t.to(DEV, BF) for t in (c.z if z is None else z)], func, _kwargs(c, not generic, cond),
                          prediction_type=pt))
    torch.cuda.synchronize()
    assert (sched.last_engine is None) == generic
    return out


def _z0(c):
    return torch.cat([t.to(DEV, BF) for t in c.z])


class _side_stream:
    """Run the body on a side stream (a capture cannot record on the legacy default stream) and wait for it."""

    def __enter__(self):
        self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()

    def __exit__(self, *a):
        self.ctx.__exit__(*a)
        self.side.synchronize()
        return False


@functools.lru_cache(maxsize=None)
def _oracle(solver, pt, name):
    p, _, z, cond = SC.build_case(R.TINY, **GC.CASE)
    with torch.no_grad():
        return torch.cat(GC.oracle_sample(R.TINY, p, z, cond, GC.TABLES[name], pt, solver))


# ---- a constant schedule is no schedule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("solver,pt", [("euler", "x1"), ("euler", "v"), ("ab2", "x1"), ("heun", "x1"), ("heun", "v")])
def test_constant_schedule_equals_no_schedule(case, solver, pt, path, graph):
    generic = path == "generic"
    const = _scheduler(solver, dict(schedule=[GC.SCALE] * STEPS), graph=graph)
    a = _sample(case, const, pt, generic)
    b = _sample(case, _scheduler(solver, graph=graph), pt, generic)
    assert torch.equal(a, b)
    if not generic:
        eng = const.last_engine
        assert eng.gtable is not None and eng.unguided == [False] * STEPS
        assert [eng.step_rows(i) for i in range(STEPS)] == [MA] * STEPS


# ---- against the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("pt", ["x1", "v"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(GC.SCHEDULES))
def test_scheduler_matches_the_oracle_under_the_schedule(case, name, solver, pt, path):
    sched = _scheduler(solver, name)
    out = _sample(case, sched, pt, generic=path == "generic")
    if path == "fast":
        eng = sched.last_engine
        assert eng.cr is not None and eng.hoist
        assert eng.gtable.tolist() == torch.tensor(GC.TABLES[name], dtype=torch.float32).tolist()
        assert [eng.step_rows(i) for i in range(STEPS)] == [MC if s == 1.0 else MA for s in GC.TABLES[name]]
    q = f"{solver}.{pt}.{name}"
    err = SC.rel_l2(out, _oracle(solver, pt, name))
    print(f"{q} {path}: rel-L2 vs oracle {err:.3e} (tolerance {GC.tol(q):.3e})")
    assert err < GC.tol(q)


# ---- the engine's own predictions through the fp64 restatement -------------------------------------------------------------

@pytest.mark.parametrize("skip", [None, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("pt", ["x1", "v"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(GC.SCHEDULES))
def test_engine_follows_the_table_on_its_own_predictions(case, name, solver, pt, skip, monkeypatch):
    ops = importlib.import_module("video-gpt_amd.ops")
    SV = importlib.import_module("tests.solver_cases")
    sched = _scheduler(solver, name, graph=False, skip_unguided_branch=skip)
    _sample(case, sched, pt)                      # builds the engine
    eng = sched.last_engine
    assert (eng.cr is not None) == (skip is None)
    preds = []                                    # engine.pred at every update launch, i.e. after every model evaluation
    real = ops.sampler_update_sched

    def spy(*a, **k):
        preds.append(eng.pred.detach().float().cpu().clone())
        return real(*a, **k)
    monkeypatch.setattr(ops, "sampler_update_sched", spy)
    for other in ("sampler_update", "euler_cfg_update"):     # an engine with a table launches neither
        monkeypatch.setattr(ops, other, lambda *a, **k: pytest.fail("the scalar update ran under a schedule"))
    z0 = _z0(case)
    eng.set_latents(z0)
    states = []
    for i in range(STEPS):
        eng.run(1, use_graph=False)
        torch.cuda.synchronize()
        states.append(eng.z.detach().double().cpu().clone())
    assert len(preds) == SV.model_evaluations(solver, STEPS)
    nf = eng.nf
    flat = lambda t: [t.reshape(nf, -1)[j].double() for j in range(nf)]
    table = GC.TABLES[name]

    def replay(tab, clean):
        it, trace = iter(preds), []
        nxt = (lambda: torch.nan_to_num(next(it))) if clean else (lambda: next(it))
        GC.solver_call(eng.sigma.cpu(), tab, flat(z0.float().cpu()), lambda zl, t: flat(nxt()), pt, solver, trace=trace)
        return [torch.stack(s) for s in trace]
    own = replay(table, clean=False)              # the unguided steps' unconditional predictions are never looked at
    for i in range(STEPS):
        err = SC.rel_l2(states[i], own[i])
        print(f"{name} {solver} {pt} step {i}: rel-L2 of the engine's z against the fp64 replay {err:.3e}")
        assert err < KERNEL_BOUND
    # one scale for the clip on the same predictions is somewhere else, from the first step whose entry is another on
    const = replay([GC.SCALE] * STEPS, clean=True)
    at = next(i for i, s in enumerate(table) if s != GC.SCALE)
    miss = SC.rel_l2(states[at], const[at])
    print(f"{name} {solver} {pt}: the constant-scale replay misses z after step {at} by {miss:.3e}")
    assert miss > 10 * KERNEL_BOUND


# ---- skipping is real and changes nothing ----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_unguided_step_leaves_the_unconditional_rows_alone(case, solver, precision):
    """NaN in pred[G:] and in the rows >= Mc of hid / ctx / act before the unguided step 0 of the "interval" schedule: they are
    there, bit for bit, after it (not written), z is finite (not read), and the clip that goes on from there -- step 1 is
    guided and recomputes every row -- ends where the scheduler's own call ended."""
    sched = _scheduler(solver, "interval", graph=False, **PRECISIONS[precision])
    want = _sample(case, sched)
    eng = sched.last_engine
    assert eng.cr is not None and eng.cr.Mc == MC and eng.Ma == MA and eng.cr.nf == G
    assert [eng.step_rows(i) for i in range(STEPS)] == [MC, MA, MA, MC]
    eng.set_latents(_z0(case))
    guarded = [eng.pred[G:], eng.hid[:, MC:], eng.ctx[:, MC:], eng.act[:, MC:]]
    for t in guarded:
        t.fill_(float("nan"))
    before = [t.clone().view(torch.int16) for t in guarded]
    eng.run(1, use_graph=False)
    torch.cuda.synchronize()
    for t, b in zip(guarded, before):
        assert torch.equal(t.view(torch.int16), b)
    assert bool(torch.isfinite(eng.z).all()) and bool(torch.isfinite(eng.z_model.float()).all())
    assert bool(torch.isfinite(eng.pred[:G].float()).all())
    eng.run(STEPS - 1, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.z.view(-1).to(BF), want.view(-1))


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(GC.SCHEDULES))
def test_skipping_changes_no_bit(case, name, solver, precision):
    """skip_unguided_branch None (skip) and False (compute every row, the kernel still takes v_c) give the same clip."""
    a_s = _scheduler(solver, name, **PRECISIONS[precision])
    b_s = _scheduler(solver, name, skip_unguided_branch=False, **PRECISIONS[precision])
    a, b = _sample(case, a_s), _sample(case, b_s)
    assert a_s.last_engine.cr is not None and b_s.last_engine.cr is None
    assert [b_s.last_engine.step_rows(i) for i in range(STEPS)] == [MA] * STEPS
    assert torch.equal(a, b)


def test_half_row_gemm_calls_get_the_full_row_kernels(case, monkeypatch):
    """Why test_skipping_changes_no_bit can ask for equality at this shape: the GEMM launch decision, read from
    vgpt_gemm_last_launches after every projection of an unguided (128-row) and a guided (256-row) eager step, gives both
    row counts the same kernel, mode and tile form for every projection.  (At cfg-2 it does not: DESIGN.md section 5b.)"""
    import ctypes
    ops = importlib.import_module("video-gpt_amd.ops")
    L = importlib.import_module("video-gpt_amd._lib")
    sched = _scheduler("euler", "interval", graph=False)
    _sample(case, sched)
    eng = sched.last_engine
    assert eng.cr is not None and eng.fuse is None and eng.mx8 is None
    seen = {}

    def wrap(name):
        real = getattr(ops, name)

        def spy(*a, **k):
            out = real(*a, **k)
            buf = (ctypes.c_int32 * 48)()
            n = L.load().vgpt_gemm_last_launches(buf, 8)
            recs = [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]
            rows = sum(r[5] for r in recs)
            seen.setdefault((name, rows), set()).add(tuple(r[:4] for r in recs))
            return out
        monkeypatch.setattr(ops, name, spy)
    for name in ("linear_qkv_rope", "linear", "gated_mlp_act"):
        wrap(name)
    eng.set_latents(_z0(case))
    eng.run(2, use_graph=False)                   # step 0 unguided (128 rows), step 1 guided (256 rows)
    torch.cuda.synchronize()
    print(f"LAUNCH {sorted(seen.items())}")
    for name in ("linear_qkv_rope", "linear", "gated_mlp_act"):
        assert (name, MC) in seen and (name, MA) in seen, sorted(seen)
        assert seen[name, MC] == seen[name, MA] and len(seen[name, MC]) == 1, (name, seen[name, MC], seen[name, MA])


def test_every_layout_skips_and_agrees(case):
    """The hoisted, the prefix-only and the no-prefix layout each skip their own conditional range, and agree within the
    5e-3 tests/test_model_gpu.py holds the three layouts to -- under Euler, the solver that bound was set for (ab2
    extrapolates the velocity and carries 1.6 x Euler's stock-bf16 error on x1 predictions,
    tests/golden/tolerance_calibration_guidance.json; the layouts differ by the bf16 noise of their tile choices)."""
    outs = {}
    for mode in ("hoist", "prefix", "none"):
        sched = _scheduler("euler", "interval", reuse_condition_prefix=mode != "none", hoist_special_rows=mode == "hoist")
        outs[mode] = _sample(case, sched)
        eng = sched.last_engine
        assert bool(eng.hoist) == (mode == "hoist") and bool(eng.S) == (mode != "none")
        assert eng.cr is not None, mode
        bl = MC // G + 2                                      # a frame block: <|diffusion|>, time, 64 image rows
        rows = {"hoist": (MC, MA), "prefix": (G * bl, 2 * G * bl), "none": ((2 + G) * bl, (2 + 2 * G) * bl)}[mode]
        assert (eng.cr.Mc, eng.Ma) == rows and eng.step_rows(0) == rows[0] and eng.step_rows(1) == rows[1]
        assert SC.rel_l2(outs[mode], _oracle("euler", "x1", "interval")) < GC.tol("euler.x1.interval")
    a, b = SC.rel_l2(outs["hoist"], outs["none"]), SC.rel_l2(outs["hoist"], outs["prefix"])
    print(f"hoist vs none {a:.3e}, hoist vs prefix {b:.3e}")
    assert a < 5e-3 and b < 5e-3


@pytest.mark.parametrize("G_fw,folded", [(8, False), (16, True)], ids=["cfg2-2048rows-separate", "4096rows-folded"])
def test_full_width_skipping(G_fw, folded):
    """One full-width layer (tests/test_weight_updates_gpu.py's case: the only width at which the RMSNorms are folded into
    the GEMMs), 4 condition frames and G 32x32 latents per CFG half.
      G = 8, the cfg-2 geometry: 4096 live rows, 2048 conditional ones.  At 2048 rows o_proj and down_proj (N = 3072: 96
        tiles of 256 x 256) are below the four-wave GEMM's half-the-chip threshold, so they have no folded-norm form
        (vgpt_gemm_norm_workspace_bytes = 0) and the conditional-rows steps keep the separate RMSNorm kernels.  Skipping on
        and off then differ as folded and separate norms do: within the 1.5e-2 of
        test_fullwidth_parity_gpu.py::test_cfg2_sampler_steps_with_folded_rmsnorms_equal_the_separate_kernels.
      G = 16: 8192 / 4096 rows, folded at both, with a workspace of its own at 4096 rows.  The same arithmetic in possibly
        another tile order: within the 5e-3 this suite holds equivalent row layouts to (equality is printed).
    In both, NaN in the unconditional half of pred and in the unconditional rows of hid / ctx / act stays untouched over an
    unguided step and reaches nothing, and the clip that goes on from there ends on the scheduler's own bits."""
    WU = importlib.import_module("tests.test_weight_updates_gpu")
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    c = WU.Case(WU.FULL1, C=4, G=G_fw, hw=(32, 32), steps=STEPS)
    c.model = SC.build_product_model(WU.FULL1, c.p, DEV)
    mc = G_fw * 256
    table = dict(schedule=[1.0, GC.SCALE, 1.0, GC.SCALE])
    on, off = _scheduler("euler", table, graph=False), _scheduler("euler", table, skip_unguided_branch=False)
    a, b = _sample(c, on), _sample(c, off)
    eng = on.last_engine
    assert eng.fuse is not None and eng.hoist and eng.cr is not None and (eng.cr.ws is not None) == folded
    assert (eng.cr.Mc, eng.Ma, eng.cr.nf) == (mc, 2 * mc, G_fw) and off.last_engine.cr is None
    err = SC.rel_l2(a, b)
    print(f"full width, {mc} conditional rows, skipping on vs off: equal {torch.equal(a, b)}, rel-L2 {err:.3e}")
    assert bool(torch.isfinite(a.float()).all()) and err < (5e-3 if folded else 1.5e-2)
    eng.set_latents(_z0(c))
    guarded = [eng.pred[G_fw:], eng.hid[:, mc:], eng.ctx[:, mc:], eng.act[:, mc:]]
    for t in guarded:
        t.fill_(float("nan"))
    before = [t.clone().view(torch.int16) for t in guarded]
    eng.run(1, use_graph=False)
    torch.cuda.synchronize()
    for t, b4 in zip(guarded, before):
        assert torch.equal(t.view(torch.int16), b4)
    assert bool(torch.isfinite(eng.z).all()) and bool(torch.isfinite(eng.pred[:G_fw].float()).all())
    eng.run(STEPS - 1, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.z.view(-1).to(BF), a.view(-1))


def test_skip_true_is_refused_where_there_is_nothing_to_skip(case):
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    with pytest.raises(VgptError, match="skip_unguided_branch=True cannot be honoured: .*unpacked batch"):
        _sample(case, _scheduler("euler", "interval", pack_padding=False, skip_unguided_branch=True))
    sched = _scheduler("euler", "interval", pack_padding=False)          # None: runs, and skips nothing
    out = _sample(case, sched)
    assert sched.last_engine.cr is None and sched.last_engine.step_rows(0) == sched.last_engine.Ma
    assert SC.rel_l2(out, _oracle("euler", "x1", "interval")) < GC.tol("euler.x1.interval")
    assert _sample(case, _scheduler("euler", "interval", skip_unguided_branch=True)) is not None
    with pytest.raises(VgptError, match="there is nothing to schedule"):
        kw = _kwargs(case)
        kw["use_img_cfg"] = False
        _scheduler("euler", "interval")([t.to(DEV, BF) for t in case.z[:G]], case.model.frame_block_forward_with_cfg, kw,
                                        prediction_type="x1")
    eng = sched.last_engine
    with pytest.raises(VgptError, match=r"set_sigma: a sigma table of 6 steps .* holds 4 scales"):
        eng.set_sigma(R.scheduler_sigma(6, 1.0))


# ---- graphs ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(GC.SCHEDULES))
def test_graph_replay_equals_eager(case, name, solver):
    g = _scheduler(solver, name, graph=True)
    a = _sample(case, g)
    b = _sample(case, _scheduler(solver, name, graph=False))
    assert torch.equal(a, b)
    eng = g.last_engine
    # one graph per (kind, Heun-last), each captured at the first step of its kind
    kinds = {(s == 1.0, solver == "heun" and i == STEPS - 1) for i, s in enumerate(GC.TABLES[name])}
    have = {(c, l) for c in (False, True) for l in (False, True)
            if getattr(eng, ("graph_c" if c else "graph") + ("_last" if l else "")) is not None}
    assert have == kinds


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(GC.SCHEDULES))
def test_partial_runs_add_up_across_a_kind_boundary(case, name, solver, graph):
    sched = _scheduler(solver, name, graph=graph)
    _sample(case, sched)                          # builds the engine (and, with graphs on, captures its steps)
    eng = sched.last_engine
    z0 = _z0(case)
    res = {}
    with _side_stream():
        for split in ((STEPS,), (2, 2), (1, 3)):  # both schedules change kind behind step 0; "interval" again behind step 2
            eng.set_latents(z0)
            for n in split:
                eng.run(n, use_graph=graph)
            res[split] = eng.z.clone().reshape(-1)
    assert torch.equal(res[2, 2], res[STEPS,]) and torch.equal(res[1, 3], res[STEPS,])
    assert int(eng.step.item()) == STEPS and eng.steps_taken == STEPS


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("solver", ["ab2", "heun"])
def test_capture_in_the_middle_of_a_clip_leaves_no_trace(case, solver, at):
    """capture() runs one eager step of the kind of the step it stands at and takes it back ("explicit": step 1 runs the
    conditional rows only, step 2 too, and the ab2 step behind it reads the history the step before wrote)."""
    sched = _scheduler(solver, "explicit", graph=False)
    _sample(case, sched)
    eng = sched.last_engine
    assert all(getattr(eng, n) is None for n in ("graph", "graph_last", "graph_c", "graph_c_last"))
    z0 = _z0(case)
    with _side_stream():
        eng.set_latents(z0)
        eng.run(STEPS, use_graph=False)
        whole = eng.z.clone()
        eng.set_latents(z0)
        eng.run(at, use_graph=False)
        eng.capture()
        assert eng.graph_c is not None and eng.graph is None          # the kind of step `at`, and no other
        eng.run(STEPS - at, use_graph=True)
        got = eng.z.clone()
    assert torch.equal(got, whole) and int(eng.step.item()) == STEPS


# ---- the engine cache ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_cached_engine_on_a_second_clip_equals_a_fresh_one(case, solver):
    case.model.__dict__.pop("_vgpt_engine_cache", None)
    g = torch.Generator("cpu").manual_seed(7)
    hw = GC.CASE["hw"]
    z2 = [torch.randn(1, 4, *hw, generator=g).to(BF).float() for _ in range(G)] * 2
    cond2 = [torch.randn(1, 4, *hw, generator=g).to(BF).float() for _ in range(GC.CASE["C"])]
    s1 = _scheduler(solver, "interval", cache=True)
    _sample(case, s1)
    s2 = _scheduler(solver, "interval", cache=True)
    second = _sample(case, s2, z=z2, cond=cond2)
    assert s2.last_engine_reused and s2.last_engine is s1.last_engine
    fresh = _sample(case, _scheduler(solver, "interval"), z=z2, cond=cond2)
    assert torch.equal(second, fresh)
    case.model.__dict__.pop("_vgpt_engine_cache", None)


@pytest.mark.parametrize("mode", ["prefix", "none"])
def test_fp8_attention_where_the_range_ends_inside_a_quantisation_block(case, mode):
    """The prefix-only and no-prefix layouts: the conditional range ends at a row that is no multiple of 32, so its last
    keys share a V block scale of the fp8 quantiser with the rows behind it.  A conditional-rows step zeroes those rows
    first: what the previous clip left there reaches nothing, and a cached engine's second clip has a fresh engine's bits
    (step 0 of "interval" is unguided: the cached engine meets the first clip's rows there, the fresh one its zero fill).
    Held to the oracle as the bf16 path is (tests/test_pipeline_gpu.py holds fp8 attention to the bf16 tolerance)."""
    case.model.__dict__.pop("_vgpt_engine_cache", None)
    opts = dict(attention_precision="fp8", reuse_condition_prefix=mode == "prefix", hoist_special_rows=False)
    g = torch.Generator("cpu").manual_seed(11)
    hw = GC.CASE["hw"]
    z2 = [torch.randn(1, 4, *hw, generator=g).to(BF).float() for _ in range(G)] * 2
    s1 = _scheduler("euler", "interval", cache=True, **opts)
    first = _sample(case, s1)
    eng = s1.last_engine
    assert eng.cr is not None and eng.attn_fp8 and (eng.S + eng.cr.Mc) % 32 != 0 and eng.cr.tail[1] > eng.cr.tail[0]
    err = SC.rel_l2(first, _oracle("euler", "x1", "interval"))
    print(f"fp8 attention, {mode} layout, skipping: rel-L2 vs oracle {err:.3e}")
    assert err < GC.tol("euler.x1.interval")
    s2 = _scheduler("euler", "interval", cache=True, **opts)
    second = _sample(case, s2, z=z2)
    assert s2.last_engine_reused and s2.last_engine is eng
    fresh = _sample(case, _scheduler("euler", "interval", **opts), z=z2)
    assert torch.equal(second, fresh)
    case.model.__dict__.pop("_vgpt_engine_cache", None)


def test_one_cache_entry_per_schedule(case):
    case.model.__dict__.pop("_vgpt_engine_cache", None)
    sa = _scheduler("euler", "interval", cache=True)
    a = _sample(case, sa)
    sb = _scheduler("euler", "explicit", cache=True)
    b = _sample(case, sb)
    assert not sb.last_engine_reused and sb.last_engine is not sa.last_engine
    assert len(case.model._vgpt_engine_cache) == 2 and not torch.equal(a, b)
    sa2 = _scheduler("euler", "interval", cache=True)
    assert torch.equal(_sample(case, sa2), a) and sa2.last_engine is sa.last_engine and sa2.last_engine_reused
    # neither the skip option nor "no schedule" shares an entry with them
    sc = _scheduler("euler", "interval", cache=True, skip_unguided_branch=False)
    assert torch.equal(_sample(case, sc), a) and not sc.last_engine_reused
    sd = _scheduler("euler", cache=True)
    _sample(case, sd)
    assert not sd.last_engine_reused and sd.last_engine.gtable is None
    case.model.__dict__.pop("_vgpt_engine_cache", None)


# ---- sharded engine --------------------------------------------------------------------------------------------------------

def _sp_worker(rank, world, port, q):
    res = {}
    try:
        SPT = importlib.import_module("tests.test_sp_engine_gpu")
        dist = SPT._init(rank, world, port)
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        c = _case()
        res["base"] = _sample(c, _scheduler("heun", "interval", skip_unguided_branch=False)).float().cpu().numpy()
        SPM.initialize_sequence_parallel_state(world)
        sched = _scheduler("heun", "interval", sequence_parallel_engine=True)
        res["sharded"] = _sample(c, sched).float().cpu().numpy()
        eng = sched.last_engine
        res["is_sharded"] = eng.sp is not None
        res["skips"] = eng.cr is not None
        res["rows"] = [eng.step_rows(i) for i in range(STEPS)]
        try:
            _sample(c, _scheduler("heun", "interval", sequence_parallel_engine=True, skip_unguided_branch=True))
            res["refused"] = ""
        except Exception as e:    # noqa: BLE001 (the message is what the parent checks)
            res["refused"] = f"{type(e).__name__}: {e}"
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


def test_sharded_engine_with_a_schedule_equals_the_single_rank_engine():
    """Two ranks over gloo on one GPU (the harness of tests/test_sp_engine_gpu.py).  A sharded engine applies the table and
    skips nothing: its shares are cut over all live rows."""
    SPT = importlib.import_module("tests.test_sp_engine_gpu")
    out = SPT._spawn(_sp_worker)
    for r in range(2):
        assert "error" not in out[r], out[r].get("error")
        assert out[r]["is_sharded"] and not out[r]["skips"] and out[r]["rows"] == [MA] * STEPS
        assert np.array_equal(out[r]["sharded"], out[r]["base"])
        assert "VgptError" in out[r]["refused"] and "sequence-parallel engine cuts its shares" in out[r]["refused"]
    assert np.array_equal(out[0]["sharded"], out[1]["sharded"])


# ---- pipeline --------------------------------------------------------------------------------------------------------------

def test_pipeline_hands_the_schedule_to_the_scheduler(monkeypatch):
    from oracle import vae_ref as VR
    cfg, vcfg = R.TINY, VR.TINY_VAE8
    p = {k: v.to(BF).float() for k, v in R.make_params(cfg, 0).items()}
    model = SC.build_product_model(cfg, p, DEV)
    V = importlib.import_module("video-gpt_amd.vae")
    vae = V.AutoencoderKL(block_out_channels=vcfg.block_out_channels, layers_per_block=vcfg.layers_per_block,
                          norm_num_groups=vcfg.norm_num_groups)
    vae.load_state_dict(VR.make_vae_params(vcfg, seed=2))
    vae = vae.to(DEV, torch.float32).eval()
    P = importlib.import_module("video-gpt_amd.processor")
    PL = importlib.import_module("video-gpt_amd.pipeline")
    S = importlib.import_module("video-gpt_amd.scheduler")
    pipe = PL.LVMPipeline(vae, model, P.LVMProcessor(P.SpecialTokenizer(10, 11, 12)), device=DEV)
    assert pipe.guidance_interval is None and pipe.guidance_schedule is None
    rec = []

    class Recording(S.LVMScheduler):
        def __call__(self, z, func, model_kwargs, **kw):
            out = super().__call__(z, func, model_kwargs, **kw)
            rec.append((self, [t.clone() for t in z], model_kwargs, kw, [t.clone() for t in out]))
            return out
    monkeypatch.setattr(PL, "LVMScheduler", Recording)
    frames = [torch.rand(3, 64, 64, generator=torch.Generator("cpu").manual_seed(50 + i)) * 2 - 1 for i in range(2)]
    vnoise = [torch.randn(1, 4, 8, 8, generator=torch.Generator("cpu").manual_seed(70 + i)) for i in range(2)]
    pipe.guidance_interval = (0.25, 0.75)
    out = pipe.prompt_condition_frame_block_autoregressive_inference(
        input_images=frames, height=64, width=64, gen_nums=[2], num_inference_steps=STEPS, use_img_guidance=True,
        img_guidance_scale=1.6, seed=42, output_type="pt", prediction_type="x1", generator_device="cpu", vae_noise=vnoise)
    assert len(out) == 2 + 2 and len(rec) == 1
    sched, z, kw, call_kw, got = rec[0]
    assert sched.guidance_interval == (0.25, 0.75) and sched.last_engine is not None
    s = float(torch.tensor(1.6, dtype=torch.float32))
    assert sched.last_engine.gtable.tolist() == [1.0, s, s, 1.0]
    # the scheduler itself, on the same noise and inputs, with a fresh engine
    direct = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=sched.time_shift, guidance_interval=(0.25, 0.75))
    direct.cache_engines = False
    ref = direct(z, model.frame_block_forward_with_cfg, kw, **call_kw)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(got), torch.cat(ref))
    plain = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=sched.time_shift)
    plain.cache_engines = False
    assert not torch.equal(torch.cat(got), torch.cat(plain(z, model.frame_block_forward_with_cfg, kw, **call_kw)))
    # the single-target entry point hands an explicit schedule on too
    rec.clear()
    pipe.guidance_interval, pipe.guidance_schedule = None, [2.0, 1.0]
    out = pipe(input_images=frames, height=64, width=64, gen_num=1, num_inference_steps=2, use_img_guidance=True,
               img_guidance_scale=1.6, seed=5, output_type="pt", prediction_type="v", generator_device="cpu", vae_noise=vnoise)
    assert len(out) == 3 and [r[0].guidance_schedule for r in rec] == [[2.0, 1.0]]
    # a round the pipeline itself runs without guidance (the img_guidance_scale == 1 shortcut) gets no schedule and runs
    rec.clear()
    out = pipe(input_images=frames, height=64, width=64, gen_num=1, num_inference_steps=2, use_img_guidance=True,
               img_guidance_scale=1, seed=5, output_type="pt", prediction_type="v", generator_device="cpu", vae_noise=vnoise)
    assert len(out) == 3 and [(r[0].guidance_schedule, r[0].guidance_interval) for r in rec] == [(None, None)]
    assert not rec[0][2]["use_img_cfg"]
