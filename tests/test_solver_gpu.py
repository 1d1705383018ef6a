"""The second-order solvers (ab2, heun) through LVMScheduler's two paths, the engine (graphs, partial runs, the engine
cache), the sharded engine and the pipeline, on the tiny model of tests/smoke_case.py::build_case with N = 4 steps.

Against the oracle (tests/solver_cases.py's restatement driving oracle/restate.py's model) the bound is the measured one of
scripts/calibrate_solvers.py; that comparison cannot tell the solvers apart (they differ by 1e-3 to 1.3e-2 at N = 4, below
the bf16 bar), so test_engine_follows_the_solver_on_its_own_predictions replays the engine's own predictions through the
fp64 restatement, at the update kernel's bound."""
import functools
import importlib
import traceback

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import smoke_case as SC
from tests import solver_cases as SV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
STEPS = 4
KERNEL_BOUND = 1e-5     # tests/test_ops_gpu.py::test_euler_cfg_update's bound on the fp32 state


@pytest.fixture(scope="module")
def case():
    WU = importlib.import_module("tests.test_weight_updates_gpu")
    c = WU.Case(R.TINY, C=2, G=2, hw=(8, 8), steps=STEPS)
    c.model = SC.build_product_model(R.TINY, c.p, DEV)
    return c


def _scheduler(solver=None, cache=False, graph=True, **opts):
    S = importlib.import_module("video-gpt_amd.scheduler")
    sched = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=1) if solver is None else \
        S.LVMScheduler(num_steps=STEPS, time_shifting_factor=1, solver=solver)
    sched.cache_engines, sched.use_graph = cache, graph
    for k, v in opts.items():
        setattr(sched, k, v)
    return sched


def _kwargs(c, layout=True, cond=None):
    kw = SC.model_kwargs(c.batch, c.cond if cond is None else cond, DEV)
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


@functools.lru_cache(maxsize=None)
def _oracle(solver, pt):
    p, batch, z, cond = SC.build_case(R.TINY)
    with torch.no_grad():
        return torch.cat(SV.oracle_sample(R.TINY, p, batch, z, cond, STEPS, pt, solver))


# ---- against the oracle --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("pt", ["x1", "v"])
@pytest.mark.parametrize("solver", ["ab2", "heun"])
def test_scheduler_matches_the_oracle_under_the_solver(case, solver, pt, path):
    sched = _scheduler(solver)
    out = _sample(case, sched, pt, generic=path == "generic")
    if path == "fast":
        eng = sched.last_engine
        assert eng.solver == importlib.import_module("video-gpt_amd.ops").SOLVERS[solver]
        assert eng.v_hist is not None and eng.graph is not None and (eng.graph_last is not None) == (solver == "heun")
    err = SC.rel_l2(out, _oracle(solver, pt))
    print(f"{solver} {pt} {path}: rel-L2 vs oracle {err:.3e} (tolerance {SV.tol(f'{solver}.{pt}'):.3e})")
    assert err < SV.tol(f"{solver}.{pt}")


# ---- the engine's own predictions through the fp64 restatement -----------------------------------------------------------

@pytest.mark.parametrize("pt", ["x1", "v"])
@pytest.mark.parametrize("solver", ["ab2", "heun"])
def test_engine_follows_the_solver_on_its_own_predictions(case, solver, pt, monkeypatch):
    ops = importlib.import_module("video-gpt_amd.ops")
    sched = _scheduler(solver, graph=False)
    _sample(case, sched, pt)                      # builds the engine
    eng = sched.last_engine
    preds = []                                    # engine.pred at every update launch, i.e. after every model evaluation
    for name in ("sampler_update", "euler_cfg_update"):
        real = getattr(ops, name)

        def spy(*a, _real=real, **k):
            preds.append(eng.pred.detach().float().cpu().clone())
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    z0 = torch.cat([t.to(DEV, BF) for t in case.z])
    eng.set_latents(z0)
    states, first_of_step = [], []
    for i in range(STEPS):
        first_of_step.append(len(preds))
        eng.run(1, use_graph=False)
        torch.cuda.synchronize()
        states.append(eng.z.detach().double().cpu().clone())
    assert len(preds) == SV.model_evaluations(solver, STEPS)
    nf = eng.nf
    flat = lambda t: [t.reshape(nf, -1)[j].double() for j in range(nf)]

    def replay(which, seq):
        it, trace = iter(seq), []
        SV.solver_call(eng.sigma.cpu(), flat(z0.float().cpu()), lambda zl, t: flat(next(it)), eng.use_cfg, eng.cfg_scale, pt,
                       which, trace=trace)
        return [torch.stack(s) for s in trace]
    own = replay(solver, preds)
    for i in range(STEPS):
        err = SC.rel_l2(states[i], own[i])
        print(f"{solver} {pt} step {i}: rel-L2 of the engine's z against the fp64 replay {err:.3e}")
        assert err < KERNEL_BOUND
    # the Euler restatement on the predictions each step started from is somewhere else.  Where: after the last step the
    # solver itself takes differently from Euler -- the final one for ab2, the one before it for heun.  Heun's final step IS
    # the Euler step, and with x1 predictions an Euler step to sigma = 1 lands on uncond + s (cond - uncond) of the last
    # prediction whatever z it started from (the two halves of z are equal), so the final z cannot tell any two solvers apart.
    euler = replay("euler", [preds[k] for k in first_of_step])
    at = STEPS - 1 if solver == "ab2" else STEPS - 2
    miss = SC.rel_l2(states[at], euler[at])
    print(f"{solver} {pt}: Euler on the same predictions misses z after step {at} by {miss:.3e} "
          f"(after the final step by {SC.rel_l2(states[-1], euler[-1]):.3e})")
    if pt == "x1":
        assert miss > 10 * KERNEL_BOUND


# ---- equalities ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["ab2", "heun"])
def test_graph_replay_equals_eager(case, solver):
    a = _sample(case, _scheduler(solver, graph=True))
    b = _sample(case, _scheduler(solver, graph=False))
    assert torch.equal(a, b)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("solver", ["ab2", "heun"])
def test_partial_runs_add_up(case, solver, graph):
    sched = _scheduler(solver, graph=graph)
    _sample(case, sched)                          # builds the engine (and, with graphs on, captures its steps)
    eng = sched.last_engine
    z0 = torch.cat([t.to(DEV, BF) for t in case.z])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.set_latents(z0)
        eng.run(STEPS, use_graph=graph)
        whole = eng.z.clone().reshape(-1)
        eng.set_latents(z0)
        eng.run(2, use_graph=graph)
        eng.run(2, use_graph=graph)
        split = eng.z.clone().reshape(-1)
        eng.set_latents(z0)
        eng.run(1, use_graph=graph)
        eng.run(3, use_graph=graph)
        split13 = eng.z.clone().reshape(-1)
    side.synchronize()
    assert torch.equal(split, whole) and torch.equal(split13, whole)
    assert int(eng.step.item()) == STEPS and eng.steps_taken == STEPS


@pytest.mark.parametrize("solver", ["ab2", "heun"])
def test_capture_in_the_middle_of_a_clip_leaves_no_trace(case, solver):
    """capture() runs one eager step and takes it back: state, step counter and the velocity history (the ab2 step after
    it reads what the step BEFORE it wrote)."""
    sched = _scheduler(solver, graph=False)
    _sample(case, sched)
    eng = sched.last_engine
    assert eng.graph is None and eng.graph_last is None
    z0 = torch.cat([t.to(DEV, BF) for t in case.z])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.set_latents(z0)
        eng.run(STEPS, use_graph=False)
        whole = eng.z.clone()
        eng.set_latents(z0)
        eng.run(2, use_graph=False)
        eng.capture()
        assert eng.graph is not None
        eng.run(2, use_graph=True)
        got = eng.z.clone()
    side.synchronize()
    assert torch.equal(got, whole) and int(eng.step.item()) == STEPS


@pytest.mark.parametrize("solver", ["ab2", "heun"])
def test_cached_engine_on_a_second_clip_equals_a_fresh_one(case, solver):
    case.model.__dict__.pop("_vgpt_engine_cache", None)
    g = torch.Generator("cpu").manual_seed(7)
    z2 = [torch.randn(1, 4, 8, 8, generator=g).to(BF).float() for _ in range(2)] * 2
    cond2 = [torch.randn(1, 4, 8, 8, generator=g).to(BF).float() for _ in range(2)]
    s1 = _scheduler(solver, cache=True)
    _sample(case, s1)
    s2 = _scheduler(solver, cache=True)
    second = _sample(case, s2, z=z2, cond=cond2)
    assert s2.last_engine_reused and s2.last_engine is s1.last_engine
    fresh = _sample(case, _scheduler(solver), z=z2, cond=cond2)
    assert torch.equal(second, fresh)
    case.model.__dict__.pop("_vgpt_engine_cache", None)


def test_solvers_do_not_share_a_cache_entry(case):
    case.model.__dict__.pop("_vgpt_engine_cache", None)
    se = _scheduler("euler", cache=True)
    euler = _sample(case, se)
    sa = _scheduler("ab2", cache=True)
    ab2 = _sample(case, sa)
    assert not sa.last_engine_reused and sa.last_engine is not se.last_engine
    assert len(case.model._vgpt_engine_cache) == 2
    assert sa.last_engine.v_hist is not None and se.last_engine.v_hist is None
    se2 = _scheduler("euler", cache=True)
    assert torch.equal(_sample(case, se2), euler) and se2.last_engine is se.last_engine
    assert not torch.equal(ab2, euler)
    case.model.__dict__.pop("_vgpt_engine_cache", None)


@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("pt", ["x1", "v"])
def test_euler_by_name_is_the_default(case, pt, path):
    generic = path == "generic"
    assert torch.equal(_sample(case, _scheduler("euler"), pt, generic), _sample(case, _scheduler(None), pt, generic))


# ---- sharded engine ------------------------------------------------------------------------------------------------------

def _sp_worker(rank, world, port, q):
    res = {}
    try:
        SPT = importlib.import_module("tests.test_sp_engine_gpu")
        dist = SPT._init(rank, world, port)
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        WU = importlib.import_module("tests.test_weight_updates_gpu")
        c = WU.Case(R.TINY, C=2, G=2, hw=(16, 16), steps=STEPS)
        c.model = SC.build_product_model(R.TINY, c.p, DEV)
        res["base"] = _sample(c, _scheduler("heun")).float().cpu().numpy()
        SPM.initialize_sequence_parallel_state(world)
        sched = _scheduler("heun", sequence_parallel_engine=True)
        res["sharded"] = _sample(c, sched).float().cpu().numpy()
        res["is_sharded"] = sched.last_engine.sp is not None
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


def test_sharded_heun_equals_the_single_rank_engine():
    """Two ranks over gloo on one GPU (the harness of tests/test_sp_engine_gpu.py): the sharded engine runs the same
    sampler_step eagerly."""
    SPT = importlib.import_module("tests.test_sp_engine_gpu")
    out = SPT._spawn(_sp_worker)
    for r in range(2):
        assert out[r]["is_sharded"]
        assert np.array_equal(out[r]["sharded"], out[r]["base"])
    assert np.array_equal(out[0]["sharded"], out[1]["sharded"])


# ---- pipeline ------------------------------------------------------------------------------------------------------------

def test_pipeline_hands_the_solver_to_the_scheduler(monkeypatch):
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
    assert pipe.solver == "euler"
    rec = []

    class Recording(S.LVMScheduler):
        def __call__(self, z, func, model_kwargs, **kw):
            out = super().__call__(z, func, model_kwargs, **kw)
            rec.append((self, [t.clone() for t in z], model_kwargs, kw, [t.clone() for t in out]))
            return out
    monkeypatch.setattr(PL, "LVMScheduler", Recording)
    frames = [torch.rand(3, 64, 64, generator=torch.Generator("cpu").manual_seed(50 + i)) * 2 - 1 for i in range(2)]
    vnoise = [torch.randn(1, 4, 8, 8, generator=torch.Generator("cpu").manual_seed(70 + i)) for i in range(2)]
    pipe.solver = "heun"
    out = pipe.prompt_condition_frame_block_autoregressive_inference(
        input_images=frames, height=64, width=64, gen_nums=[2], num_inference_steps=STEPS, use_img_guidance=True,
        img_guidance_scale=1.6, seed=42, output_type="pt", prediction_type="x1", generator_device="cpu", vae_noise=vnoise)
    assert len(out) == 2 + 2 and out[0].shape == (64, 64, 3)
    assert len(rec) == 1
    sched, z, kw, call_kw, got = rec[0]
    assert sched.solver == "heun" and sched.last_engine is not None and sched.last_engine.graph_last is not None
    # the scheduler itself, on the same noise and inputs, with a fresh engine
    direct = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=sched.time_shift, solver="heun")
    direct.cache_engines = False
    ref = direct(z, model.frame_block_forward_with_cfg, kw, **call_kw)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(got), torch.cat(ref))
    euler = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=sched.time_shift)
    euler.cache_engines = False
    assert not torch.equal(torch.cat(got), torch.cat(euler(z, model.frame_block_forward_with_cfg, kw, **call_kw)))
    # the single-target entry point hands it on too
    rec.clear()
    pipe.solver = "ab2"
    out = pipe(input_images=frames, height=64, width=64, gen_num=1, num_inference_steps=2, use_img_guidance=True,
               img_guidance_scale=1.6, seed=5, output_type="pt", prediction_type="v", generator_device="cpu", vae_noise=vnoise)
    assert len(out) == 3 and [r[0].solver for r in rec] == ["ab2"]
