"""Stochastic sampler steps (eta) through LVMScheduler's two paths, the engine (graphs, partial runs, the seed in device
memory, the engine cache, a guidance schedule with skipped rows, fp8 options), the sharded engine and the pipeline
(DESIGN.md section 5c), on the tiny model of tests/test_guidance_gpu.py: C = 2, G = 2, 16x16 latents, N = 4 steps.

Against the oracle (tests/sde_cases.py's restatement driving oracle/restate.py's model, with its own fp64 noise from the same
Philox words) the bound is the measured one of scripts/calibrate_sde.py.  test_engine_follows_the_definition_on_its_own_
predictions replays the engine's own predictions through the fp64 restatement at the update kernel's bound."""
import functools
import importlib
import traceback

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import guidance_cases as GC
from tests import sde_cases as SD
from tests import smoke_case as SC
from tests import test_guidance_gpu as TG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
STEPS = SD.STEPS
KERNEL_BOUND = 1e-5     # tests/test_ops_gpu.py::test_euler_cfg_update's bound on the fp32 state
MA, MC, G = TG.MA, TG.MC, TG.G
SEED, STREAM = 20261021, 3


@pytest.fixture(scope="module")
def case():
    return TG._case()


def _scheduler(eta=None, cache=False, graph=True, seed=SEED, stream=STREAM, solver="euler", **opts):
    """eta None: the scheduler without any of the new arguments."""
    S = importlib.import_module("video-gpt_amd.scheduler")
    new = {} if eta is None else dict(eta=eta, noise_seed=seed, noise_stream=stream)
    ctor = {k: opts.pop(k) for k in ("eta_interval", "guidance_interval", "guidance_schedule") if k in opts}
    sched = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=1, solver=solver, **new, **ctor)
    sched.cache_engines, sched.use_graph = cache, graph
    for k, v in opts.items():
        setattr(sched, k, v)
    return sched


def _sample(c, sched, pt="x1", generic=False, z=None, cond=None):
    func = c.model.frame_block_forward_with_cfg
    if generic:
        def func(zl, ts, past_key_values=None, prediction_type="x1", **mk):   # not a bound LVM method -> generic path
            return c.model.frame_block_forward_with_cfg(zl, ts, past_key_values=past_key_values,
                                                        prediction_type=prediction_type, **mk)
    out = torch.cat(sched([t.to(DEV, BF) for t in (c.z if z is None else z)], func, TG._kwargs(c, not generic, cond),
                          prediction_type=pt))
    torch.cuda.synchronize()
    assert (sched.last_engine is None) == generic
    return out


@functools.lru_cache(maxsize=None)
def _oracle(eta, pt):
    p, batch, z, cond = SC.build_case(R.TINY, **SD.CASE)
    with torch.no_grad():
        return torch.cat(SD.oracle_sample(R.TINY, p, batch, z, cond, STEPS, pt, [eta] * STEPS, SEED, STREAM))


# ---- off by default ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("pt", ["x1", "v"])
def test_eta_zero_equals_no_argument(case, pt, path, graph):
    generic = path == "generic"
    base = _sample(case, _scheduler(graph=graph), pt, generic)
    zero = _scheduler(0.0, graph=graph)
    assert torch.equal(_sample(case, zero, pt, generic), base)
    empty = _scheduler(0.5, graph=graph, eta_interval=(0.8, 0.9))            # covers no step of 0, 1/4, 1/2, 3/4
    assert torch.equal(_sample(case, empty, pt, generic), base)
    if not generic:
        assert zero.last_engine.etable is None and empty.last_engine.etable is None
    for solver in ("ab2", "heun"):                                              # nothing stochastic: their own clip
        a = _sample(case, _scheduler(0.5, graph=graph, solver=solver, eta_interval=(0.8, 0.9)), pt, generic)
        assert torch.equal(a, _sample(case, _scheduler(graph=graph, solver=solver), pt, generic))


# ---- against the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("pt", ["x1", "v"])
@pytest.mark.parametrize("eta", SD.ETAS)
def test_scheduler_matches_the_oracle(case, eta, pt, path):
    sched = _scheduler(eta)
    out = _sample(case, sched, pt, generic=path == "generic")
    if path == "fast":
        eng = sched.last_engine
        assert eng.etable.tolist() == [eta] * STEPS and eng.rng.tolist() == [SEED, STREAM] and eng.hoist
    q = f"eta{eta}.{pt}"
    err = SC.rel_l2(out, _oracle(eta, pt))
    away = SC.rel_l2(out, _sample(case, _scheduler(), pt, generic=path == "generic"))
    print(f"{q} {path}: rel-L2 vs oracle {err:.3e} (tolerance {SD.tol(q):.3e}); vs the deterministic clip {away:.3e}")
    assert err < SD.tol(q)


# ---- the engine's own predictions through the fp64 restatement -------------------------------------------------------------

@pytest.mark.parametrize("pt", ["x1", "v"])
@pytest.mark.parametrize("etas", [[0.5] * 4, [1.0] * 4, [0.0, 0.5, 1.0, 0.5]], ids=["half", "one", "mixed"])
def test_engine_follows_the_definition_on_its_own_predictions(case, etas, pt, monkeypatch):
    ops = importlib.import_module("video-gpt_amd.ops")
    sched = _scheduler(0.5, graph=False)
    monkeypatch.setattr(sched, "_eta_table", lambda: torch.tensor(etas, dtype=torch.float32))   # any table, not only an interval
    _sample(case, sched, pt)                      # builds the engine
    eng = sched.last_engine
    assert eng.etable.tolist() == etas and eng.rng.tolist() == [SEED, STREAM]
    preds = []
    real = ops.sampler_update_sde

    def spy(*a, **k):
        preds.append(eng.pred.detach().float().cpu().clone())
        return real(*a, **k)
    monkeypatch.setattr(ops, "sampler_update_sde", spy)
    for other in ("sampler_update", "euler_cfg_update", "sampler_update_sched"):
        monkeypatch.setattr(ops, other, lambda *a, **k: pytest.fail("a deterministic update ran under an eta table"))
    z0 = TG._z0(case)
    eng.set_latents(z0)
    states = []
    for i in range(STEPS):
        eng.run(1, use_graph=False)
        torch.cuda.synchronize()
        states.append(eng.z.detach().double().cpu().clone())
    assert len(preds) == STEPS
    nf = eng.nf
    flat = lambda t: [t.reshape(nf, -1)[j].double() for j in range(nf)]

    def replay(table):
        it, trace = iter(preds), []
        SD.sde_call(eng.sigma.cpu(), table, flat(z0.float().cpu()), lambda zl, t: flat(next(it)), pt, SEED, STREAM, guide=True,
                    scale=float(torch.tensor(SD.SCALE, dtype=torch.float32)), trace=trace)
        return [torch.stack(s) for s in trace]
    own = replay(etas)
    for i in range(STEPS):
        err = SC.rel_l2(states[i], own[i])
        print(f"etas {etas} {pt} step {i}: rel-L2 of the engine's z against the fp64 replay {err:.3e}")
        assert err < KERNEL_BOUND
    det = replay([0.0] * STEPS)
    at = next(i for i, e in enumerate(etas) if e != 0.0)
    miss = SC.rel_l2(states[at], det[at])
    print(f"etas {etas} {pt}: the eta = 0 replay misses z after step {at} by {miss:.3e}")
    assert miss > 1e-2


# ---- determinism, graphs, partial runs -------------------------------------------------------------------------------------

@pytest.mark.parametrize("pt", ["x1", "v"])
def test_graph_replay_partial_runs_and_seeds(case, pt):
    g = _scheduler(0.5, graph=True)
    a = _sample(case, g, pt)
    assert torch.equal(a, _sample(case, _scheduler(0.5, graph=False), pt))
    eng = g.last_engine
    assert eng.graph is not None and eng.graph_last is None and eng.graph_c is None
    z0 = TG._z0(case)
    res = {}
    with TG._side_stream():
        for use_graph in (True, False):
            for split in ((STEPS,), (1, 3), (2, 2)):
                eng.set_latents(z0)
                for n in split:
                    eng.run(n, use_graph=use_graph)
                res[use_graph, split] = eng.z.clone().reshape(-1)
        assert int(eng.step.item()) == STEPS
        # the same engine and graph, other keys: written to device memory, nothing recaptured
        graph = eng.graph
        clips = {}
        for key in ((SEED, STREAM), (SEED + 1, STREAM), (SEED, STREAM + 1), (SEED + (1 << 32), STREAM), (SEED, STREAM)):
            eng.set_noise_seed(*key)
            eng.set_latents(z0)
            eng.run(STEPS, use_graph=True)
            clips.setdefault(key, []).append(eng.z.clone().reshape(-1))
        assert eng.graph is graph
    for v in res.values():
        assert torch.equal(v, res[True, (STEPS,)])
    assert torch.equal(res[True, (STEPS,)].to(BF), a.reshape(-1))
    assert torch.equal(clips[SEED, STREAM][0], clips[SEED, STREAM][1]) and torch.equal(clips[SEED, STREAM][0], res[True, (STEPS,)])
    others = [v[0] for k, v in clips.items() if k != (SEED, STREAM)]
    assert len(others) == 3
    for i, o in enumerate(others):
        assert not torch.equal(o, clips[SEED, STREAM][0])
        assert all(not torch.equal(o, p) for p in others[:i])


# ---- the engine cache ------------------------------------------------------------------------------------------------------

def test_cached_engine_serves_a_new_seed_and_tables_do_not_share(case):
    case.model.__dict__.pop("_vgpt_engine_cache", None)
    s1 = _scheduler(0.5, cache=True, seed=1, stream=0)
    first = _sample(case, s1)
    s2 = _scheduler(0.5, cache=True, seed=2, stream=5)
    second = _sample(case, s2)
    assert s2.last_engine_reused and s2.last_engine is s1.last_engine and len(case.model._vgpt_engine_cache) == 1
    assert s2.last_engine.rng.tolist() == [2, 5]
    fresh = _sample(case, _scheduler(0.5, seed=2, stream=5))
    assert torch.equal(second, fresh) and not torch.equal(second, first)
    s3 = _scheduler(0.5, cache=True, seed=1, stream=0)
    assert torch.equal(_sample(case, s3), first) and s3.last_engine_reused
    # one entry per eta table (and one for none); the seed makes none
    s4 = _scheduler(1.0, cache=True, seed=1, stream=0)
    _sample(case, s4)
    assert not s4.last_engine_reused and s4.last_engine is not s1.last_engine and len(case.model._vgpt_engine_cache) == 2
    s5 = _scheduler(cache=True)
    _sample(case, s5)
    assert not s5.last_engine_reused and s5.last_engine.etable is None
    case.model.__dict__.pop("_vgpt_engine_cache", None)


# ---- with a guidance interval and skipped rows -----------------------------------------------------------------------------

@pytest.mark.parametrize("pt", ["x1", "v"])
def test_guidance_interval_with_skipping(case, pt):
    """The "interval" schedule of tests/guidance_cases.py (steps 0 and 3 unguided) with eta = 0.5: the unguided steps run the
    conditional rows only and leave pred[G:] alone; skipping on and off give the same clip; the oracle under both tables
    agrees within the larger of the two calibrated bounds' quantities (guidance: euler.<pt>.interval, eta: eta0.5.<pt>)."""
    gi = GC.SCHEDULES["interval"]["interval"]
    on = _scheduler(0.5, graph=False, guidance_interval=gi)
    want = _sample(case, on, pt)
    off = _scheduler(0.5, guidance_interval=gi, skip_unguided_branch=False)
    assert torch.equal(_sample(case, off, pt), want)
    assert torch.equal(_sample(case, _scheduler(0.5, guidance_interval=gi), pt), want)        # graphs per step kind
    eng = on.last_engine
    assert eng.cr is not None and off.last_engine.cr is None and eng.gtable is not None and eng.etable is not None
    assert [eng.step_rows(i) for i in range(STEPS)] == [MC, MA, MA, MC]
    eng.set_latents(TG._z0(case))
    eng.pred[G:].fill_(float("nan"))
    before = eng.pred[G:].clone().view(torch.int16)
    eng.run(1, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.pred[G:].view(torch.int16), before)
    assert bool(torch.isfinite(eng.z).all()) and bool(torch.isfinite(eng.z_model.float()).all())
    eng.run(STEPS - 1, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.z.view(-1).to(BF), want.view(-1))
    p, batch, z, cond = SC.build_case(R.TINY, **SD.CASE)
    with torch.no_grad():
        ref = torch.cat(SD.oracle_sample(R.TINY, p, batch, z, cond, STEPS, pt, [0.5] * STEPS, SEED, STREAM,
                                         guidance=GC.TABLES["interval"]))
    err = SC.rel_l2(want, ref)
    bound = max(SD.tol(f"eta0.5.{pt}"), GC.tol(f"euler.{pt}.interval"))
    print(f"eta 0.5 + interval {pt}: rel-L2 vs oracle {err:.3e} (bound {bound:.3e})")
    assert err < bound
    gen = _sample(case, _scheduler(0.5, guidance_interval=gi), pt, generic=True)
    assert SC.rel_l2(gen, ref) < bound


# ---- composition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["attn_fp8", "lin_fp8"])
def test_fp8_options_graph_equals_eager(case, precision):
    opts = TG.PRECISIONS[precision]
    a = _sample(case, _scheduler(0.5, graph=True, **opts))
    b = _sample(case, _scheduler(0.5, graph=False, **opts))
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    assert not torch.equal(a, _sample(case, _scheduler(graph=True, **opts)))


def _sp_worker(rank, world, port, q):
    res = {}
    try:
        SPT = importlib.import_module("tests.test_sp_engine_gpu")
        dist = SPT._init(rank, world, port)
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        c = TG._case()
        res["base"] = _sample(c, _scheduler(0.5)).float().cpu().numpy()
        SPM.initialize_sequence_parallel_state(world)
        sched = _scheduler(0.5, sequence_parallel_engine=True)
        res["sharded"] = _sample(c, sched).float().cpu().numpy()
        res["is_sharded"] = sched.last_engine.sp is not None
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


def test_sharded_engine_equals_the_single_rank_engine():
    """Two ranks over gloo on one GPU (the harness of tests/test_sp_engine_gpu.py): the update runs on the replicated state
    and the noise is a function of (seed, stream, step, element), so every rank has the single-rank clip."""
    SPT = importlib.import_module("tests.test_sp_engine_gpu")
    out = SPT._spawn(_sp_worker)
    for r in range(2):
        assert "error" not in out[r], out[r].get("error")
        assert out[r]["is_sharded"]
        assert np.array_equal(out[r]["sharded"], out[r]["base"])
    assert np.array_equal(out[0]["sharded"], out[1]["sharded"])


# ---- pipeline --------------------------------------------------------------------------------------------------------------

@pytest.fixture
def dropin():
    """video-gpt_amd/dropin on sys.path, as tests/test_dropin_imports.py sets it up."""
    import os
    import sys
    importlib.import_module("video-gpt_amd")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-gpt_amd", "dropin")
    saved = {k: v for k, v in sys.modules.items() if k == "LVM" or k.startswith("LVM.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, path)
    yield
    sys.path.remove(path)
    for k in [k for k in sys.modules if k == "LVM" or k.startswith("LVM.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_pipeline_hands_eta_and_the_noise_key_to_the_scheduler(monkeypatch, dropin):
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
    PL = importlib.import_module("LVM.pipeline")                  # the drop-in package's classes are the product's
    S = importlib.import_module("video-gpt_amd.scheduler")
    assert importlib.import_module("LVM.scheduler").LVMScheduler is S.LVMScheduler
    PLP = importlib.import_module("video-gpt_amd.pipeline")
    assert PL.LVMPipeline is PLP.LVMPipeline
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    pipe = PL.LVMPipeline(vae, model, P.LVMProcessor(P.SpecialTokenizer(10, 11, 12)), device=DEV)
    assert pipe.eta == 0.0 and pipe.eta_interval is None
    rec = []

    class Recording(S.LVMScheduler):
        def __call__(self, z, func, model_kwargs, **kw):
            out = super().__call__(z, func, model_kwargs, **kw)
            rec.append((self, [t.clone() for t in z], model_kwargs, kw, [t.clone() for t in out]))
            return out
    monkeypatch.setattr(PLP, "LVMScheduler", Recording)
    frames = [torch.rand(3, 64, 64, generator=torch.Generator("cpu").manual_seed(50 + i)) * 2 - 1 for i in range(2)]
    vnoise = [torch.randn(1, 4, 8, 8, generator=torch.Generator("cpu").manual_seed(70 + i)) for i in range(8)]
    run = lambda **kw: pipe.prompt_condition_frame_block_autoregressive_inference(
        input_images=frames, height=64, width=64, num_inference_steps=STEPS, use_img_guidance=True, img_guidance_scale=1.6,
        output_type="pt", prediction_type="x1", generator_device="cpu", vae_noise=vnoise, clean_image_noise_level=0.0, **kw)
    pipe.eta, pipe.eta_interval = 0.5, (0.0, 0.75)
    out = run(gen_nums=[2, 2], seed=42)
    assert len(out) == 2 + 2 + 2 and len(rec) == 2
    assert [(r[0].eta, r[0].eta_interval, r[0].noise_seed, r[0].noise_stream) for r in rec] == \
        [(0.5, (0.0, 0.75), 42, 0), (0.5, (0.0, 0.75), 42, 1)]
    for k, (sched, z, kw, call_kw, got) in enumerate(rec):
        assert sched.last_engine is not None and sched.last_engine.etable.tolist() == [0.5, 0.5, 0.5, 0.0]
        assert sched.last_engine.rng.tolist() == [42, k]
        # the scheduler itself, on the same initial noise and inputs, with a fresh engine
        direct = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=sched.time_shift, eta=0.5, eta_interval=(0.0, 0.75),
                                noise_seed=42, noise_stream=k)
        direct.cache_engines = False
        ref = direct(z, model.frame_block_forward_with_cfg, kw, **call_kw)
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(got), torch.cat(ref))
        other = S.LVMScheduler(num_steps=STEPS, time_shifting_factor=sched.time_shift, eta=0.5, eta_interval=(0.0, 0.75),
                               noise_seed=42, noise_stream=1 - k)
        other.cache_engines = False
        assert not torch.equal(torch.cat(got), torch.cat(other(z, model.frame_block_forward_with_cfg, kw, **call_kw)))
    rec.clear()
    run(gen_nums=[2], seed=None)
    assert [(r[0].noise_seed, r[0].noise_stream) for r in rec] == [(0, 0)]
    # the single-target entry point: the generic path, the same arguments, stream = the generation's index
    rec.clear()
    out = pipe(input_images=frames, height=64, width=64, gen_num=2, num_inference_steps=2, use_img_guidance=True,
               img_guidance_scale=1.6, seed=5, output_type="pt", prediction_type="v", generator_device="cpu", vae_noise=vnoise,
               clean_image_noise_level=0.0)
    assert [(r[0].eta, r[0].noise_seed, r[0].noise_stream, r[0].last_engine) for r in rec] == [(0.5, 5, 0, None), (0.5, 5, 1, None)]
    sched, z, kw, call_kw, got = rec[0]
    assert len(got) == 2 and torch.equal(got[0], got[1])        # v predictions: func guided both halves, the noise is shared
    pipe.eta = 0.0
    rec.clear()
    pipe(input_images=frames, height=64, width=64, gen_num=1, num_inference_steps=2, use_img_guidance=True,
         img_guidance_scale=1.6, seed=5, output_type="pt", prediction_type="v", generator_device="cpu", vae_noise=vnoise)
    assert not torch.equal(torch.cat(list(rec[0][4])), torch.cat(list(got)))
    # second-order solvers with eta > 0 are refused by name, before anything runs
    pipe.eta = 0.5
    for solver in ("ab2", "heun"):
        pipe.solver = solver
        with pytest.raises(VgptError, match=r"solver='%s' with eta=0\.5 at step 0: only solver='euler'" % solver):
            run(gen_nums=[2], seed=1)
