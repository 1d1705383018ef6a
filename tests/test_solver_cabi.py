"""The second-order sampler solvers without a GPU: vgpt_sampler_update is declared, exported and bound under ABI version 8;
every host-side refusal happens before any launch and names the offending value; the scheduler and the engine refuse an
unknown solver by name; and the restatement the GPU tests check against (tests/solver_cases.py) is itself second order
for ab2 and heun and first order for euler on the tiny oracle model."""
import importlib
import os
import re

import pytest
import torch

from oracle import restate as R
from tests import smoke_case as SC
from tests import solver_cases as SV

FAKE = 1 << 20   # a non-null address that is never dereferenced: every call below fails its checks first
INVALID = -1
EULER, AB2, HEUN = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("video-gpt_amd")


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib.load()


def _refused(lib, rc, *texts):
    msg = lib.vgpt_last_error()
    assert rc == INVALID, (rc, msg)
    for t in texts:
        assert t in msg, msg


def _update(lib, z=FAKE, z_model=FAKE, pred=FAKE, v_hist=FAKE, sigma=FAKE, step=FAKE, n_steps=4, n_frames=4, elems=64,
            pred_type=0, use_cfg=1, cfg_scale=1.6, solver=AB2, stage=0):
    return lib.vgpt_sampler_update(z, z_model, pred, v_hist, sigma, step, n_steps, n_frames, elems, pred_type, use_cfg,
                                   cfg_scale, solver, stage, None)


def test_entry_point_is_declared_exported_and_bound_under_abi_8(pkg, lib):
    with open(os.path.join(ROOT, "include", "vgpt.h")) as f:
        header = f.read()
    assert re.search(r"#define VGPT_ABI_VERSION 8\b", header)
    assert pkg._lib.ABI_VERSION == 8 and lib.vgpt_abi_version() == 8
    name = "vgpt_sampler_update"
    assert hasattr(lib, name)
    proto = re.search(r"\bint %s\(([^;]*)\);" % name, header, re.S).group(1)
    assert len(pkg._lib.SIGNATURES[name][1]) == proto.count(",") + 1 == 15
    for macro, value in (("VGPT_SOLVER_EULER", 0), ("VGPT_SOLVER_AB2", 1), ("VGPT_SOLVER_HEUN", 2)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    ops = importlib.import_module("video-gpt_amd.ops")
    assert ops.SOLVERS == {"euler": 0, "ab2": 1, "heun": 2}
    assert (ops.SOLVER_EULER, ops.SOLVER_AB2, ops.SOLVER_HEUN) == (0, 1, 2)
    # the Euler entry point keeps its signature
    assert len(pkg._lib.SIGNATURES["vgpt_euler_cfg_update"][1]) == 12


@pytest.mark.parametrize("solver", [EULER, AB2, HEUN])
def test_null_pointers_are_refused(lib, solver):
    for name in ("z", "z_model", "pred", "sigma", "step"):
        _refused(lib, _update(lib, solver=solver, **{name: None}), b"vgpt_sampler_update: null pointer", b"(nil)")
    if solver == EULER:   # no history: the call gets as far as the launch, which this machine cannot make, so only the
        return            # refusal of the OTHER solvers is checked here
    _refused(lib, _update(lib, solver=solver, v_hist=None), b"vgpt_sampler_update: null v_hist with solver %d" % solver)


def test_unknown_solver_and_stage_are_refused(lib):
    for bad in (3, -1, 17):
        _refused(lib, _update(lib, solver=bad), b"vgpt_sampler_update: unknown solver %d" % bad)
    for bad in (2, -1):
        _refused(lib, _update(lib, solver=HEUN, stage=bad), b"vgpt_sampler_update: unknown stage %d" % bad)
    for solver in (EULER, AB2):
        _refused(lib, _update(lib, solver=solver, stage=1),
                 b"vgpt_sampler_update: stage 1 of the one-stage solver %d" % solver)


@pytest.mark.parametrize("solver,stage", [(EULER, 0), (AB2, 0), (HEUN, 0), (HEUN, 1)])
def test_bad_shapes_and_types_are_refused(lib, solver, stage):
    kw = dict(solver=solver, stage=stage)
    for nf in (3, 5):
        _refused(lib, _update(lib, n_frames=nf, use_cfg=1, **kw), b"CFG needs an even number of frames (got %d)" % nf)
    for n in (0, -2):
        _refused(lib, _update(lib, n_steps=n, **kw), b"vgpt_sampler_update: n_steps %d <= 0" % n)
    for pt in (2, -1):
        _refused(lib, _update(lib, pred_type=pt, **kw), b"vgpt_sampler_update: unknown prediction type %d" % pt)
    assert _update(lib, n_frames=0, **kw) == 0 and _update(lib, elems=0, **kw) == 0   # nothing to do, nothing read


def test_scheduler_and_engine_refuse_an_unknown_solver_by_name():
    S = importlib.import_module("video-gpt_amd.scheduler")
    E = importlib.import_module("video-gpt_amd.engine")
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    with pytest.raises(VgptError, match="unknown sampler solver 'rk4'"):
        S.LVMScheduler(num_steps=4, solver="rk4")
    for name in ("euler", "ab2", "heun"):
        assert S.LVMScheduler(num_steps=4, solver=name).solver == name
    assert S.LVMScheduler(num_steps=4).solver == "euler"

    class Untouchable:            # any attribute access would raise AttributeError, not VgptError
        __slots__ = ()
    with pytest.raises(VgptError, match="unknown sampler solver 'midpoint'"):
        E.StaticDenoiser(Untouchable(), None, None, None, None, None, None, None, 2, (8, 8), True, 1.6, solver="midpoint")
    P = importlib.import_module("video-gpt_amd.pipeline")
    assert "self.solver = \"euler\"" in open(P.__file__).read()


def test_solver_cases_euler_is_the_oracles_scheduler_call():
    p, batch, z, cond = SC.build_case(R.TINY)
    with torch.no_grad():
        for pt in ("x1", "v"):
            a = SV.oracle_sample(R.TINY, p, batch, z, cond, 3, pt, "euler")
            b = SC.oracle_sample(R.TINY, p, batch, z, cond, 3, pt)
            assert torch.equal(torch.cat(a), torch.cat(b))
    assert [SV.model_evaluations(s, 25) for s in SV.SOLVERS] == [25, 25, 49]


@pytest.fixture(scope="module")
def convergence():
    """rel-L2 of the final latents against a 256-step Heun run: fp32, v prediction, CFG 1.6, shift 1, parameter seeds 0 and 1
    of the tiny oracle model."""
    err = {}
    with torch.no_grad():
        for seed in (0, 1):
            p, batch, z, cond = SC.build_case(R.TINY, seed=seed)
            ref = torch.cat(SV.oracle_sample(R.TINY, p, batch, z, cond, 256, "v", "heun"))
            for solver in SV.SOLVERS:
                for n in (8, 16):
                    err[seed, solver, n] = SC.rel_l2(torch.cat(SV.oracle_sample(R.TINY, p, batch, z, cond, n, "v", solver)), ref)
    return err


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_is_second_order_for_ab2_and_heun_and_first_for_euler(convergence, seed):
    e = {k[1:]: v for k, v in convergence.items() if k[0] == seed}
    print({f"{s}@{n}": f"{v:.3e}" for (s, n), v in e.items()})
    for solver in ("ab2", "heun"):
        assert e[solver, 8] / e[solver, 16] >= 3, (solver, e)
    assert e["euler", 8] / e["euler", 16] <= 2.5, e
    assert e["ab2", 16] < e["euler", 16] / 4, e
