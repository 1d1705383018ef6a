"""The per-step guidance scale without a GPU: vgpt_sampler_update_sched is declared, exported and
bound under ABI version 8 and refuses bad operands on the host, naming the value; scheduler.guidance_table against
hand-written tables; step_plan.conditional_live_rows over the layout set of tests/test_step_plan.py, checked against the dense
mask; and the calibration file of tests/guidance_cases.py::tol() against a rerun of one of its quantities."""
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import guidance_cases as GC
from tests import test_step_plan as TSP
from tests.test_collator import P, TOK, side

FAKE = 1 << 20   # a non-null address that is never dereferenced: every call below fails its checks first
INVALID = -1
EULER, AB2, HEUN = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vgpt_sampler_update_sched"

S = importlib.import_module("video-gpt_amd.scheduler")
SP = importlib.import_module("video-gpt_amd.step_plan")
VgptError = importlib.import_module("video-gpt_amd.ops").VgptError


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


def _update(lib, z=FAKE, z_model=FAKE, pred=FAKE, v_hist=FAKE, sigma=FAKE, cfg_table=FAKE, step=FAKE, n_steps=4, n_frames=4,
            elems=64, pred_type=0, solver=AB2, stage=0):
    return lib.vgpt_sampler_update_sched(z, z_model, pred, v_hist, sigma, cfg_table, step, n_steps, n_frames, elems,
                                         pred_type, solver, stage, None)


# ---- the entry point -----------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_exported_and_bound_under_abi_8(pkg, lib):
    with open(os.path.join(ROOT, "include", "vgpt.h")) as f:
        header = f.read()
    assert re.search(r"#define VGPT_ABI_VERSION 8\b", header)
    assert pkg._lib.ABI_VERSION == 8 and lib.vgpt_abi_version() == 8
    assert hasattr(lib, NAME)
    proto = re.search(r"\bint %s\(([^;]*)\);" % NAME, header, re.S).group(1)
    assert "const float* cfg_table" in proto and "use_cfg" not in proto and "cfg_scale" not in proto
    assert len(pkg._lib.SIGNATURES[NAME][1]) == proto.count(",") + 1 == 14
    # nothing existing changed its signature
    assert len(pkg._lib.SIGNATURES["vgpt_sampler_update"][1]) == 15
    assert len(pkg._lib.SIGNATURES["vgpt_euler_cfg_update"][1]) == 12
    assert callable(importlib.import_module("video-gpt_amd.ops").sampler_update_sched)


@pytest.mark.parametrize("solver", [EULER, AB2, HEUN])
def test_null_pointers_are_refused(lib, solver):
    for name in ("z", "z_model", "pred", "sigma", "step"):
        _refused(lib, _update(lib, solver=solver, **{name: None}), b"%s: null pointer" % NAME.encode(), b"(nil)")
    _refused(lib, _update(lib, solver=solver, cfg_table=None), b"%s: null cfg_table ((nil))" % NAME.encode())
    if solver != EULER:
        _refused(lib, _update(lib, solver=solver, v_hist=None), b"%s: null v_hist with solver %d" % (NAME.encode(), solver))


def test_unknown_solver_and_stage_are_refused(lib):
    for bad in (3, -1, 17):
        _refused(lib, _update(lib, solver=bad), b"%s: unknown solver %d" % (NAME.encode(), bad))
    for bad in (2, -1):
        _refused(lib, _update(lib, solver=HEUN, stage=bad), b"%s: unknown stage %d" % (NAME.encode(), bad))
    for solver in (EULER, AB2):
        _refused(lib, _update(lib, solver=solver, stage=1), b"%s: stage 1 of the one-stage solver %d" % (NAME.encode(), solver))


@pytest.mark.parametrize("solver,stage", [(EULER, 0), (AB2, 0), (HEUN, 0), (HEUN, 1)])
def test_bad_shapes_and_types_are_refused(lib, solver, stage):
    kw = dict(solver=solver, stage=stage)
    for nf in (3, 5):
        _refused(lib, _update(lib, n_frames=nf, **kw), b"CFG needs an even number of frames (got %d)" % nf)
    for n in (0, -2):
        _refused(lib, _update(lib, n_steps=n, **kw), b"%s: n_steps %d <= 0" % (NAME.encode(), n))
    for pt in (2, -1):
        _refused(lib, _update(lib, pred_type=pt, **kw), b"%s: unknown prediction type %d" % (NAME.encode(), pt))
    assert _update(lib, n_frames=0, **kw) == 0 and _update(lib, elems=0, **kw) == 0   # nothing to do, nothing read


# ---- guidance_table ------------------------------------------------------------------------------------------------------

def test_guidance_table_by_hand():
    sig = S.LVMScheduler(num_steps=4).sigma               # 0, 1/4, 1/2, 3/4, 1
    assert sig.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    gt = lambda **kw: S.guidance_table(sig, 1.6, **kw)
    assert gt() is None                                   # neither given: the scalar path
    t = gt(interval=(0.25, 0.75))
    assert t.dtype == torch.float32 and tuple(t.shape) == (4,)
    s = float(torch.tensor(1.6, dtype=torch.float32))
    assert t.tolist() == [1.0, s, s, 1.0]                 # lo included, hi excluded
    assert gt(interval=(0.26, 0.75)).tolist() == [1.0, 1.0, s, 1.0]
    assert gt(interval=(0.25, 0.76)).tolist() == [1.0, s, s, s]
    assert gt(interval=(0.0, 1.0)).tolist() == [s] * 4    # sigma[N] = 1 is no step: every step guided
    assert gt(interval=(0.5, 0.5)).tolist() == [1.0] * 4  # an empty interval guides nothing
    assert gt(schedule=[2.0, 1.0, 1.0, 1.25]).tolist() == [2.0, 1.0, 1.0, 1.25]
    assert gt(schedule=torch.tensor([2.0, 1.0, 1.0, 1.25])).tolist() == [2.0, 1.0, 1.0, 1.25]
    assert gt(schedule=lambda x: 1.0 + x).tolist() == [1.0, 1.25, 1.5, 1.75]
    assert GC.TABLES["interval"] == [1.0, 1.6, 1.6, 1.0] and gt(**GC.SCHEDULES["interval"]).tolist() == t.tolist()
    assert gt(**GC.SCHEDULES["explicit"]).tolist() == GC.TABLES["explicit"]


def test_guidance_table_on_a_shifted_sigma_table():
    sig = S.LVMScheduler(num_steps=4, time_shifting_factor=3).sigma     # t / (3 - 2 t): 0, 1/10, 1/4, 1/2, 1
    assert torch.allclose(sig, torch.tensor([0.0, 0.1, 0.25, 0.5, 1.0]))
    assert S.guidance_table(sig, 2.0, interval=(0.2, 0.6)).tolist() == [1.0, 1.0, 2.0, 2.0]
    assert S.guidance_table(sig, 2.0, interval=(0.05, 0.25)).tolist() == [1.0, 2.0, 1.0, 1.0]


def test_guidance_table_refusals_name_the_value():
    sig = S.LVMScheduler(num_steps=4).sigma
    with pytest.raises(VgptError, match=r"interval lo=0\.75 > hi=0\.25"):
        S.guidance_table(sig, 1.6, interval=(0.75, 0.25))
    with pytest.raises(VgptError, match=r"schedule has 3 entries, num_steps is 4"):
        S.guidance_table(sig, 1.6, schedule=[1.0, 2.0, 1.0])
    with pytest.raises(VgptError, match=r"schedule has 5 entries, num_steps is 4"):
        S.guidance_table(sig, 1.6, schedule=[1.0] * 5)
    with pytest.raises(VgptError, match=r"non-finite scale nan at step 2"):
        S.guidance_table(sig, 1.6, schedule=[1.0, 2.0, float("nan"), 1.0])
    with pytest.raises(VgptError, match=r"non-finite scale inf at step 0"):
        S.guidance_table(sig, 1.6, schedule=lambda x: float("inf"))
    with pytest.raises(VgptError, match=r"non-finite scale inf at step 1"):
        S.guidance_table(sig, float("inf"), interval=(0.25, 0.5))
    with pytest.raises(VgptError, match=r"both interval=\(0\.25, 0\.75\) and schedule=\[1\.0, 1\.0, 1\.0, 1\.0\]"):
        S.guidance_table(sig, 1.6, interval=(0.25, 0.75), schedule=[1.0] * 4)
    # the scheduler refuses the same at construction
    with pytest.raises(VgptError, match=r"interval lo=0\.75 > hi=0\.25"):
        S.LVMScheduler(num_steps=4, guidance_interval=(0.75, 0.25))
    with pytest.raises(VgptError, match=r"schedule has 3 entries, num_steps is 4"):
        S.LVMScheduler(num_steps=4, guidance_schedule=[1.0, 2.0, 1.0])
    sched = S.LVMScheduler(num_steps=4, guidance_interval=(0.25, 0.75))
    assert sched.guidance_interval == (0.25, 0.75) and sched.guidance_schedule is None and sched.skip_unguided_branch is None
    with pytest.raises(VgptError, match=r"guidance_interval=\(0\.25, 0\.75\).*use_img_cfg=False: there is nothing to schedule"):
        sched._guidance({"use_img_cfg": False, "img_cfg_scale": 1.6})
    assert S.LVMScheduler(num_steps=4)._guidance({"use_img_cfg": False}) is None


# ---- conditional_live_rows -----------------------------------------------------------------------------------------------

def _owner_of_rows(plan):
    owner = np.full(plan.B * plan.L, -1)
    for b, m in enumerate(plan.row_map):
        owner[m[m >= 0]] = b
    return owner


@pytest.mark.parametrize("name", list(TSP.CASES))
def test_conditional_live_rows_over_the_layout_set(name):
    """C = 2: no prefix is reused, every row is live (the "none" layout); C = 8: the prefix layout, hoisted or not (a bad tail
    falls back to the gap path).  Packed CFG batches must give a range; the unpacked one must give None."""
    (C, G, N, fmt), opts, badtail = TSP.CASES[name]
    batch, plan = TSP._planned(name)
    nf = len(plan.x_rows)
    got = SP.conditional_live_rows(plan, plan.attention_mask, nf)
    if not plan.packed:
        assert got is None
        return
    if badtail:
        # the frame dict of this case lacks one conditional frame on purpose while the time rows keep it (no hoisting, the
        # gap path): the live time rows do not go with the frames one to one, so there is no range to run alone
        assert nf == 2 * G - 1 and len(plan.t_rows) == 2 * G and not plan.hoist and plan.S
        assert got is None
        return
    assert got is not None, name
    a, e, ncf, segs = got
    S, L = plan.S, plan.L
    owner = _owner_of_rows(plan)
    M = TSP._flat_mask(plan)
    # the leading range of the live rows, and exactly the live rows of sequence 0
    assert a == S and S < e < L
    live0 = np.nonzero(owner[S:] == 0)[0] + S
    assert np.array_equal(live0, np.arange(a, e))
    assert (owner[e:] == 1).all()
    # sees nothing live outside itself; everything else it sees is a cached row below S
    assert not M[a:e, e:].any()
    seen = np.nonzero(M[a:e].any(axis=0))[0]
    assert ((seen < S) | ((seen >= a) & (seen < e))).all()
    # the frames of the range are the leading ones, the rest lies behind it
    assert ncf == G == nf // 2
    assert all(a <= x < e for x in plan.x_rows[:ncf]) and all(x >= e for x in plan.x_rows[ncf:])
    if not plan.hoist:
        assert all(a <= t < e for t in plan.t_rows[:ncf]) and all(t >= e for t in plan.t_rows[ncf:])
    # the restricted attention segments: the first of the plan's, covering the range
    seg = plan.seg_live if S else plan.seg_all
    assert segs == (seg[0],) == ((0, a, e),)
    if plan.hoist:
        assert e - a == G * N                       # image rows only


def test_conditional_live_rows_is_none_where_it_must_be():
    name = "c8g3n16_layout_reuse1_hoist1"
    batch, plan = TSP._planned(name)
    nf = len(plan.x_rows)
    assert SP.conditional_live_rows(plan, plan.attention_mask, nf) is not None
    # a pre-packed mask: nothing is known about who sees whom
    ops = importlib.import_module("video-gpt_amd.ops")
    pm = ops.PackedMask(torch.zeros(1), torch.zeros(1), plan.B, plan.L)
    assert SP.conditional_live_rows(plan, pm, nf) is None
    # another number of frames than the plan's
    assert SP.conditional_live_rows(plan, plan.attention_mask, nf + 2) is None
    # a mask in which the range sees a live row behind it: verified from the mask, not assumed
    a, e, _, _ = SP.conditional_live_rows(plan, plan.attention_mask, nf)
    lay = plan.attention_mask
    leaky = lay.with_groups(np.where(lay.kind == 2, 7, lay.grp))     # every noisy token in ONE clip group: the halves meet
    assert leaky.to_bool()[0, a:e, e:].any()
    assert SP.conditional_live_rows(plan, leaky, nf) is None
    dense = torch.from_numpy(lay.to_bool())
    assert SP.conditional_live_rows(plan, dense, nf) is not None
    dense[0, e - 1, e] = True
    assert SP.conditional_live_rows(plan, dense, nf) is None
    # one sequence (no CFG): nothing to split
    C, G, N = 8, 3, 16
    proc = P.LVMProcessor(TOK, mask_format="layout")
    prompt = "".join(f"<img><|image_{i+1}|></img>" if i < C else f"<|diffusion|><|image_{i+1}|>" for i in range(C + G))
    imgs = [torch.zeros(3, side(N), side(N)) for _ in range(C)]
    one = proc.prompt_condition_frame_block_inference([prompt], [imgs], height=side(N), width=side(N), use_img_cfg=False,
                                                      frame_blocks=[C, G])
    for reuse in (False, True):
        p1 = SP.plan_step_rows(one["input_ids"], one["position_ids"], one["attention_mask"], one["input_image_sizes"],
                               one["denoise_image_sizes"], one["time_emb_inx"], pack_padding=True,
                               reuse_condition_prefix=reuse, hoist_special_rows=True)
        assert len(p1.x_rows) == G
        assert SP.conditional_live_rows(p1, p1.attention_mask, G) is None


# ---- the calibration file ------------------------------------------------------------------------------------------------

def test_calibration_file_is_what_the_script_measures():
    """One quantity of tests/golden/tolerance_calibration_guidance.json measured again (one seed of three, the cheapest
    solver): the recorded figure is this computation's.  The rerun may differ from the record by the summation order of
    stock bf16 matmuls under another thread count, far inside 25 %; a figure from another case or another method is not."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        CG = importlib.import_module("calibrate_guidance")
    finally:
        sys.path.pop(0)
    doc = json.load(open(GC.PATH))
    assert set(doc["quantities"]) == {f"{s}.{pt}.{n}" for s in GC.SOLVERS for pt in ("x1", "v") for n in GC.TABLES}
    for q in doc["quantities"].values():
        assert q["samples"] == 3 and q["tolerance"] == pytest.approx(2 * q["stock_bf16_rel_l2_max"], abs=2e-6)
        assert q["stock_bf16_rel_l2_seed0"] <= q["stock_bf16_rel_l2_max"]
    rec = doc["quantities"]["euler.x1.interval"]
    again = CG.measure("euler", "x1", "interval", 0)
    print(f"euler.x1.interval seed 0: recorded {rec['stock_bf16_rel_l2_seed0']:.4e}, measured again {again:.4e}")
    assert abs(again - rec["stock_bf16_rel_l2_seed0"]) <= 0.25 * rec["stock_bf16_rel_l2_seed0"]
    assert GC.tol("euler.x1.interval") == rec["tolerance"]
