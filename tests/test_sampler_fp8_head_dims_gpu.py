"""The sampler's MX-fp8 options (attention_precision / linear_precision = "fp8") on models with 64- and 128-wide heads
(tests/head_dim_cases.py CONFIGS): 3 Euler steps with CFG, C = 2, G = 2, 16x16 latents, with and without prefix reuse /
special-row hoisting, fp8 attention alone, fp8 projections alone and both -- against the fp32 oracle and against the bf16
engine, plus one graph replay against eager launches.

Tolerances are measured, not set: scripts/calibrate_fp8_head_dims.py runs the oracle's sampler on these cases with stock bf16
ops and the operands of attention / the projections rounded through a numpy model of MX-fp8, and records 2 x its largest
rel-L2 over three seeds against the fp32 run (hdD.mode) and against the stock bf16 run (hdD.mode.vs_bf16) in
tests/golden/tolerance_calibration_fp8_head_dims.json."""
import importlib
import json
import os

import pytest
import torch

from tests import head_dim_cases as HC

DEV = "cuda:0"
BF = torch.bfloat16
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tolerance_calibration_fp8_head_dims.json")
PREC = {"attention": ("fp8", "bf16"), "linear": ("bf16", "fp8"), "both": ("fp8", "fp8")}   # (attention, linear) precision
STEPS, C, G, HW = 3, 2, 2, (16, 16)
_CACHE = {}


def tol(hd, quantity):
    return float(json.load(open(PATH))["quantities"][f"hd{hd}.{quantity}"]["tolerance"])


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def case(hd):
    """(cfg, params, batch, z, cond, product model, layout, oracle latents) of a head dim, built once."""
    if ("case", hd) not in _CACHE:
        from tests import smoke_case as SC
        P = importlib.import_module("video-gpt_amd.processor")
        LY = importlib.import_module("video-gpt_amd.layout")
        cfg = HC.CONFIGS[hd]
        bl = (HW[0] // 2) * (HW[1] // 2) + 2
        p, batch, z, cond = SC.build_case(cfg, C=C, G=G, hw=HW, use_cfg=True)
        lay = LY.TokenLayout.from_plans([(P.plan_inference([C, G])[0], bl, 0), (P.plan_inference([0, G])[0], bl, C * bl)], (C + G) * bl)
        ref = torch.cat(SC.oracle_sample(cfg, p, batch, z, cond, STEPS, "x1", use_cfg=True))
        _CACHE["case", hd] = (cfg, p, batch, z, cond, SC.build_product_model(cfg, p, DEV), lay, ref)
    return _CACHE["case", hd]


def sample(hd, mode, attn, lin, use_graph=True):
    from tests import smoke_case as SC
    S = importlib.import_module("video-gpt_amd.scheduler")
    cfg, p, batch, z, cond, model, lay, _ = case(hd)
    sched = S.LVMScheduler(num_steps=STEPS)
    sched.reuse_condition_prefix = sched.hoist_special_rows = mode == "hoist"
    sched.attention_precision, sched.linear_precision = attn, lin
    sched.use_graph = use_graph
    sched.cache_engines = False
    kw = SC.model_kwargs(batch, cond, DEV, use_cfg=True)
    kw["attention_mask"] = lay
    out = torch.cat(sched([x.to(DEV, BF) for x in z], model.frame_block_forward_with_cfg, kw, prediction_type="x1"))
    return out, sched.last_engine


def bf16_engine(hd, mode):
    if ("bf16", hd, mode) not in _CACHE:
        out, eng = sample(hd, mode, "bf16", "bf16")
        assert not eng.attn_fp8 and not eng.lin_fp8
        _CACHE["bf16", hd, mode] = out
    return _CACHE["bf16", hd, mode]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("mode", ["hoist", "none"])
@pytest.mark.parametrize("hd", [64, 128])
def test_sampler_with_fp8_options(hd, mode, prec):
    attn, lin = PREC[prec]
    out8, eng = sample(hd, mode, attn, lin)
    assert eng.attn_fp8 == (attn == "fp8") and eng.lin_fp8 == (lin == "fp8") and eng.heads[2] == hd
    out16, ref = bf16_engine(hd, mode), case(hd)[-1]
    e_ref, e_bf = rel_l2(out8, ref), rel_l2(out8, out16)
    print(f"sampler head_dim {hd}, fp8 {prec} ({mode}): rel-L2 vs oracle {e_ref:.3e} (tolerance {tol(hd, prec):.3e}), vs bf16 engine "
          f"{e_bf:.3e} (tolerance {tol(hd, prec + '.vs_bf16'):.3e}); bf16 engine vs oracle {rel_l2(out16, ref):.3e}")
    assert torch.isfinite(out8).all() and not torch.equal(out8, out16)
    assert e_ref < tol(hd, prec)
    assert e_bf < tol(hd, prec + ".vs_bf16")


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [64, 128])
def test_graph_replay_equals_eager(hd):
    replay, eng = sample(hd, "hoist", "fp8", "fp8", use_graph=True)
    eager, _ = sample(hd, "hoist", "fp8", "fp8", use_graph=False)
    assert eng.attn_fp8 and eng.lin_fp8
    assert torch.isfinite(replay).all() and torch.equal(replay, eager)


class _Stub:
    """Enough of a model for StaticDenoiser to reach its precision checks: they run before anything touches the device."""

    def __init__(self, head_dim):
        self.llm = type("LLM", (), {})()
        self.llm.config = type("Cfg", (), {"head_dim": head_dim})()

    def _check_ready(self):
        return None


@pytest.mark.parametrize("opt", ["attention_precision", "linear_precision"])
@pytest.mark.parametrize("hd", [32, 80, 256])
def test_engine_refuses_other_head_dims_when_it_is_built(hd, opt):
    E = importlib.import_module("video-gpt_amd.engine")
    with pytest.raises(Exception, match=rf"{opt}='fp8'.*\(64, 96, 128\).*head_dim {hd}\b"):
        E.StaticDenoiser(_Stub(hd), None, None, None, None, None, None, None, 1, (2, 2), False, 1.0, **{opt: "fp8"})


def test_engine_still_refuses_fp8_under_sequence_parallel(monkeypatch):
    E = importlib.import_module("video-gpt_amd.engine")
    SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
    monkeypatch.setattr(SPM, "sp_world", lambda group=None: 2)
    for opt in ("attention_precision", "linear_precision"):
        with pytest.raises(Exception, match=f"{opt}='fp8' is not supported with sequence_parallel"):
            E.StaticDenoiser(_Stub(64), None, None, None, None, None, None, None, 1, (2, 2), False, 1.0, sequence_parallel=True,
                             **{opt: "fp8"})
