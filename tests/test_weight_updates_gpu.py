"""The sampler follows every update of the model's weights.

The bf16 sampler folds a decoder layer's two RMSNorms into the GEMMs around them (engine.py `fuse`): qkv_proj and gate_up_proj
then read DERIVED weights, W * gain (engine.folded_weights), and a cached engine's captured graph reads them at fixed addresses.
The rule every case here checks: a sample from a model whose weights were just updated equals, bit for bit, a sample from a
freshly built model holding the same updated weights (new storage: nothing can be shared with the old one).  Once per kind of
update the fresh sample is also compared with the fp32 oracle, so the fresh side is right and not merely equal.

Update kinds: one Stage1Trainer step (AdamW writes the parameters through raw pointers: autograd's version counters do not
move; with and without the optimizer overlapped with the next forward), Stage1Trainer.load_checkpoint of a checkpoint from
another step, an in-place model.load_state_dict, an in-place torch update of every parameter (an EMA).  Each really changes
every parameter the folded path reads, the RMSNorm gains included.

  * full width (FULL1, the cfg-2 geometry of test_fullwidth_parity_gpu): the only width at which the folded path exists
    (vgpt_gemm_norm_workspace_bytes is 0 below 128 tiles of 256 x 256), every update kind, engine cache on and off;
  * tiny width: regression guards of the other sampler paths (bf16 / MX-fp8 projections x bf16 / MX-fp8 attention), one
    trainer step each;
  * the engine cache and the GEMM kernel family (vgpt_gemm_set_family decides whether an engine folds its norms);
  * vgpt_gemm_bf16_resid_rstd under a forced tile width (VGPT_GEMM_W4_NI, read once per process: a child process per case):
    the workspace size the library reports is the size the launch uses."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

from oracle import restate as R
from tests import smoke_case as SC
from tests.test_fullwidth_parity_gpu import FULL1

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FW_STEPS, TINY_STEPS = 2, 3
LR = 5e-3   # one AdamW step moves every weight with a gradient by about lr: more than half a bf16 ulp of the gains (1 +- 0.1)


def params_from(state_dict):
    """A model's state dict -> the fp32 parameter dict build_product_model and the oracle take (bf16 values: exact)."""
    return {k: v.detach().float().cpu() for k, v in state_dict.items()}


class Case:
    def __init__(self, cfg, C, G, hw, steps):
        P = importlib.import_module("video-gpt_amd.processor")
        LY = importlib.import_module("video-gpt_amd.layout")
        bl = (hw[0] // 2) * (hw[1] // 2) + 2
        self.cfg, self.steps = cfg, steps
        self.p, self.batch, self.z, self.cond = SC.build_case(cfg, C=C, G=G, hw=hw)
        self.lay = LY.TokenLayout.from_plans([(P.plan_inference([C, G])[0], bl, 0), (P.plan_inference([0, G])[0], bl, C * bl)],
                                             (C + G) * bl)

    def sample(self, model, cache, lin="bf16", attn="bf16"):
        S = importlib.import_module("video-gpt_amd.scheduler")
        sched = S.LVMScheduler(num_steps=self.steps, time_shifting_factor=1)
        sched.attention_precision, sched.linear_precision = attn, lin
        sched.use_graph = True
        sched.cache_engines = cache
        kw = SC.model_kwargs(self.batch, self.cond, DEV)
        kw["attention_mask"] = self.lay
        out = torch.cat(sched([t.to(DEV, BF) for t in self.z], model.frame_block_forward_with_cfg, kw, prediction_type="x1"))
        return out, sched

    def oracle(self, params):
        with torch.no_grad():
            return torch.cat(SC.oracle_sample(self.cfg, params, self.batch, self.z, self.cond, self.steps, "x1"))


def stage1_inputs(F_list, n_tok, hw, seed):
    """A stage-1 batch on the device and its latents / noise / times (the cfg-3 batch at full width)."""
    batch = R.collate_stage1(F_list, n_tok)
    gen = torch.Generator("cpu").manual_seed(seed)
    nd = sum(len(v) for v in batch["denoise_image_sizes"].values())
    nc = sum(len(v) for v in batch["input_image_sizes"].values())
    mk = lambda n: torch.randn(n, 4, *hw, generator=gen)
    x1, x0, clean, x0i = mk(nd), mk(nd), mk(nc), mk(nc)
    t = torch.rand(nd, generator=gen)
    ti = 0.9 + 0.1 * torch.rand(nc, generator=gen)
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    return dbatch, x1, x0, t, clean, x0i, ti


def read_by_fold(model):
    """Every parameter of the decoder layers and the final norm: what the folded path reads, gains included."""
    return {n: p_ for n, p_ in model.named_parameters() if n.startswith("llm.layers.") or n == "llm.norm.weight"}


def snapshot(model):
    return {n: p_.detach().clone() for n, p_ in read_by_fold(model).items()}


def assert_all_changed(model, before):
    same = [n for n, p_ in read_by_fold(model).items() if torch.equal(p_.detach(), before[n])]
    assert not same, f"the update left these parameters unchanged: {same}"


def check_update(case, model, update, cache, lin="bf16", attn="bf16", fused=None, oracle=False):
    """Sample, update, sample again, and compare with a freshly built model holding the updated weights."""
    first, s1 = case.sample(model, cache, lin, attn)
    eng = s1.last_engine
    if fused is not None:
        assert (eng.fuse is not None) == fused
    before = snapshot(model)
    update()
    again, s2 = case.sample(model, cache, lin, attn)
    if cache:
        assert s2.last_engine_reused and s2.last_engine is eng
    else:
        assert not s2.last_engine_reused and s2.last_engine is not eng
    params = params_from(model.state_dict())     # state_dict() waits for an overlapped optimizer update
    assert_all_changed(model, before)
    fresh_model = SC.build_product_model(case.cfg, params, DEV)
    fresh, s3 = case.sample(fresh_model, False, lin, attn)
    if fused is not None:
        assert (s2.last_engine.fuse is not None) == fused and (s3.last_engine.fuse is not None) == fused
    assert not torch.equal(again, first)
    assert torch.equal(again, fresh), f"rel-L2 of the updated model's sample vs a fresh model's: {SC.rel_l2(again, fresh):.3e}"
    if oracle:
        err = SC.rel_l2(fresh, case.oracle(params))
        print(f"fresh sample vs oracle after the update: rel-L2 {err:.3e}")
        assert err < 2e-2
    return eng


# ---- full width: the folded RMSNorms ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fw():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    return Case(FULL1, C=4, G=8, hw=(32, 32), steps=FW_STEPS)


@pytest.fixture(scope="module")
def fw_other():
    """Another set of weights for load_state_dict / the EMA (bf16-representable)."""
    return {k: v.to(BF).float() for k, v in R.make_params(FULL1, seed=12).items()}


@pytest.fixture(scope="module")
def fw_stage1():
    """The cfg-3 stage-1 batch: 2 x (8 frames at 256^2) = 2 x 3870 tokens."""
    return stage1_inputs([8, 8], 256, (32, 32), seed=3)


@pytest.mark.parametrize("cache", [True, False], ids=["engine-cache", "no-cache"])
@pytest.mark.parametrize("overlap", [False, True], ids=["serial-adamw", "overlapped-adamw"])
def test_full_width_sample_after_a_trainer_step(fw, fw_stage1, overlap, cache):
    TR = importlib.import_module("video-gpt_amd.train")
    model = SC.build_product_model(FULL1, fw.p, DEV, cls_name="LVMTraining")
    tr = TR.Stage1Trainer(model, lr=LR, weight_decay=0.1, overlap_optimizer=overlap)   # re-points the parameters' storage
    check_update(fw, model, lambda: tr.step(*fw_stage1), cache, fused=True, oracle=cache and not overlap)


@pytest.mark.parametrize("cache", [True, False], ids=["engine-cache", "no-cache"])
def test_full_width_sample_after_loading_a_checkpoint(fw, fw_stage1, cache, tmp_path):
    TR = importlib.import_module("video-gpt_amd.train")
    model = SC.build_product_model(FULL1, fw.p, DEV, cls_name="LVMTraining")
    tr = TR.Stage1Trainer(model, lr=LR, weight_decay=0.1)
    batch, x1, *rest = fw_stage1
    tr.step(batch, x1, *rest)
    path = tr.save_checkpoint(str(tmp_path))
    tr.step(batch, 1.1 * x1, *rest)
    check_update(fw, model, lambda: tr.load_checkpoint(path), cache, fused=True, oracle=cache)
    assert tr.step_count == 1


@pytest.mark.parametrize("cache", [True, False], ids=["engine-cache", "no-cache"])
def test_full_width_sample_after_load_state_dict(fw, fw_other, cache):
    model = SC.build_product_model(FULL1, fw.p, DEV)
    ptrs = [p_.data_ptr() for p_ in model.parameters()]
    check_update(fw, model, lambda: model.load_state_dict(fw_other), cache, fused=True, oracle=cache)
    assert [p_.data_ptr() for p_ in model.parameters()] == ptrs        # in place


@pytest.mark.parametrize("cache", [True, False], ids=["engine-cache", "no-cache"])
def test_full_width_sample_after_an_ema_update(fw, fw_other, cache):
    model = SC.build_product_model(FULL1, fw.p, DEV)

    def ema():
        with torch.no_grad():
            for n, p_ in model.named_parameters():
                p_.mul_(0.9).add_(fw_other[n].to(DEV, BF), alpha=0.1)
    check_update(fw, model, ema, cache, fused=True, oracle=cache)


def test_cached_engine_follows_the_gemm_family(fw):
    """An engine cached under kernel family 0 folds its norms (a family-1 engine cannot: vgpt_gemm_norm_workspace_bytes is 0
    there); after switching to family 1 the same layout samples without an error and equals a fresh family-1 engine."""
    lib = importlib.import_module("video-gpt_amd._lib").load()
    model = SC.build_product_model(FULL1, fw.p, DEV)
    prev = lib.vgpt_gemm_set_family(0)
    try:
        first, s1 = fw.sample(model, True)
        assert s1.last_engine.fuse is not None
        lib.vgpt_gemm_set_family(1)
        again, s2 = fw.sample(model, True)
        fresh, s3 = fw.sample(SC.build_product_model(FULL1, fw.p, DEV), False)
        assert s3.last_engine.fuse is None
        assert torch.equal(again, fresh), f"rel-L2 {SC.rel_l2(again, fresh):.3e}"
        assert not torch.equal(first, again)           # the other family's kernels really ran
    finally:
        lib.vgpt_gemm_set_family(prev)


# ---- tiny width: the other sampler paths -------------------------------------------------------------------------------

@pytest.mark.parametrize("cache", [True, False], ids=["engine-cache", "no-cache"])
@pytest.mark.parametrize("attn", ["bf16", "fp8"])
@pytest.mark.parametrize("lin", ["bf16", "fp8"])
def test_tiny_sample_after_a_trainer_step(lin, attn, cache):
    TR = importlib.import_module("video-gpt_amd.train")
    case = Case(R.TINY, C=2, G=2, hw=(16, 16), steps=TINY_STEPS)
    model = SC.build_product_model(R.TINY, case.p, DEV, cls_name="LVMTraining")
    tr = TR.Stage1Trainer(model, lr=LR, weight_decay=0.1)
    inputs = stage1_inputs([3, 2], 16, (8, 8), seed=0)
    eng = check_update(case, model, lambda: tr.step(*inputs), cache, lin, attn, fused=False)
    assert (eng.mx8 is not None) == (lin == "fp8") and eng.attn_fp8 == (attn == "fp8")


# ---- the folded norm's workspace under a forced tile width ---------------------------------------------------------------

def _forced_width_child(M, N, K):
    """Runs in a child process started with VGPT_GEMM_W4_NI set: vgpt_gemm_bf16_resid_rstd inside a workspace of exactly the
    reported size, followed (same allocation) by a sentinel tail as large as the partial sums of the narrower tiles."""
    ops = importlib.import_module("video-gpt_amd.ops")
    eps = 1e-5
    nbytes = ops.norm_workspace_bytes(M, N, K)
    cnt = (-(-M // 256) * 4 + 255) // 256 * 256
    assert nbytes > cnt
    tail = 2 * -(-N // 192) * M * 4
    buf = torch.zeros(nbytes + tail, dtype=torch.uint8, device=DEV)
    buf[cnt:nbytes].view(torch.float32).fill_(float("nan"))           # partial sums: nothing stale can pass for a written one
    buf[nbytes:].fill_(0xA5)
    g = lambda s: torch.Generator("cpu").manual_seed(s)
    a = (torch.randn(M, K, generator=g(82))).to(DEV, BF)
    w = (torch.randn(N, K, generator=g(83)) * 0.1).to(DEV, BF)
    r = (torch.randn(M, N, generator=g(84))).to(DEV, BF)
    ref = ops.linear(a, w, residual=r)
    rstd = torch.full((M,), float("nan"), dtype=torch.float32, device=DEV)
    out = ops.linear_resid_rstd(a, w, r, rstd, buf[:nbytes], eps, out=torch.empty_like(r))
    torch.cuda.synchronize()
    assert int((buf[nbytes:] != 0xA5).sum()) == 0, "partial sums written past the reported workspace"
    assert int(buf[:cnt].view(torch.int32).abs().sum()) == 0, "arrival counters not back at zero"
    assert torch.equal(out, ref)
    want = torch.rsqrt(ref.cpu().double().pow(2).mean(-1) + eps)
    got = rstd.cpu().double()
    assert torch.isfinite(got).all(), "1 / rms read partial sums nothing wrote"
    assert torch.allclose(got, want, rtol=3e-6)
    print(f"forced-width child ok: M={M} N={N} K={K} workspace {nbytes} bytes")


@pytest.mark.parametrize("natural", [256, 192], ids=["cost-model-256", "cost-model-192"])
def test_folded_norm_workspace_under_a_forced_tile_width(ops, natural):
    """The library's own answer picks the shape: the partial-sum count of the workspace it reports is 2 x the tiles per row at
    the width its cost model takes.  A child process then forces the OTHER width (6 = 192, 8 = 256 columns)."""
    cnt = lambda M: (-(-M // 256) * 4 + 255) // 256 * 256
    picked = None
    for M, N, K in ((4000, 3076, 128), (3000, 3076, 192), (4000, 2000, 128), (3000, 2000, 256), (4000, 1540, 128)):
        nb = ops.norm_workspace_bytes(M, N, K)
        if nb == 0:
            continue
        parts = (nb - cnt(M)) // (4 * M)
        assert parts in (2 * -(-N // 256), 2 * -(-N // 192))
        if parts == 2 * -(-N // natural):
            picked = (M, N, K)
            break
    assert picked is not None, f"no candidate shape where the cost model takes {natural}-wide tiles"
    M, N, K = picked
    assert M % 256 and N % 192 and N % 256                               # ragged in both directions
    env = dict(os.environ, VGPT_GEMM_W4_NI="6" if natural == 256 else "8")
    code = f"from tests.test_weight_updates_gpu import _forced_width_child; _forced_width_child({M}, {N}, {K})"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
