"""Stage1Trainer on checkpoints whose heads are 64 and 128 wide (attention backward: vgpt_attn_blockmask_bwd_hd).

Two configs (tests/head_dim_cases.py): R.TINY at hidden size 256 with 4 heads / 2 kv heads (head dim 64, GQA) and with
2 heads / 1 kv head (head dim 128).  Each trainer mode is checked the way its own test file checks it at head dim 96:
loss and every gradient against autograd on the fp32 oracle, the stage-2 frame-block layout, gradient checkpointing,
deterministic=True, LoRA adapters, sequence parallelism over two spawned ranks (head dim 64: 4 heads), and the
forward-only evaluation trainer.  Tolerances: 2 x the error of stock bf16 ops on these configs
(tests/golden/tolerance_calibration_head_dims.json, scripts/calibrate_tolerances.py --head-dims).

Without the per-head-dim backward every test here stops at the first backward pass ("head_dim 64 unsupported")."""
import dataclasses
import importlib
import math
import traceback

import pytest
import torch

from oracle import restate as R
from tests import glue_cases as GC
from tests import head_dim_cases as HC
from tests import smoke_case as SC
from tests.test_ops_gpu import g, rel_l2
from tests.test_sp_train_gpu import EPS_BF16, _init, _spawn, _stage2_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
HEAD_DIMS = [64, 128]
MODS = ("qkv_proj", "o_proj")


@pytest.fixture(scope="module")
def TR():
    return importlib.import_module("video-gpt_amd.train")


def _dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


_CASES = {}


def _case(hd):
    """The stage-1 case of the config and autograd on the fp32 oracle, computed once per head dim."""
    if hd not in _CASES:
        cfg = HC.CONFIGS[hd]
        p, batch, *args = GC.stage1_case(cfg)
        x1, x0, t, clean, x0i, ti = args
        pr = {k: v.clone().requires_grad_(k != "pos_embed") for k, v in p.items()}
        loss_ref, xt_ref = R.stage1_loss(pr, cfg, list(x1.split(1)), list(x0.split(1)), t, list(clean.split(1)),
                                         list(x0i.split(1)), ti, batch)
        loss_ref.mean().backward()
        _CASES[hd] = dict(cfg=cfg, p=p, batch=batch, dbatch=_dev(batch), args=tuple(args), loss_ref=loss_ref.detach(),
                          xt_ref=torch.cat(xt_ref).detach(), grads_ref={k: v.grad for k, v in pr.items() if k != "pos_embed"})
    return _CASES[hd]


def _model(cfg, p, cls="LVMTraining", ck=False):
    model = SC.build_product_model(cfg, p, DEV, cls_name=cls)
    if ck:
        model.llm.gradient_checkpointing_enable()
    return model


def _check_against(hd, tr, loss, loss_ref, grads_ref, what):
    e_loss = rel_l2(loss, loss_ref)
    errs = {k: rel_l2(tr.grads[k], ref) for k, ref in grads_ref.items()}
    worst = max(errs, key=errs.get)
    print(f"MEASURE {what} hd {hd}: loss error {e_loss:.3e} (tol {HC.tol(hd, 'loss'):.3e}), worst gradient error "
          f"{errs[worst]:.3e} at {worst} (tol {HC.tol(hd, 'param_grads'):.3e})")
    assert e_loss < HC.tol(hd, "loss"), e_loss
    bad = {k: v for k, v in errs.items() if not v < HC.tol(hd, "param_grads")}
    assert not bad, bad


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_stage1_loss_and_gradients_match_autograd(TR, hd):
    c = _case(hd)
    cfg = c["cfg"]
    assert cfg.head_dim == hd
    model = _model(cfg, c["p"])
    tr = TR.Stage1Trainer(model, lr=1e-3, weight_decay=0.1, max_grad_norm=1.0)
    loss = tr.step(c["dbatch"], *c["args"], update=False)
    assert rel_l2(tr.last["xt"], c["xt_ref"]) < 4e-3
    _check_against(hd, tr, loss, c["loss_ref"], c["grads_ref"], "stage-1")
    # the full step: clip to 1.0 on the global norm, AdamW on fp32 master weights
    total = math.sqrt(sum(float(v.double().pow(2).sum()) for v in c["grads_ref"].values()))
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith("_proj.weight")}
    tr.step(c["dbatch"], *c["args"], update=True)
    assert abs(float(tr.grad_norm) - total) < 5e-2 * total
    after = model.state_dict()
    for k, v in before.items():      # every decoder matrix moved, qkv_proj (fed by the attention backward) among them
        assert float((after[k].float() - v.float()).abs().max()) > 0, k
    l0 = float(loss.mean())
    for _ in range(5):
        l1 = float(tr.step(c["dbatch"], *c["args"]).mean())
    assert l1 < l0


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_stage2_frame_block_layout_gradients(TR, hd):
    """The frame-block batch of tests/test_train_gpu.py::test_stage2_frame_block_layout_gradients (noisy clips of 2, 1 and
    2 frames, clean groups between them, one t per block) through LVMTraining_CP."""
    cfg = HC.CONFIGS[hd]
    _, batch, (x1, x0, t, clean, x0i, ti) = _stage2_case()
    p = {k: v.to(BF).float() for k, v in R.make_params(cfg, 4).items()}
    pr = {k: v.clone().requires_grad_(k != "pos_embed") for k, v in p.items()}
    loss_ref, _ = R.stage1_loss(pr, cfg, list(x1.split(1)), list(x0.split(1)), t, list(clean.split(1)),
                                list(x0i.split(1)), ti, batch)
    loss_ref.mean().backward()
    tr = TR.Stage1Trainer(_model(cfg, p, "LVMTraining_CP"))
    loss = tr.step(_dev(batch), x1, x0, t, clean, x0i, ti, update=False)
    _check_against(hd, tr, loss, loss_ref.detach(), {k: v.grad for k, v in pr.items() if k != "pos_embed"}, "stage-2")


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_gradient_checkpointing_gives_bit_identical_gradients(TR, hd):
    c = _case(hd)
    out = {}
    for ck in (False, True):
        tr = TR.Stage1Trainer(_model(c["cfg"], c["p"], ck=ck), lr=1e-3, weight_decay=0.1)
        assert tr.gradient_checkpointing == ck
        loss = tr.step(c["dbatch"], *c["args"], update=False)
        torch.cuda.synchronize()
        out[ck] = (loss.clone(), {k: v.clone() for k, v in tr.grads.items()}, tr._ws["qkv"].shape[0])
    assert out[False][2] == c["cfg"].num_hidden_layers and out[True][2] == 1
    assert torch.equal(out[False][0], out[True][0])
    big = {k for names in tr.layer_names for k in names}
    assert any("qkv_proj" in k for k in big)
    for k in big:                     # the decoder matrices: deterministic GEMMs behind a deterministic attention backward
        assert torch.equal(out[True][1][k], out[False][1][k]), k


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_deterministic_runs_are_the_same_run(TR, hd):
    c = _case(hd)
    x1, *rest = c["args"]
    runs = []
    for _ in range(2):
        model = _model(c["cfg"], c["p"])
        tr = TR.Stage1Trainer(model, lr=1e-3, weight_decay=0.1, max_grad_norm=0.5, deterministic=True)
        assert tr.deterministic
        snaps = []
        for i in range(2):
            loss = tr.step(c["dbatch"], x1 * (1 + 0.1 * i), *rest)
            tr.finish_optimizer()
            torch.cuda.synchronize()
            snap = {"loss": loss.detach().clone()}
            snap.update({f"grad:{k}": v.clone() for k, v in tr.grads.items()})
            snap.update({f"param:{k}": v.detach().clone() for k, v in model.state_dict().items()})
            snaps.append(snap)
        runs.append(snaps)
    assert not torch.equal(runs[0][0]["param:llm.norm.weight"], runs[0][1]["param:llm.norm.weight"])     # the chain moves
    for i, (a, b) in enumerate(zip(*runs)):
        assert a.keys() == b.keys()
        bad = [k for k in a if not torch.equal(a[k], b[k])]
        assert not bad, f"step {i}: differ in {bad[:8]} ({len(bad)} of {len(a)})"


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_lora_adapter_gradients_match_autograd_and_the_base_stays_frozen(TR, hd):
    """As tests/test_lora_gpu.py::test_adapter_gradients_match_autograd: the oracle run with W + s B @ A on qkv_proj / o_proj,
    A and B fp32 leaves."""
    c = _case(hd)
    cfg = c["cfg"]
    model = _model(cfg, c["p"])
    torch.manual_seed(11)
    tr = TR.Stage1Trainer(model, lora_rank=4, lr=1e-3)
    gen = g(44)
    for k, v in tr.lora.items():         # lora_B away from its zero init, so that dA is not trivially zero
        if ".lora_B." in k:
            v.copy_((torch.randn(v.shape, generator=gen) * 0.02).to(BF))
    tr.lora_master.copy_(tr.lora_param)
    leaves = {k: v.detach().float().cpu().clone().requires_grad_() for k, v in tr.lora.items()}
    pr = {k: v.clone() for k, v in c["p"].items()}
    for i in range(cfg.num_hidden_layers):
        for mod in MODS:
            wn = f"llm.layers.{i}.self_attn.{mod}.weight"
            pr[wn] = pr[wn] + tr.lora_scale * (leaves[TR.lora_key(i, mod, "B")] @ leaves[TR.lora_key(i, mod, "A")])
    x1, x0, t, clean, x0i, ti = c["args"]
    loss_ref, _ = R.stage1_loss(pr, cfg, list(x1.split(1)), list(x0.split(1)), t, list(clean.split(1)), list(x0i.split(1)),
                                ti, c["batch"])
    loss_ref.mean().backward()
    loss = tr.step(c["dbatch"], *c["args"], update=False)
    ref = {k: v.grad for k, v in leaves.items()}
    assert set(tr.grads) == set(ref) and len(ref) == 2 * len(MODS) * cfg.num_hidden_layers
    assert all(float(v.abs().max()) > 0 for v in ref.values())
    _check_against(hd, tr, loss, loss_ref.detach(), ref, "lora r=4")
    base = {k: v.detach().clone() for k, v in model.state_dict().items()}
    adapters = tr.lora_param.clone()
    tr.step(c["dbatch"], *c["args"])
    tr.finish_optimizer()
    torch.cuda.synchronize()
    for k, v in model.state_dict().items():
        assert torch.equal(v, base[k]), f"base weight {k} moved"
    assert not torch.equal(tr.lora_param, adapters)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_evaluation_trainer_gives_the_trainers_forward_loss(TR, hd):
    c = _case(hd)
    model = _model(c["cfg"], c["p"])
    tr = TR.Stage1Trainer(model, lr=1e-3)
    loss = tr.step(c["dbatch"], *c["args"], update=False).clone()
    ev = TR.Stage1Trainer.for_evaluation(model)
    assert ev.forward_only and ev is TR.Stage1Trainer.for_evaluation(model)
    assert torch.equal(ev.step(c["dbatch"], *c["args"], update=False), loss)
    assert rel_l2(loss, c["loss_ref"]) < HC.tol(hd, "loss")


def test_a_width_that_cannot_train_is_refused_when_the_trainer_is_built(TR):
    """Head dim 80 (hidden 160, 2 heads): refused at construction with the value, not in the first backward; a forward-only
    trainer needs no backward and is built."""
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    cfg = dataclasses.replace(R.TINY, hidden_size=160, num_attention_heads=2, num_key_value_heads=2)
    assert cfg.head_dim == 80
    model = _model(cfg, {k: v.to(BF).float() for k, v in R.make_params(cfg, 0).items()})
    with pytest.raises(VgptError, match="head_dim 80 cannot train"):
        TR.Stage1Trainer(model, lr=1e-3)
    assert TR.Stage1Trainer(model, forward_only=True).forward_only


# ---- sequence parallelism: two spawned ranks over gloo on the one GPU, head dim 64 (4 heads / 2 kv heads: 2 / 1 per rank) ----
def _sp_worker(rank, world, port, q):
    res = {}
    try:
        importlib.import_module("video-gpt_amd")
        TRm = importlib.import_module("video-gpt_amd.train")
        E = importlib.import_module("video-gpt_amd.engine")
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        cfg = HC.CONFIGS[64]
        p, batch, *args = GC.stage1_case(cfg)
        db = _dev(batch)
        # P = 1 first: no process group exists yet
        tr1 = TRm.Stage1Trainer(_model(cfg, p), lr=1e-3, weight_decay=0.1)
        loss1 = tr1.step(db, *args, update=False).clone()
        torch.cuda.synchronize()
        dh1 = tr1._ws["dh"].clone()
        g1 = {k: v.clone() for k, v in tr1.grads.items()}
        big = [k for names in tr1.layer_names for k in names]
        _init(rank, world, port)
        import torch.distributed as dist
        SPM.initialize_sequence_parallel_state(world)
        trs = TRm.Stage1Trainer(_model(cfg, p), lr=1e-3, weight_decay=0.1, sequence_parallel=True)
        res["sharded"] = trs._sp is not None and trs._sp["P"] == world
        loss = trs.step(db, *args, update=False).clone()
        torch.cuda.synchronize()
        r0, r1 = E.sp_shares(trs._ws["seq_all"].shape[0], world)[0][rank]
        res["loss_equal"] = bool(torch.equal(loss, loss1))
        res["dh_equal"] = bool(torch.equal(trs._ws["dh"], dh1[r0:r1])) and float(dh1[r0:r1].float().norm()) > 0
        gsp = {k: v.clone() for k, v in trs.grads.items()}
        trs.skip_allreduce = True                     # this rank's partial sums
        trs.step(db, *args, update=False)
        torch.cuda.synchronize()
        trs.skip_allreduce = False
        nrm = lambda t_: float(t_.double().norm())    # noqa: E731
        res["matrices"] = {k: (nrm(gsp[k].double() - g1[k].double()), nrm(gsp[k]), nrm(g1[k]), nrm(trs.grads[k])) for k in big}
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


def test_sequence_parallel_two_ranks_head_dim_64():
    """Loss and the share's rows of d(sequence) are the P = 1 bits; a decoder gradient is within three bf16 roundings of the
    P = 1 gradient, the bound of tests/test_sp_train_gpu.py::test_stage1_decoder_gradients_within_three_bf16_roundings."""
    two = _spawn(_sp_worker, 2)
    for r in range(2):
        assert two[r]["sharded"] and two[r]["loss_equal"] and two[r]["dh_equal"]
        for k, (diff, n_sp, n_1, _) in two[r]["matrices"].items():
            partials = sum(two[q_]["matrices"][k][3] for q_ in range(2))
            bound = 1.25 * EPS_BF16 * (n_sp + n_1 + partials)
            print(f"MEASURE rank {r} {k}: |g_sp - g_1| {diff:.4e} bound {bound:.4e}")
            assert n_1 > 0 and diff <= bound, (r, k, diff, bound)
            assert all(two[q_]["matrices"][k][3] > 0 for q_ in range(2))
