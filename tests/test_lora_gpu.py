"""LoRA fine-tuning through Stage1Trainer(lora_rank=r) (LVM/train/train_x1_stage1_noiseinput.py:204-223), the adapter
files and the merge (LVM/pipeline.py:97-101), at tiny width.

The gradient oracle is the existing R.stage1_loss called with the qkv_proj / o_proj weights replaced by W + s B @ A, A and
B fp32 leaf tensors: autograd gives dA and dB, the oracle itself is unchanged."""
import importlib
import json
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import glue_cases as GC
from tests import smoke_case as SC
from tests.test_ops_gpu import g, rel_l2
from tests.test_train_kernels_gpu import U32, _ulp, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
MODS = ("qkv_proj", "o_proj")


@pytest.fixture(scope="module")
def TR():
    return importlib.import_module("video-gpt_amd.train")


@pytest.fixture(scope="module")
def case():
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(R.TINY)
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    return dict(p=p, batch=batch, args=(x1, x0, t, clean, x0i, ti), dbatch=dbatch)


def _trainer(TR, p, r, cls="LVMTraining", seed=11, b_seed=None, ck=False, **kw):
    """A LoRA trainer on a fresh model; adapters drawn from torch's global generator seeded with `seed`; b_seed: lora_B set
    to seeded N(0, 0.02) (working copy and master) so that dA is not trivially zero."""
    model = SC.build_product_model(R.TINY, p, DEV, cls_name=cls)
    if ck:
        model.llm.gradient_checkpointing_enable()
    torch.manual_seed(seed)
    tr = TR.Stage1Trainer(model, lora_rank=r, **kw)
    if b_seed is not None:
        gen = g(b_seed)
        for k, v in tr.lora.items():
            if ".lora_B." in k:
                v.copy_((torch.randn(v.shape, generator=gen) * 0.02).to(BF))
        if not tr.forward_only:
            tr.lora_master.copy_(tr.lora_param)
    return tr


def _with_adapters(TR, p, lora, scale):
    """The oracle's parameter dict with W + s B @ A on the adapted projections; returns it and the fp32 leaves."""
    leaves = {k: v.detach().float().cpu().clone().requires_grad_() for k, v in lora.items()}
    pr = {k: v.clone() for k, v in p.items()}
    for i in range(R.TINY.num_hidden_layers):
        for mod in MODS:
            if TR.lora_key(i, mod, "A") not in leaves:
                continue
            wn = f"llm.layers.{i}.self_attn.{mod}.weight"
            pr[wn] = pr[wn] + scale * (leaves[TR.lora_key(i, mod, "B")] @ leaves[TR.lora_key(i, mod, "A")])
    return pr, leaves


def _oracle_grads(TR, p, tr, batch, args):
    x1, x0, t, clean, x0i, ti = args
    pr, leaves = _with_adapters(TR, p, tr.lora, tr.lora_scale)
    loss, _ = R.stage1_loss(pr, R.TINY, list(x1.split(1)), list(x0.split(1)), t, list(clean.split(1)), list(x0i.split(1)), ti,
                            batch)
    loss.mean().backward()
    return loss.detach(), {k: v.grad for k, v in leaves.items()}


def _grad_tol():
    """SC.tol("param_grads") holds for every adapter gradient (measured: 3.4e-3 .. 4.8e-3 against 1.6e-2), so the SURVEY
    section 8(d) fallback of a tolerance file of its own is not needed."""
    return SC.tol("param_grads")


def _check_grads(TR, p, tr, batch, dbatch, args, what):
    loss = tr.step(dbatch, *args, update=False)
    loss_ref, ref = _oracle_grads(TR, p, tr, batch, args)
    e_loss = rel_l2(loss, loss_ref)
    errs = {k: rel_l2(tr.grads[k], ref[k]) for k in ref}
    worst = max(errs, key=errs.get)
    print(f"MEASURE {what}: loss error {e_loss:.3e} (tol {SC.tol('loss'):.3e}), worst adapter gradient error "
          f"{errs[worst]:.3e} at {worst} (tol {_grad_tol():.3e})")
    assert e_loss < SC.tol("loss"), e_loss
    assert set(tr.grads) == set(ref) and len(ref) == 2 * len(tr.lora_targets) * R.TINY.num_hidden_layers
    bad = {k: v for k, v in errs.items() if not v < _grad_tol()}
    assert not bad, bad
    return loss


# ---- 1. gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [4, 8, 24])
def test_adapter_gradients_match_autograd(TR, case, r):
    tr = _trainer(TR, case["p"], r, b_seed=40 + r)
    assert tr.lora_rp == (16 if r <= 16 else 32) and tr.lora_scale == 1.0
    _check_grads(TR, case["p"], tr, case["batch"], case["dbatch"], case["args"], f"stage-1 r={r}")


@pytest.mark.parametrize("target", MODS)
def test_adapter_gradients_with_one_target_module(TR, case, target):
    """lora_target_modules may name one of the two projections: the other keeps its fused forward and gets no adapter."""
    tr = _trainer(TR, case["p"], 8, b_seed=50, lora_target_modules=(target,))
    assert tr.lora_targets == (target,) and all(f".{target}." in k for k in tr.lora)
    _check_grads(TR, case["p"], tr, case["batch"], case["dbatch"], case["args"], f"stage-1 r=8, {target} only")


def _stage2_case():
    """The stage-2 frame-block batch test_train_gpu.test_stage2_frame_block_layout_gradients builds."""
    cfg = R.TINY
    P = importlib.import_module("video-gpt_amd.processor")
    p = {k: v.to(BF).float() for k, v in R.make_params(cfg, 4).items()}
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12))
    fbs = [2, 1, 2]
    prompt, i, j, n = "", 0, 0, 0
    for k, fb in enumerate(fbs):
        for _ in range(fb):
            prompt += f"<|diffusion|><|image_{i + 1}|>"; i += 1; n += 1
        if k != len(fbs) - 1:
            for _ in range(fb):
                prompt += f"<img><|image_{j + 1}|></img>"; j += 1
    row = proc.process_multi_modal_prompt_frame_block_training(prompt, [torch.zeros(3, 64, 64) for _ in range(n)], fbs)
    row["frame_blocks"] = fbs
    ids, pos, mask, pv, sizes, fb = proc.collator.process_mllm_input_frame_block_training([row])
    den, inp, tix, idx = {0: []}, {0: []}, {0: []}, 0
    for k, f in enumerate(fbs):
        if k != len(fbs) - 1:
            for _ in range(f):
                den[0].append(sizes[0][idx]); inp[0].append(sizes[0][idx + f]); tix[0].append(sizes[0][idx][0] - 1); idx += 1
            idx += f
        else:
            for _ in range(f):
                den[0].append(sizes[0][idx]); tix[0].append(sizes[0][idx][0] - 1); idx += 1
    batch = dict(input_ids=ids, position_ids=pos, attention_mask=mask, denoise_image_sizes=den, input_image_sizes=inp,
                 time_emb_inx=tix)
    gen = torch.Generator("cpu").manual_seed(9)
    nd, nc = len(den[0]), len(inp[0])
    mk = lambda m: torch.randn(m, 4, 8, 8, generator=gen)
    x1, x0, clean, x0i = mk(nd), mk(nd), mk(nc), mk(nc)
    tb = torch.rand(len(fbs), generator=gen)
    t = torch.cat([tb[k].repeat(f) for k, f in enumerate(fbs)])
    ti = 0.9 + 0.1 * torch.rand(nc, generator=gen)
    return p, batch, (x1, x0, t, clean, x0i, ti)


def test_adapter_gradients_on_the_stage2_frame_block_batch(TR):
    p, batch, args = _stage2_case()
    tr = _trainer(TR, p, 8, cls="LVMTraining_CP", b_seed=77)
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    _check_grads(TR, p, tr, batch, dbatch, args, "stage-2 frame blocks r=8")


# ---- 2. zero-B init ----------------------------------------------------------------------------------------------------
def test_zero_b_init(TR, case):
    tr = _trainer(TR, case["p"], 8)
    for k, v in tr.lora.items():
        if ".lora_B." in k:
            assert not v.any(), k
        else:   # peft "gaussian": N(0, (1/r)^2); 8 x 64 or more draws per matrix
            assert tuple(v.shape)[0] == 8 and 0.5 / 8 < float(v.float().std()) < 1.5 / 8, (k, float(v.float().std()))
    loss = tr.step(case["dbatch"], *case["args"], update=False)
    for k, v in tr.grads.items():
        if ".lora_A." in k:
            assert not v.any(), f"{k}: dA must be exactly zero while B is zero"
        else:
            assert float(v.abs().max()) > 0, f"{k}: dB must not be zero"
    full = TR.Stage1Trainer(SC.build_product_model(R.TINY, case["p"], DEV, cls_name="LVMTraining"), forward_only=True)
    loss_full = full.step(case["dbatch"], *case["args"], update=False, backward=False)
    assert rel_l2(loss, loss_full) < SC.tol("loss")


# ---- 3. base frozen, optimizer state, one AdamW step ---------------------------------------------------------------------
def test_base_frozen_and_adamw(TR, case):
    tr = _trainer(TR, case["p"], 8, b_seed=5, lr=1e-2, weight_decay=0.1, max_grad_norm=0.5, betas=(0.8, 0.95), eps=1e-7)
    base = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in tr.model.named_parameters()}
    for name in ("master_layers", "master_small", "m_layers", "v_layers", "m_small", "v_small", "layer_buckets", "small_bucket",
                 "param_layers", "param_small"):
        assert not hasattr(tr, name), f"a LoRA trainer must not hold {name}"
    n = tr.lora_param.numel()
    at = tr.model.llm.layers[0].self_attn
    assert n == R.TINY.num_hidden_layers * 16 * (sum(at.qkv_proj.weight.shape) + sum(at.o_proj.weight.shape))   # rp-padded
    assert tr.lora_master.numel() + tr.lora_m.numel() + tr.lora_v.numel() == 3 * n and tr.lora_bucket.numel() == n
    # one update == torch.optim.AdamW on fp32 copies, fed the trainer's own gradient and clip coefficient
    tr.step(case["dbatch"], *case["args"], update=False)
    ref = torch.nn.Parameter(tr.lora_master.detach().clone())
    opt = torch.optim.AdamW([ref], lr=1e-2, weight_decay=0.1, betas=(0.8, 0.95), eps=1e-7)
    grad = tr.lora_bucket.detach().clone()
    tr.optimizer_step()
    norm = float(grad.double().norm())
    assert abs(float(tr.grad_norm) - norm) < 1e-5 * norm
    ref.grad = grad * min(1.0, 0.5 / (norm + 1e-6))
    opt.step()
    assert rel_l2(tr.lora_master, ref.detach()) < 1e-6, rel_l2(tr.lora_master, ref.detach())
    assert torch.equal(tr.lora_param, tr.lora_master.to(BF))
    before = tr.lora_param.clone()
    for _ in range(2):
        tr.step(case["dbatch"], *case["args"])
    torch.cuda.synchronize()
    assert tr.step_count == 3 and not torch.equal(tr.lora_param, before)
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, base[k]), f"base parameter {k} moved"
    assert all(v.data_ptr() == ptrs[k] for k, v in tr.model.named_parameters()), "base parameters were re-pointed"
    for (i, mod), w in tr._lora_w.items():          # the padded ranks stay exactly zero through the updates
        assert not w["A"][8:].any() and not w["B"][:, 8:].any(), (i, mod)


# ---- 4. checkpointing / overlap_optimizer --------------------------------------------------------------------------------
def test_gradient_checkpointing_is_bit_identical(TR, case):
    out = {}
    for ck in (False, True):
        tr = _trainer(TR, case["p"], 8, b_seed=6, ck=ck)
        assert tr.gradient_checkpointing == ck
        loss = tr.step(case["dbatch"], *case["args"], update=False)
        torch.cuda.synchronize()
        out[ck] = (loss.clone(), tr.lora_bucket.clone(), tr._ws["u_q"].shape[0])
    assert out[False][2] == R.TINY.num_hidden_layers and out[True][2] == 1
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])
    assert float(out[False][1].abs().max()) > 0


def test_overlap_optimizer_is_the_same_run(TR, case):
    x1, x0, t, clean, x0i, ti = case["args"]
    out = {}
    for ov in (False, True):
        tr = _trainer(TR, case["p"], 8, b_seed=7, lr=1e-3, weight_decay=0.1, max_grad_norm=0.5, overlap_optimizer=ov)
        assert tr.overlap_optimizer == ov
        losses = [tr.step(case["dbatch"], x1 * (1 + 0.1 * i), x0, t, clean, x0i, ti).clone() for i in range(4)]
        tr.finish_optimizer()
        torch.cuda.synchronize()
        out[ov] = (torch.stack(losses), tr.lora_master.clone(), tr.lora_v.clone(), tr.lora_param.clone())
    # the bounds of test_train_gpu.test_optimizer_overlapped_with_the_next_forward_is_the_same_training_run
    assert rel_l2(out[True][0], out[False][0]) < 1e-5
    assert rel_l2(out[True][1], out[False][1]) < 2e-6 and rel_l2(out[True][2], out[False][2]) < 2e-6
    assert rel_l2(out[True][3], out[False][3]) < 1e-4


# ---- 5. merge ------------------------------------------------------------------------------------------------------------
def test_merge(TR, case, tmp_path):
    LORA = importlib.import_module("video-gpt_amd.lora")
    WU = importlib.import_module("tests.test_weight_updates_gpu")
    p = case["p"]
    tr = _trainer(TR, p, 8, b_seed=8, lr=5e-3, lora_alpha=16)
    assert tr.lora_scale == 2.0
    for _ in range(3):
        tr.step(case["dbatch"], *case["args"])
    loss_lora = tr.step(case["dbatch"], *case["args"], update=False, backward=False).clone()
    path = tr.save_checkpoint(str(tmp_path))
    adapter = LORA.load_adapter(path)
    # merged weights within 1 bf16 ulp of float64 W + s B A (chain: r - 1 additions, s, the addition to W)
    model = SC.build_product_model(R.TINY, p, DEV, cls_name="LVMTraining")
    scase = WU.Case(R.TINY, C=2, G=2, hw=(16, 16), steps=2)
    smodel = SC.build_product_model(R.TINY, scase.p, DEV)
    first, s1 = scase.sample(smodel, True)                  # an engine is cached on the base weights
    LORA.merge_adapter(model, adapter)
    for i in range(R.TINY.num_hidden_layers):
        for mod in MODS:
            wn = f"llm.layers.{i}.self_attn.{mod}.weight"
            a, b = (adapter[1][TR.lora_key(i, mod, ab)].to(DEV, F64) for ab in "AB")
            w = p[wn].to(DEV, F64)
            ref, mag = w + 2.0 * (b @ a), w.abs() + 2.0 * (b.abs() @ a.abs())
            got = model.state_dict()[wn]
            _within(got, ref, _ulp(ref) + (16 + 2) * U32 * mag, f"merged {wn}")
            assert not torch.equal(got.cpu().float(), p[wn])
    # the merged model computes what the LoRA trainer computes, and what the oracle computes with W + s B A
    fo = TR.Stage1Trainer(model, forward_only=True)
    loss_merged = fo.step(case["dbatch"], *case["args"], update=False, backward=False)
    x1, x0, t, clean, x0i, ti = case["args"]
    pr, _ = _with_adapters(TR, p, {k: v for k, v in adapter[1].items()}, 2.0)
    with torch.no_grad():
        loss_ref, _ = R.stage1_loss(pr, R.TINY, list(x1.split(1)), list(x0.split(1)), t, list(clean.split(1)),
                                    list(x0i.split(1)), ti, case["batch"])
    print(f"MEASURE merge: merged vs LoRA trainer {rel_l2(loss_merged, loss_lora):.3e}, merged vs oracle "
          f"{rel_l2(loss_merged, loss_ref):.3e}, LoRA trainer vs oracle {rel_l2(loss_lora, loss_ref):.3e}")
    assert rel_l2(loss_merged, loss_lora) < SC.tol("loss")
    assert rel_l2(loss_merged, loss_ref) < SC.tol("loss") and rel_l2(loss_lora, loss_ref) < SC.tol("loss")
    # sampling with a cached engine follows the merge (weight generation bumped): equal, bit for bit, to a model built from
    # the merged state dict
    LORA.merge_adapter(smodel, adapter)
    again, s2 = scase.sample(smodel, True)
    fresh, _ = scase.sample(SC.build_product_model(R.TINY, WU.params_from(smodel.state_dict()), DEV), False)
    assert torch.equal(again, fresh) and not torch.equal(again, first)
    # merged_weights(): the current adapters inside, the base back bit for bit outside
    base = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    with tr.merged_weights() as mm:
        inside = {k: v.detach().clone() for k, v in mm.state_dict().items()}
    for k, v in model.state_dict().items():
        assert torch.equal(inside[k], v), k                      # the same merge as merge_adapter's
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, base[k]), k


# ---- 6. files ------------------------------------------------------------------------------------------------------------
def test_adapter_files_and_resume(TR, case, tmp_path):
    LORA = importlib.import_module("video-gpt_amd.lora")
    from safetensors.torch import load_file
    kw = dict(lr=2e-3, weight_decay=0.05, lora_alpha=4)
    a = _trainer(TR, case["p"], 4, b_seed=9, **kw)
    for _ in range(2):
        a.step(case["dbatch"], *case["args"])
    path = a.save_checkpoint(str(tmp_path))
    assert path.endswith("checkpoint-2")
    cfg = json.load(open(os.path.join(path, "adapter_config.json")))
    want = dict(peft_type="LORA", r=4, lora_alpha=4, target_modules=["qkv_proj", "o_proj"], init_lora_weights="gaussian",
                bias="none", fan_in_fan_out=False, use_rslora=False, use_dora=False)
    assert {k: cfg[k] for k in want} == want
    sd = load_file(os.path.join(path, "adapter_model.safetensors"))
    H = R.TINY.hidden_size
    keys = {f"base_model.model.llm.layers.{i}.self_attn.{m}.lora_{ab}.weight" for i in range(R.TINY.num_hidden_layers)
            for m in MODS for ab in "AB"}
    assert set(sd) == keys == set(a.lora)
    assert all(v.dtype == BF for v in sd.values())
    assert tuple(sd["base_model.model.llm.layers.0.self_attn.qkv_proj.lora_A.weight"].shape) == (4, H)
    assert tuple(sd["base_model.model.llm.layers.1.self_attn.o_proj.lora_B.weight"].shape) == (H, 4)
    assert not os.path.exists(os.path.join(path, "model.safetensors"))     # the base is frozen: nothing to write
    b = _trainer(TR, case["p"], 4, seed=99, lr=1e-5, weight_decay=0.5)     # other adapters, other hyper-parameters
    assert not torch.equal(a.lora_param, b.lora_param)
    assert b.auto_resume(str(tmp_path)) == 2 and b.step_count == 2 and b.lr == 2e-3 and b.wd == 0.05 and b.lora_scale == 1.0
    la = a.step(case["dbatch"], *case["args"])
    lb = b.step(case["dbatch"], *case["args"])
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for ta, tb in ((a.lora_param, b.lora_param), (a.lora_master, b.lora_master), (a.lora_m, b.lora_m), (a.lora_v, b.lora_v)):
        assert torch.equal(ta, tb)
    # a full-fine-tuning trainer does not resume an adapter checkpoint, nor a trainer of another rank
    with pytest.raises(TR.VgptError):
        TR.Stage1Trainer(SC.build_product_model(R.TINY, case["p"], DEV, cls_name="LVMTraining")).load_checkpoint(path)
    with pytest.raises(TR.VgptError, match="does not match"):
        _trainer(TR, case["p"], 8).load_checkpoint(path)
    # every configuration field the merge does not implement is refused
    for field, value in (("use_dora", True), ("use_rslora", True), ("bias", "all"), ("rank_pattern", {"qkv_proj": 2}),
                         ("alpha_pattern", {"o_proj": 3}), ("modules_to_save", ["final_layer"]),
                         ("target_modules", ["qkv_proj", "gate_up_proj"]), ("r", 65), ("peft_type", "IA3")):
        bad = tmp_path / f"bad-{field}"
        shutil.copytree(path, bad)
        c = dict(cfg); c[field] = value
        json.dump(c, open(bad / "adapter_config.json", "w"))
        with pytest.raises(TR.VgptError):
            LORA.load_adapter(str(bad))
    assert LORA.load_adapter(path)[0]["r"] == 4


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_constructor_refusals(TR, case, monkeypatch):
    model = SC.build_product_model(R.TINY, case["p"], DEV, cls_name="LVMTraining")
    with pytest.raises(TR.VgptError, match="lora_target_modules"):
        TR.Stage1Trainer(model, lora_rank=8, lora_target_modules=("qkv_proj", "gate_up_proj"))
    with pytest.raises(TR.VgptError, match="lora_rank"):
        TR.Stage1Trainer(model, lora_rank=65)
    with pytest.raises(TR.VgptError, match="lora_rank"):
        TR.Stage1Trainer(model, lora_rank=0)
    with pytest.raises(TR.VgptError, match="nothing to shard"):
        TR.Stage1Trainer(model, lora_rank=8, dp_sharding="optimizer")
    monkeypatch.setenv("VGPT_DP_SHARDING", "optimizer")             # the environment default is ignored in this mode
    assert TR.Stage1Trainer(model, lora_rank=8).dp_sharding == "none"


# ---- 8. data parallel: 2 ranks on one GPU over gloo (the harness of test_train_gpu) ---------------------------------------
def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    TRm = importlib.import_module("video-gpt_amd.train")
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(R.TINY)
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    data = [torch.randn(x1.shape, generator=torch.Generator("cpu").manual_seed(500 + r_)) for r_ in range(world)]
    tr = _trainer(TRm, p, 8, b_seed=10, lr=1e-3, max_grad_norm=1.0)
    # every rank's own gradient, without the exchange, then the reduced one (the sum; 1 / world is folded into the clip)
    tr.skip_allreduce = True
    single = []
    for r_ in range(world):
        tr.step(dbatch, data[r_], x0, t, clean, x0i, ti, update=False)
        single.append(tr.lora_bucket.clone())
    tr.skip_allreduce = False
    tr.step(dbatch, data[rank], x0, t, clean, x0i, ti, update=False)
    torch.cuda.synchronize()
    err = SC.rel_l2(tr.lora_bucket / world, sum(single) / world)
    for _ in range(2):
        tr.step(dbatch, data[rank], x0, t, clean, x0i, ti)
    torch.cuda.synchronize()
    q.put((rank, tr.lora_param.float().cpu().numpy(), tr.lora_m.cpu().numpy(), tr.lora_v.cpu().numpy(), float(tr.grad_norm),
           err, float(SC.rel_l2(single[0], single[1]))))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_two_ranks(TR):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda x: x[0])
    for p_ in procs:
        p_.join(timeout=120)
        assert p_.exitcode == 0
    (_, w0, m0, v0, n0, e0, d0), (_, w1, m1, v1, n1, e1, d1) = res
    assert d0 > 1e-2, "the ranks must see different data"
    assert e0 < 1e-6 and e1 < 1e-6, (e0, e1)          # all-reduced bucket / world == mean of the single-rank gradients (fp32 sums)
    assert n0 == n1 and n0 > 0
    assert np.array_equal(w0, w1) and np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert np.abs(m0).max() > 0
