"""Stage1Trainer(deterministic=True) on the GPU: with the three atomic reductions of the step replaced by
their fixed-order twins a training run is a pure function of its inputs, so everything below is compared with
torch.equal -- the per-frame loss, every gradient, the fp32 master weights, both Adam moments (the EMA where there is
one) and the bf16 parameters -- where the tests of the default path (tests/test_train_gpu.py) can only bound the small
fp32 gradients.  Tiny stage-1 configuration and batch (tests/glue_cases.py) and the stage-2 frame-block batch."""
import importlib
import socket

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import glue_cases as GC
from tests import smoke_case as SC
from tests.test_ops_gpu import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
KW = dict(lr=1e-3, weight_decay=0.1, max_grad_norm=0.5)


@pytest.fixture(scope="module")
def TR():
    return importlib.import_module("video-gpt_amd.train")


def _on_device(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


@pytest.fixture(scope="module")
def stage1():
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(R.TINY)
    return dict(p=p, cls="LVMTraining", batch=_on_device(batch), args=(x1, x0, t, clean, x0i, ti))


@pytest.fixture(scope="module")
def stage2():
    """The frame-block layout of test_stage2_frame_block_layout_gradients: noisy clips of several frames + clean groups."""
    P = importlib.import_module("video-gpt_amd.processor")
    p = {k: v.to(BF).float() for k, v in R.make_params(R.TINY, 4).items()}
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
    mk = lambda m: torch.randn(m, 4, 8, 8, generator=gen)   # noqa: E731
    x1, x0, clean, x0i = mk(nd), mk(nd), mk(nc), mk(nc)
    tb = torch.rand(len(fbs), generator=gen)
    t = torch.cat([tb[k].repeat(f) for k, f in enumerate(fbs)])
    ti = 0.9 + 0.1 * torch.rand(nc, generator=gen)
    return dict(p=p, cls="LVMTraining_CP", batch=_on_device(batch), args=(x1, x0, t, clean, x0i, ti))


def _trainer(TR, case, checkpointing=False, **kw):
    model = SC.build_product_model(R.TINY, case["p"], DEV, cls_name=case["cls"])
    if checkpointing:
        model.llm.gradient_checkpointing_enable()
    for k, v in KW.items():
        kw.setdefault(k, v)
    kw.setdefault("deterministic", True)
    tr = TR.Stage1Trainer(model, **kw)
    assert tr.deterministic == kw["deterministic"]
    return tr


def _step(tr, case, i=0, **kw):
    """Step i of a chain: the case's batch with the target latents scaled, so that no two steps see the same data."""
    x1, *rest = case["args"]
    return tr.step(case["batch"], x1 * (1 + 0.1 * i), *rest, **kw)


def _snapshot(tr, loss):
    """Everything a step produces: loss, gradients, parameters, fp32 masters, moments, EMA."""
    tr.finish_optimizer()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone()}
    if getattr(tr, "lora", None) is not None and tr.lora:
        out["grad:lora"] = tr.lora_bucket.clone()
        for k in ("lora_param", "lora_master", "lora_m", "lora_v"):
            out[k] = getattr(tr, k).clone()
    else:
        out.update({f"grad:{k}": v.clone() for k, v in tr.grads.items()})
        for t_, key, _ in tr._optimizer_tensors() + tr._ema_tensors():
            out[f"state:{key}"] = t_.detach().clone()
    out.update({f"param:{k}": v.detach().clone() for k, v in tr.model.state_dict().items()})
    return out


def _assert_equal(a, b, what):
    assert a.keys() == b.keys(), what
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: differ in {bad[:8]} ({len(bad)} of {len(a)})"


def _run(TR, case, steps=4, **kw):
    tr = _trainer(TR, case, **kw)
    return [_snapshot(tr, _step(tr, case, i)) for i in range(steps)], tr


@pytest.mark.parametrize("which", ["stage1", "stage2"])
def test_two_runs_are_the_same_run(TR, request, which):
    case = request.getfixturevalue(which)
    a, tr = _run(TR, case)
    b, _ = _run(TR, case)
    assert any(k.startswith("state:v.") for k in a[0]) and "grad:llm.embed_tokens.weight" in a[0]
    assert float(a[0]["grad:llm.embed_tokens.weight"].abs().max()) > 0 and float(a[0]["grad:llm.norm.weight"].abs().max()) > 0
    assert not torch.equal(a[0]["state:master_small"], a[3]["state:master_small"])     # the chain moves
    for i, (sa, sb) in enumerate(zip(a, b)):
        _assert_equal(sa, sb, f"{which} step {i}")


def test_gradient_checkpointing_gives_every_gradient_bit_for_bit(TR, stage1):
    out = {}
    for ck in (False, True):
        tr = _trainer(TR, stage1, checkpointing=ck)
        assert tr.gradient_checkpointing == ck
        out[ck] = _snapshot(tr, _step(tr, stage1, update=False))
    for k in ("llm.norm.weight", "llm.embed_tokens.weight", "llm.layers.0.input_layernorm.weight",
              "llm.layers.1.post_attention_layernorm.weight", "final_layer.adaLN_modulation.1.weight",
              "final_layer.adaLN_modulation.1.bias"):
        assert f"grad:{k}" in out[True], k          # the ones the default path can only bound
    _assert_equal(out[False], out[True], "checkpointing on / off")


def test_optimizer_overlap_is_the_same_run(TR, stage1):
    a, _ = _run(TR, stage1, overlap_optimizer=False)
    b, tr = _run(TR, stage1, overlap_optimizer=True)
    assert tr.overlap_optimizer
    for i, (sa, sb) in enumerate(zip(a, b)):
        _assert_equal(sa, sb, f"overlap step {i}")


def test_resume_continues_the_same_run(TR, stage1, tmp_path):
    whole, _ = _run(TR, stage1)
    a = _trainer(TR, stage1)
    for i in range(2):
        _step(a, stage1, i)
    path = a.save_checkpoint(str(tmp_path))
    b = _trainer(TR, stage1)
    assert b.load_checkpoint(path) == 2
    for i in (2, 3):
        _assert_equal(_snapshot(b, _step(b, stage1, i)), whole[i], f"resumed step {i}")


def test_accumulation_and_ema(TR, stage1):
    runs = [_run(TR, stage1, gradient_accumulation_steps=2, use_ema=True, ema_decay=0.5) for _ in range(2)]
    (a, tr), (b, _) = runs
    assert tr.step_count == 2 and "state:ema_small" in a[0]
    assert not torch.equal(a[3]["state:ema_small"], a[3]["state:master_small"])
    for i, (sa, sb) in enumerate(zip(a, b)):
        _assert_equal(sa, sb, f"accumulation + EMA micro-step {i}")


def test_lora(TR, stage1):
    def run():
        torch.manual_seed(11)
        tr = _trainer(TR, stage1, lora_rank=4)
        gen = torch.Generator("cpu").manual_seed(48)
        for k, v in tr.lora.items():          # lora_B away from its zero init, so that dA is not trivially zero
            if ".lora_B." in k:
                v.copy_((torch.randn(v.shape, generator=gen) * 0.02).to(BF))
        tr.lora_master.copy_(tr.lora_param)
        return [_snapshot(tr, _step(tr, stage1, i)) for i in range(4)]
    a, b = run(), run()
    assert "grad:lora" in a[0] and float(a[0]["grad:lora"].abs().max()) > 0
    assert not torch.equal(a[0]["lora_param"], a[3]["lora_param"])
    for i, (sa, sb) in enumerate(zip(a, b)):
        _assert_equal(sa, sb, f"LoRA step {i}")


def test_lora_optimizer_overlap_is_the_same_run(TR, stage1):
    """The adapter update on the optimizer's stream against the inline one, to the bit (tests/test_lora_gpu.py bounds it)."""
    def run(ov):
        torch.manual_seed(11)
        tr = _trainer(TR, stage1, lora_rank=4, overlap_optimizer=ov)
        assert tr.overlap_optimizer == ov
        gen = torch.Generator("cpu").manual_seed(48)
        for k, v in tr.lora.items():          # lora_B away from its zero init, as in test_lora
            if ".lora_B." in k:
                v.copy_((torch.randn(v.shape, generator=gen) * 0.02).to(BF))
        tr.lora_master.copy_(tr.lora_param)
        return [_snapshot(tr, _step(tr, stage1, i)) for i in range(3)]
    a, b = run(False), run(True)
    assert float(a[0]["grad:lora"].abs().max()) > 0 and not torch.equal(a[0]["lora_param"], a[2]["lora_param"])
    for i, (sa, sb) in enumerate(zip(a, b)):
        _assert_equal(sa, sb, f"LoRA overlap step {i}")


def test_flag_on_against_flag_off(TR, stage1):
    out = {}
    for det in (False, True):
        tr = _trainer(TR, stage1, deterministic=det)
        out[det] = _snapshot(tr, _step(tr, stage1, update=False))
    assert torch.equal(out[True]["loss"], out[False]["loss"])          # the forward pass is untouched
    big = {k for names in tr.layer_names for k in names}
    for k, v in out[False].items():
        if not k.startswith("grad:"):
            continue
        if k[5:] in big:        # decoder matrices: GEMMs fed by dx chains that are the same bits in both modes
            assert torch.equal(out[True][k], v), k
        else:                   # the same fp32 sums in another order: the bound the default path's tests use for that
            assert rel_l2(out[True][k], v) < 1e-5, k


def test_forward_only_trainers_take_the_flag(TR, stage1):
    model = SC.build_product_model(R.TINY, stage1["p"], DEV, cls_name="LVMTraining")
    a = TR.Stage1Trainer(model, forward_only=True, deterministic=True)
    b = TR.Stage1Trainer(model, forward_only=True)
    assert a.deterministic and not b.deterministic
    assert torch.equal(_step(a, stage1, update=False), _step(b, stage1, update=False))
    assert TR.Stage1Trainer.for_evaluation(model, deterministic=True).deterministic


# ---- two data-parallel ranks on the one GPU, gloo transport: the pattern of test_data_parallel_two_ranks_stay_in_sync ----
def _dp_worker(rank, world, port, q):
    import os
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(R.TINY)
    x1 = torch.randn(x1.shape, generator=torch.Generator("cpu").manual_seed(500 + rank))     # different data on every rank
    model = SC.build_product_model(R.TINY, p, DEV, cls_name="LVMTraining")
    TR = importlib.import_module("video-gpt_amd.train")
    tr = TR.Stage1Trainer(model, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0, deterministic=True)
    dbatch = _on_device(batch)
    for _ in range(2):
        tr.step(dbatch, x1, x0, t, clean, x0i, ti)
    tr.finish_optimizer()
    torch.cuda.synchronize()
    sd = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    q.put((rank, sd, float(tr.grad_norm)))       # numpy: pickled by value
    dist.barrier()
    dist.destroy_process_group()


def _sharded_overlap_worker(rank, world, port, q):
    """dp_sharding="optimizer" with overlap_optimizer off and on, three steps each: what differs between the two runs."""
    import os
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(R.TINY)
    x1 = torch.randn(x1.shape, generator=torch.Generator("cpu").manual_seed(500 + rank))     # different data on every rank
    case = dict(p=p, cls="LVMTraining", batch=_on_device(batch), args=(x1, x0, t, clean, x0i, ti))
    TR = importlib.import_module("video-gpt_amd.train")
    runs = {}
    for ov in (False, True):
        runs[ov], tr = _run(TR, case, steps=3, dp_sharding="optimizer", overlap_optimizer=ov)
        assert tr._sharded and tr.overlap_optimizer == ov
    moved = not torch.equal(runs[False][0]["state:master_small"], runs[False][2]["state:master_small"])
    bad = [f"step {i}: {k}" for i, (sa, sb) in enumerate(zip(runs[False], runs[True]))
           for k in sa.keys() | sb.keys() if k not in sa or k not in sb or not torch.equal(sa[k], sb[k])]
    q.put((rank, bad, moved))
    dist.barrier()
    dist.destroy_process_group()


def _dp_job(worker=_dp_worker):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, 2, port, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    try:
        res = sorted((q.get(timeout=300) for _ in procs), key=lambda x: x[0])
        for p_ in procs:
            p_.join(timeout=120)
            assert p_.exitcode == 0, p_.exitcode       # an abort or a hang ends the test here: no second job is started
    finally:
        for p_ in procs:
            if p_.is_alive():
                p_.kill()
    return res


def test_two_data_parallel_ranks_twice():
    first = _dp_job()
    second = _dp_job()
    (_, sd0, n0), (_, sd1, n1) = first
    (_, sd0b, n0b), _ = second
    assert n0 == n1 == n0b and n0 > 0
    assert sd0.keys() == sd1.keys() == sd0b.keys()
    for k in sd0:
        assert np.array_equal(sd0[k], sd1[k]), f"{k}: rank 0 and rank 1 differ"
        assert np.array_equal(sd0[k], sd0b[k]), f"{k}: the two jobs differ"


def test_sharded_optimizer_overlap_is_the_same_run():
    for rank, bad, moved in _dp_job(_sharded_overlap_worker):
        assert moved, f"rank {rank}: the chain does not move"
        assert not bad, f"rank {rank}: overlap on / off differ in {bad[:8]} ({len(bad)})"
