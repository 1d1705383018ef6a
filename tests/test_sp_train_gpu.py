"""Ulysses sequence parallelism through the training step (train.Stage1Trainer(sequence_parallel=True)).

Ranks are spawned processes over gloo on the one GPU of the test box, as in tests/test_sp_engine_gpu.py (RCCL refuses two
ranks on one device; the exchanges go through host memory).  In every worker the P = 1 trainer runs FIRST, before any
process group exists (world 1: no collective at all), then the group is initialised and the sharded trainer runs on the
same case in the same process.

What is exact and what is not.  The rows of a GEMM do not depend on M, every head's attention (forward and backward) is
one rank's over all rows with the same kernels, and the heads behind the gathered final norm run replicated: the loss
vector and the share's rows of d(sequence) are the P = 1 run's BITS.  A weight gradient is a sum over rows: a rank's
partial over its share, rounded to bf16, then added to the other ranks' -- three bf16 roundings instead of one, hence the
norm bound of test_stage1_gradients_*.  The small fp32 gradients are summed with atomics (tests/test_train_gpu.py)."""
import dataclasses
import hashlib
import importlib
import math
import random
import socket
import traceback

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import glue_cases as GC
from tests import smoke_case as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
CFG = R.TINY
SEED = 1000                 # the loss function's RNG seed of SP rank r is SEED + r
EPS_BF16 = 2.0 ** -9        # half an ulp of bf16 relative to the value: one rounding to nearest


# ---- processes ------------------------------------------------------------------------------------------------------

def _spawn(target, world, timeout=600):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    try:
        res = dict(q.get(timeout=timeout) for _ in procs)
    finally:
        for p_ in procs:
            p_.join(timeout=60)
            if p_.is_alive():
                p_.kill()
    for r in range(world):
        assert "error" not in res[r], f"rank {r} failed:\n{res[r]['error']}"
    for p_ in procs:
        assert p_.exitcode == 0
    return [res[r] for r in range(world)]


def _init(rank, world, port):
    import os
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


# ---- cases ----------------------------------------------------------------------------------------------------------

def _dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _stage1_case():
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(CFG)
    return p, batch, (x1, x0, t, clean, x0i, ti)


def _stage2_case():
    """The frame-block layout of tests/test_train_gpu.py::test_stage2_frame_block_layout_gradients: noisy clips of 2, 1
    and 2 frames with clean groups between them, one t per frame block."""
    P = importlib.import_module("video-gpt_amd.processor")
    p = {k: v.to(BF).float() for k, v in R.make_params(CFG, 4).items()}
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


def _np(t):
    return t.detach().float().cpu().numpy()          # bf16 -> fp32 is exact: equal arrays are equal bits


def _digest(model):
    h = hashlib.sha1()
    for k, v in model.state_dict().items():
        h.update(k.encode()); h.update(v.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def _trainer(p, cls="LVMTraining", **kw):
    TR = importlib.import_module("video-gpt_amd.train")
    return TR.Stage1Trainer(SC.build_product_model(CFG, p, DEV, cls_name=cls), **kw)


def _bucket_sumsq(tr):
    """Sum of squares of what this rank holds of the exchanged buckets (its shard when the optimizer is sharded)."""
    return sum(float(tr._shard(b).double().pow(2).sum()) for b in tr.layer_buckets + [tr.small_bucket])


def _loss_fn_call(tr, p, batch, x1, clean, seed):
    LS = importlib.import_module("video-gpt_amd.loss")
    kw = {k: (batch[k].to(DEV) if torch.is_tensor(batch[k]) else batch[k]) for k in GC.BATCH_KEYS}
    kw["input_img_latents"] = list(clean.split(1))
    torch.manual_seed(seed); random.seed(seed)       # CPU latents -> CPU draws; frame blocks -> python's RNG for t
    fbs = {b: [len(v)] for b, v in batch["denoise_image_sizes"].items()}
    return LS.training_losses_x1_noise_input(tr, list(x1.split(1)), dict(kw), device=DEV, frame_blocks=fbs)["loss"]


ACCUM_KW = dict(lr=1e-3, weight_decay=0.1, max_grad_norm=1.0, gradient_accumulation_steps=2, use_ema=True,
                overlap_optimizer=True)


def _accum_cycle(tr, db, args):
    """One accumulation cycle of two micro-steps on the same clip; returns grad_norm (the norm of the SUM over both)."""
    for _ in range(2):
        tr.step(db, *args)
    tr.finish_optimizer()
    torch.cuda.synchronize()
    return float(tr.grad_norm)


def _two_steps(tr, db, args):
    norms, sumsq = [], []
    for _ in range(2):
        tr.step(db, *args)
        tr.finish_optimizer()
        torch.cuda.synchronize()
        norms.append(float(tr.grad_norm)); sumsq.append(_bucket_sumsq(tr))
    return norms, sumsq


# ---- two ranks ------------------------------------------------------------------------------------------------------

def _two_rank_worker(rank, world, port, q):
    res = {}
    try:
        importlib.import_module("video-gpt_amd")
        TR = importlib.import_module("video-gpt_amd.train")
        E = importlib.import_module("video-gpt_amd.engine")
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
        p, batch, args = _stage1_case()
        db = _dev(batch)
        p2, batch2, args2 = _stage2_case()
        db2 = _dev(batch2)
        # ================= P = 1: no process group exists yet =================
        tr1 = _trainer(p, lr=1e-3, weight_decay=0.1)
        loss1 = tr1.step(db, *args, update=False).clone()
        torch.cuda.synchronize()
        dh1 = tr1._ws["dh"].clone()
        g1 = {k: v.clone() for k, v in tr1.grads.items()}
        small1 = tr1.small_bucket.clone()
        big = [k for names in tr1.layer_names for k in names]
        res["base_norms"], _ = _two_steps(_trainer(p, lr=1e-3, weight_decay=0.1, max_grad_norm=1.0), db, args)
        res["base_accum_norm"] = _accum_cycle(_trainer(p, **ACCUM_KW), db, args)
        res["base_loss2"] = _np(_trainer(p2, "LVMTraining_CP").step(db2, *args2, update=False))
        res["base_lossfn"] = _np(_loss_fn_call(_trainer(p), p, batch, args[0], args[3], SEED))       # seeded as SP rank 0
        try:
            _trainer(p, sequence_parallel=True)
            res["refuse_nogroup"] = None
        except VgptError as e_:
            res["refuse_nogroup"] = str(e_)
        # ================= the group =================
        dist = _init(rank, world, port)
        SPM.initialize_sequence_parallel_state(world)
        # ---- 1. stage-1 layout, stand-alone backward ----
        trs = _trainer(p, lr=1e-3, weight_decay=0.1, sequence_parallel=True)
        res["sharded"] = trs._sp is not None and trs._sp["P"] == world
        loss = trs.step(db, *args, update=False).clone()
        torch.cuda.synchronize()
        M = trs._ws["seq_all"].shape[0]
        shares, _ = E.sp_shares(M, world)
        r0, r1 = shares[rank]
        res["M"], res["shares"], res["x_rows"] = M, shares, [int(v) for v in trs._prepare(db)["x_rows"].tolist()]
        res["loss_equal"] = bool(torch.equal(loss, loss1))
        res["loss"] = _np(loss)
        res["dh_rows"] = int(trs._ws["dh"].shape[0])
        res["dh_equal"] = bool(torch.equal(trs._ws["dh"], dh1[r0:r1]))
        res["dh_norm"] = float(dh1[r0:r1].float().norm())
        gsp = {k: v.clone() for k, v in trs.grads.items()}
        small_sp = trs.small_bucket.clone()
        trs.skip_allreduce = True                     # gradient collectives only: the exchanges of the forward stay
        loss_b = trs.step(db, *args, update=False)
        torch.cuda.synchronize()
        trs.skip_allreduce = False
        res["loss_equal_partial_run"] = bool(torch.equal(loss_b, loss1))
        nrm = lambda t_: float(t_.double().norm())
        res["matrices"] = {k: (nrm(gsp[k].double() - g1[k].double()), nrm(gsp[k]), nrm(g1[k]), nrm(trs.grads[k])) for k in big}
        res["small_rel_l2"] = SC.rel_l2(small_sp, small1)
        res["small_partial_norm"], res["small_norm"] = nrm(trs.small_bucket), nrm(small_sp)
        res["replicated_partial"] = {k: nrm(v) for k, v in trs.grads.items() if k.startswith(TR.SP_REPLICATED)}
        if rank == 0:
            res["grads"] = {k: _np(v) for k, v in gsp.items()}
        # ---- 2. stage-2 frame-block layout, LVMTraining_CP, with and without checkpointing ----
        out = {}
        for ck in (False, True):
            tr = _trainer(p2, "LVMTraining_CP", sequence_parallel=True, gradient_checkpointing=ck)
            l2 = tr.step(db2, *args2, update=False).clone()
            torch.cuda.synchronize()
            out[ck] = (l2, {k: tr.grads[k].clone() for k in big}, tuple(tr._ws["qkv"].shape), tuple(tr._ws["qkv_heads"].shape),
                       tuple(tr._ws["n1"].shape))
        M2 = out[False][3][1]
        res["s2_loss_equal"] = bool(np.array_equal(_np(out[False][0]), res["base_loss2"]))
        res["s2_ck_loss_equal"] = bool(torch.equal(out[False][0], out[True][0]))
        res["s2_ck_grads_differ"] = [k for k in big if not torch.equal(out[False][1][k], out[True][1][k])]
        res["s2_shapes"] = {ck: out[ck][2:] for ck in (False, True)}
        res["s2_share"] = E.sp_shares(M2, world)[0][rank]
        # ---- 3. two optimizer steps, replicated and sharded optimizer state ----
        for mode in ("none", "optimizer"):
            tr = _trainer(p, lr=1e-3, weight_decay=0.1, max_grad_norm=1.0, sequence_parallel=True, dp_sharding=mode)
            norms, sumsq = _two_steps(tr, db, args)
            res[f"opt_{mode}"] = dict(norms=norms, sumsq=sumsq, digest=_digest(tr.model), sharded=tr._sharded)
        # ---- 3b. what only sees buckets composes: accumulation over two micro-steps, EMA, the overlapped optimizer ----
        tr = _trainer(p, sequence_parallel=True, **ACCUM_KW)
        res["accum"] = dict(norm=_accum_cycle(tr, db, args), digest=_digest(tr.model), steps=tr.step_count,
                            ema=hashlib.sha1(_np(tr.ema_small).tobytes()).hexdigest())
        # ---- 5. the loss function: every rank seeds its own RNGs, the group trains on SP rank 0's draws ----
        res["lossfn"] = _np(_loss_fn_call(_trainer(p, sequence_parallel=True), p, batch, args[0], args[3], SEED + rank))
        # ---- 6. refusals ----
        for name, make in (("lora", lambda: _trainer(p, lora_rank=4, sequence_parallel=True)),
                           ("heads", lambda: TR.Stage1Trainer(_three_head_model(), sequence_parallel=True))):
            try:
                make()
                res[f"refuse_{name}"] = None
            except VgptError as e_:
                res[f"refuse_{name}"] = str(e_)
        x1, x0, t, clean, x0i, ti = args
        try:
            trs.step(db, x1, x0, t + 0.125 * rank, clean, x0i, ti, update=False)
            res["refuse_t"] = None
        except VgptError as e_:
            res["refuse_t"] = str(e_)
        # nobody was left waiting: the ranks are still in step
        res["after_refusal_loss_equal"] = bool(torch.equal(trs.step(db, *args, update=False), loss1))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


def _three_head_model():
    cfg3 = dataclasses.replace(CFG, hidden_size=288, num_attention_heads=3, num_key_value_heads=3)
    return SC.build_product_model(cfg3, {k: v.to(BF).float() for k, v in R.make_params(cfg3, 0).items()}, DEV,
                                  cls_name="LVMTraining")


@pytest.fixture(scope="module")
def two():
    return _spawn(_two_rank_worker, 2)


@pytest.fixture(scope="module")
def oracle():
    """Autograd on the fp32 oracle, as tests/test_train_gpu.py::test_stage1_loss_and_gradients_match_autograd."""
    p, batch, (x1, x0, t, clean, x0i, ti) = _stage1_case()
    pr = {k: v.clone().requires_grad_(k != "pos_embed") for k, v in p.items()}
    loss_ref, _ = R.stage1_loss(pr, CFG, list(x1.split(1)), list(x0.split(1)), t, list(clean.split(1)),
                                list(x0i.split(1)), ti, batch)
    loss_ref.mean().backward()
    return loss_ref.detach(), {k: v.grad for k, v in pr.items() if k != "pos_embed"}


def test_stage1_rows_are_shared_raggedly_across_frame_seams(two):
    for r in range(2):
        t = two[r]
        assert t["sharded"]
        (a0, b0), (a1, b1) = t["shares"]
        assert a0 == 0 and b0 == a1 and b1 == t["M"] and b0 - a0 != b1 - a1           # ragged
        assert t["dh_rows"] == t["shares"][r][1] - t["shares"][r][0]
        # the cut falls inside a frame's rows (16 tokens per frame), not on a seam
        assert any(x < b0 < x + 16 for x in t["x_rows"]), (b0, t["x_rows"])


def test_stage1_loss_and_sequence_gradient_are_the_p1_bits(two):
    for r in range(2):
        assert two[r]["loss_equal"] and two[r]["loss_equal_partial_run"]
        assert two[r]["dh_equal"] and two[r]["dh_norm"] > 0
    assert np.array_equal(two[0]["loss"], two[1]["loss"])


def test_stage1_decoder_gradients_within_three_bf16_roundings(two):
    """|g_sp - g_1| <= 1.25 * 2^-9 * (|g_sp| + |g_1| + sum_r |p_r|): g_1 is one bf16 rounding of the exact sum, every
    partial p_r one rounding of its share's sum, g_sp one rounding of their sum (triangle inequality over the three);
    1.25 covers the fp32 accumulation-order difference of products over at most 128 rows."""
    worst = 0.0
    for r in range(2):
        for k, (diff, n_sp, n_1, _) in two[r]["matrices"].items():
            partials = sum(two[q_]["matrices"][k][3] for q_ in range(2))
            bound = 1.25 * EPS_BF16 * (n_sp + n_1 + partials)
            worst = max(worst, diff / bound)
            print(f"rank {r} {k}: |g_sp - g_1| {diff:.4e} bound {bound:.4e} (|g_sp| {n_sp:.4e} |g_1| {n_1:.4e} partials {partials:.4e})")
            assert n_1 > 0 and diff <= bound, (r, k, diff, bound)
            # really partial sums: neither rank alone holds the gradient
            assert all(two[q_]["matrices"][k][3] > 0 for q_ in range(2))
    print(f"worst ratio to the bound {worst:.3f}")
    for k in two[0]["matrices"]:
        assert two[0]["matrices"][k][:3] == two[1]["matrices"][k][:3]      # the exchanged gradient is the same on both ranks


def test_stage1_small_gradients_and_replicated_heads(two):
    for r in range(2):
        print(f"rank {r}: small bucket rel-L2 to P = 1 {two[r]['small_rel_l2']:.3e}")
        assert two[r]["small_rel_l2"] < 1e-5
        assert two[r]["small_partial_norm"] < two[r]["small_norm"]
    # gradients computed on replicated rows enter the sum once: SP rank 0 holds them, SP rank 1 holds zeros
    assert two[0]["replicated_partial"] and all(v > 0 for k, v in two[0]["replicated_partial"].items()
                                                  if not k.startswith("input_final_layer."))
    assert all(v == 0 for v in two[1]["replicated_partial"].values())


def test_stage1_sharded_gradients_match_autograd(two, oracle):
    loss_ref, grads_ref = oracle
    e_loss = SC.rel_l2(torch.from_numpy(two[0]["loss"]), loss_ref)
    assert e_loss < SC.tol("loss"), e_loss
    bad, worst = {}, 0.0
    for name, ref in grads_ref.items():
        err = SC.rel_l2(torch.from_numpy(two[0]["grads"][name]), ref)
        worst = max(worst, err)
        if not err < SC.tol("param_grads"):
            bad[name] = err
    print(f"sharded stage-1 tiny: loss error {e_loss:.3e}, worst gradient error {worst:.3e} (tol {SC.tol('param_grads'):.3e})")
    assert not bad, bad


def test_stage2_frame_block_layout_and_checkpointing(two):
    for r in range(2):
        t = two[r]
        assert t["s2_loss_equal"]
        assert t["s2_ck_loss_equal"] and t["s2_ck_grads_differ"] == []
        a, b = t["s2_share"]
        W, Wl = 3 * CFG.num_attention_heads * CFG.head_dim, 3 * (CFG.num_attention_heads // 2) * CFG.head_dim
        for ck in (False, True):
            qkv, heads, n1 = t["s2_shapes"][ck]
            ns = 1 if ck else CFG.num_hidden_layers
            assert qkv == (b - a, W)                                     # the share's rows only
            assert heads == (ns, heads[1], Wl) and heads[1] > b - a      # all rows, this rank's heads
            assert n1 == (ns, b - a, CFG.hidden_size)


@pytest.mark.parametrize("mode", ["none", "optimizer"])
def test_two_optimizer_steps(two, mode):
    a, b = two[0][f"opt_{mode}"], two[1][f"opt_{mode}"]
    assert a["sharded"] == b["sharded"] == (mode == "optimizer")
    assert a["digest"] == b["digest"]                                    # parameters bit-identical on both ranks
    for i in range(2):
        total = a["sumsq"][i] + b["sumsq"][i] if mode == "optimizer" else a["sumsq"][i]
        for t in (a, b):
            assert abs(t["norms"][i] - math.sqrt(total)) <= 1e-5 * math.sqrt(total), (i, t["norms"][i], math.sqrt(total))
            base = two[0]["base_norms"][i]
            print(f"{mode} step {i}: grad_norm {t['norms'][i]:.6f}, P = 1 {base:.6f}")
            assert abs(t["norms"][i] - base) <= 2.0 ** -7 * base, (i, t["norms"][i], base)      # not twice it


def test_accumulation_ema_and_overlapped_optimizer_compose(two):
    """The replicated heads' gradients are zeroed on SP rank 1 BEFORE the accumulator reads the small bucket: counted once per
    micro-step, the accumulated norm is the P = 1 cycle's (twice one micro-batch's), not more."""
    a, b = two[0]["accum"], two[1]["accum"]
    assert a["steps"] == b["steps"] == 1
    assert a["digest"] == b["digest"] and a["ema"] == b["ema"]
    for r in range(2):
        base = two[r]["base_accum_norm"]
        print(f"rank {r}: accumulated grad_norm {two[r]['accum']['norm']:.6f}, P = 1 {base:.6f}")
        assert abs(two[r]["accum"]["norm"] - base) <= 2.0 ** -7 * base
        assert abs(base - 2 * two[r]["base_norms"][0]) <= 2.0 ** -7 * base


def test_loss_function_draws_come_from_sp_rank_0(two):
    assert np.array_equal(two[0]["lossfn"], two[1]["lossfn"])
    for r in range(2):
        assert np.array_equal(two[r]["lossfn"], two[r]["base_lossfn"])


def test_refusals(two):
    for r in range(2):
        t = two[r]
        assert t["refuse_nogroup"] is not None and "needs a group" in t["refuse_nogroup"]
        assert t["refuse_lora"] is not None and "lora_rank with sequence_parallel" in t["refuse_lora"]
        assert t["refuse_heads"] is not None and "divisible by 2" in t["refuse_heads"]
        assert t["refuse_t"] is not None and "different inputs" in t["refuse_t"]
        assert t["after_refusal_loss_equal"]


# ---- four ranks: 2 replicas x 2 SP ----------------------------------------------------------------------------------

def _four_rank_worker(rank, world, port, q):
    res = {}
    try:
        importlib.import_module("video-gpt_amd")
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        torch.set_num_threads(4)
        p, batch, args = _stage1_case()
        db = _dev(batch)
        tr1 = _trainer(p, lr=1e-3, weight_decay=0.1, max_grad_norm=1.0)
        loss1 = tr1.step(db, *args).clone()
        tr1.finish_optimizer()
        torch.cuda.synchronize()
        res["base_norm"] = float(tr1.grad_norm)
        dist = _init(rank, world, port)
        SPM.initialize_sequence_parallel_state(2)            # groups {0, 1} and {2, 3}: two replicas of two ranks
        tr = _trainer(p, lr=1e-3, weight_decay=0.1, max_grad_norm=1.0, sequence_parallel=True)
        res["P"], res["sp_rank"] = tr._sp["P"], tr._sp["r"]
        loss = tr.step(db, *args)                            # the same clip in both replicas
        tr.finish_optimizer()
        torch.cuda.synchronize()
        res["loss_equal"] = bool(torch.equal(loss, loss1))
        res["norm"] = float(tr.grad_norm)
        res["digest"] = _digest(tr.model)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


def test_four_ranks_two_replicas_of_two():
    four = _spawn(_four_rank_worker, 4)
    for r in range(4):
        t = four[r]
        assert t["P"] == 2 and t["sp_rank"] == r % 2
        assert t["loss_equal"]
        # grad_norm is the norm of the SUM over the replicas: twice the P = 1 norm for the same clip in both
        print(f"rank {r}: grad_norm {t['norm']:.6f}, 2 x P = 1 {2 * t['base_norm']:.6f}")
        assert abs(t["norm"] - 2 * t["base_norm"]) <= 2.0 ** -7 * 2 * t["base_norm"]
        assert t["digest"] == four[0]["digest"]
