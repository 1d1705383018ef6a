"""Stage1Trainer(skip_bad_steps=True, skip_grad_norm_above=...) on the GPU, on the tiny stage-1 configuration and batch of
tests/test_accum_ema_gpu.py (glue_cases.stage1_case), whose helpers this file shares.

Every comparison is torch.equal on the raw bits.  Two separate runs agree bit for bit only when the small fp32 gradients
(summed with fp32 atomics) are pinned or the trainer is deterministic (tests/test_accum_ema_gpu.py): where
two runs see the same sequence of batches the second replays the first's small gradients (`_pin_small`); where one of them
sees an extra, bad batch both are built with deterministic=True instead, so nothing has to be replayed around the skipped
step.  LoRA runs are bit-reproducible as they are (vgpt_lora_grad adds in a fixed order).

A bad batch is the good batch with one NaN, or one +inf, written into one element of x1; a spike is x1 * 1e4 under a
threshold of ten times the largest good norm read off a first run."""
import contextlib
import importlib
import json
import os
import socket
import traceback

import pytest
import torch

from tests.test_accum_ema_gpu import _assert_same_state, _case, _micro, _pin_small, _state, _trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
# trainer_state.json of a full trainer as it was before the guard existed, key for key and in this order
PARENT_RECORD_KEYS = ["step_count", "global_step", "lr", "weight_decay", "betas", "eps", "lr_scheduler", "lr_warmup_steps",
                      "lr_num_training_steps", "lr_num_cycles", "lr_power", "gradient_accumulation_steps", "use_ema",
                      "ema_decay", "small_names"]


@pytest.fixture(scope="module")
def TR():
    return importlib.import_module("video-gpt_amd.train")


@pytest.fixture(scope="module")
def case():
    p, dbatch, args = _case()
    return dict(p=p, dbatch=dbatch, args=args)


def _bad(case, i, kind):
    """Micro-batch i made bad: one NaN / one +inf in one element of x1, or x1 * 1e4."""
    db, x1, *rest = _micro(case, i)
    x1 = x1.clone()
    if kind == "spike":
        x1 = x1 * 1e4
    else:
        x1.view(-1)[x1.numel() // 3] = float("nan") if kind == "nan" else float("inf")
    return (db, x1, *rest)


def _full_state(tr):
    out = _state(tr)
    if tr.lora_rank is not None:
        out["lora_param"] = tr.lora_param.detach().clone()
    return out


def _finite(state):
    return all(bool(torch.isfinite(v.float()).all()) for v in state.values())


# ---- 1. guard on, good data: the unguarded run, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(gradient_accumulation_steps=2, use_ema=True, ema_decay=0.5), dict(lora_rank=4),
                                dict(overlap_optimizer=True), dict(deterministic=True)],
                         ids=["plain", "accum2-ema", "lora4", "overlap-optimizer", "deterministic"])
def test_guard_on_good_data_equals_guard_off(TR, case, kw):
    A = kw.get("gradient_accumulation_steps", 1)
    pinned = "lora_rank" not in kw and not kw.get("deterministic")
    tape, runs = [], []
    for guard in (False, True):
        torch.manual_seed(11)                       # the adapters' gaussian init
        tr = _trainer(TR, case["p"], lr_scheduler="constant_with_warmup", lr_warmup_steps=2, skip_bad_steps=guard,
                      skip_grad_norm_above=1e30 if guard else None, **kw)
        seen = []
        with (_pin_small(TR, tr, tape, record=not guard) if pinned else contextlib.nullcontext()):
            for i in range(3 * A):
                loss = tr.step(*_micro(case, i))
                if (i + 1) % A == 0:
                    tr.finish_optimizer()
                    torch.cuda.synchronize()
                    seen.append(dict(loss=loss.clone(), grad_norm=tr.grad_norm.clone(), last_lr=tr.last_lr,
                                     grads={k: g.detach().clone() for k, g in tr.grads.items()}, state=_full_state(tr)))
        assert tr.step_count == 3
        runs.append((tr, seen))
    (off, seen_off), (on, seen_on) = runs
    assert on.skip_bad_steps and not off.skip_bad_steps
    assert on.skipped_steps == 0 and on.last_step_skipped is False and on.last_skip_reason is None
    assert off.skipped_steps == 0 and off.last_step_skipped is False and off.last_skip_reason is None
    for i, (a, b) in enumerate(zip(seen_off, seen_on)):
        assert torch.equal(a["loss"], b["loss"]) and a["last_lr"] == b["last_lr"], i
        assert torch.equal(a["grad_norm"].view(torch.int32), b["grad_norm"].view(torch.int32)), i
        assert a["grads"].keys() == b["grads"].keys() and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"]), i
        _assert_same_state(a["state"], b["state"])
    assert seen_off[0]["last_lr"] == 0.0 and seen_off[2]["last_lr"] == 1e-3            # the warm-up ran
    assert not torch.equal(seen_off[1]["state"]["lora_master" if "lora_rank" in kw else "master.0"],
                           seen_off[2]["state"]["lora_master" if "lora_rank" in kw else "master.0"])


# ---- 2. a skipped step leaves no trace -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_run(TR, case):
    """The unguarded deterministic trainer stepped through [b0, b2, b3]: its final state, and its per-step norms and LRs."""
    tr = _trainer(TR, case["p"], deterministic=True, lr_scheduler="cosine", lr_warmup_steps=2, lr_num_training_steps=10)
    norms, lrs = [], []
    for i in (0, 2, 3):
        tr.step(*_micro(case, i))
        norms.append(float(tr.grad_norm)); lrs.append(tr.last_lr)
    torch.cuda.synchronize()
    return dict(state=_state(tr), norms=norms, lrs=lrs, next_lr=tr.current_lr(), grad_norm=tr.grad_norm.clone())


@pytest.mark.parametrize("kind", ["nan", "inf", "spike"])
def test_a_skipped_step_leaves_no_trace(TR, case, clean_run, kind):
    thr = 10.0 * max(clean_run["norms"]) if kind == "spike" else None
    tr = _trainer(TR, case["p"], deterministic=True, lr_scheduler="cosine", lr_warmup_steps=2, lr_num_training_steps=10,
                  skip_bad_steps=True, skip_grad_norm_above=thr)
    tr.step(*_micro(case, 0))
    assert tr.last_step_skipped is False and tr.step_count == 1
    after_first, lr_next = _state(tr), tr.current_lr()
    tr.step(*_bad(case, 1, kind))
    assert tr.last_step_skipped is True                      # read right after the bad step
    assert tr.last_skip_reason == ("grad_norm" if kind == "spike" else "nonfinite")
    assert tr.skipped_steps == 1 and tr.step_count == 1 and tr.current_lr() == lr_next
    bad_norm = float(tr.grad_norm)
    if kind == "spike":
        assert bad_norm == bad_norm and thr < bad_norm < float("inf")
    else:
        assert not bad_norm < float("inf")                   # NaN or +inf
    assert int(tr.coef.view(torch.int32)) == 0               # the clip kernel left +0.0 for the launches that did nothing
    torch.cuda.synchronize()
    _assert_same_state(after_first, _state(tr))
    lrs = [tr.last_lr]
    tr.step(*_micro(case, 2))
    assert tr.last_step_skipped is False and tr.last_skip_reason is None and tr.step_count == 2
    lrs.append(tr.last_lr)
    tr.step(*_micro(case, 3))
    lrs.append(tr.last_lr)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 3 and tr.last_step_skipped is False
    # the bad step was handed the LR of the step it did not take; the applied steps ran on the clean run's schedule
    assert lrs == [clean_run["lrs"][1]] + clean_run["lrs"][1:] and tr.current_lr() == clean_run["next_lr"]
    assert len(set(clean_run["lrs"])) == 3                   # warm-up shorter than the run, then the cosine: the position matters
    assert torch.equal(tr.grad_norm.view(torch.int32), clean_run["grad_norm"].view(torch.int32))
    _assert_same_state(clean_run["state"], _state(tr))
    assert _finite(clean_run["state"])


# ---- 3. accumulation: a bad micro-batch drops its cycle, and only its cycle ----------------------------------------------
def test_a_bad_micro_batch_skips_its_cycle_and_the_next_cycle_is_clean(TR, case):
    kw = dict(deterministic=True, gradient_accumulation_steps=3, use_ema=True, ema_decay=0.5)
    tr = _trainer(TR, case["p"], skip_bad_steps=True, **kw)
    start = _state(tr)
    tr.step(*_micro(case, 0))
    tr.step(*_bad(case, 1, "nan"))                           # the second of three micro-batches
    assert tr.skipped_steps == 0 and tr._micro == 2          # nothing is decided before the cycle's optimizer stage
    tr.step(*_micro(case, 2))
    assert tr.last_step_skipped is True and tr.last_skip_reason == "nonfinite" and tr.skipped_steps == 1
    assert tr.step_count == 0 and tr._micro == 0
    torch.cuda.synchronize()
    _assert_same_state(start, _state(tr))
    assert not _finite({"acc": tr._acc[1][0]})               # the accumulators are poisoned; mode 0 overwrites them
    fresh = _trainer(TR, case["p"], **kw)                    # unguarded, in the same (initial) state
    for t in (tr, fresh):
        for i in (3, 4, 5):
            t.step(*_micro(case, i))
    torch.cuda.synchronize()
    assert tr.step_count == 1 and fresh.step_count == 1 and tr.last_step_skipped is False and tr.skipped_steps == 1
    for a, b in zip(tr.layer_buckets + [tr.small_bucket], fresh.layer_buckets + [fresh.small_bucket]):
        assert torch.equal(a, b)
    assert torch.equal(tr.grad_norm.view(torch.int32), fresh.grad_norm.view(torch.int32))
    s = _state(tr)
    _assert_same_state(_state(fresh), s)
    assert _finite(s) and not torch.equal(s["master.0"], start["master.0"])


# ---- 4. two ranks on the one GPU over gloo (the harness of tests/test_dp_sharding_gpu.py) ---------------------------------
def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _run_ranks(rank)))
    except Exception:
        q.put((rank, traceback.format_exc()))
        raise
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(rank):
    import hashlib
    TR = importlib.import_module("video-gpt_amd.train")
    p, dbatch, args = _case()
    case = dict(p=p, dbatch=dbatch, args=args)

    def batch(i, bad=False):          # different data on every rank and every step
        db, x1, *rest = _micro(case, 0)
        x1 = torch.randn(x1.shape, generator=torch.Generator("cpu").manual_seed(800 + 10 * i + rank))
        if bad:
            x1.view(-1)[5] = float("nan")
        return (db, x1, *rest)
    res = {}
    for mode in ("none", "optimizer"):
        kw = dict(deterministic=True, dp_sharding=mode, use_ema=True, ema_decay=0.5)
        guarded = _trainer(TR, p, skip_bad_steps=True, **kw)
        assert guarded._sharded == (mode == "optimizer")
        flags = []
        for i in range(3):            # only rank 1 receives the bad batch, in step 2 of 3
            guarded.step(*batch(i, bad=(i == 1 and rank == 1)))
            flags.append((guarded.last_step_skipped, guarded.last_skip_reason, guarded.step_count))
        plain = _trainer(TR, p, **kw)  # the two-rank run without that step
        for i in (0, 2):
            plain.step(*batch(i))
        for t in (guarded, plain):
            t.finish_optimizer()
        torch.cuda.synchronize()
        sg, sp_ = _state(guarded), _state(plain)
        h = hashlib.sha1()
        for k in sorted(sg):
            if k.startswith("param:") or mode == "none":         # replicas: parameters always, the state when not sharded
                h.update(sg[k].contiguous().view(torch.uint8).cpu().numpy().tobytes())
        res[mode] = dict(flags=flags, skipped=guarded.skipped_steps, steps=(guarded.step_count, plain.step_count),
                         differ=[k for k in sg if not torch.equal(sg[k], sp_[k])], keys=sg.keys() == sp_.keys(),
                         finite=_finite(sg), digest=h.hexdigest(), grad_norm=float(guarded.grad_norm) == float(plain.grad_norm))
    return res


def test_two_ranks_skip_together_when_one_rank_has_the_bad_batch():
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = []
    try:
        for _ in procs:              # a failed rank reports first; the other then waits in a collective: stop it
            res.append(q.get(timeout=240))
            if isinstance(res[-1][1], str):
                break
    finally:
        ok = len(res) == 2 and not any(isinstance(r[1], str) for r in res)
        for p_ in procs:
            p_.join(timeout=60 if ok else 5)
            if p_.is_alive():
                p_.terminate()
    bad = [r for r in res if isinstance(r[1], str)]
    assert not bad, bad[0][1]
    assert [p_.exitcode for p_ in procs] == [0, 0]
    r0, r1 = (r[1] for r in sorted(res, key=lambda x: x[0]))
    for mode in ("none", "optimizer"):
        for r in (r0[mode], r1[mode]):                           # both ranks skip, the one with good data too
            assert r["flags"] == [(False, None, 1), (True, "nonfinite", 1), (False, None, 2)], (mode, r["flags"])
            assert r["skipped"] == 1 and r["steps"] == (2, 2) and r["keys"] and r["finite"] and r["grad_norm"]
            assert not r["differ"], (mode, r["differ"])          # == the two-rank run without that step, bit for bit
        assert r0[mode]["digest"] == r1[mode]["digest"], mode    # the replicas stay bit-identical to each other


# ---- 5. checkpoints ------------------------------------------------------------------------------------------------------------
def test_checkpoint_right_after_a_skipped_step_resumes_the_run(TR, case, tmp_path):
    kw = dict(deterministic=True, lr_scheduler="cosine", lr_warmup_steps=2, lr_num_training_steps=10, skip_bad_steps=True)
    a = _trainer(TR, case["p"], **kw)
    a.step(*_micro(case, 0))
    a.step(*_bad(case, 1, "inf"))
    path = a.save_checkpoint(str(tmp_path))                      # resolves the verdict in flight
    assert path.endswith("checkpoint-1")
    with open(os.path.join(path, "trainer_state.json")) as f:
        rec = json.load(f)
    assert rec["skipped_steps"] == 1 and rec["step_count"] == 1 and list(rec)[:len(PARENT_RECORD_KEYS)] == PARENT_RECORD_KEYS
    b = _trainer(TR, case["p"], **kw)
    assert b.load_checkpoint(path) == 1
    assert b.skipped_steps == 1 and b.step_count == 1 and b.last_step_skipped is False and b.current_lr() == a.current_lr()
    for t in (a, b):
        for i in (2, 3):
            t.step(*_micro(case, i))
    torch.cuda.synchronize()
    assert a.step_count == 3 and b.step_count == 3 and a.skipped_steps == 1 and b.skipped_steps == 1
    _assert_same_state(_state(a), _state(b))
    assert _finite(_state(b))
    # a checkpoint written with the key loads into a trainer without the guard, and the other way round
    plain = _trainer(TR, case["p"])
    assert plain.load_checkpoint(path) == 1 and plain.skipped_steps == 0 and plain.step_count == 1
    plain_path = plain.save_checkpoint(str(tmp_path / "plain"))
    c = _trainer(TR, case["p"], **kw)
    assert c.load_checkpoint(plain_path) == 1 and c.skipped_steps == 0 and c.step_count == 1


def test_guard_off_checkpoint_record_is_what_it_always_was(TR, case, tmp_path):
    texts = []
    for name, kw in (("implicit", dict()), ("explicit", dict(skip_bad_steps=False, skip_grad_norm_above=None))):
        tr = _trainer(TR, case["p"], deterministic=True, **kw)
        tr.step(*_micro(case, 0))
        path = tr.save_checkpoint(str(tmp_path / name))
        with open(os.path.join(path, "trainer_state.json")) as f:
            texts.append(f.read())
    assert texts[0] == texts[1]
    assert list(json.loads(texts[0])) == PARENT_RECORD_KEYS      # the parent commit's record: no new key, no other order
    rec = json.loads(texts[0])
    want = json.dumps({"step_count": 1, "global_step": 1, "lr": 1e-3, "weight_decay": 0.1, "betas": [0.9, 0.999], "eps": 1e-8,
                       "lr_scheduler": "constant", "lr_warmup_steps": 0, "lr_num_training_steps": None, "lr_num_cycles": None,
                       "lr_power": 1.0, "gradient_accumulation_steps": 1, "use_ema": False, "ema_decay": 0.9999,
                       "small_names": rec["small_names"]})
    assert texts[0] == want                                      # byte for byte the text the parent's json.dump call writes


# ---- 6. reports ------------------------------------------------------------------------------------------------------------------
def test_reports_name_the_tensor_and_the_bucket_norms_add_up(TR, case):
    tr = _trainer(TR, case["p"], skip_bad_steps=True)
    tr.step(*_micro(case, 0))                                    # a good step
    torch.cuda.synchronize()
    assert tr.nonfinite_report() == [] and tr.last_step_skipped is False
    norms = tr.bucket_grad_norms()
    assert list(norms) == list(range(len(tr.layer_buckets))) + ["small"] and len(norms) == len(tr.buckets)
    total = torch.zeros((), dtype=F32)
    for k, v in norms.items():                                   # the trainer's order of the sum: layers, then the small bucket
        assert v > 0.0
        total = total + torch.tensor(v * v, dtype=F32)
    assert torch.equal(total.view(torch.int32), tr.sumsq.cpu().view(torch.int32)[0])
    assert float(tr.grad_norm) == float(torch.sqrt(total))
    before = _state(tr)
    for name, value, want in ((tr.layer_names[-1][1], float("nan"), (1, 0)), ("llm.norm.weight", float("-inf"), (0, 1))):
        tr.step(*_micro(case, 1), update=False)                  # a stand-alone backward, then one bad element by hand
        tr.grads[name].view(-1)[7] = value
        tr.optimizer_step()
        assert tr.last_step_skipped is True and tr.last_skip_reason == "nonfinite"
        assert tr.nonfinite_report() == [(name, *want)]
    torch.cuda.synchronize()
    assert tr.skipped_steps == 2 and tr.step_count == 1
    _assert_same_state(before, _state(tr))
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    with pytest.raises(VgptError, match="skip_bad_steps=True"):
        _trainer(TR, case["p"]).bucket_grad_norms()


def test_reports_cover_the_lora_slots(TR, case):
    torch.manual_seed(11)
    tr = _trainer(TR, case["p"], lora_rank=4, skip_bad_steps=True)
    tr.step(*_micro(case, 0), update=False)
    name = [k for k in tr.lora if ".lora_B." in k][-1]
    tr.grads[name][2, 1] = float("nan")
    before = tr.lora_master.clone()
    tr.optimizer_step()
    assert tr.last_step_skipped is True and tr.nonfinite_report() == [(name, 1, 0)]
    assert list(tr.bucket_grad_norms()) == ["lora"] and torch.equal(tr.lora_master, before) and tr.step_count == 0


# ---- 7. what the guard is for ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_without_the_guard_one_bad_batch_destroys_the_run(TR, case, kind):
    tr = _trainer(TR, case["p"])
    tr.step(*_micro(case, 0))
    tr.step(*_bad(case, 1, kind))
    torch.cuda.synchronize()
    assert tr.step_count == 2 and tr.skipped_steps == 0 and tr.last_step_skipped is False
    s = _state(tr)
    assert not bool(torch.isfinite(s["master.0"]).all()) and not bool(torch.isfinite(s["m.0"]).all())
    assert not _finite({k: v for k, v in s.items() if k.startswith("param:")})
