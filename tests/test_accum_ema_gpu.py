"""Stage1Trainer(gradient_accumulation_steps=A, use_ema=True) on the GPU, on the tiny stage-1 configuration and batch of
tests/test_train_gpu.py (glue_cases.stage1_case).

What is compared bit for bit, and the one thing that has to be pinned for it: the decoder matrices' gradients (the bf16 layer
buckets, all but 2 % of the parameters) come from deterministic GEMMs, but the small fp32 gradients (norm gains, embeddings,
heads) are summed with fp32 atomics whose order may vary between two runs (tests/test_train_gpu.py,
tests/test_dp_sharding_gpu.py).  Two SEPARATE runs therefore agree bit for bit on the layer buckets only; wherever a test
below compares two runs bit for bit on everything, the second run receives the first run's small-bucket gradients (the
`_pin_small` recorder, what test_world_one_optimizer_mode_is_the_replicated_run does by hand with small_bucket.copy_).
Within one run nothing is pinned: the accumulated small bucket is compared with the sum of the very micro-gradients that run
produced, bit for bit, and with the stand-alone backward's gradients to the rounding of the atomics (1e-5, the figure of
test_gradient_checkpointing_gives_bit_identical_gradients)."""
import contextlib
import importlib
import json
import os
import socket
import traceback

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import glue_cases as GC
from tests import smoke_case as SC
from tests.test_accum_ema_kernels_gpu import U32, _ema_bound
from tests.test_ops_gpu import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32


@pytest.fixture(scope="module")
def TR():
    return importlib.import_module("video-gpt_amd.train")


def _case():
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(R.TINY)
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    return p, dbatch, (x1, x0, t, clean, x0i, ti)


@pytest.fixture(scope="module")
def case():
    p, dbatch, args = _case()
    return dict(p=p, dbatch=dbatch, args=args)


def _micro(case, i):
    """Micro-batch i: the shared batch with other target latents (i = 0: the case as it is)."""
    x1, *rest = case["args"]
    if i:
        x1 = x1 + 0.5 * torch.randn(x1.shape, generator=torch.Generator("cpu").manual_seed(70 + i))
    return (case["dbatch"], x1, *rest)


def _trainer(TR, p, **kw):
    kw.setdefault("lr", 1e-3); kw.setdefault("weight_decay", 0.1)
    return TR.Stage1Trainer(SC.build_product_model(R.TINY, p, DEV, cls_name="LVMTraining"), **kw)


def _state(tr):
    """Everything an optimizer step changes: parameters, master weights, moments and (with use_ema) the EMA."""
    out = {f"param:{k}": v.detach().clone() for k, v in tr.model.state_dict().items()}
    for t, key, _ in tr._optimizer_tensors() + tr._ema_tensors():
        out[key] = t.detach().clone()
    return out


def _assert_same_state(a, b, skip=()):
    assert a.keys() == b.keys()
    bad = [k for k in a if not k.startswith(tuple(skip) or ("\0",)) and not torch.equal(a[k], b[k])]
    assert not bad, bad


@contextlib.contextmanager
def _pin_small(TR, tr, tape, record):
    """The small fp32 gradients of `tr`, call by call: recorded onto `tape` (record=True) or replaced by the tape's (False)
    right where the trainer consumes them -- in front of grad_accumulate on the small bucket under accumulation, in front of
    optimizer_step otherwise."""
    T, pos = TR.T, [0]
    real_acc, real_opt = T.grad_accumulate, tr.optimizer_step
    n = tr._small_numel

    def pin():
        if record:
            tape.append(tr.small_bucket[:n].clone())
        else:
            tr.small_bucket[:n].copy_(tape[pos[0]])
            pos[0] += 1

    def acc(a, g, mode):
        if g.data_ptr() == tr.small_bucket.data_ptr():
            pin()
        return real_acc(a, g, mode)

    def opt(*a, **k):
        if tr.accum_steps == 1:
            pin()
        return real_opt(*a, **k)
    T.grad_accumulate, tr.optimizer_step = acc, opt
    try:
        yield
    finally:
        T.grad_accumulate = real_acc
        del tr.optimizer_step


@contextlib.contextmanager
def _spy(TR, tr):
    """Records every grad_accumulate call (accumulator id, mode, the gradient before and after) and the gradient buckets as
    optimizer_step finds them."""
    T, log = TR.T, dict(acc=[], opt=[])
    real_acc, real_opt = T.grad_accumulate, tr.optimizer_step

    def acc(a, g, mode):
        before = g.clone()
        real_acc(a, g, mode)
        log["acc"].append((g.data_ptr(), mode, before, g.clone()))

    def opt(*a, **k):
        buckets = [tr.lora_bucket] if tr.lora_rank is not None else tr.layer_buckets + [tr.small_bucket]
        log["opt"].append((a, k, [b.clone() for b in buckets]))
        return real_opt(*a, **k)
    T.grad_accumulate, tr.optimizer_step = acc, opt
    try:
        yield log
    finally:
        T.grad_accumulate = real_acc
        del tr.optimizer_step


# ---- 1. accumulation is the sum ----------------------------------------------------------------------------------------
def test_accumulated_buckets_hold_the_once_rounded_sum(TR, case):
    ref = _trainer(TR, case["p"])
    alone = []
    for i in (0, 1):      # what a stand-alone backward leaves in the buckets for each micro-batch
        ref.step(*_micro(case, i), update=False)
        alone.append([b.clone() for b in ref.layer_buckets + [ref.small_bucket]])
    assert not torch.equal(alone[0][0], alone[1][0])          # two different micro-batches
    tr = _trainer(TR, case["p"], gradient_accumulation_steps=2)
    with _spy(TR, tr) as log:
        tr.step(*_micro(case, 0))
        assert not log["opt"] and tr.step_count == 0
        tr.step(*_micro(case, 1))
    torch.cuda.synchronize()
    assert len(log["opt"]) == 1 and log["opt"][0][1] == dict(micro_batches=2) and tr.step_count == 1
    found = log["opt"][0][2]
    nl = len(tr.layer_buckets)
    for i in range(nl):   # deterministic GEMMs: bit for bit against the stand-alone backwards
        want = (alone[0][i].float() + alone[1][i].float()).to(BF)
        assert torch.equal(found[i], want), f"layer bucket {i}"
        assert found[i].dtype == BF and float(found[i].float().abs().max()) > 0
    # every bucket, the small one included: bit for bit the sum of the micro-gradients THIS run produced
    ptrs = [b.data_ptr() for b in tr.layer_buckets + [tr.small_bucket]]
    for j, ptr in enumerate(ptrs):
        calls = [c for c in log["acc"] if c[0] == ptr]
        assert [c[1] for c in calls] == [0, 2], (j, [c[1] for c in calls])
        g1, g2 = calls[0][2], calls[1][2]
        assert torch.equal(calls[0][3], g1)                                   # mode 0 leaves the bucket alone
        assert torch.equal(calls[1][3], (g1.float() + g2.float()).to(g1.dtype)) and torch.equal(calls[1][3], found[j]), j
    small = (alone[0][nl] + alone[1][nl])
    assert found[nl].dtype == F32 and rel_l2(found[nl], small) < 1e-5       # atomics: two runs agree to rounding
    # a layer's accumulate sits right behind that layer's backward: last layer first, the small bucket last
    order = [c[0] for c in log["acc"][:nl + 1]]
    assert order == [b.data_ptr() for b in reversed(tr.layer_buckets)] + [tr.small_bucket.data_ptr()]


# ---- 2. A copies of one batch are the single step ----------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("clip", [None, 1.0], ids=["no-clip", "clip-1.0"])
def test_accumulating_one_batch_A_times_is_the_single_step(TR, case, A, clip):
    """A and 1/A are powers of two, so the fp32 sums A g and the factor 1/A are exact.  Without clipping the coefficient is
    1/A exactly and the whole state is bit-identical to the A = 1 step.  With max_grad_norm = 1 and nrm the norm of the
    mean gradient, the A = 1 run scales g by c1 = min(1, 1 / (nrm + 1e-6)) and the accumulated run scales A g by
    min(1, A / (A nrm + 1e-6)) / A, i.e. g by cA = min(1 / A ... ) = min(1, 1 / (nrm + 1e-6 / A)): the two differ only
    through clip_coef's 1e-6 term, by at most delta = 1e-6 / nrm relative (0 when the clip is idle), plus 8 u for the fp32
    roundings of the norm, the sum and the division (u = 2^-24).  From zero moments, one step: m = (1 - b1) c g carries
    delta, v = (1 - b2) (c g)^2 carries 2 delta, and the update lr m^ / (sqrt(v^) + eps) has magnitude <= lr and moves by
    at most delta relative (numerator and denominator scale together; eps only damps it)."""
    tape = []
    one = _trainer(TR, case["p"], max_grad_norm=clip)
    with _pin_small(TR, one, tape, record=True):
        one.step(*_micro(case, 0))
    acc = _trainer(TR, case["p"], max_grad_norm=clip, gradient_accumulation_steps=A)
    with _pin_small(TR, acc, tape * A, record=False):
        for _ in range(A):
            acc.step(*_micro(case, 0))
    torch.cuda.synchronize()
    assert acc.step_count == 1 and one.step_count == 1
    nrm = float(one.grad_norm)
    # grad_norm reports the norm of the SUM over the micro-batches (the sums of squares scale by A^2 exactly; 4 u for sqrt)
    assert abs(float(acc.grad_norm) - A * nrm) <= 4 * U32 * A * nrm, (float(acc.grad_norm), nrm)
    s1, sA = _state(one), _state(acc)
    if clip is None:
        _assert_same_state(s1, sA)
        return
    lr = 1e-3
    assert nrm > clip, nrm          # the clip is ACTIVE on this case, so the 1e-6 term it is meant to bound is reached
    delta = (1e-6 / nrm if nrm + 1e-6 > clip else 0.0) + 8 * U32
    print(f"MEASURE A={A}: norm of the mean gradient {nrm:.4g}, delta {delta:.3g}")
    for k in s1:
        a, b = s1[k].double(), sA[k].double()
        if k.startswith("m"):
            if k.startswith("master"):
                bound = lr * (delta + 16 * U32) + 2 * U32 * a.abs()
            else:
                bound = (delta + 4 * U32) * a.abs() + 1e-30
        elif k.startswith("v"):
            bound = (2 * delta + 6 * U32) * a.abs() + 1e-30
        else:       # bf16 parameters: roundings of masters that differ by at most the bound above: one bf16 spacing (<= 2^-7 |a|)
            bound = 2.0 ** -7 * a.abs() + lr * (delta + 16 * U32)
        assert bool(((a - b).abs() <= bound).all()), (k, float(((a - b).abs() / bound).max()))


# ---- 3. micro-steps are silent ------------------------------------------------------------------------------------------
def test_micro_steps_change_nothing_but_the_accumulators(TR, case, tmp_path):
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    tr = _trainer(TR, case["p"], gradient_accumulation_steps=3, lr_scheduler="linear", lr_num_training_steps=10)
    s0, lr0 = _state(tr), tr.current_lr()
    assert lr0 == 1e-3 and tr._acc is None            # accumulators are allocated on first use
    for i in range(2):
        tr.step(*_micro(case, i))
        torch.cuda.synchronize()
        assert tr.step_count == 0 and tr.current_lr() == lr0 and tr._micro == i + 1
        _assert_same_state(s0, _state(tr))
        with pytest.raises(VgptError, match="accumulation cycle"):
            tr.save_checkpoint(str(tmp_path))
        assert not os.listdir(tmp_path)
    # a stand-alone backward in the middle of the cycle: buckets overwritten, accumulators and the counter untouched
    accs = [a.clone() for a in [tr._acc[0]] + tr._acc[1]]
    tr.step(*_micro(case, 5), update=False)
    tr.step(*_micro(case, 5), update=False, backward=False)
    assert tr._micro == 2 and all(torch.equal(a, b) for a, b in zip(accs, [tr._acc[0]] + tr._acc[1]))
    _assert_same_state(s0, _state(tr))
    tr.step(*_micro(case, 2))
    torch.cuda.synchronize()
    assert tr.step_count == 1 and tr._micro == 0 and tr.last_lr == lr0
    assert abs(tr.current_lr() - 0.9e-3) < 1e-15      # "linear" over 10 steps, counted in optimizer steps
    s1 = _state(tr)
    assert not any(torch.equal(s0[k], s1[k]) for k in s1 if k.startswith(("master.", "m.", "v.")))
    path = tr.save_checkpoint(str(tmp_path))          # on the boundary it saves, and the record carries A and the schedule
    with open(os.path.join(path, "trainer_state.json")) as f:
        rec = json.load(f)
    assert rec["gradient_accumulation_steps"] == 3 and rec["lr_scheduler"] == "linear" and rec["lr_num_training_steps"] == 10
    assert rec["lr_num_cycles"] is None and rec["lr_power"] == 1.0 and rec["use_ema"] is False
    other = _trainer(TR, case["p"], gradient_accumulation_steps=2)       # another A resumes; the schedule comes back
    assert other.load_checkpoint(path) == 1 and other.accum_steps == 2
    assert other.lr_scheduler == "linear" and other.lr_num_training_steps == 10 and other.current_lr() == tr.current_lr()
    _assert_same_state(s1, _state(other))


# ---- 4. LoRA -------------------------------------------------------------------------------------------------------------
def test_lora_accumulation_is_the_sum_and_leaves_the_base_alone(TR, case):
    def lora_trainer(**kw):
        torch.manual_seed(11)
        tr = _trainer(TR, case["p"], lora_rank=8, **kw)
        gen = torch.Generator("cpu").manual_seed(48)
        for k, v in tr.lora.items():          # lora_B away from its zero init, so that dA is not trivially zero
            if ".lora_B." in k:
                v.copy_((torch.randn(v.shape, generator=gen) * 0.02).to(BF))
        tr.lora_master.copy_(tr.lora_param)
        return tr
    ref = lora_trainer()
    alone = []
    for i in (0, 1):
        ref.step(*_micro(case, i), update=False)
        alone.append(ref.lora_bucket.clone())
    tr = lora_trainer(gradient_accumulation_steps=2)
    base = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    before = tr.lora_param.clone()
    with _spy(TR, tr) as log:
        tr.step(*_micro(case, 0))
        assert not log["opt"] and tr.step_count == 0 and torch.equal(tr.lora_param, before)
        tr.step(*_micro(case, 1))
    torch.cuda.synchronize()
    assert len(log["opt"]) == 1 and tr.step_count == 1
    want = alone[0] + alone[1]                # an fp32 bucket: the fp32 sum itself
    assert want.dtype == F32 and float(want.abs().max()) > 0
    assert torch.equal(log["opt"][0][2][0], want)          # vgpt_lora_grad is bit-identical from run to run
    assert [c[1] for c in log["acc"]] == [0, 2]
    assert not torch.equal(tr.lora_param, before)
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, base[k]), k


# ---- 5. EMA does not perturb training -----------------------------------------------------------------------------------
def test_ema_rides_along_without_changing_the_training_run(TR, case):
    d = 0.5
    tape = []
    plain = _trainer(TR, case["p"])
    with _pin_small(TR, plain, tape, record=True):
        for i in range(3):
            plain.step(*_micro(case, i))
    tr = _trainer(TR, case["p"], use_ema=True, ema_decay=d)
    keys = [k for _, k, _ in tr._ema_tensors()]
    masters = {"ema_small": lambda: tr.master_small, **{f"ema.{i}": (lambda i=i: tr.master_layers[i]) for i in range(len(tr.master_layers))}}
    for t, k, _ in tr._ema_tensors():
        assert torch.equal(t, masters[k]()) and t.data_ptr() != masters[k]().data_ptr()    # starts as a COPY of the master
    ref = {k: masters[k]().double().clone() for k in keys}        # the recursion in float64, from the master snapshots
    err = {k: torch.zeros_like(ref[k]) for k in keys}             # its bound, compounded
    D = float(np.float32(d))
    with _pin_small(TR, tr, tape, record=False):
        for i in range(3):
            tr.step(*_micro(case, i))
            torch.cuda.synchronize()
            for t, k, _ in tr._ema_tensors():
                # one step of the kernel test's bound on top of D times the error so far (that error also enters |X|)
                X, b = _ema_bound(d, masters[k](), ref[k])
                err[k] = D * err[k] * (1 + 2 * U32) + b
                ref[k] = X
                ratio = float(((t.double() - X).abs() / err[k]).max())
                assert ratio <= 1.0, (i, k, ratio)
    sp, se = _state(plain), _state(tr)
    assert set(se) - set(sp) == set(keys)
    _assert_same_state(sp, {k: v for k, v in se.items() if k in sp})
    for t, k, _ in tr._ema_tensors():
        assert not torch.equal(t, masters[k]())                   # decay 0.5: the EMA lags the master


# ---- 6. ema_weights() ----------------------------------------------------------------------------------------------------
def test_ema_weights_context_swaps_the_ema_in_and_the_training_weights_back(TR, case, tmp_path):
    from safetensors.torch import load_file
    WU = importlib.import_module("tests.test_weight_updates_gpu")
    scase = WU.Case(R.TINY, C=2, G=2, hw=(16, 16), steps=2)
    tape = []
    tr = _trainer(TR, case["p"], use_ema=True, ema_decay=0.5, lr=5e-3)
    assert tr.last_load is None                                   # nothing loaded yet
    twin = _trainer(TR, case["p"], use_ema=True, ema_decay=0.5, lr=5e-3)        # never enters the context
    with _pin_small(TR, tr, tape, record=True):
        for i in range(3):
            tr.step(*_micro(case, i))
    outside, _ = scase.sample(tr.model, True)                     # an engine is cached on the training weights
    before = _state(tr)
    ptrs = [p_.data_ptr() for p_ in tr.model.parameters()]
    path = tr.save_checkpoint(str(tmp_path))
    with tr.ema_weights() as mm:
        assert mm is tr.model
        live = dict(mm.named_parameters())
        assert set(live) == {k for _, _, names in tr._ema_buckets() for k in names}
        for ema, param, names in tr._ema_buckets():
            assert torch.equal(param, ema.to(BF))
            o = 0
            for k in names:                                       # every model parameter, through the model's own views
                sz = tr.params[k].numel()
                assert torch.equal(live[k].detach().reshape(-1), ema[o:o + sz].to(BF)), k
                o += sz
        inside, _ = scase.sample(mm, True)
        # training or saving inside would use the EMA values as the model's weights: refused, and nothing has moved
        for call in (lambda: tr.step(*_micro(case, 3)), tr.optimizer_step, lambda: tr.save_checkpoint(str(tmp_path / "inside")),
                     lambda: tr.load_checkpoint(path), lambda: tr.ema_weights().__enter__()):
            with pytest.raises(Exception, match="ema_weights"):
                call()
        assert tr.step_count == 3 and not os.path.exists(tmp_path / "inside")
        tr.step(*_micro(case, 3), update=False, backward=False)          # evaluating the EMA weights is allowed
    assert not torch.equal(inside, outside)
    ema_sd = load_file(os.path.join(path, "ema.safetensors"))
    assert set(ema_sd) == set(tr.model.state_dict()) and all(v.dtype == BF for k, v in ema_sd.items() if k in tr.params)
    fresh, _ = scase.sample(SC.build_product_model(R.TINY, WU.params_from(ema_sd), DEV), False)
    assert torch.equal(inside, fresh)                             # the cached engine was refreshed on entry ...
    again, _ = scase.sample(tr.model, True)
    assert torch.equal(again, outside)                            # ... and on exit
    _assert_same_state(before, _state(tr))                        # training weights (and all state) back bit for bit
    assert [p_.data_ptr() for p_ in tr.model.parameters()] == ptrs            # nothing re-pointed
    with _pin_small(TR, tr, tape, record=True):
        tr.step(*_micro(case, 3))
    with _pin_small(TR, twin, tape, record=False):
        for i in range(4):
            twin.step(*_micro(case, i))
    torch.cuda.synchronize()
    _assert_same_state(_state(twin), _state(tr))                  # the next step is that of a trainer that never entered
    for master, param in zip([tr.master_small] + tr.master_layers, [tr.param_small] + tr.param_layers):
        assert torch.equal(param, master.to(BF))                  # AdamW still writes the storage the model reads
    plain = _trainer(TR, case["p"])
    with pytest.raises(Exception, match="no EMA"):
        plain.ema_weights().__enter__()
    with pytest.raises(Exception, match="no EMA"):
        plain.ema_state_dict()


# ---- 7. checkpoints -------------------------------------------------------------------------------------------------------
def test_ema_checkpoint_resume(TR, case, tmp_path):
    from safetensors.torch import load_file
    tape = []
    a = _trainer(TR, case["p"], use_ema=True, ema_decay=0.5)
    with _pin_small(TR, a, tape, record=True):
        for i in range(2):
            a.step(*_micro(case, i))
        path = a.save_checkpoint(str(tmp_path))
        saved = _state(a)
        a.step(*_micro(case, 2))
    opt = load_file(os.path.join(path, "optimizer.safetensors"))
    assert {"ema_small", "master_small"} | {f"ema.{i}" for i in range(len(a.ema_layers))} <= set(opt)
    assert all(torch.equal(opt[k], t.cpu()) for k, t in saved.items() if not k.startswith("param:"))
    ema_sd = load_file(os.path.join(path, "ema.safetensors"))
    want_sd = {}
    for ema, _, names in a._ema_buckets():
        o = 0
        for k in names:
            want_sd[k] = saved["ema_small" if names is a.small_names else f"ema.{a.layer_names.index(names)}"][o:o + a.params[k].numel()]
            o += a.params[k].numel()
    for k, v in ema_sd.items():
        if k in want_sd:
            assert v.dtype == BF and torch.equal(v.reshape(-1), want_sd[k].to(BF).cpu()), k
    with open(os.path.join(path, "trainer_state.json")) as f:
        rec = json.load(f)
    assert rec["use_ema"] is True and rec["ema_decay"] == 0.5
    b = _trainer(TR, case["p"], use_ema=True, ema_decay=0.5)
    assert b.load_checkpoint(path) == 2 and b.last_load["ema"] == "restored"
    _assert_same_state(saved, _state(b))
    with _pin_small(TR, b, tape[2:], record=False):
        b.step(*_micro(case, 2))
    torch.cuda.synchronize()
    _assert_same_state(_state(a), _state(b))                      # step 3 of the resumed run == step 3 of the uninterrupted one
    # an EMA checkpoint into a trainer without EMA: the EMA tensors are ignored
    c = _trainer(TR, case["p"])
    assert c.load_checkpoint(path) == 2 and c.last_load["ema"] == "none"
    _assert_same_state({k: v for k, v in saved.items() if not k.startswith("ema")}, _state(c))
    # a checkpoint without EMA into an EMA trainer: the EMA starts from the loaded master weights, and the load says so
    plain_path = c.save_checkpoint(str(tmp_path / "plain"))
    assert not os.path.exists(os.path.join(plain_path, "ema.safetensors"))
    assert not any(k.startswith("ema") for k in load_file(os.path.join(plain_path, "optimizer.safetensors")))
    e = _trainer(TR, case["p"], use_ema=True)
    assert e.load_checkpoint(plain_path) == 2 and e.last_load["ema"] == "initialised from master"
    assert torch.equal(e.ema_small, e.master_small) and torch.equal(e.master_small, saved["master_small"])
    assert all(torch.equal(x, y) for x, y in zip(e.ema_layers, e.master_layers))


# ---- 8. two ranks on the one GPU over gloo (the harness of tests/test_train_gpu.py / test_dp_sharding_gpu.py) ------------
def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _run_ranks(rank, world)))
    except Exception:
        q.put((rank, traceback.format_exc()))
        raise
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(rank, world):
    import hashlib
    import torch.distributed as dist
    TR = importlib.import_module("video-gpt_amd.train")
    SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
    p, dbatch, args = _case()
    case = dict(p=p, dbatch=dbatch, args=args)

    def micro(i):          # different data on every rank and every micro-step
        db, x1, *rest = _micro(case, 0)
        return (db, torch.randn(x1.shape, generator=torch.Generator("cpu").manual_seed(500 + 10 * i + rank)), *rest)
    names = ("all_reduce", "reduce_scatter_tensor", "all_gather_into_tensor", "all_gather")
    saved = {n: getattr(dist, n) for n in names}
    calls = []
    for n_, f_ in saved.items():
        setattr(dist, n_, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(f_, n_))
    tape, res, trs = [], {}, {}
    try:
        for mode in ("none", "optimizer"):
            # no clipping: at P = 2 the sum of two operands is the same under all-reduce and reduce-scatter, while the norm
            # is summed per shard in one mode and per bucket in the other (tests/test_dp_sharding_gpu.py)
            tr = _trainer(TR, p, max_grad_norm=None, dp_sharding=mode, gradient_accumulation_steps=2, use_ema=True,
                          ema_decay=0.5)
            assert tr._sharded == (mode == "optimizer")
            per_micro = []
            with _pin_small(TR, tr, tape, record=(mode == "none")):
                for i in range(4):          # two optimizer steps of two micro-steps each
                    n0 = len(calls)
                    tr.step(*micro(i))
                    tr.finish_optimizer()
                    torch.cuda.synchronize()
                    per_micro.append(len(calls) - n0)
            assert tr.step_count == 2
            res[f"calls:{mode}"] = per_micro
            trs[mode] = tr
        rep, sh = trs["none"], trs["optimizer"]
        h = hashlib.sha1()
        same = {}
        for (t_s, key, n), (t_r, key_r, _) in zip(sh._optimizer_tensors() + sh._ema_tensors(),
                                                  rep._optimizer_tensors() + rep._ema_tensors()):
            full = SPM.all_gather_flat(t_s, dist.group.WORLD).view(-1)
            assert key == key_r and not bool(full[n:].any())
            same[key] = bool(torch.equal(full[:n], t_r))
            h.update(t_r.cpu().numpy().tobytes())
        esd_s, esd_r = sh.ema_state_dict(), rep.ema_state_dict()
        same["ema_state_dict"] = esd_s.keys() == esd_r.keys() and all(torch.equal(esd_s[k], esd_r[k]) for k in esd_r)
        for (k, v), (k2, v2) in zip(sh.model.state_dict().items(), rep.model.state_dict().items()):
            same[f"param:{k}"] = k == k2 and bool(torch.equal(v, v2))
            h.update(v2.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
        res["same"] = same
        res["digest"] = h.hexdigest()
        res["moved"] = not torch.equal(rep.ema_layers[0], rep.master_layers[0]) and float(rep.m_layers[0].abs().max()) > 0
    finally:
        for n_, f_ in saved.items():
            setattr(dist, n_, f_)
    return res


def test_two_ranks_accumulate_and_average_in_step():
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
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
    assert r0["digest"] == r1["digest"]                          # replicas bit-identical after two optimizer steps
    for r in (r0, r1):
        for mode in ("none", "optimizer"):
            c = r[f"calls:{mode}"]
            assert c[0] == 0 and c[2] == 0 and c[1] > 0 and c[3] > 0, (mode, c)     # no collective on non-final micro-steps
        wrong = [k for k, v in r["same"].items() if not v]
        assert not wrong, wrong                                  # sharded (gathered) == replicated, EMA and parameters, bit for bit
        assert r["moved"]


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def test_constructor_refusals(TR, case):
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    model = SC.build_product_model(R.TINY, case["p"], DEV, cls_name="LVMTraining")
    with pytest.raises(VgptError, match="EMA of adapters is not built"):
        TR.Stage1Trainer(model, use_ema=True, lora_rank=4)
    with pytest.raises(VgptError, match="forward_only"):
        TR.Stage1Trainer(model, use_ema=True, forward_only=True)
    for bad in (0, 1.5, -2, True, "2"):
        with pytest.raises(VgptError, match="gradient_accumulation_steps"):
            TR.Stage1Trainer(model, gradient_accumulation_steps=bad)
    for bad in (-0.1, 1.0001):
        with pytest.raises(VgptError, match="ema_decay"):
            TR.Stage1Trainer(model, use_ema=True, ema_decay=bad)
    for name in ("linear", "cosine", "cosine_with_restarts", "polynomial"):
        with pytest.raises(VgptError, match="lr_num_training_steps"):
            TR.Stage1Trainer(model, lr_scheduler=name)
    with pytest.raises(VgptError, match="cosine_with_restarts"):          # the message lists what is built
        TR.Stage1Trainer(model, lr_scheduler="inverse_sqrt")
    assert dict(model.named_parameters())["llm.norm.weight"].data_ptr()   # a refused constructor leaves the model usable
