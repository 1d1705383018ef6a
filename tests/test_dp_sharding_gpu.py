"""Stage1Trainer(dp_sharding="optimizer") on the GPU: the n-partial clip coefficient, world 1 (inert), and ranks spawned on
the one GPU over gloo (RCCL refuses two ranks per device) the way tests/test_train_gpu.py::_dp_worker does it, with
different data on every rank.

What is compared bit for bit and what is not: the decoder matrices' gradients come from deterministic GEMMs, but the small
fp32 gradients (norm gains, embeddings, heads) are summed with fp32 atomics whose order may vary between two runs
(tests/test_train_gpu.py), and they feed the next forward.  So the ranks of ONE run are compared bit for bit, as are
checkpoint files against the state that wrote them; two separate runs (sharded against replicated, a variant against the
plain sharded run) are compared at the tolerances test_train_gpu.py uses for that effect, except at world 1, where the small
gradients are pinned and the whole run is compared bit for bit."""
import hashlib
import importlib
import os
import socket
import traceback

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import smoke_case as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _case():
    from tests import glue_cases as GC
    p, batch, x1, x0, t, clean, x0i, ti = GC.stage1_case(R.TINY)
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    return p, dbatch, x1, x0, t, clean, x0i, ti


def _state(tr):
    """Losses aside, everything a step changes: parameters, master weights, moments (this trainer's own tensors)."""
    out = {f"param:{k}": v.detach().clone() for k, v in tr.model.state_dict().items()}
    for t, key, _ in tr._optimizer_tensors():
        out[key] = t.detach().clone()
    return out


# ---- vgpt_clip_coef with n partial sums ----
def _clip_reference(vals, max_norm, extra):
    """The kernel's order in numpy fp32: lane l adds values l, l + 64, ... in order, then wave_sum's butterfly."""
    lanes = np.zeros(64, np.float32)
    for i, v in enumerate(vals):
        lanes[i % 64] = np.float32(lanes[i % 64] + v)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(np.float32)
    nrm = np.sqrt(lanes[0], dtype=np.float32)
    c = np.float32(max_norm) / (nrm + np.float32(1e-6)) if max_norm > 0 else np.float32(1.0)
    return nrm, np.float32(min(c, np.float32(1.0)) * np.float32(extra))


@pytest.mark.parametrize("n", [1, 2, 3, 8, 64, 65, 200])
def test_clip_coef_adds_n_partials_in_a_fixed_order(n):
    T = importlib.import_module("video-gpt_amd.ops_train")
    rng = np.random.default_rng(n)
    vals = (rng.random(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    ss = torch.from_numpy(vals).to(DEV)
    coef, nrm = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    seq = np.float32(0)
    for v in vals:
        seq = np.float32(seq + v)                   # sequential fp32 sum
    for max_norm, extra in ((0.0, 0.5), (1e9, 1.0), (float(np.sqrt(seq)) * 0.5, 1 / 3)):
        T.clip_coef(ss, coef, nrm, max_norm, extra)
        torch.cuda.synchronize()
        rn, rc = _clip_reference(vals, max_norm, extra)
        assert float(nrm) == float(rn) and float(coef) == float(rc), (n, float(nrm), float(rn), float(coef), float(rc))
        assert abs(float(nrm) - float(np.sqrt(seq))) <= 1e-6 * float(np.sqrt(seq))
    if n == 1:       # the former single-value kernel: sqrt(s), min(1, max / (norm + 1e-6)) * extra, all in fp32
        old = np.sqrt(vals[0], dtype=np.float32)
        T.clip_coef(ss, coef, nrm, 0.25, 0.5)
        torch.cuda.synchronize()
        assert float(nrm) == float(old)
        assert float(coef) == float(np.float32(min(np.float32(0.25) / (old + np.float32(1e-6)), np.float32(1.0)) * np.float32(0.5)))


# ---- world 1: the option is inert ----
def test_world_one_optimizer_mode_is_the_replicated_run(monkeypatch):
    TR = importlib.import_module("video-gpt_amd.train")
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    p, db, x1, x0, t, clean, x0i, ti = _case()
    with pytest.raises(VgptError, match="dp_sharding"):
        TR.Stage1Trainer(SC.build_product_model(R.TINY, p, DEV, cls_name="LVMTraining"), dp_sharding="zero3")
    trs = {}
    for mode in ("none", "optimizer"):
        monkeypatch.setenv("VGPT_DP_SHARDING", mode)            # the default comes from the environment
        trs[mode] = TR.Stage1Trainer(SC.build_product_model(R.TINY, p, DEV, cls_name="LVMTraining"), lr=1e-3,
                                     weight_decay=0.1, max_grad_norm=0.5)
        assert trs[mode].dp_sharding == mode
    a, b = trs["none"], trs["optimizer"]
    assert not b._sharded
    sizes = lambda tr: [x.numel() for x in tr.layer_buckets + [tr.small_bucket] + tr.param_layers + [tr.param_small]
                        + tr.master_layers + [tr.master_small]]
    assert sizes(a) == sizes(b)                                 # no padding, full optimizer state
    for i in range(3):
        la = a.step(db, x1 * (1 + 0.1 * i), x0, t, clean, x0i, ti, update=False)
        lb = b.step(db, x1 * (1 + 0.1 * i), x0, t, clean, x0i, ti, update=False)
        assert torch.equal(la, lb)
        for ga, gb in zip(a.layer_buckets, b.layer_buckets):
            assert torch.equal(ga, gb)
        b.small_bucket.copy_(a.small_bucket)                    # pin the fp32-atomic small gradients
        a.optimizer_step(); b.optimizer_step()
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(a.grad_norm, b.grad_norm)


# ---- ranks on the one GPU ----
def _digest(tr):
    h = hashlib.sha1()
    for k, v in tr.model.state_dict().items():
        h.update(k.encode()); h.update(v.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def _flat_params(tr):
    return torch.cat([v.detach().float().reshape(-1).cpu() for v in tr.model.state_dict().values()])


def _worker(rank, world, port, q, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _run_ranks(rank, world, out_dir)))
    except Exception:
        q.put((rank, traceback.format_exc()))
        raise
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(rank, world, out_dir):
    import torch.distributed as dist
    TR = importlib.import_module("video-gpt_amd.train")
    SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
    p, db, x1, x0, t, clean, x0i, ti = _case()
    x1 = torch.randn(x1.shape, generator=torch.Generator("cpu").manual_seed(500 + rank))   # different data on every rank
    args = lambda i: (db, x1 * (1 + 0.1 * i), x0, t, clean, x0i, ti)
    clip = None if world == 2 else 1e-3
    group = dist.group.WORLD

    def build(mode, **kw):
        model = SC.build_product_model(R.TINY, p, DEV, cls_name="LVMTraining")
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(DEV)
        tr = TR.Stage1Trainer(model, lr=1e-3, weight_decay=0.1, max_grad_norm=clip, dp_sharding=mode, **kw)
        torch.cuda.synchronize()
        return tr, torch.cuda.memory_allocated(DEV) - before

    norms = {}

    def run(tr, steps=3, first=0):
        losses = []
        for i in range(steps):
            losses.append(tr.step(*args(first + i)).clone())
            norms.setdefault(id(tr), []).append(float(tr.grad_norm))
        tr.finish_optimizer()
        torch.cuda.synchronize()
        return torch.stack(losses).cpu()

    res = {}
    rep, mem_rep = build("none")
    l_rep = run(rep)
    sh, mem_sh = build("optimizer")
    assert sh._sharded and not rep._sharded
    l_sh = run(sh)
    # ---- state per rank: 1/P of the fp32 optimizer elements ----
    n_rep = sum(x.numel() for x in rep.master_layers) + rep.master_small.numel()
    n_sh = sum(x.numel() for x in sh.master_layers) + sh.master_small.numel()
    expect = sum(TR.shard_partition(n, world)[1] for n in sh._bucket_numel + [sh._small_numel])
    res["numel"] = (n_rep, n_sh, expect)
    res["mem"] = (mem_rep, mem_sh)
    res["padded"] = any(b.numel() > n for b, n in zip(sh.layer_buckets + [sh.small_bucket],
                                                       sh._bucket_numel + [sh._small_numel]))
    res["loss"] = (SC.rel_l2(l_sh, l_rep), bool(torch.equal(l_sh[0], l_rep[0])))
    res["grad_norm"] = (norms[id(rep)], norms[id(sh)])      # per step
    res["digest"] = _digest(sh)
    res["params_rel"] = SC.rel_l2(_flat_params(sh), _flat_params(rep))
    res["params_rel_max"] = max(SC.rel_l2(v.float(), rep.model.state_dict()[k].float())
                                for k, v in sh.model.state_dict().items())
    # gathered optimizer state against the replicated trainer's
    rel = {}
    for (t_, key, n), (tr_, key_r, _) in zip(sh._optimizer_tensors(), rep._optimizer_tensors()):
        full = SPM.all_gather_flat(t_, group).view(-1)
        assert key == key_r and bool((full[n:] == 0).all())              # the padding stays zero
        rel[key] = SC.rel_l2(full[:n], tr_)
    res["opt_rel"] = rel
    if world == 3:
        return res
    # ---- variants of the sharded run ----
    var = {}
    for name, kw, attr in (("overlap_optimizer", dict(overlap_optimizer=True), None),
                           ("gradient_checkpointing", dict(gradient_checkpointing=True), None),
                           ("allreduce_after_backward", {}, ("overlap_allreduce", False))):
        tr, _ = build("optimizer", **kw)
        if attr:
            setattr(tr, *attr)
        lv = run(tr)
        var[name] = (SC.rel_l2(lv, l_sh), SC.rel_l2(_flat_params(tr), _flat_params(sh)), _digest(tr))
        if name == "overlap_optimizer":
            ov = tr
    res["variants"] = var
    # ---- checkpoints: the sharded files hold the replicated layout, gathered from the shards bit for bit ----
    from safetensors.torch import load_file
    path_rep = rep.save_checkpoint(os.path.join(out_dir, "rep"))
    path_sh = sh.save_checkpoint(os.path.join(out_dir, "sh"))
    opt = load_file(os.path.join(path_sh, "optimizer.safetensors"))
    mine_ok = []
    for t_, key, n in sh._optimizer_tensors():
        s = t_.numel(); lo = rank * s
        want = torch.zeros(s)
        hi = min(lo + s, n)
        if hi > lo:
            want[:hi - lo] = opt[key][lo:hi]
        mine_ok.append(torch.equal(t_.cpu(), want) and opt[key].shape == (n,))
    msd = load_file(os.path.join(path_sh, "model.safetensors"))
    mine_ok.append(all(torch.equal(msd[k], v.cpu()) for k, v in sh.model.state_dict().items()))
    res["ckpt_slices"] = all(mine_ok)
    # a replicated checkpoint loaded into a sharded trainer: its slices, then the same next step as the replicated run
    sh2, _ = build("optimizer")
    assert sh2.load_checkpoint(path_rep) == 3 and sh2.step_count == 3
    opt_r = load_file(os.path.join(path_rep, "optimizer.safetensors"))
    ok = []
    for t_, key, n in sh2._optimizer_tensors():
        s = t_.numel(); lo = rank * s; hi = min(lo + s, n)
        ok.append(torch.equal(t_[:max(hi - lo, 0)].cpu(), opt_r[key][lo:hi]) and not bool(t_[max(hi - lo, 0):].any()))
    res["ckpt_load_slices"] = all(ok)
    la = run(rep, 1, first=3)
    lb = run(sh2, 1, first=3)
    res["ckpt_continue"] = (bool(torch.equal(la, lb)), SC.rel_l2(_flat_params(sh2), _flat_params(rep)), _digest(sh2))
    # ---- the sampler on rank 0 right after an overlapped sharded step waits for the update and its gathers ----
    ov.step(*args(3))                   # no finish_optimizer(): the update and the gathers may still be in flight
    if rank == 0:
        from tests.test_weight_updates_gpu import Case, params_from
        case = Case(R.TINY, C=2, G=2, hw=(16, 16), steps=2)
        got, _ = case.sample(ov.model, False)
        fresh, _ = case.sample(SC.build_product_model(R.TINY, params_from(ov.model.state_dict()), DEV), False)
        replicated, _ = case.sample(rep.model, False)
        res["sampler"] = (bool(torch.equal(got, fresh)), SC.rel_l2(got, replicated))
    # ---- skip_allreduce: a whole sharded step without one collective ----
    calls = []
    saved = {n: getattr(dist, n) for n in ("all_reduce", "reduce_scatter_tensor", "all_gather_into_tensor", "all_gather")}
    for n_, f_ in saved.items():
        setattr(dist, n_, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(f_, n_))
    try:
        sh.skip_allreduce = True
        sh.step(*args(4))
        sh.finish_optimizer()
        torch.cuda.synchronize()
    finally:
        for n_, f_ in saved.items():
            setattr(dist, n_, f_)
        sh.skip_allreduce = False
    res["skip_calls"] = list(calls)
    return res


def _spawn(world, out_dir):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, str(out_dir))) for r in range(world)]
    for p_ in procs:
        p_.start()
    res = []
    try:
        for _ in procs:              # a failed rank reports first; the others then wait in a collective: stop them
            res.append(q.get(timeout=300))
            if isinstance(res[-1][1], str):
                break
    finally:
        ok = len(res) == world and not any(isinstance(r[1], str) for r in res)
        for p_ in procs:
            p_.join(timeout=120 if ok else 5)
            if p_.is_alive():
                p_.terminate()
    res.sort(key=lambda x: x[0])
    bad = [r for r in res if isinstance(r[1], str)]
    assert not bad, bad[0][1]
    assert [p_.exitcode for p_ in procs] == [0] * world
    return [r[1] for r in res]


def _check_state_per_rank(res, world):
    for r in res:
        n_rep, n_sh, expect = r["numel"]
        assert n_sh == expect and n_sh * world < n_rep + world * world * 256 * 3, r["numel"]
        mem_rep, mem_sh = r["mem"]
        assert mem_rep - mem_sh >= 0.8 * 12 * (n_rep - n_sh), r["mem"]   # fp32 master + m + v: 12 B per element saved


def test_sharded_two_ranks_match_the_replicated_run(tmp_path):
    """P = 2 without clipping: a sum of two operands is the same under all-reduce and reduce-scatter, the norm is not used."""
    res = _spawn(2, tmp_path)
    r0, r1 = res
    print("P=2 per rank:", {k: r0[k] for k in ("numel", "mem", "loss", "grad_norm", "params_rel", "params_rel_max")})
    _check_state_per_rank(res, 2)
    assert r0["digest"] == r1["digest"]                                   # ranks bit-identical
    for r in res:
        assert r["loss"][1] and r["loss"][0] < 1e-5                       # first loss bitwise, later ones to rounding
        assert r["params_rel_max"] < 1e-4                                 # bf16 parameters: a flipped last bit here and there
        assert all(v < (2e-6 if k.startswith("master") else 1e-4) for k, v in r["opt_rel"].items()), r["opt_rel"]
        for name, (lrel, prel, dig) in r["variants"].items():
            assert lrel < 1e-5 and prel < 1e-4, (name, lrel, prel)
        assert r["ckpt_slices"] and r["ckpt_load_slices"]
        assert r["ckpt_continue"][0] and r["ckpt_continue"][1] < 1e-4
        assert r["skip_calls"] == [], r["skip_calls"]
    for name in r0["variants"]:
        assert r0["variants"][name][2] == r1["variants"][name][2], name     # every variant keeps the ranks identical
    assert r0["ckpt_continue"][2] == r1["ckpt_continue"][2]
    same, rel = r0["sampler"]
    print("P=2 sampler after an overlapped sharded step: rel-L2 to the replicated model's sample", rel)
    assert same and rel < 1e-2
    # the checkpoint files: sharded == replicated, key for key, to the tolerance of two separate runs
    from safetensors.torch import load_file
    for f, tol in (("optimizer.safetensors", 1e-4), ("model.safetensors", 1e-4)):
        a = load_file(str(tmp_path / "sh" / "checkpoint-3" / f))
        b = load_file(str(tmp_path / "rep" / "checkpoint-3" / f))
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            assert SC.rel_l2(a[k].float(), b[k].float()) < (2e-6 if k.startswith("master") else tol), k
    # ... and the sharded checkpoint resumes at world 1
    TR = importlib.import_module("video-gpt_amd.train")
    p, db, x1, x0, t, clean, x0i, ti = _case()
    one = TR.Stage1Trainer(SC.build_product_model(R.TINY, p, DEV, cls_name="LVMTraining"), lr=1e-3, weight_decay=0.1)
    assert one.load_checkpoint(str(tmp_path / "sh" / "checkpoint-3")) == 3
    opt = load_file(str(tmp_path / "sh" / "checkpoint-3" / "optimizer.safetensors"))
    msd = load_file(str(tmp_path / "sh" / "checkpoint-3" / "model.safetensors"))
    for t_, key, _ in one._optimizer_tensors():
        assert torch.equal(t_.cpu(), opt[key]), key
    for k, v in one.model.state_dict().items():
        assert torch.equal(v.cpu(), msd[k]), k
    one.step(db, x1, x0, t, clean, x0i, ti)
    torch.cuda.synchronize()


def test_sharded_three_ranks_with_clipping(tmp_path):
    """P = 3 (padding in the small bucket), clipping active: the norm is combined from three partial sums in rank order."""
    res = _spawn(3, tmp_path)
    print("P=3 per rank:", [{k: r[k] for k in ("numel", "mem", "grad_norm", "params_rel", "params_rel_max", "loss")}
                            for r in res])
    _check_state_per_rank(res, 3)
    assert len({r["digest"] for r in res}) == 1                          # ranks bit-identical
    assert all(r["padded"] for r in res)
    for r in res:
        g_rep, g_sh = r["grad_norm"]
        assert all(g / 3 > 1e-3 for g in g_sh)                            # the clip is active (norm of the mean > max)
        assert abs(g_sh[0] - g_rep[0]) <= 1e-6 * g_rep[0], r["grad_norm"]   # the same reduced gradient, summed per shard
        assert all(abs(a - b) <= 1e-5 * b for a, b in zip(g_sh, g_rep)), r["grad_norm"]   # later steps: separate runs
        assert r["params_rel"] < 1e-3, r["params_rel"]
    assert len({tuple(r["grad_norm"][1]) for r in res}) == 1
