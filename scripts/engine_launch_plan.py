#!/usr/bin/env python3
"""What the sampler engine (engine.StaticDenoiser) asks of the device, as text two commits can be diffed on: for every
configuration below one sample is drawn through LVMScheduler while every C-ABI call of the product modules is recorded --
entry point, scalar arguments verbatim, every pointer argument replaced by the index of that address's first appearance in
the configuration's run (the aliasing structure without the addresses; _lib.SIGNATURES tells pointers from integers).
Per configuration: the call sequence -- as its length, its sha256 and the entry points with their counts in order of first
use; --calls prints the recorded lines themselves, to find where two commits part once the hashes differ -- the growth of
torch.cuda.memory_allocated() across the sampler call with the engine still held (its buffers, plans and derived weights),
the sha256 of the sampled latents' bytes.  A host-side change of the engine that is invisible to the device leaves this
output byte-identical.

Configurations, the smallest that reach each branch: the tiny model under every sampler option and the two batches of
tests/test_model_gpu.py::test_sampler_fast_path; two full-width layers (the only width with the folded RMSNorms); two
ranks over gloo on one GPU (fresh child processes, as tests/test_sp_engine_gpu.py; one trace per rank).  Only public
surface is used (LVMScheduler options, the test cases' inputs), so the script runs unchanged on any commit that has them.
    python3 scripts/engine_launch_plan.py [--calls] > OUT.txt        # seconds of GPU time + two-layer full-width parameters on the host
"""
import ctypes
import hashlib
import importlib
import os
import socket
import sys
import textwrap
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
TINY_CASE = dict(C=2, G=2, hw=(16, 16), steps=3)
FULL_CALLS = "--calls" in sys.argv[1:]


class Recorder:
    """Wraps the `call` binding: in _lib, for the modules imported from now on, and in every loaded product module that
    has imported it already."""

    def __init__(self):
        for name in ("_lib", "ops", "ops_train", "scheduler", "engine"):
            importlib.import_module("video-gpt_amd." + name)
        L = sys.modules["video-gpt_amd._lib"]
        self.sig, self.orig, self.lines, self.seen = L.SIGNATURES, L.call, None, None
        for name, mod in list(sys.modules.items()):
            if name.startswith("video-gpt_amd") and mod is not None and getattr(mod, "call", None) is self.orig:
                mod.call = self

    def __call__(self, name, *args):
        if self.lines is not None:
            out = []
            for ty, v in zip(self.sig[name][1], args):
                if ty is ctypes.c_void_p:
                    out.append("null" if v is None else f"p{self.seen.setdefault(int(v), len(self.seen))}")
                elif isinstance(v, (int, float)):
                    out.append(repr(v))
                else:
                    out.append("ref")        # a byref() result slot
            self.lines.append(f"{name}({', '.join(out)})")
        return self.orig(name, *args)

    def start(self):
        self.lines, self.seen = [], {}

    def stop(self):
        lines, self.lines = self.lines, None
        return lines


def scheduler(steps, **opts):
    S = importlib.import_module("video-gpt_amd.scheduler")
    sched = S.LVMScheduler(num_steps=steps, time_shifting_factor=1)
    sched.cache_engines = False
    for k, v in opts.items():
        setattr(sched, k, v)
    return sched


def sample(rec, title, sched, model, z, kw, times=1):
    """`times` sampler calls on one scheduler (the second of a cached engine goes through rebind), as one report."""
    import torch
    zs = [t.to(DEV, torch.bfloat16) for t in z]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    rec.start()
    for _ in range(times):
        out = torch.cat(sched(zs, model.frame_block_forward_with_cfg, kw, prediction_type="x1"))
    torch.cuda.synchronize()
    lines = rec.stop()
    digest = hashlib.sha256(out.float().cpu().numpy().tobytes()).hexdigest()
    del out
    growth = torch.cuda.memory_allocated() - before
    eng = sched.last_engine
    model.__dict__.pop("_vgpt_engine_cache", None)      # the next configuration builds its own engine
    count = {}
    for l in lines:
        name = l.split("(")[0]
        count[name] = count.get(name, 0) + 1
    points = textwrap.wrap("entry points: " + ", ".join(f"{n[5:]} x{c}" for n, c in count.items()), 120, subsequent_indent="  ")
    return "\n".join([f"== {title} ==", f"calls {len(lines)} sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}",
                      *points, *(lines if FULL_CALLS else []), f"alloc_growth_bytes {growth}",
                      f"engine S={eng.S} Ma={eng.Ma} B={eng.B} hoist={bool(eng.hoist)} fuse={eng.fuse is not None} "
                      f"sharded={getattr(eng, 'sp', None) is not None}", f"latents_sha256 {digest}", ""])


def case_sample(rec, title, case, model, times=1, **opts):
    from tests import smoke_case as SC
    kw = SC.model_kwargs(case.batch, case.cond, DEV)
    kw["attention_mask"] = case.lay
    return sample(rec, title, scheduler(case.steps, **opts), model, case.z, kw, times)


def single_gpu(rec):
    from oracle import restate as R
    from tests import smoke_case as SC
    WU = importlib.import_module("tests.test_weight_updates_gpu")
    FULL2 = importlib.import_module("tests.test_sp_engine_gpu").FULL2
    case = WU.Case(R.TINY, **TINY_CASE)
    model = SC.build_product_model(R.TINY, case.p, DEV)
    for title, opts in (("tiny defaults", {}), ("tiny use_graph=False", dict(use_graph=False)),
                        ("tiny hoist_special_rows=False", dict(hoist_special_rows=False)),
                        ("tiny reuse_condition_prefix=False", dict(reuse_condition_prefix=False)),
                        ("tiny attention fp8", dict(attention_precision="fp8")),
                        ("tiny linear fp8", dict(linear_precision="fp8")),
                        ("tiny attention fp8 + linear fp8", dict(attention_precision="fp8", linear_precision="fp8"))):
        print(case_sample(rec, title, case, model, **opts), flush=True)
    print(case_sample(rec, "tiny cache_engines=True, two clips (the second through rebind)", case, model, times=2,
                      cache_engines=True), flush=True)
    # the inputs of tests/test_model_gpu.py::test_sampler_fast_path: two left-padded rows under a dense 3-D mask
    p, batch, z, cond = SC.build_case(R.TINY)
    m2 = SC.build_product_model(R.TINY, p, DEV)
    for title, pack in (("tiny two left-padded rows, packed", True), ("tiny two left-padded rows, dense mask, pack_padding=False", False)):
        print(sample(rec, title, scheduler(3, pack_padding=pack), m2, z, SC.model_kwargs(batch, cond, DEV)), flush=True)
    del model, m2
    case = WU.Case(FULL2, C=4, G=8, hw=(32, 32), steps=2)
    model = SC.build_product_model(FULL2, case.p, DEV)
    print(case_sample(rec, "full width x 2 layers, defaults (folded norms)", case, model), flush=True)
    print(case_sample(rec, "full width x 2 layers, fuse_norms=False", case, model, fuse_norms=False), flush=True)


def rank_worker(rank, world, port, q):
    try:
        os.dup2(2, 1)       # the report travels through the queue: keep the libraries' chatter on stdout out of it
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.set_num_threads(8)
        importlib.import_module("video-gpt_amd")
        importlib.import_module("video-gpt_amd.scheduler")
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        from oracle import restate as R
        from tests import smoke_case as SC
        WU = importlib.import_module("tests.test_weight_updates_gpu")
        FULL2 = importlib.import_module("tests.test_sp_engine_gpu").FULL2
        rec = Recorder()
        SPM.initialize_sequence_parallel_state(world)
        out = []
        case = WU.Case(R.TINY, **TINY_CASE)
        model = SC.build_product_model(R.TINY, case.p, DEV)
        for title, opts in (("defaults", {}), ("fuse_norms=False", dict(fuse_norms=False)),
                            ("hoist_special_rows=False", dict(hoist_special_rows=False)),
                            ("reuse_condition_prefix=False", dict(reuse_condition_prefix=False))):
            out.append(case_sample(rec, f"rank {rank} of {world}: tiny {title}", case, model, sequence_parallel_engine=True, **opts))
        del model
        case = WU.Case(FULL2, C=4, G=12, hw=(32, 32), steps=2)
        model = SC.build_product_model(FULL2, case.p, DEV)
        out.append(case_sample(rec, f"rank {rank} of {world}: full width x 2 layers, 6144 live rows (folded norms on the shares)",
                               case, model, sequence_parallel_engine=True))
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "\n".join(out)))
    except Exception:
        q.put((rank, "ERROR\n" + traceback.format_exc()))


def two_ranks(world=2, timeout=900):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    try:
        res = dict(q.get(timeout=timeout) for _ in procs)
    finally:
        for p_ in procs:
            p_.join(timeout=120)
            if p_.is_alive():
                p_.kill()
    for r in range(world):
        print(res[r], flush=True)
    if any(res[r].startswith("ERROR") for r in range(world)) or any(p_.exitcode != 0 for p_ in procs):
        raise SystemExit("a rank failed")


def main():
    importlib.import_module("video-gpt_amd")
    importlib.import_module("video-gpt_amd.scheduler")
    single_gpu(Recorder())
    two_ranks()


if __name__ == "__main__":
    main()
