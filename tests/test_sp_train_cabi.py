"""The sharded training step's additions without a GPU: the two re-layout entry points (include/vgpt.h, vgpt_sp_pack_ctx /
vgpt_sp_unpack_qkv_rope) are declared, exported and bound, the ABI version did not move (additions only), their host-side
checks refuse bad calls with the documented codes before any launch, and the trainer's option defaults to off."""
import importlib
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vgpt_sp_pack_ctx", "vgpt_sp_unpack_qkv_rope")


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib


def test_header_exports_and_binding_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vgpt.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(vgpt_[a-z0-9_]+)\s*\(", text))
    cdll = lib.load()
    ops = importlib.import_module("video-gpt_amd.ops")
    for name in NEW:
        assert name in syms and name in lib.SIGNATURES and hasattr(cdll, name)
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[name][1])
        assert callable(getattr(ops, name[len("vgpt_"):]))
    assert not lib.missing_exports()
    # additions only: no exported signature changed, so the version stays where the existing tests pin it
    assert int(re.search(r"#define VGPT_ABI_VERSION (\d+)", text).group(1)) == lib.ABI_VERSION == cdll.vgpt_abi_version() == 8


def test_pack_ctx_checks_arguments_before_launching(lib):
    cdll = lib.load()
    fake = 1 << 20          # 16-byte aligned, never dereferenced: every call below fails its host-side checks first
    rc = cdll.vgpt_sp_pack_ctx(None, fake, 4, 96, 2, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_ctx(fake, None, 4, 96, 2, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_ctx(fake, fake, 4, 0, 2, None)
    assert rc == -1 and b"bad shape" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_ctx(fake, fake, -1, 96, 2, None)
    assert rc == -1 and b"bad shape" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_ctx(fake, fake, 4, 12, 2, None)
    assert rc == -2 and b"multiple of 8" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_ctx(fake + 8, fake, 4, 96, 2, None)
    assert rc == -2 and b"16-byte aligned" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_ctx(fake, fake, 1 << 28, 96, 2, None)
    assert rc == -2 and b"2^31" in cdll.vgpt_last_error()
    assert cdll.vgpt_sp_pack_ctx(fake, fake, 0, 96, 2, None) == 0               # no rows: nothing to launch


def test_unpack_qkv_rope_checks_arguments_before_launching(lib):
    cdll = lib.load()
    fake = 1 << 20
    f = cdll.vgpt_sp_unpack_qkv_rope
    rc = f(None, fake, None, None, 4, 32, 32, 96, 2, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    rc = f(fake, None, fake, fake, 4, 32, 32, 96, 2, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    for cos, sin in ((fake, None), (None, fake)):                               # exactly one table
        rc = f(fake, fake, cos, sin, 4, 32, 32, 96, 2, None)
        assert rc == -1 and b"together" in cdll.vgpt_last_error()
    rc = f(fake, fake, None, None, 4, 32, 32, 96, 3, None)
    assert rc == -1 and b"multiples of n_ranks" in cdll.vgpt_last_error()
    rc = f(fake, fake, None, None, 4, 32, 8, 96, 16, None)
    assert rc == -1 and b"multiples of n_ranks" in cdll.vgpt_last_error()
    rc = f(fake, fake, None, None, -1, 32, 32, 96, 2, None)
    assert rc == -1 and b"bad shape" in cdll.vgpt_last_error()
    rc = f(fake, fake, None, None, 4, 2, 2, 100, 2, None)
    assert rc == -2 and b"multiple of 8" in cdll.vgpt_last_error()
    rc = f(fake, fake, fake, fake, 4, 2, 2, 24, 2, None)                        # copies at hd 24, cannot rotate it
    assert rc == -2 and b"head_dim/2" in cdll.vgpt_last_error()
    rc = f(fake, fake + 8, None, None, 4, 2, 2, 96, 2, None)
    assert rc == -2 and b"16-byte aligned" in cdll.vgpt_last_error()
    rc = f(fake, fake, fake + 4, fake, 4, 2, 2, 96, 2, None)
    assert rc == -2 and b"16-byte aligned" in cdll.vgpt_last_error()
    rc = f(fake, fake, None, None, 1 << 22, 32, 32, 96, 2, None)
    assert rc == -2 and b"2^31" in cdll.vgpt_last_error()
    assert f(fake, fake, None, None, 0, 2, 2, 96, 2, None) == 0                 # no rows: nothing to launch
    assert f(fake, fake, fake, fake, 0, 2, 2, 96, 2, None) == 0


def test_trainer_option_defaults_off():
    TR = importlib.import_module("video-gpt_amd.train")
    sig = inspect.signature(TR.Stage1Trainer.__init__).parameters
    assert sig["sequence_parallel"].default is False and sig["sp_group"].default is None
    assert sig["check_sp_inputs"].default is True


def test_broadcast_batch_is_exported_and_an_identity_without_a_group():
    import sys
    SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
    obj = {"a": [1, 2], "b": (3,)}
    assert SPM.broadcast_batch(obj, 0, None) is obj
    # the drop-in package exports it beside vae_encode (as tests/test_dropin_imports.py puts the package on the path)
    path = os.path.join(ROOT, "video-gpt_amd", "dropin")
    saved = {k: v for k, v in sys.modules.items() if k == "LVM" or k.startswith("LVM.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, path)
    try:
        U = importlib.import_module("LVM.utils")
        assert U.broadcast_batch is SPM.broadcast_batch and callable(U.broadcast_data) and callable(U.vae_encode)
    finally:
        sys.path.remove(path)
        for k in [k for k in sys.modules if k == "LVM" or k.startswith("LVM.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def _broadcast_worker(rank, port, q):
    try:
        import torch
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=2)
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        SPM.initialize_sequence_parallel_state(2)
        obj = {"a": torch.full((3,), float(rank)), "b": [rank, (torch.arange(2) + rank,)], "c": None}
        out = SPM.broadcast_batch(obj, 1)
        q.put((rank, out["a"].tolist(), out["b"][0], out["b"][1][0].tolist(), type(out["b"][1]).__name__, out["c"]))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


def test_broadcast_batch_hands_every_rank_the_source_ranks_object():
    """Two CPU ranks over gloo: nested dicts / lists / tuples / tensors / plain values of global rank 1 arrive on rank 0."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_broadcast_worker, args=(r, port, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    try:
        res = sorted(q.get(timeout=120) for _ in procs)
    finally:
        for p_ in procs:
            p_.join(timeout=60)
            if p_.is_alive():
                p_.kill()
    assert [r[1:] for r in res] == [([1.0, 1.0, 1.0], 1, [1, 2], "tuple", None)] * 2, res
