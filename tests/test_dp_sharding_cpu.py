"""Stage1Trainer(dp_sharding="optimizer") without a GPU: the bucket partition, the host-staged reduce-scatter and all-gather
of sequence_parallel.py over gloo on CPU tensors (world 2 and 8), and the C ABI of the n-partial vgpt_clip_coef."""
import ctypes
import importlib
import os
import re
import socket

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_partition_tiles_the_padded_bucket(world):
    TR = importlib.import_module("video-gpt_amd.train")
    g = world * TR.SHARD_GRANULE
    for n in sorted({1, 255, 256, g - 1, g, g + 1, 3 * g + 5, 442368, 1000003}):
        padded, s = TR.shard_partition(n, world)
        if world == 1:
            assert (padded, s) == (n, n)                      # one rank: no padding, the whole bucket is the shard
            continue
        assert padded % g == 0 and n <= padded < n + g       # the smallest multiple of P * 256 that holds the bucket
        assert s * world == padded and s % TR.SHARD_GRANULE == 0
        bounds = [(r * s, (r + 1) * s) for r in range(world)]
        assert bounds[0][0] == 0 and bounds[-1][1] == padded
        assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))   # contiguous, disjoint, covering
        assert all((lo * 2) % 16 == 0 and (lo * 4) % 16 == 0 for lo, _ in bounds)   # bf16 / fp32 shards 16-byte aligned


def test_partition_refuses_bad_input():
    TR = importlib.import_module("video-gpt_amd.train")
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    for n, w in ((-1, 2), (10, 0)):
        with pytest.raises(VgptError):
            TR.shard_partition(n, w)


# ---- the exchange helpers over gloo with CPU tensors: reduce-scatter + all-gather == all-reduce ----
def _exchange_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    SP = importlib.import_module("video-gpt_amd.sequence_parallel")
    TR = importlib.import_module("video-gpt_amd.train")
    group = dist.group.WORLD
    out = []
    for dtype in (torch.bfloat16, torch.float32):
        for n in (1, 700, 4099, world * 256):
            padded, s = TR.shard_partition(n, world)
            gen = torch.Generator().manual_seed(1000 * rank + n)
            buf = torch.zeros(padded, dtype=dtype)
            # integer values, |partial sums| <= 8 * 16 = 128: exact in bf16 whatever the order of the additions
            buf[:n] = torch.randint(-16, 17, (n,), generator=gen).to(dtype)
            mine_before = buf.clone()
            ref = buf.clone()
            dist.all_reduce(ref)
            lo, hi = rank * s, (rank + 1) * s
            got = SP.reduce_scatter_flat(buf, group)
            in_place = got.data_ptr() == buf[lo:hi].data_ptr()
            reduced = torch.equal(buf[lo:hi], ref[lo:hi])
            rest_kept = torch.equal(buf[:lo], mine_before[:lo]) and torch.equal(buf[hi:], mine_before[hi:])
            SP.all_gather_flat(buf[lo:hi], group, out=buf)
            gathered = torch.equal(buf, ref)
            out.append((str(dtype), n, in_place, reduced, rest_kept, gathered))
    # the list form of all_gather_flat (the sharded sampler engine's call) is unchanged: row i from rank i
    x = torch.full((5,), float(rank), dtype=torch.bfloat16)
    every = SP.all_gather_flat(x, group)
    out.append(("stack", tuple(every.shape) == (world, 5), torch.equal(every[:, 0].float(), torch.arange(world).float())))
    # async_op on a host-staged transport: finished before returning, no handle
    b = torch.ones(world * 256)
    h = SP.reduce_scatter_flat(b, group, async_op=True)
    out.append(("async", h is None, bool((b[rank * 256:(rank + 1) * 256] == world).all())))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 8])
def test_reduce_scatter_then_all_gather_equals_all_reduce(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=180) for _ in procs), key=lambda x: x[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert [p.exitcode for p in procs] == [0] * world
    for rank, out in res:
        for rec in out:
            assert all(v for v in rec if isinstance(v, bool)), (rank, rec)


# ---- C ABI of the changed vgpt_clip_coef ----
@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib


def test_clip_coef_header_export_and_binding_agree(lib):
    from ctypes import c_float, c_int, c_void_p
    hdr = open(os.path.join(ROOT, "include", "vgpt.h")).read()
    assert int(re.search(r"#define VGPT_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION == 8
    decl = re.search(r"int vgpt_clip_coef\(([^)]*)\);", hdr).group(1)
    types = [re.sub(r"\s+", "", re.sub(r"\w+$", "", a.strip())) for a in decl.split(",")]
    assert types == ["constfloat*", "int", "float*", "float*", "float", "float", "void*"], types
    assert lib.SIGNATURES["vgpt_clip_coef"] == (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_float, c_float, c_void_p])
    cdll = lib.load()
    assert cdll.vgpt_abi_version() == 8 and hasattr(cdll, "vgpt_clip_coef")


def test_clip_coef_refuses_bad_arguments_before_any_launch(lib):
    """Checked on the host before the launch: VGPT_ERR_INVALID (-1) for n < 1 and for a null sumsq / coef."""
    cdll = lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    for n in (0, -3):
        assert cdll.vgpt_clip_coef(p, n, p, None, 1.0, 1.0, None) == -1
        assert b"n must be >= 1" in cdll.vgpt_last_error()
    assert cdll.vgpt_clip_coef(None, 1, p, None, 1.0, 1.0, None) == -1
    assert b"null pointer" in cdll.vgpt_last_error()
    assert cdll.vgpt_clip_coef(p, 1, None, None, 1.0, 1.0, None) == -1
    assert b"null pointer" in cdll.vgpt_last_error()


def test_clip_coef_wrapper_refuses_host_tensors():
    """ops_train.clip_coef reads n from the tensor and only passes device memory to the library."""
    T = importlib.import_module("video-gpt_amd.ops_train")
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    with pytest.raises(VgptError, match="GPU tensor"):
        T.clip_coef(torch.zeros(3), torch.zeros(1), None, 1.0)
