"""The Ulysses re-layout entry points of the sharded sampler engine (include/vgpt.h, vgpt_sp_pack_qkv / vgpt_sp_unpack_ctx)
without a GPU: the header declares them, the library exports them, the binding types them, host-side argument checks
refuse bad calls with the documented codes before any launch; the row shares and the engine's option checks."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vgpt_sp_pack_qkv", "vgpt_sp_unpack_ctx")


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
    for name in NEW:
        assert name in syms and name in lib.SIGNATURES and hasattr(cdll, name)
    # argument counts of the declarations == the binding's
    for name in NEW:
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[name][1])
    assert int(re.search(r"#define VGPT_ABI_VERSION (\d+)", text).group(1)) == lib.ABI_VERSION == cdll.vgpt_abi_version()


def test_pack_and_unpack_check_arguments_before_launching(lib):
    cdll = lib.load()
    fake = 1 << 20          # 16-byte aligned, never dereferenced: every call below fails its host-side checks first
    rc = cdll.vgpt_sp_pack_qkv(None, fake, 4, 32, 32, 96, 2, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_qkv(fake, fake, 4, 32, 32, 96, 3, None)
    assert rc == -1 and b"multiples of n_ranks" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_qkv(fake, fake, 4, 32, 8, 96, 16, None)
    assert rc == -1 and b"multiples of n_ranks" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_qkv(fake, fake, -1, 32, 32, 96, 2, None)
    assert rc == -1 and b"bad shape" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_qkv(fake, fake, 4, 2, 2, 100, 2, None)
    assert rc == -2 and b"multiple of 8" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_pack_qkv(fake + 8, fake, 4, 2, 2, 96, 2, None)
    assert rc == -2 and b"16-byte aligned" in cdll.vgpt_last_error()
    assert cdll.vgpt_sp_pack_qkv(fake, fake, 0, 2, 2, 96, 2, None) == 0         # no rows: nothing to launch
    rc = cdll.vgpt_sp_unpack_ctx(fake, None, 4, 96, 2, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_unpack_ctx(fake, fake, 4, 0, 2, None)
    assert rc == -1 and b"bad shape" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_unpack_ctx(fake, fake, 4, 12, 2, None)
    assert rc == -2 and b"multiple of 8" in cdll.vgpt_last_error()
    rc = cdll.vgpt_sp_unpack_ctx(fake, fake + 2, 4, 96, 2, None)
    assert rc == -2 and b"16-byte aligned" in cdll.vgpt_last_error()
    assert cdll.vgpt_sp_unpack_ctx(fake, fake, 0, 96, 2, None) == 0


def test_row_shares():
    E = importlib.import_module("video-gpt_amd.engine")
    # cfg-2-like live rows: whole 256-row tiles per rank
    shares, cut = E.sp_shares(3584, 2)
    assert cut == 256 and shares == [(0, 1792), (1792, 3584)]
    shares, cut = E.sp_shares(3000, 4)
    assert cut == 256 and shares == [(0, 768), (768, 1536), (1536, 2304), (2304, 3000)]
    # too few rows for 256-row shares on every rank: a finer cut
    shares, cut = E.sp_shares(260, 2)
    assert cut == 16 and shares == [(0, 144), (144, 260)]
    shares, cut = E.sp_shares(256, 2)                       # the tiny sampler's live rows
    assert cut == 64 and shares == [(0, 128), (128, 256)]
    shares, cut = E.sp_shares(10, 4)
    assert cut == 1 and shares == [(0, 3), (3, 6), (6, 8), (8, 10)]
    for M in (5, 17, 255, 256, 1000, 20000):
        for P in (1, 2, 4, 8):
            if M < P:
                continue
            shares, cut = E.sp_shares(M, P)
            assert shares[0][0] == 0 and shares[-1][1] == M
            assert all(a < b for a, b in shares) and all(s[1] == t[0] for s, t in zip(shares, shares[1:]))
            assert max(b - a for a, b in shares) <= -(-(-(-M // P)) // cut) * cut
    with pytest.raises(Exception, match="cannot be shared"):
        E.sp_shares(3, 4)


def test_scheduler_option_defaults_off():
    S = importlib.import_module("video-gpt_amd.scheduler")
    PL = importlib.import_module("video-gpt_amd.pipeline")
    assert S.LVMScheduler(num_steps=2).sequence_parallel_engine is False
    assert PL.LVMPipeline.__init__.__code__.co_names.count("sequence_parallel_engine") == 1
