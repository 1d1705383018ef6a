"""The per-head-dim attention backward entry points (include/vgpt.h: vgpt_attn_blockmask_bwd_hd, vgpt_attn_bwd_supported)
without a GPU: exported, declared and bound; the query answers for the built widths only; bad calls are refused before any
launch with the offending value in vgpt_last_error(); empty problems return 0 without reading anything."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def pkg():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _refused(lib, rc, code, *texts):
    assert rc == code, (rc, lib.vgpt_last_error())
    for text in texts:
        assert text in lib.vgpt_last_error(), lib.vgpt_last_error()


def _strides(L=200, nh=4, nkv=2, hd=64):
    """The 24 strides of ops_train.attention_qkv_bwd as a real int64 array (the host reads them)."""
    width = (nh + 2 * nkv) * hd
    st = [L * width, hd, width] * 3 + [L * nh * hd, hd, nh * hd] * 2 + [L * width, hd, width] * 3
    return (ctypes.c_int64 * 24)(*st)


def _bwd(lib, B=1, L=200, nh=4, nkv=2, hd=64, strides=None, null_at=None, scale=0.1):
    ptrs = [FAKE] * 12
    if null_at is not None:
        ptrs[null_at] = None
    st = _strides(L, nh, nkv, hd if hd % 8 == 0 else 64) if strides is None else strides
    return lib.vgpt_attn_blockmask_bwd_hd(*ptrs, B, L, nh, nkv, hd, st, scale, None)


def test_symbols_are_exported_declared_bound_and_abi_stays_8(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vgpt.h")).read()
    for name in ("vgpt_attn_blockmask_bwd_hd", "vgpt_attn_bwd_supported"):
        assert hasattr(raw, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pkg._lib.SIGNATURES, name
    assert re.search(r"#define\s+VGPT_ABI_VERSION\s+8\b", header)
    assert lib.vgpt_abi_version() == 8
    # the declaration names the reference lines the backward replaces
    decl = header[header.index("vgpt_attn_blockmask_bwd_hd") - 600: header.index("vgpt_attn_blockmask_bwd_hd")]
    assert re.search(r"sdpa_transform\.py:\d+", decl), decl


@pytest.mark.parametrize("hd,want", [(64, 1), (96, 1), (128, 1), (0, 0), (32, 0), (80, 0), (256, 0)])
def test_supported_query(pkg, lib, hd, want):
    assert lib.vgpt_attn_bwd_supported(hd) == want
    T = importlib.import_module("video-gpt_amd.ops_train")
    assert T.attention_bwd_supported(hd) is bool(want)


def test_refuses_other_head_dims_with_the_value(lib):
    _refused(lib, _bwd(lib, hd=80), UNSUPPORTED, b"vgpt_attn_blockmask_bwd_hd", b"head_dim 80 unsupported")
    _refused(lib, _bwd(lib, hd=256), UNSUPPORTED, b"head_dim 256 unsupported")
    _refused(lib, _bwd(lib, hd=0), UNSUPPORTED, b"head_dim 0 unsupported")
    _refused(lib, _bwd(lib, hd=-64), UNSUPPORTED, b"head_dim -64 unsupported")


@pytest.mark.parametrize("hd", [64, 96, 128])
def test_refuses_bad_head_counts_with_the_values(lib, hd):
    _refused(lib, _bwd(lib, hd=hd, nh=3, nkv=2), INVALID, b"bad shape", b"n_heads 3", b"n_kv_heads 2")
    _refused(lib, _bwd(lib, hd=hd, nh=4, nkv=0), INVALID, b"bad shape", b"n_kv_heads 0")
    _refused(lib, _bwd(lib, hd=hd, nh=0, nkv=1), INVALID, b"bad shape", b"n_heads 0")
    _refused(lib, _bwd(lib, hd=hd, B=-1), INVALID, b"bad shape", b"B -1")
    _refused(lib, _bwd(lib, hd=hd, L=-5), INVALID, b"bad shape", b"L -5")
    _refused(lib, _bwd(lib, hd=hd, scale=0.0), INVALID, b"bad shape", b"scale 0")


@pytest.mark.parametrize("hd", [64, 96, 128])
@pytest.mark.parametrize("i,bad", [(0, 12), (2, 8 * 64 + 4), (1, 100), (4, 66), (8, 1028), (10, 4), (14, 390),   # inputs: 8
                                   (15, 6), (17, 98), (19, 130), (20, 1022), (22, 2), (23, 774)])                  # outputs: 4
def test_refuses_each_misaligned_stride_class_with_the_value(lib, hd, i, bad):
    st = _strides(hd=hd)
    st[i] = bad
    _refused(lib, _bwd(lib, hd=hd, strides=st), UNSUPPORTED, b"strides must be multiples of 8", b"stride %d " % i,
             b"is %d" % bad)


def test_outputs_may_be_4_element_aligned_inputs_may_not(lib):
    st = _strides()
    for i in range(15, 24):
        st[i] += 4                       # still multiples of 4: accepted; the call then stops at B == 0
    assert lib.vgpt_attn_blockmask_bwd_hd(*([FAKE] * 12), 0, 200, 4, 2, 64, st, 0.1, None) == 0
    st[3] += 4
    _refused(lib, lib.vgpt_attn_blockmask_bwd_hd(*([FAKE] * 12), 0, 200, 4, 2, 64, st, 0.1, None), UNSUPPORTED,
             b"stride 3 (k, batch)")


@pytest.mark.parametrize("hd", [64, 96, 128])
def test_refuses_null_pointers(lib, hd):
    for i in range(12):
        _refused(lib, _bwd(lib, hd=hd, null_at=i), INVALID, b"vgpt_attn_blockmask_bwd_hd: null pointer")
    rc = lib.vgpt_attn_blockmask_bwd_hd(*([FAKE] * 12), 1, 200, 4, 2, hd, None, 0.1, None)
    _refused(lib, rc, INVALID, b"null pointer")


@pytest.mark.parametrize("hd", [64, 96, 128])
def test_empty_problems_return_ok_without_reading(lib, hd):
    assert _bwd(lib, hd=hd, B=0) == 0
    assert _bwd(lib, hd=hd, L=0) == 0
    assert _bwd(lib, hd=hd, B=0, L=0) == 0


def test_the_96_only_entry_point_keeps_its_refusals(lib):
    st = _strides(hd=96)
    for hd in (64, 128):
        rc = lib.vgpt_attn_blockmask_bwd(*([FAKE] * 12), 1, 200, 4, 2, hd, st, 0.1, None)
        _refused(lib, rc, UNSUPPORTED, b"vgpt_attn_blockmask_bwd: head_dim %d unsupported (96)" % hd)

