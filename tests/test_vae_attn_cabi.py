"""vgpt_vae_attn_fwd (include/vgpt.h, fused mid-block attention of the VAE) without a GPU: the symbol is exported and bound,
the ABI version is unchanged, and the host-side checks refuse every bad call before any launch with the documented return
code and the offending value in vgpt_last_error()."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # non-null, 16-byte aligned addresses that are never dereferenced: every call below returns before a launch
Q, K, V, O = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE
OK, INVALID, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def binding():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib


@pytest.fixture(scope="module")
def lib(binding):
    return binding.load()


def _call(lib, q=Q, k=K, v=V, o=O, N=1, C=64, HW=16, ld=None, bs=None, scale=0.125):
    ld = HW if ld is None else ld
    bs = max(C, 0) * ld if bs is None else bs
    return lib.vgpt_vae_attn_fwd(q, k, v, o, N, C, HW, ld, bs, scale, None)


def _refused(lib, rc, code, *texts):
    msg = lib.vgpt_last_error()
    assert rc == code, (rc, msg)
    for t in texts:
        assert t in msg, msg


def test_symbol_is_exported_declared_and_bound(binding, lib):
    assert hasattr(lib, "vgpt_vae_attn_fwd")
    assert "vgpt_vae_attn_fwd" in binding.SIGNATURES and len(binding.SIGNATURES["vgpt_vae_attn_fwd"][1]) == 11
    hdr = open(os.path.join(ROOT, "include", "vgpt.h")).read()
    assert re.search(r"\bint vgpt_vae_attn_fwd\(const float\* q, const float\* k, const float\* v, float\* o,", hdr)
    for name in ("VGPT_VAE_ATTN_TQ", "VGPT_VAE_ATTN_TK", "VGPT_VAE_ATTN_MAX_C"):
        assert re.search(rf"#define {name} \d+", hdr), name


def test_abi_version_is_still_8(binding, lib):
    assert lib.vgpt_abi_version() == 8 == binding.ABI_VERSION


@pytest.mark.parametrize("which", ["q", "k", "v", "o"])
def test_null_pointer(lib, which):
    _refused(lib, _call(lib, **{which: None}), INVALID, b"vgpt_vae_attn_fwd", b"null pointer")


def test_bad_sizes_are_invalid_and_name_the_value(lib):
    _refused(lib, _call(lib, N=-3), INVALID, b"N = -3")
    _refused(lib, _call(lib, HW=0), INVALID, b"HW = 0")
    _refused(lib, _call(lib, HW=-7, ld=8), INVALID, b"HW = -7")
    _refused(lib, _call(lib, HW=25, ld=24), INVALID, b"ld = 24", b"HW = 25")
    _refused(lib, _call(lib, C=128, HW=25, ld=28, bs=128 * 28 - 1), INVALID, b"batch_stride = 3583", b"3584")
    _refused(lib, _call(lib, scale=0.0), INVALID, b"scale = 0")
    _refused(lib, _call(lib, scale=-0.5), INVALID, b"scale = -0.5")


@pytest.mark.parametrize("C", [0, 32, 96, 576, 1024])
def test_unsupported_channel_counts(lib, C):
    _refused(lib, _call(lib, C=C, bs=4096 * 16), UNSUPPORTED, b"C = %d" % C)
    _refused(lib, _call(lib, C=C, bs=4096 * 16, N=0), UNSUPPORTED, b"C = %d" % C)


@pytest.mark.parametrize("C", [64, 128, 512])
def test_supported_channel_counts_pass_the_channel_check(lib, C):
    """N = 0 returns VGPT_OK without a launch once every check has passed, so it shows that C was accepted; a bad stride
    behind an accepted C is refused for the stride."""
    assert _call(lib, C=C, N=0) == OK
    assert _call(lib, C=C, N=0, HW=25, ld=28, bs=C * 28 + 5) == OK
    _refused(lib, _call(lib, C=C, bs=C * 16 - 1), INVALID, b"batch_stride")


@pytest.mark.parametrize("which", ["q", "k", "v"])
def test_output_aliasing_an_input(lib, which):
    C, HW = 64, 16
    _refused(lib, _call(lib, o={"q": Q, "k": K, "v": V}[which]), INVALID, b"overlaps an input")
    # partial overlap: o starts inside the input's last row / the input starts inside o
    inside = {"q": Q, "k": K, "v": V}[which] + 4 * (C * HW - 1)
    _refused(lib, _call(lib, o=inside), INVALID, b"overlaps an input")
    _refused(lib, _call(lib, **{which: O + 4 * (C * HW - 1)}), INVALID, b"overlaps an input")
    # inputs may alias each other
    assert _call(lib, q=Q, k=Q, v=Q, N=0) == OK
