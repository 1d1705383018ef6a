"""The LoRA entry points (include/vgpt.h, "LoRA adapters") without a GPU: header, exports and bindings list the same
symbols, the ABI version did not move, and every host-side refusal returns its documented code before any launch."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
INVALID, UNSUPPORTED = -1, -2
SYMBOLS = ("vgpt_lora_down", "vgpt_lora_up_add", "vgpt_lora_grad", "vgpt_lora_grad_workspace_bytes")


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


def _refused(lib, rc, code, text):
    assert rc == code, (rc, lib.vgpt_last_error())
    assert text in lib.vgpt_last_error(), lib.vgpt_last_error()


def test_header_exports_and_bindings_agree(binding, lib):
    hdr = open(os.path.join(ROOT, "include", "vgpt.h")).read()
    declared = set(re.findall(r"\b(vgpt_lora_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(SYMBOLS)
    assert {n for n in binding.SIGNATURES if n.startswith("vgpt_lora_")} == declared
    assert all(hasattr(lib, n) for n in SYMBOLS)
    assert int(re.search(r"#define VGPT_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.vgpt_abi_version() == 8 and binding.ABI_VERSION == 8


def _down(lib, X=FAKE, S=FAKE, U=FAKE, M=100, K=192, rp=16, ldx=192, tr=0):
    return lib.vgpt_lora_down(X, S, U, M, K, rp, ldx, tr, 1.0, None)


def _up(lib, Y=FAKE, U=FAKE, S=FAKE, cos=None, sin=None, M=100, N=384, rp=16, ldy=384, tr=0, nq=2, nk=1, hd=96):
    return lib.vgpt_lora_up_add(Y, U, S, cos, sin, M, N, rp, ldy, tr, nq, nk, hd, 1.0, None)


def _grad(lib, Y=FAKE, U=FAKE, G=FAKE, M=100, N=192, rp=16, ldy=192, ldu=16, ws=FAKE, ws_bytes=1 << 30):
    return lib.vgpt_lora_grad(Y, U, G, M, N, rp, ldy, ldu, 0, 1.0, ws, ws_bytes, None)


def test_null_pointers(lib):
    for kw in (dict(X=None), dict(S=None), dict(U=None)):
        _refused(lib, _down(lib, **kw), INVALID, b"null pointer")
    for kw in (dict(Y=None), dict(U=None), dict(S=None), dict(cos=FAKE), dict(sin=FAKE)):   # one table without the other
        _refused(lib, _up(lib, **kw), INVALID, b"null pointer")
    for kw in (dict(Y=None), dict(U=None), dict(G=None)):
        _refused(lib, _grad(lib, **kw), INVALID, b"null pointer")


@pytest.mark.parametrize("rp", [0, 8, 24, 80, -16])
def test_padded_rank(lib, rp):
    _refused(lib, _down(lib, rp=rp), UNSUPPORTED, b"padded rank")
    _refused(lib, _up(lib, rp=rp), UNSUPPORTED, b"padded rank")
    _refused(lib, _grad(lib, rp=rp, ldu=96), UNSUPPORTED, b"padded rank")
    assert lib.vgpt_lora_grad_workspace_bytes(7740, 3072, rp) == 0


def test_row_strides_and_widths(lib):
    _refused(lib, _down(lib, ldx=184), INVALID, b"ldx")                 # ld < width
    _refused(lib, _down(lib, ldx=196), INVALID, b"ldx")                 # ld % 8
    _refused(lib, _down(lib, K=196, ldx=200), INVALID, b"multiple of 8")
    _refused(lib, _up(lib, ldy=376), INVALID, b"ldy")
    _refused(lib, _up(lib, ldy=388), INVALID, b"ldy")
    _refused(lib, _up(lib, N=388, ldy=392), INVALID, b"N=388 is not a multiple of 8")
    _refused(lib, _grad(lib, ldy=184), INVALID, b"ldy")
    _refused(lib, _grad(lib, ldy=196), INVALID, b"ldy")
    _refused(lib, _grad(lib, ldu=8), INVALID, b"ldu")
    _refused(lib, _grad(lib, ldu=20), INVALID, b"ldu")
    _refused(lib, _grad(lib, N=196, ldy=200), INVALID, b"N=196 is not a multiple of 8")
    for fn in (_down, _up, _grad):
        _refused(lib, fn(lib, M=0), INVALID, b"bad size")
    _refused(lib, _down(lib, X=FAKE + 8), INVALID, b"16-byte aligned")
    _refused(lib, _up(lib, Y=FAKE + 2), INVALID, b"16-byte aligned")
    _refused(lib, _grad(lib, U=FAKE + 4), INVALID, b"16-byte aligned")


def test_rope_head_layout(lib):
    # N = 384 is (2 + 2 * 1) heads of 96
    _refused(lib, _up(lib, cos=FAKE, sin=FAKE, hd=80), INVALID, b"does not divide the q/k span")
    _refused(lib, _up(lib, cos=FAKE, sin=FAKE, nq=3), INVALID, b"does not divide the q/k span")
    _refused(lib, _up(lib, cos=FAKE, sin=FAKE, nq=0), INVALID, b"bad head counts")
    _refused(lib, _up(lib, cos=FAKE, sin=FAKE, N=4 * 72, ldy=4 * 72, hd=72), UNSUPPORTED, b"head_dim=72")
    _refused(lib, _up(lib, cos=FAKE, sin=FAKE, N=4 * 256, ldy=4 * 256, hd=256), UNSUPPORTED, b"head_dim=256")


def test_grad_workspace(lib):
    need = lib.vgpt_lora_grad_workspace_bytes(7740, 3072, 16)
    assert need > 0 and need % (3072 * 16 * 4) == 0          # whole (N, rp) fp32 slices
    assert lib.vgpt_lora_grad_workspace_bytes(64, 3072, 16) == 0      # one 64-row chunk: nothing to slice
    kw = dict(M=7740, N=3072, ldy=3072)
    _refused(lib, _grad(lib, ws=None, **kw), INVALID, b"workspace")
    _refused(lib, _grad(lib, ws_bytes=need - 4, **kw), INVALID, b"workspace")
    _refused(lib, _grad(lib, ws=FAKE + 4, ws_bytes=need, **kw), INVALID, b"workspace")
