"""The bf16 GEMM entry points (include/vgpt.h: vgpt_gemm_bf16, _tr, _rope, _rope_prenorm, _resid_rstd, vgpt_gated_mlp_act_fwd,
_keep, _prenorm, vgpt_gemm_last_launches) without a GPU: host-side argument checks refuse bad calls before any launch, with
the documented return code and a message in vgpt_last_error(), and a refused call leaves no launch record."""
import ctypes
import importlib
import os

import pytest

FAKE = 1 << 20   # a non-null, 256-byte aligned address that is never dereferenced: every call below fails its checks first
INVALID, UNSUPPORTED = -1, -2
EPI_NONE, EPI_RESID, EPI_BIAS = 0, 1, 2
ACT_SILU = 0


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib.load()


def _refused(lib, rc, code, text):
    assert rc == code, (rc, lib.vgpt_last_error())
    assert text in lib.vgpt_last_error(), lib.vgpt_last_error()
    assert lib.vgpt_gemm_last_launches(None, 0) == 0   # nothing was launched


def _gemm(lib, A=FAKE, W=FAKE, C=FAKE, extra=FAKE, M=300, N=512, K=128, lda=128, ldw=128, ldc=512, ldr=512, epi=EPI_NONE):
    return lib.vgpt_gemm_bf16(A, W, C, extra, M, N, K, lda, ldw, ldc, ldr, epi, None)


def _tr(lib, A=FAKE, W=FAKE, C=FAKE, extra=FAKE, M=304, N=512, K=128, lda=128, ldw=512, ldc=512, ldr=512, epi=EPI_NONE,
        atr=0, wtr=1):
    return lib.vgpt_gemm_bf16_tr(A, W, C, extra, M, N, K, lda, ldw, ldc, ldr, epi, atr, wtr, None)


def _rope(lib, prenorm=False, A=FAKE, W=FAKE, C=FAKE, cos=FAKE, sin=FAKE, rstd=FAKE, M=300, N=512, K=128, lda=128, ldw=128,
          ldc=512, n_rot=4, hd=64):
    if prenorm:
        return lib.vgpt_gemm_bf16_rope_prenorm(A, W, C, cos, sin, rstd, M, N, K, lda, ldw, ldc, n_rot, hd, None)
    return lib.vgpt_gemm_bf16_rope(A, W, C, cos, sin, M, N, K, lda, ldw, ldc, n_rot, hd, None)


def _gated(lib, form="fwd", A=FAKE, W=FAKE, out=FAKE, gu=FAKE, rstd=FAKE, M=300, I=512, K=128, lda=128, ldw=128, ldo=512,
           ld_gu=1024, act=ACT_SILU):
    if form == "keep":
        return lib.vgpt_gated_mlp_act_fwd_keep(A, W, out, gu, M, I, K, lda, ldw, ldo, ld_gu, act, None)
    if form == "prenorm":
        return lib.vgpt_gated_mlp_act_fwd_prenorm(A, W, out, rstd, M, I, K, lda, ldw, ldo, act, None)
    return lib.vgpt_gated_mlp_act_fwd(A, W, out, M, I, K, lda, ldw, ldo, act, None)


def _resid_rstd(lib, A=FAKE, W=FAKE, C=FAKE, resid=FAKE, rstd=FAKE, ws=FAKE, ws_bytes=1 << 30, M=4096, N=4096, K=128, lda=128,
                ldw=128, ldc=4096, ldr=4096, eps=1e-5):
    return lib.vgpt_gemm_bf16_resid_rstd(A, W, C, resid, rstd, ws, ws_bytes, eps, M, N, K, lda, ldw, ldc, ldr, None)


def test_plain_gemm_refuses_bad_calls(lib):
    for K in (100, 63, 65):
        _refused(lib, _gemm(lib, K=K), UNSUPPORTED, b"not a multiple of 64")
    for kw in (dict(N=510), dict(ldc=514), dict(ldr=514, epi=EPI_RESID)):
        _refused(lib, _gemm(lib, **kw), UNSUPPORTED, b"N/ldc/ldr must be multiples of 4")
    assert _gemm(lib, ldr=514, epi=EPI_BIAS, M=0) == 0          # ldr only means something with a residual
    for kw in (dict(lda=132), dict(ldw=132), dict(A=FAKE + 8), dict(W=FAKE + 8), dict(C=FAKE + 4)):
        _refused(lib, _gemm(lib, **kw), UNSUPPORTED, b"16-byte aligned rows")
    for epi in (EPI_RESID, EPI_BIAS):
        _refused(lib, _gemm(lib, extra=None, epi=epi), INVALID, b"epilogue needs `extra`")
    for epi in (3, -1):
        _refused(lib, _gemm(lib, epi=epi), INVALID, b"unknown epilogue")
    for kw in (dict(A=None), dict(W=None), dict(C=None)):
        _refused(lib, _gemm(lib, **kw), INVALID, b"null pointer")
    for kw in (dict(M=-1), dict(N=0), dict(K=0)):
        _refused(lib, _gemm(lib, **kw), INVALID, b"bad shape")
    _refused(lib, _gemm(lib, M=1 << 30), UNSUPPORTED, b"dimension too large")


def test_transposed_gemm_refuses_bad_calls(lib):
    _refused(lib, _tr(lib, atr=1, wtr=0), UNSUPPORTED, b"a transposed A needs a transposed W")
    for kw in (dict(N=508), dict(N=4), dict(M=300, atr=1), dict(M=4, atr=1)):
        _refused(lib, _tr(lib, **kw), UNSUPPORTED, b"must be a multiple of 8")
    _refused(lib, _tr(lib, K=100), UNSUPPORTED, b"must be a multiple of 64 unless both operands are transposed")
    for kw in (dict(ldc=514), dict(ldr=514, epi=EPI_RESID)):
        _refused(lib, _tr(lib, **kw), UNSUPPORTED, b"ldc/ldr must be multiples of 4")
    for kw in (dict(lda=132), dict(ldw=516), dict(A=FAKE + 8), dict(W=FAKE + 8), dict(C=FAKE + 4)):
        _refused(lib, _tr(lib, **kw), UNSUPPORTED, b"16-byte aligned rows")
    _refused(lib, _tr(lib, extra=None, epi=EPI_RESID), INVALID, b"epilogue needs `extra`")
    _refused(lib, _tr(lib, epi=7), INVALID, b"unknown epilogue")
    _refused(lib, _tr(lib, C=None), INVALID, b"null pointer")
    _refused(lib, _tr(lib, K=1 << 20, ldw=1 << 12), UNSUPPORTED, b"dimension too large")
    # neither operand transposed: the plain entry point's rules and its messages
    _refused(lib, _tr(lib, wtr=0, K=100), UNSUPPORTED, b"vgpt_gemm_bf16: K=100 not a multiple of 64")


@pytest.mark.parametrize("prenorm", [False, True], ids=["rope", "rope_prenorm"])
def test_rope_gemm_refuses_bad_calls(lib, prenorm):
    r = lambda **kw: _rope(lib, prenorm, **kw)
    for hd in (40, 72, 100):
        _refused(lib, r(hd=hd, n_rot=1), UNSUPPORTED, b"must be a multiple of 16 and the rotated heads must fit in N")
    _refused(lib, r(hd=64, n_rot=9), UNSUPPORTED, b"the rotated heads must fit in N")
    for N in (520, 516):
        _refused(lib, r(N=N, ldc=N), UNSUPPORTED, b"N must be a multiple of 16")
    _refused(lib, r(ldc=514), UNSUPPORTED, b"ldc of 4")
    _refused(lib, r(K=96), UNSUPPORTED, b"not a multiple of 64")
    for kw in (dict(lda=132), dict(ldw=132), dict(A=FAKE + 8), dict(W=FAKE + 8), dict(C=FAKE + 4), dict(cos=FAKE + 4),
               dict(sin=FAKE + 8)):
        _refused(lib, r(**kw), UNSUPPORTED, b"16-byte aligned rows")
    for kw in (dict(A=None), dict(cos=None), dict(sin=None)):
        _refused(lib, r(**kw), INVALID, b"null pointer")
    for kw in (dict(n_rot=0), dict(hd=0), dict(N=0)):
        _refused(lib, r(**kw), INVALID, b"bad shape")
    if prenorm:
        _refused(lib, r(rstd=None), INVALID, b"needs the rows' 1 / rms")


@pytest.mark.parametrize("form", ["fwd", "keep", "prenorm"])
def test_gated_mlp_refuses_bad_calls(lib, form):
    f = lambda **kw: _gated(lib, form, **kw)
    for I in (8, 24, 520):
        _refused(lib, f(I=I, ld_gu=2 * I), UNSUPPORTED, b"I must be a multiple of 16, ldo of 4")
    _refused(lib, f(ldo=514), UNSUPPORTED, b"I must be a multiple of 16, ldo of 4")
    _refused(lib, f(K=100), UNSUPPORTED, b"not a multiple of 64")
    for act in (3, -1, 17):
        _refused(lib, f(act=act), INVALID, b"unknown activation")
    for kw in (dict(lda=132), dict(ldw=132), dict(A=FAKE + 8), dict(W=FAKE + 8), dict(out=FAKE + 4)):
        _refused(lib, f(**kw), UNSUPPORTED, b"16-byte aligned rows")
    for kw in (dict(A=None), dict(W=None), dict(out=None)):
        _refused(lib, f(**kw), INVALID, b"null pointer")
    if form == "keep":
        for kw in (dict(ld_gu=1020), dict(ld_gu=1026), dict(gu=None), dict(gu=FAKE + 4)):
            _refused(lib, f(**kw), INVALID, b"gate_up_out must be an 8-byte aligned (M, >= 2I) buffer")
    if form == "prenorm":
        _refused(lib, f(rstd=None), INVALID, b"needs the rows' 1 / rms")


def test_resid_rstd_refuses_bad_calls(lib):
    need = lib.vgpt_gemm_norm_workspace_bytes(4096, 4096, 128)
    assert need > 0 and need % 4 == 0
    _refused(lib, _resid_rstd(lib, ws_bytes=need - 1), INVALID, b"workspace too small or not 256-byte aligned")
    _refused(lib, _resid_rstd(lib, ws_bytes=0), INVALID, b"workspace too small or not 256-byte aligned")
    _refused(lib, _resid_rstd(lib, ws=FAKE + 128), INVALID, b"workspace too small or not 256-byte aligned")
    for kw in (dict(K=100), dict(N=4090, ldc=4096), dict(ldc=4098), dict(ldr=4098), dict(lda=132), dict(ldw=132),
               dict(A=FAKE + 8), dict(C=FAKE + 4), dict(resid=FAKE + 4), dict(eps=-1.0)):
        _refused(lib, _resid_rstd(lib, **kw), UNSUPPORTED, b"shape / alignment as vgpt_gemm_bf16")
    for kw in (dict(resid=None), dict(rstd=None), dict(ws=None)):
        _refused(lib, _resid_rstd(lib, **kw), INVALID, b"null pointer")
    # it always runs the four-wave kernel: strides that kernel's 32-bit offsets cannot reach are refused, not rerouted
    for kw in (dict(ldc=1 << 21), dict(ldr=1 << 21), dict(lda=1 << 22), dict(ldw=1 << 19)):
        _refused(lib, _resid_rstd(lib, **kw), UNSUPPORTED, b"row strides beyond the four-wave kernel's offset range")
    assert _resid_rstd(lib, ldc=(1 << 21) - 4, ldr=(1 << 21) - 4, M=0) == 0
    # shapes the four-wave kernel does not take report no workspace and are refused: a grid under 128 tiles, one k-tile
    assert lib.vgpt_gemm_norm_workspace_bytes(300, 512, 256) == 0
    _refused(lib, _resid_rstd(lib, M=300, N=512, ldc=512, ldr=512), UNSUPPORTED, b"not a shape of the four-wave kernel")
    assert lib.vgpt_gemm_norm_workspace_bytes(4096, 4096, 64) == 0
    _refused(lib, _resid_rstd(lib, K=64), UNSUPPORTED, b"not a shape of the four-wave kernel")


def test_no_rows_is_ok_and_touches_nothing(lib):
    """M == 0 returns OK before anything is read or launched: every pointer here is fake, and the launch record stays empty."""
    assert _gemm(lib, M=0, epi=EPI_RESID) == 0
    assert lib.vgpt_gemm_last_launches(None, 0) == 0
    assert _tr(lib, M=0) == 0 and _tr(lib, M=0, atr=1) == 0      # no rows: the width rule of a transposed A has nothing to check
    assert _rope(lib, M=0) == 0 and _rope(lib, True, M=0) == 0
    assert _rope(lib, M=0, A=None, W=None, C=None, cos=None, sin=None) == 0
    for form in ("fwd", "keep", "prenorm"):
        assert _gated(lib, form, M=0) == 0
    assert _resid_rstd(lib, M=0) == 0
    assert lib.vgpt_gemm_last_launches(None, 0) == 0


def test_last_launches_with_no_room(lib):
    """cap 0 writes nothing (a null or a real buffer alike) and still reports the count; a negative cap is no room either."""
    assert _gemm(lib, K=100) == UNSUPPORTED
    buf = (ctypes.c_int32 * 12)(*([-7] * 12))
    assert lib.vgpt_gemm_last_launches(None, 0) == 0
    assert lib.vgpt_gemm_last_launches(buf, 0) == 0
    assert lib.vgpt_gemm_last_launches(buf, -3) == 0
    assert lib.vgpt_gemm_last_launches(None, 2) == 0
    assert list(buf) == [-7] * 12
