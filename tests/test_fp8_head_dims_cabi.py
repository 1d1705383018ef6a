"""The MX-fp8 entry points for 64-, 96- and 128-wide heads (include/vgpt.h: vgpt_attn_fp8_supported,
vgpt_attn_fp8_workspace_bytes_hd, vgpt_attn_fp8_quantize_hd, vgpt_attn_fwd_plan_fp8_hd, vgpt_gemm_mx8_hd) without a GPU: the
header declares them, the library exports them, the ABI version did not move, the workspace size follows the documented record
layout, and every host-side check refuses a bad call before any launch with a message that starts with the entry point's name
and carries the offending value.  EVERY call in this file either fails a host check or returns early: the pointers are fake, a
launch would fault."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vgpt_attn_fp8_supported", "vgpt_attn_fp8_workspace_bytes_hd", "vgpt_attn_fp8_quantize_hd", "vgpt_attn_fwd_plan_fp8_hd",
       "vgpt_gemm_mx8_hd")
FAKE = 1 << 20   # a non-null, 256-byte aligned address that is never dereferenced
INVALID, UNSUPPORTED = -1, -2
HEAD_DIMS = (64, 96, 128)


@pytest.fixture(scope="module")
def L_():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib


@pytest.fixture(scope="module")
def lib(L_):
    return L_.load()


def _refused(lib, rc, code, name, *texts):
    msg = lib.vgpt_last_error()
    assert rc == code, (rc, msg)
    assert msg.startswith(name + b": "), msg
    for t in texts:
        assert t in msg, (t, msg)


def rec_bytes(D):
    """One 64-key tile record: K8 [key][D] | KS [key][4] | V8 [D/32][2][32][32] | VS [D/32][2][32], padded to whole KiB."""
    return (64 * D + 256 + (D // 32) * 2048 + (D // 32) * 64 + 1023) // 1024 * 1024


def a256(n):
    return (n + 255) // 256 * 256


def test_symbols_are_declared_exported_and_the_abi_version_is_8(L_, lib):
    text = open(os.path.join(ROOT, "include", "vgpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = set(re.findall(r"\b(vgpt_[a-z0-9_]+)\s*\(", code))
    for name in NEW:
        assert name in syms and name in L_.SIGNATURES and hasattr(lib, name), name
    assert L_.ABI_VERSION == 8 and lib.vgpt_abi_version() == 8
    assert re.search(r"#define VGPT_ABI_VERSION 8\b", text)
    # the _hd entries take the parameter lists of their namesakes
    for name in NEW[1:]:
        assert L_.SIGNATURES[name] == L_.SIGNATURES[name[:-3]], name
    assert L_.missing_exports() == []


def test_supported_head_dims(lib):
    assert [lib.vgpt_attn_fp8_supported(hd) for hd in (32, 64, 80, 96, 128, 256)] == [0, 1, 0, 1, 1, 0]


def test_record_sizes():
    assert [rec_bytes(D) for D in HEAD_DIMS] == [9 * 1024, 13 * 1024, 17 * 1024]


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_workspace_bytes_follow_the_documented_layout(lib, D):
    ws = lib.vgpt_attn_fp8_workspace_bytes_hd
    for B, L, nh, nkv in ((2, 300, 4, 2), (1, 1, 1, 1), (1, 150, 2, 1), (3, 64, 2, 2), (1, 5248, 32, 8)):
        want = a256(B * nh * L * D) + a256(B * nh * L * 4) + B * nkv * ((L + 63) // 64) * rec_bytes(D)
        assert ws(B, L, nh, nkv, D) == want, (B, L, nh, nkv)
    for args in ((0, 300, 2, 2, D), (-1, 300, 2, 2, D), (1, 0, 2, 2, D), (1, -5, 2, 2, D), (1, 300, 0, 2, D), (1, 300, 2, 0, D),
                 (1, 300, -2, 2, D), (1, 300, 2, -1, D)):
        assert ws(*args) == -1, args
    if D == 96:
        assert ws(2, 300, 4, 2, 96) == lib.vgpt_attn_fp8_workspace_bytes(2, 300, 4, 2, 96)


def test_workspace_bytes_refuse_other_head_dims(lib):
    for hd in (0, 32, 80, 95, 160, 256, -96):
        assert lib.vgpt_attn_fp8_workspace_bytes_hd(1, 300, 2, 2, hd) == -1, hd


def _strides(hd, nh=2, nkv=2, L=300):
    w = (nh + 2 * nkv) * hd
    return dict(q_sb=L * w, q_sh=hd, q_ss=w, k_sb=L * w, k_sh=hd, k_ss=w, v_sb=L * w, v_sh=hd, v_ss=w,
                o_sb=L * nh * hd, o_sh=hd, o_ss=nh * hd)


STRIDE_NAMES = list(_strides(96))


def _quant(lib, q=FAKE, k=FAKE, v=FAKE, ws=FAKE, B=1, L=300, row_begin=0, nh=2, nkv=2, hd=96, scale=0.1, **kw):
    st = _strides(hd)
    st.update(kw)
    return lib.vgpt_attn_fp8_quantize_hd(q, k, v, ws, B, L, row_begin, nh, nkv, hd, *[st[n] for n in STRIDE_NAMES[:9]], scale, None)


def _plan8(lib, ws=FAKE, o=FAKE, bits=FAKE, items=FAKE, isum=FAKE, order=FAKE, n_items=3, B=1, L=300, nh=2, nkv=2, hd=96, **kw):
    st = _strides(hd)
    st.update(kw)
    return lib.vgpt_attn_fwd_plan_fp8_hd(ws, o, bits, items, isum, order, n_items, B, L, nh, nkv, hd, *[st[n] for n in STRIDE_NAMES[9:]],
                                         None)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_quantize_hd_refuses_bad_calls(lib, D):
    name = b"vgpt_attn_fp8_quantize_hd"
    f = lambda **kw: _quant(lib, hd=D, **kw)   # noqa: E731
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(ws=None)):
        _refused(lib, f(**kw), INVALID, name, b"null pointer")
    for hd in (80, 32, 0, 256):
        _refused(lib, _quant(lib, hd=hd), UNSUPPORTED, name, b"head_dim %d unsupported (64, 96, 128)" % hd)
    for kw, text in ((dict(B=0), b"B 0,"), (dict(L=0), b"L 0,"), (dict(L=(1 << 22) + 1), b"L 4194305,"), (dict(nh=0), b"n_heads 0,"),
                     (dict(nkv=0), b"n_kv_heads 0)"), (dict(nh=4, nkv=3), b"n_heads 4, n_kv_heads 3)")):
        _refused(lib, f(**kw), INVALID, name, b"bad shape", text)
    for scale, text in ((0.0, b"got 0)"), (-1.0, b"got -1)")):
        _refused(lib, f(scale=scale), INVALID, name, b"scale must be positive", text)
    for row_begin in (100, 32, 65, -64, 320, 384):
        _refused(lib, f(row_begin=row_begin), INVALID, name, b"row_begin must be a multiple of 64 in [0, L]",
                 b"got %d, L 300" % row_begin)
    assert f(row_begin=256, L=256) == 0                          # nothing left to quantise: OK without a launch
    st = _strides(D)
    for i, n in enumerate(STRIDE_NAMES[:9]):
        _refused(lib, f(**{n: st[n] + 4}), UNSUPPORTED, name, b"strides must be multiples of 8 elements",
                 b"stride %d (%s %s) is %d" % (i, n[:1].encode(), {"sb": b"batch", "sh": b"head", "ss": b"seq"}[n[2:]], st[n] + 4))
    for kw, bad in ((dict(q=FAKE + 8), FAKE + 8), (dict(k=FAKE + 8), FAKE + 8), (dict(v=FAKE + 4), FAKE + 4), (dict(ws=FAKE + 8), FAKE + 8)):
        _refused(lib, f(**kw), UNSUPPORTED, name, b"must be 16-byte aligned", b"%#x" % bad)
    _refused(lib, f(B=4096, L=1 << 22, nh=8, nkv=8), UNSUPPORTED, name, b"problem too large")


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_fwd_plan_fp8_hd_refuses_bad_calls(lib, D):
    name = b"vgpt_attn_fwd_plan_fp8_hd"
    f = lambda **kw: _plan8(lib, hd=D, **kw)   # noqa: E731
    for kw in (dict(ws=None), dict(o=None), dict(bits=None), dict(items=None), dict(isum=None), dict(order=None)):
        _refused(lib, f(**kw), INVALID, name, b"null pointer")
    for hd in (80, 32, 0, 256):
        _refused(lib, _plan8(lib, hd=hd), UNSUPPORTED, name, b"head_dim %d unsupported (64, 96, 128)" % hd)
    for kw, text in ((dict(B=0), b"B 0,"), (dict(L=0), b"L 0,"), (dict(L=(1 << 22) + 1), b"L 4194305,"), (dict(n_items=-1), b"n_items -1,"),
                     (dict(n_items=65536), b"n_items 65536,"), (dict(nh=0), b"n_heads 0,"), (dict(nkv=0), b"n_kv_heads 0)"),
                     (dict(nh=4, nkv=3), b"n_heads 4, n_kv_heads 3)")):
        _refused(lib, f(**kw), INVALID, name, b"bad shape", text)
    st = _strides(D)
    for kw, text in ((dict(o_sb=st["o_sb"] + 2), b"%d" % (st["o_sb"] + 2)), (dict(o_sh=D + 2), b", %d," % (D + 2)),
                     (dict(o_ss=2 * D + 2), b"%d, o" % (2 * D + 2)), (dict(o=FAKE + 4), b"%#x" % (FAKE + 4)),
                     (dict(o=FAKE + 2), b"%#x" % (FAKE + 2))):
        _refused(lib, f(**kw), UNSUPPORTED, name, b"o strides must be multiples of 4 elements, o 8-byte aligned", text)
    assert f(n_items=0) == 0 and f(n_items=0, o_ss=100, o=FAKE + 8) == 0


def _gemm(lib, A=FAKE, W=FAKE, C=FAKE, resid=None, rstd=FAKE, cos=FAKE, sin=FAKE, M=64, N=None, K=64, ldc=None, ldr=0, epi=2, nrot=2,
          hd=96, act=0):
    N = 3 * hd if N is None else N
    ldc = N if ldc is None else ldc
    return lib.vgpt_gemm_mx8_hd(A, W, C, resid, rstd, cos, sin, M, N, K, ldc, ldr, epi, nrot, hd, act, None)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_gemm_mx8_hd_refuses_bad_rope_calls(lib, D):
    name = b"vgpt_gemm_mx8_hd"
    f = lambda **kw: _gemm(lib, hd=D, **kw)   # noqa: E731
    for kw in (dict(A=None), dict(W=None), dict(C=None)):
        _refused(lib, f(**kw), INVALID, name, b"null pointer")
    for kw in (dict(rstd=None), dict(cos=None), dict(sin=None)):
        _refused(lib, f(**kw), INVALID, name, b"null pointer (rstd / cos / sin)")
    for kw, text in ((dict(M=0), b"got 0, %d, 64" % (3 * D)), (dict(N=0), b"got 64, 0, 64"), (dict(K=0), b", 0)"), (dict(K=104), b", 104)"),
                     (dict(K=-64), b", -64)")):
        _refused(lib, f(**kw), INVALID, name, b"K a positive multiple of 32", text)
    _refused(lib, f(N=3 * D + 8, ldc=4 * D), UNSUPPORTED, name, b"N must be a multiple of 32", b"got %d" % (3 * D + 8))
    _refused(lib, f(M=1 << 26), UNSUPPORTED, name, b"problem too large", b"M 67108864")
    for kw, bad in ((dict(A=FAKE + 128), FAKE + 128), (dict(W=FAKE + 16), FAKE + 16), (dict(C=FAKE + 4), FAKE + 4)):
        _refused(lib, f(**kw), UNSUPPORTED, name, b"records 256-byte aligned, C 8-byte aligned", b"%#x" % bad)
    _refused(lib, f(ldc=3 * D + 2), UNSUPPORTED, name, b"ldc a multiple of 4", b"ldc %d" % (3 * D + 2))
    _refused(lib, f(ldc=3 * D - 4), INVALID, name, b"ldc %d < output columns %d" % (3 * D - 4, 3 * D))
    # N is a multiple of 32 but not of the head dim; more rotated heads than N holds; a negative count
    _refused(lib, f(N=3 * D + 32), UNSUPPORTED, name, b"N a multiple of head_dim", b"N %d, head_dim %d" % (3 * D + 32, D))
    _refused(lib, f(nrot=4), UNSUPPORTED, name, b"n_rot_heads * head_dim <= N", b"n_rot_heads 4")
    _refused(lib, f(nrot=-1), UNSUPPORTED, name, b"n_rot_heads -1")
    for kw, bad in ((dict(cos=FAKE + 4), FAKE + 4), (dict(sin=FAKE + 8), FAKE + 8)):
        _refused(lib, f(**kw), UNSUPPORTED, name, b"cos / sin 16-byte aligned", b"%#x" % bad)


def test_gemm_mx8_hd_refuses_other_head_dims_and_epilogues(lib):
    name = b"vgpt_gemm_mx8_hd"
    for hd in (32, 80, 160, 256, 0):
        _refused(lib, _gemm(lib, hd=hd, N=1920, nrot=0), UNSUPPORTED, name, b"head_dim 64, 96 or 128", b"got %d" % hd)
    for epi in (7, -1, 4):
        _refused(lib, _gemm(lib, epi=epi), INVALID, name, b"unknown epilogue %d" % epi)
    # the other three epilogues are vgpt_gemm_mx8 itself: its checks, its messages
    assert _gemm(lib, epi=1, resid=None) == INVALID and b"vgpt_gemm_mx8: null pointer (resid)" in lib.vgpt_last_error()
    assert _gemm(lib, epi=0, K=104) == INVALID and b"vgpt_gemm_mx8: " in lib.vgpt_last_error()
    assert _gemm(lib, epi=3, rstd=None, N=128) == INVALID and b"vgpt_gemm_mx8: null pointer (rstd)" in lib.vgpt_last_error()


def test_old_entry_points_still_refuse_64_and_128(lib):
    """The head_dim 96 entries keep their behaviour: the new widths come through the _hd entries only."""
    for hd in (64, 128):
        assert lib.vgpt_attn_fp8_workspace_bytes(1, 300, 2, 2, hd) == -1
        st = _strides(hd)
        rc = lib.vgpt_attn_fp8_quantize(FAKE, FAKE, FAKE, FAKE, 1, 300, 0, 2, 2, hd, *[st[n] for n in STRIDE_NAMES[:9]], 0.1, None)
        assert rc == UNSUPPORTED and b"vgpt_attn_fp8_quantize: head_dim must be 96" in lib.vgpt_last_error()
        rc = lib.vgpt_attn_fwd_plan_fp8(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 3, 1, 300, 2, 2, hd, *[st[n] for n in STRIDE_NAMES[9:]], None)
        assert rc == UNSUPPORTED and b"vgpt_attn_fwd_plan_fp8: head_dim must be 96" in lib.vgpt_last_error()
    rc = lib.vgpt_gemm_mx8(FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, 64, 256, 64, 256, 256, 2, 2, 128, 0, None)
    assert rc == UNSUPPORTED and b"head_dim 96" in lib.vgpt_last_error()


def test_ops_carry_the_hd_surface():
    """The Python layer: the three _hd functions and the supported set the engine's refusal names."""
    ops = importlib.import_module("video-gpt_amd.ops")
    assert ops.FP8_HEAD_DIMS == HEAD_DIMS
    for n in ("attention_fp8_workspace_hd", "attention_fp8_quantize_hd", "attention_qkv_fp8_hd"):
        assert callable(getattr(ops, n))
