"""The training entry points (include/vgpt.h, "stage-1 pre-training step") without a GPU: host-side argument checks refuse
bad calls before any launch, with the documented return code and a message in vgpt_last_error()."""
import ctypes
import importlib
import os

import pytest

FAKE = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
INVALID, UNSUPPORTED = -1, -2


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


def _attn_strides(L=200, nh=4, nkv=2, hd=96):
    """The 24 strides of ops_train.attention_qkv_bwd (fused qkv rows, (B, L, nh*hd) out / dout) as a real int64 array:
    the host reads them, so they are never a fake pointer."""
    width = (nh + 2 * nkv) * hd
    st = [L * width, hd, width] * 3 + [L * nh * hd, hd, nh * hd] * 2 + [L * width, hd, width] * 3
    return (ctypes.c_int64 * 24)(*st)


def _attn_bwd(lib, B=1, L=200, nh=4, nkv=2, hd=96, strides=None, null_at=None):
    ptrs = [FAKE] * 12
    if null_at is not None:
        ptrs[null_at] = None
    st = _attn_strides(L, nh, nkv, 96) if strides is None else strides
    return lib.vgpt_attn_blockmask_bwd(*ptrs, B, L, nh, nkv, hd, st, 0.1, None)


def test_attention_backward_refuses_bad_calls(lib):
    _refused(lib, _attn_bwd(lib, hd=64), UNSUPPORTED, b"head_dim 64 unsupported")
    _refused(lib, _attn_bwd(lib, hd=128), UNSUPPORTED, b"head_dim 128 unsupported")
    _refused(lib, _attn_bwd(lib, nh=3, nkv=2), INVALID, b"bad shape")
    _refused(lib, _attn_bwd(lib, nh=4, nkv=0), INVALID, b"bad shape")
    for i, bad in ((2, 8 * 96 + 4), (1, 100), (14, 390), (17, 98), (23, 774)):   # input rows / output rows
        st = _attn_strides()
        st[i] = bad
        _refused(lib, _attn_bwd(lib, strides=st), UNSUPPORTED, b"strides must be multiples of 8")
    for i in (0, 6, 11):
        _refused(lib, _attn_bwd(lib, null_at=i), INVALID, b"null pointer")
    rc = lib.vgpt_attn_blockmask_bwd(*([FAKE] * 12), 1, 200, 4, 2, 96, None, 0.1, None)
    _refused(lib, rc, INVALID, b"null pointer")


@pytest.mark.parametrize("H", [4104, 8192, 196, 4])
def test_row_kernels_refuse_widths_they_were_not_built_for(lib, H):
    rc = lib.vgpt_rmsnorm_bwd(FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, 16, H, 1e-5, None)
    _refused(lib, rc, UNSUPPORTED, b"H must be a multiple of 8 and <= 4096")
    rc = lib.vgpt_ln_mod_fwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 16, H, 1e-6, None)
    _refused(lib, rc, UNSUPPORTED, b"vgpt_ln_mod_fwd: bad shape")
    rc = lib.vgpt_ln_mod_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 16, H, None)
    _refused(lib, rc, UNSUPPORTED, b"vgpt_ln_mod_bwd: bad shape")
    if H % 8:
        _refused(lib, lib.vgpt_gather_rows(FAKE, FAKE, FAKE, 3, 2, H, None), INVALID, b"vgpt_gather_rows: bad argument")


def test_row_kernels_refuse_null_pointers(lib):
    rc = lib.vgpt_rmsnorm_bwd(FAKE, FAKE, FAKE, None, FAKE, FAKE, None, 16, 192, 1e-5, None)   # no rstd workspace
    _refused(lib, rc, INVALID, b"null pointer")
    rc = lib.vgpt_ln_mod_bwd(FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, 2, 16, 192, None)       # no dst_row
    _refused(lib, rc, INVALID, b"null pointer")
    rc = lib.vgpt_ln_mod_fwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 0, 192, 1e-6, None)        # ntok 0
    _refused(lib, rc, UNSUPPORTED, b"bad shape")


def _adamw(lib, master=FAKE, param=FAKE, grad=FAKE, grad_f32=0, m=FAKE, v=FAKE, n=1000, step=1):
    return lib.vgpt_adamw_step(master, param, grad, grad_f32, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.1, step, None, None)


def test_adamw_refuses_misaligned_buffers_and_step_zero(lib):
    for kw in (dict(master=FAKE + 4), dict(m=FAKE + 8), dict(v=FAKE + 12), dict(param=FAKE + 2), dict(grad=FAKE + 6),
               dict(grad=FAKE + 8, grad_f32=1)):   # an fp32 gradient is read 16 bytes at a time, a bf16 one 8
        _refused(lib, _adamw(lib, **kw), UNSUPPORTED, b"aligned")
    _refused(lib, _adamw(lib, step=0), INVALID, b"bad argument")
    _refused(lib, _adamw(lib, step=-3), INVALID, b"bad argument")
    _refused(lib, _adamw(lib, n=-1), INVALID, b"bad argument")
    _refused(lib, _adamw(lib, m=None), INVALID, b"null pointer")
    assert _adamw(lib, master=FAKE + 4, n=0) == 0   # n == 0: nothing to do, nothing read


def test_patch_kernels_refuse_other_layouts(lib):
    for C, h, w in ((3, 8, 8), (8, 8, 8), (4, 5, 8), (4, 8, 7)):
        _refused(lib, lib.vgpt_patchify(FAKE, FAKE, 2, C, h, w, None), INVALID, b"vgpt_patchify: bad argument")
        _refused(lib, lib.vgpt_unpatchify_bwd(FAKE, FAKE, 2, C, h, w, None), INVALID, b"vgpt_unpatchify_bwd: bad argument")


def test_gather_rows_refuses_bad_segments(lib):
    _refused(lib, lib.vgpt_gather_rows(FAKE, FAKE, FAKE, 3, 0, 64, None), INVALID, b"bad argument")
    _refused(lib, lib.vgpt_gather_rows(FAKE, FAKE, FAKE, -1, 2, 64, None), INVALID, b"bad argument")
    _refused(lib, lib.vgpt_gather_rows(FAKE, None, FAKE, 3, 2, 64, None), INVALID, b"bad argument")
