"""The VAE entry points (include/vgpt.h -> csrc/vae.hip) without a GPU: host-side argument checks refuse bad calls
before any launch, with the documented return code and a message in vgpt_last_error(); empty batches return VGPT_OK
without touching a pointer; the packed-weight sizes follow their documented formulas."""
import importlib
import os

import pytest

FAKE = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before a launch
OK, INVALID, UNSUPPORTED = 0, -1, -2


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


def _conv(lib, x=FAKE, w=FAKE, y=FAKE, stats=None, gamma=None, beta=None, N=1, Cin=8, H=4, W=4, Cout=8, ksize=3, stride=1,
          up=0, groups=0):
    return lib.vgpt_conv2d_fwd(x, w, None, None, stats, gamma, beta, y, N, Cin, H, W, Cout, ksize, stride, up, groups, 0, 0,
                               Cin * ksize * ksize, 0, None)


def test_conv2d_refuses_bad_calls(lib):
    only = b"only 3x3 (stride 1, 2) and 1x1 convolutions"
    _refused(lib, _conv(lib, ksize=2), UNSUPPORTED, only)
    _refused(lib, _conv(lib, ksize=5), UNSUPPORTED, only)
    _refused(lib, _conv(lib, ksize=1, stride=2), UNSUPPORTED, only)
    _refused(lib, _conv(lib, ksize=3, stride=3), UNSUPPORTED, only)
    _refused(lib, _conv(lib, stride=2, up=1), UNSUPPORTED, b"upsample needs stride 1")
    gn = b"GroupNorm prologue needs stats/gamma/beta and Cin % groups == 0"
    _refused(lib, _conv(lib, groups=4), INVALID, gn)                                          # no stats / gamma / beta
    _refused(lib, _conv(lib, groups=4, stats=FAKE, gamma=FAKE), INVALID, gn)                  # no beta
    _refused(lib, _conv(lib, groups=3, stats=FAKE, gamma=FAKE, beta=FAKE), INVALID, gn)       # 8 % 3
    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        _refused(lib, _conv(lib, **kw), INVALID, b"vgpt_conv2d_fwd: null pointer")
    for kw in (dict(N=-1), dict(Cin=0), dict(H=0), dict(W=-4), dict(Cout=0)):
        _refused(lib, _conv(lib, **kw), INVALID, b"vgpt_conv2d_fwd: bad shape")


def _bx3(lib, x=FAKE, packed=FAKE, y=FAKE, stats=None, N=1, Cin=16, H=4, W=4, Cout=8, groups=0):
    return lib.vgpt_conv2d_bx3_fwd(x, packed, None, None, stats, stats, stats, y, N, Cin, H, W, Cout, 0, groups, 0, None)


def _b1(lib, x=FAKE, packed=FAKE, y=FAKE, stats=None, N=1, Cin=32, HW=16, Cout=8, groups=0):
    return lib.vgpt_conv1x1_bx3_fwd(x, packed, None, None, stats, stats, stats, y, N, Cin, HW, Cout, groups, 0, None)


def test_split_bf16_convs_refuse_bad_calls(lib):
    for fn, name in ((_bx3, b"vgpt_conv2d_bx3_fwd"), (_b1, b"vgpt_conv1x1_bx3_fwd")):
        for off in (2, 4, 8):
            _refused(lib, fn(lib, packed=FAKE + off), UNSUPPORTED, name + b": packed weights must be 16-byte aligned")
        for kw in (dict(x=None), dict(packed=None), dict(y=None)):
            _refused(lib, fn(lib, **kw), INVALID, name + b": null pointer")
        for kw in (dict(N=-1), dict(Cin=0), dict(Cout=-2)):
            _refused(lib, fn(lib, **kw), INVALID, name + b": bad shape")
        _refused(lib, fn(lib, groups=8), INVALID, name + b": GroupNorm prologue needs")             # no stats
        _refused(lib, fn(lib, groups=5, stats=FAKE), INVALID, name + b": GroupNorm prologue needs")  # Cin % 5
    _refused(lib, _bx3(lib, H=0), INVALID, b"bad shape")
    _refused(lib, _b1(lib, HW=0), INVALID, b"bad shape")
    for Cin in (3, 16, 48, 100):
        _refused(lib, _b1(lib, Cin=Cin), UNSUPPORTED, b"Cin must be a multiple of 32 (got %d)" % Cin)
    _refused(lib, _b1(lib, Cin=512, HW=1 << 22), UNSUPPORTED, b"image too large")   # Cin * HW = 2^31
    _refused(lib, _b1(lib, Cin=2048, HW=1 << 20), UNSUPPORTED, b"image too large")


def test_small_vae_kernels_refuse_bad_calls(lib):
    _refused(lib, lib.vgpt_groupnorm_stats(FAKE, FAKE, 1, 30, 16, 4, 1e-6, None), INVALID, b"vgpt_groupnorm_stats: bad shape")
    _refused(lib, lib.vgpt_groupnorm_stats(FAKE, FAKE, 1, 32, 0, 4, 1e-6, None), INVALID, b"vgpt_groupnorm_stats: bad shape")
    _refused(lib, lib.vgpt_groupnorm_stats(FAKE, FAKE, 1, 32, 16, 0, 1e-6, None), INVALID, b"vgpt_groupnorm_stats: bad shape")
    _refused(lib, lib.vgpt_groupnorm_stats(None, FAKE, 1, 32, 16, 4, 1e-6, None), INVALID, b"vgpt_groupnorm_stats: null pointer")
    _refused(lib, lib.vgpt_groupnorm_stats(FAKE, None, 1, 32, 16, 4, 1e-6, None), INVALID, b"vgpt_groupnorm_stats: null pointer")
    _refused(lib, lib.vgpt_col_softmax(None, 1, 4, 4, 1.0, None), INVALID, b"vgpt_col_softmax: null pointer")
    for N, keys, queries in ((-1, 4, 4), (1, 0, 4), (1, 4, 0)):
        _refused(lib, lib.vgpt_col_softmax(FAKE, N, keys, queries, 1.0, None), INVALID, b"vgpt_col_softmax: bad shape")
    for ptrs in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        _refused(lib, lib.vgpt_vae_sample(*ptrs, 1, 64, 0.0, 1.0, None), INVALID, b"vgpt_vae_sample: null pointer")
    _refused(lib, lib.vgpt_vae_sample(FAKE, FAKE, FAKE, 1, 0, 0.0, 1.0, None), INVALID, b"vgpt_vae_sample: bad shape")
    _refused(lib, lib.vgpt_vae_sample(FAKE, FAKE, FAKE, -2, 64, 0.0, 1.0, None), INVALID, b"vgpt_vae_sample: bad shape")
    _refused(lib, lib.vgpt_vae_postprocess_u8(None, FAKE, 1, 3, 4, 4, None), INVALID, b"vgpt_vae_postprocess_u8: null pointer")
    _refused(lib, lib.vgpt_vae_postprocess_u8(FAKE, None, 1, 3, 4, 4, None), INVALID, b"vgpt_vae_postprocess_u8: null pointer")
    for shape in ((-1, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)):
        _refused(lib, lib.vgpt_vae_postprocess_u8(FAKE, FAKE, *shape, None), INVALID, b"vgpt_vae_postprocess_u8: bad shape")
    _refused(lib, lib.vgpt_affine_to_f32(None, 0, FAKE, 8, 1.0, 0.0, None), INVALID, b"vgpt_affine_to_f32: null pointer")
    _refused(lib, lib.vgpt_affine_to_f32(FAKE, 1, None, 8, 1.0, 0.0, None), INVALID, b"vgpt_affine_to_f32: null pointer")
    _refused(lib, lib.vgpt_affine_to_f32(FAKE, 0, FAKE, -8, 1.0, 0.0, None), INVALID, b"vgpt_affine_to_f32: bad shape")
    for fn in (lib.vgpt_conv_pack_weights_bx3, lib.vgpt_conv1x1_pack_weights_bx3):
        for args in ((None, FAKE, 8, 8), (FAKE, None, 8, 8), (FAKE, FAKE, 0, 8), (FAKE, FAKE, 8, -1)):
            _refused(lib, fn(*args, None), INVALID, b"bad argument")


def test_empty_batches_are_no_ops(lib):
    """N = 0 (n = 0): VGPT_OK before anything is read or launched -- the pointers here are never valid."""
    assert _conv(lib, N=0) == OK
    assert _conv(lib, N=0, ksize=1) == OK
    assert _bx3(lib, N=0) == OK
    assert _b1(lib, N=0) == OK
    assert lib.vgpt_groupnorm_stats(FAKE, FAKE, 0, 32, 16, 4, 1e-6, None) == OK
    assert lib.vgpt_col_softmax(FAKE, 0, 4, 4, 1.0, None) == OK
    assert lib.vgpt_vae_sample(FAKE, FAKE, FAKE, 0, 64, 0.0, 1.0, None) == OK
    assert lib.vgpt_vae_postprocess_u8(FAKE, FAKE, 0, 3, 4, 4, None) == OK
    assert lib.vgpt_affine_to_f32(FAKE, 0, FAKE, 0, 1.0, 0.0, None) == OK


# (Cout, Cin) of sdxl-vae's 3x3 and 1x1 layers (block_out_channels 128, 256, 512, 512; latent 4 / 8) and ragged sizes
@pytest.mark.parametrize("Cout,Cin", [(128, 3), (128, 128), (256, 128), (256, 256), (512, 256), (512, 512), (8, 512), (512, 4),
                                      (3, 128), (1, 1), (64, 16), (65, 17), (70, 20), (500, 33)])
def test_packed_weight_sizes(lib, Cout, Cin):
    cdiv = lambda a, b: -(-a // b)
    assert lib.vgpt_conv_bx3_packed_bytes(Cout, Cin) == cdiv(Cout, 64) * cdiv(Cin, 16) * 48 * 1024
    assert lib.vgpt_conv1x1_bx3_packed_bytes(Cout, Cin) == cdiv(Cout, 64) * cdiv(Cin, 32) * 16 * 1024
