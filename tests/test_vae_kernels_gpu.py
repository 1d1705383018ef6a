"""Each VAE kernel (video-gpt_amd/ops.py -> csrc/vae.hip) against a float64 restatement of the same operation, evaluated
on the fp32 values the kernel reads, at the tiles production runs and at the shapes where kernels go wrong: both tile
variants of the 3x3 split-bf16 convolution (the 16-row tile is chosen by tiles_x * tiles_co * N * ceil(Hout / 16) >= 256,
which no other test reaches), ragged rows / columns / channel tiles, partial channel chunks, scalar epilogues, the 1x1
kernel's last partial 512-pixel tile, stride 2 on odd sizes, padded weight strides, GroupNorm statistics at every loop
structure and with outliers, the column softmax's ragged blocks and empty key quarters, the elementwise kernels' clamps
and index arithmetic.  tests/test_vae_gpu.py checks the same kernels through one global rel-L2 per tensor; here every
global rel-L2 has an element-wise bound beside it.

Tolerance style (as tests/test_train_kernels_gpu.py): bounds are element-wise, relative to the sum of the absolute terms
(mag = conv(|f(x)|, |w|) + |bias| + |resid| in float64), each with its derivation; index kernels are bit-exact; the
worst |err| / bound of every check is printed as a MEASURE line (profiles/r10_vae_kernel_tests.log) and quoted in
the comment of the bound it belongs to.  The float64 references run on the GPU as unfold + matmul in torch.float64.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_train_kernels_gpu import _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
F64 = torch.float64
U32 = 2.0 ** -24    # fp32 unit roundoff
TINY = 2.0 ** -126  # smallest normal fp32: results below it may be flushed to zero


def g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def rel_l2(a, b):
    a, b = a.double(), b.double().to(a.device)
    return float((a - b).norm() / (b.norm() + 1e-30))


def cdiv(a, b):
    return -(-a // b)


# ============================================================================================================
# float64 restatements (on the GPU, in torch.float64)
# ============================================================================================================
def _conv64(h, w, stride=1, pad=(1, 1, 1, 1)):
    """(conv(h, w), conv(|h|, |w|)) in float64: zero pad (left, right, top, bottom), unfold, one matmul each."""
    k = w.shape[-1]
    hp = F.pad(h.double(), pad)
    N, _, Hp, Wp = hp.shape
    Ho, Wo = (Hp - k) // stride + 1, (Wp - k) // stride + 1
    cols = F.unfold(hp, k, stride=stride)                      # (N, Cin * k * k, Ho * Wo)
    wm = w.double().reshape(w.shape[0], -1).to(h.device)
    return (wm @ cols).view(N, -1, Ho, Wo), (wm.abs() @ cols.abs()).view(N, -1, Ho, Wo)


def _prologue64(x, gn, up):
    """f(x) = upsample(SiLU?(GroupNorm(x))) in float64 from the KERNEL'S OWN statistics (so their error does not count
    against the convolution), and a = (|x| + |mean|) * rstd * |gamma| + |beta|, the magnitude the GroupNorm FMA's
    rounding scales with (None without GroupNorm).  gn = (stats, gamma, beta, groups, silu) as ops.conv2d takes it."""
    h, a = x.double(), None
    if gn is not None:
        st, gamma, beta, groups, silu = gn
        cpg = x.shape[1] // groups
        mean = st[..., 0].double().repeat_interleave(cpg, 1)[:, :, None, None]
        rstd = st[..., 1].double().repeat_interleave(cpg, 1)[:, :, None, None]
        ga, be = gamma.double()[None, :, None, None], beta.double()[None, :, None, None]
        a = (h.abs() + mean.abs()) * rstd * ga.abs() + be.abs()
        h = (h - mean) * rstd * ga + be
        if silu:
            h = h * torch.sigmoid(h)
    if up:
        h = F.interpolate(h, scale_factor=2.0, mode="nearest")
        a = None if a is None else F.interpolate(a, scale_factor=2.0, mode="nearest")
    return h, a


def _bx_bound(K, mag, amag):
    """Split-bf16 convolutions: (2^-16 + (K/8 + 8) 2^-24) mag.  hi keeps 8 bits, so |lo| <= 2^-9 |x|; the dropped lo*lo
    is <= 2^-18 of a product and rounding each lo to bf16 adds two more 2^-18: under 2^-16 per term; the fp32
    accumulation inside the MFMA and across chunks is the second term.  A GroupNorm prologue adds 8 * 2^-24 * conv(a, |w|):
    the kernels normalise with one FMA x * sc + sh, sh = beta - mean * sc, whose rounding scales with |mean| * rstd and
    not with the (possibly cancelled) result; 8 covers that FMA, the two table entries and the v_exp_f32 / v_rcp_f32
    SiLU (1 ulp each by the ISA manual, derivative of SiLU at most 1.1)."""
    b = (2.0 ** -16 + (K / 8 + 8) * U32) * mag
    return b if amag is None else b + 8 * U32 * amag


def _exact_bound(K, mag, amag=None):
    """Exact-fp32 convolution: one FMA chain of K terms plus bias and residual: (K + 4) 2^-24 mag; its GroupNorm
    prologue ((x - mean) * rstd * gamma + beta, expf SiLU) is covered by the same 8 * 2^-24 * conv(a, |w|)."""
    b = (K + 4) * U32 * mag
    return b if amag is None else b + 8 * U32 * amag


def _mk_gn(ops, x, groups, silu, seed, beta_scale=0.1):
    C = x.shape[1]
    gamma = (1 + 0.1 * torch.randn(C, generator=g(seed))).to(DEV)
    beta = (beta_scale * torch.randn(C, generator=g(seed + 1))).to(DEV)
    return (ops.groupnorm_stats(x, groups, 1e-6), gamma, beta, groups, silu)


def _bx3_product(N, Cout, Hout, Wout):
    """What vgpt_conv2d_bx3_fwd compares with 256 to choose the 16-row tile (>=) or the 8-row tile (<)."""
    return cdiv(Wout, 32) * cdiv(Cout, 64) * N * cdiv(Hout, 16)


def _run_bx3(ops, x, w, b, resid, gn, up, big, what, l2=3e-5):
    """One 3x3 split-bf16 case: which tile it runs on is asserted, then element-wise bound and global rel-L2."""
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    prod = _bx3_product(N, Cout, Ho, Wo)
    assert (prod >= 256) == big, f"{what}: tile product {prod} is on the wrong side of 256"
    out = ops.conv2d_bx3(x, ops.conv_pack_bx3(w), b, resid=resid, gn=gn, upsample=up)
    h, a = _prologue64(x, gn, up)
    ref, mag = _conv64(h, w)
    amag = None if a is None else _conv64(a, w)[1]
    if b is not None:
        ref, mag = ref + b.double()[None, :, None, None], mag + b.double().abs()[None, :, None, None]
    if resid is not None:
        ref, mag = ref + resid.double(), mag + resid.double().abs()
    assert out.shape == ref.shape
    bound = _bx_bound(Cin * 9, mag, amag)
    _within(out, ref, bound, what)
    err = rel_l2(out, ref)
    assert err < l2, f"{what}: rel-L2 {err:.3g}"
    return out, ref, bound


def _inputs3(N, Cin, Cout, H, W, seed, up=False, bias=True, res=True, ksize=3, scale=1.0, shift=0.0):
    x = (torch.randn(N, Cin, H, W, generator=g(seed)) * scale + shift).to(DEV)
    w = (torch.randn(Cout, Cin, ksize, ksize, generator=g(seed + 1)) / (Cin * ksize * ksize) ** 0.5).to(DEV)
    b = torch.randn(Cout, generator=g(seed + 2)).to(DEV) if bias else None
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    r = torch.randn(N, Cout, Ho, Wo, generator=g(seed + 3)).to(DEV) if res else None
    return x, w, b, r


# ============================================================================================================
# A. 3x3 split-bf16, both tile variants
# ============================================================================================================
# The bound is the derived one of _bx_bound.  Measured worst |err| / bound (profiles/r10_vae_kernel_tests.log): 0.52 on the
# 16-row tile (Cin = 3, where the 2^-16 term is nearly all of it), 0.21 on the 8-row tile, 0.16 on the beta ~ 3 border
# ring, 0.05 on the 256^2 production layer, 0.015 where mean / std = 100 (the conv(a, |w|) term is then 100 times the rest).
def test_bx3_16row_tile_ragged_everywhere(ops):
    """N=2, 16 -> 500, 121 x 63: product exactly 256; Hout % 16 = 9, Wout % 4 != 0 (scalar epilogue), partial last co tile."""
    x, w, b, r = _inputs3(2, 16, 500, 121, 63, 100)
    _run_bx3(ops, x, w, b, r, None, False, True, "bx3 16-row ragged 2x16x500x121x63")


@pytest.mark.parametrize("up", [False, True])
def test_bx3_16row_tile_groupnorm_silu(ops, up):
    """N=8, 128 -> 128, output 64 x 128 (product 256), GroupNorm(32) + SiLU, with and without the folded x2 upsample."""
    H, W = (32, 64) if up else (64, 128)
    x, w, b, r = _inputs3(8, 128, 128, H, W, 110, up=up, scale=2.0, shift=0.5)
    _run_bx3(ops, x, w, b, r, _mk_gn(ops, x, 32, 1, 114), up, True, f"bx3 16-row GN+SiLU up={int(up)} 8x128x128x64x128")


@pytest.mark.parametrize("Cin", [3, 20])
def test_bx3_16row_tile_partial_channel_chunk(ops, Cin):
    """Cin % 16 != 0: the clamped-channel loader and the zero weights past Cin; N=2, Cout=512, 128 x 64 (product 256)."""
    x, w, b, r = _inputs3(2, Cin, 512, 128, 64, 120 + Cin)
    _run_bx3(ops, x, w, b, r, None, False, True, f"bx3 16-row partial chunk Cin={Cin}")


def test_bx3_production_layer_256(ops):
    """One resnet convolution as the 256^2 decode runs it: N=1, 128 -> 128, 256 x 256, GroupNorm + SiLU + residual
    (product 256).  The float64 reference covers the whole image (it runs on the GPU), so every tile seam is in it."""
    x, w, b, r = _inputs3(1, 128, 128, 256, 256, 130, scale=2.0, shift=0.5)
    _run_bx3(ops, x, w, b, r, _mk_gn(ops, x, 32, 1, 134), False, True, "bx3 production 1x128x128x256x256")


def test_bx3_tile_variants_bit_identical(ops):
    """The same image at N=1 (product 128: 8-row tile) and twice at N=2 (product 256: 16-row tile).  Both variants add
    the same chunks in the same MFMA order per output element, so the results are bit-identical."""
    x, w, b, r = _inputs3(1, 32, 512, 128, 64, 140, scale=2.0, shift=0.5)
    gn = _mk_gn(ops, x, 8, 1, 144)
    small = _run_bx3(ops, x, w, b, r, gn, False, False, "bx3 threshold pair N=1 (8-row)")[0]
    x2, r2 = x.repeat(2, 1, 1, 1).contiguous(), r.repeat(2, 1, 1, 1).contiguous()
    gn2 = (ops.groupnorm_stats(x2, 8, 1e-6),) + gn[1:]
    assert torch.equal(gn2[0][0], gn[0][0]) and torch.equal(gn2[0][1], gn[0][0])
    big = _run_bx3(ops, x2, w, b, r2, gn2, False, True, "bx3 threshold pair N=2 (16-row)")[0]
    assert torch.equal(big[0], small[0]) and torch.equal(big[1], small[0])


# (bias, residual, GroupNorm: None / silu 0 / silu 1, upsample): every feature on and off, alone and together
BX3_OPTS = [(0, 0, None, 0), (1, 0, None, 0), (0, 1, None, 0), (1, 1, None, 1), (1, 1, 0, 0), (1, 0, 1, 0), (0, 1, 1, 1),
            (1, 1, 0, 1)]


@pytest.mark.parametrize("W", [1, 31, 32, 33, 66])
@pytest.mark.parametrize("H", [1, 7, 8, 9])
def test_bx3_8row_tile_edges(ops, H, W):
    """8-row tile at one row, one column, one short of / exactly / one past a tile in each direction; Cin 24 (partial
    chunk under GroupNorm, groups of 6 channels) and 32 alternate; Cout 20."""
    for i, (bias, res, silu, up) in enumerate(BX3_OPTS):
        Cin = (24, 32)[i % 2]
        x, w, b, r = _inputs3(1, Cin, 20, H, W, 200 + i, up=bool(up), bias=bool(bias), res=bool(res), scale=2.0, shift=0.5)
        gn = None if silu is None else _mk_gn(ops, x, 4, silu, 210 + i)
        _run_bx3(ops, x, w, b, r, gn, bool(up), False, f"bx3 8-row {H}x{W} Cin={Cin} bias={bias} res={res} gn={silu} up={up}")


def test_bx3_groupnorm_mean_over_std_100(ops):
    """mean / std = 100: the rounding of the one-FMA normalisation (|mean| * rstd = 100 ulps of an O(1) result) is what
    decides here, so the conv(a, |w|) term of the bound is exercised on both tiles."""
    for N, big in ((1, False), (2, True)):
        x, w, b, r = _inputs3(N, 32, 512, 128, 64, 150, scale=0.5, shift=50.0)
        _run_bx3(ops, x, w, b, r, _mk_gn(ops, x, 8, 1, 154), False, big, f"bx3 GN mean/std=100 N={N}")


@pytest.mark.parametrize("N,H,W,big", [(1, 9, 33, False), (2, 128, 64, True)])
def test_bx3_padding_applies_after_groupnorm(ops, N, H, W, big):
    """|beta| ~ 3 with SiLU: zero padding applied to x before the normalisation instead of to the normalised activation
    would change every border pixel by O(1).  The border ring is asserted on its own."""
    x, w, b, r = _inputs3(N, 32, 512 if big else 20, H, W, 160)
    gn = list(_mk_gn(ops, x, 8, 1, 164))
    gn[2] = (3.0 * torch.sign(torch.randn(32, generator=g(166))) + 0.1 * torch.randn(32, generator=g(167))).to(DEV)
    out, ref, bound = _run_bx3(ops, x, w, b, r, tuple(gn), False, big, f"bx3 halo beta~3 {N}x{H}x{W}")
    ring = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    _within(out[:, :, ring], ref[:, :, ring], bound[:, :, ring], f"bx3 halo beta~3 {N}x{H}x{W} border ring")


@pytest.mark.parametrize("Cout,Cin", [(70, 20), (64, 16), (1, 1), (130, 33)])
def test_conv_pack_bx3_layout_and_idempotence(ops, Cout, Cin):
    """The packed buffer byte for byte (layout above conv_pack_bx3_kernel): per (64-channel co tile, 16-channel chunk) a
    48-KiB image = hi plane then lo plane, each [co_local 64][336 bytes] with bf16 k = tap * 16 + channel; the tenth tap
    slot, the 16 pad bytes of a row, channels / output channels past the end and the image's tail are zero."""
    w = torch.randn(Cout, Cin, 3, 3, generator=g(170)).to(DEV)
    p1, p2 = ops.conv_pack_bx3(w)[0], ops.conv_pack_bx3(w)[0]
    assert torch.equal(p1, p2)
    tiles, nch = cdiv(Cout, 64), cdiv(Cin, 16)
    assert p1.numel() == tiles * nch * 48 * 1024
    wp = torch.zeros(tiles * 64, nch * 16, 9, dtype=F32)
    wp[:Cout, :Cin] = w.cpu().reshape(Cout, Cin, 9)
    hi = wp.bfloat16()
    lo = (wp - hi.float()).bfloat16()
    expect = torch.zeros(tiles, nch, 48 * 1024 // 2, dtype=torch.int16)
    for plane, v in enumerate((hi, lo)):
        rows = torch.zeros(tiles, nch, 64, 168, dtype=torch.int16)   # 336-byte rows
        # (tile, co_local, chunk, channel, tap) -> (tile, chunk, co_local, tap, channel)
        rows[..., :144] = v.view(torch.int16).view(tiles, 64, nch, 16, 9).permute(0, 2, 1, 4, 3).reshape(tiles, nch, 64, 144)
        expect[:, :, plane * 64 * 168:(plane + 1) * 64 * 168] = rows.view(tiles, nch, -1)
    got = p1.cpu().view(torch.int16).view(tiles, nch, -1)
    assert torch.equal(got, expect)


# ============================================================================================================
# B. 1x1 split-bf16
# ============================================================================================================
# (bias, residual, GroupNorm: None / silu 0 (the attention's q, k, v) / silu 1)
B1_OPTS = [(1, 0, None), (0, 0, None), (1, 1, None), (1, 0, 0), (0, 1, 1), (1, 1, 0)]


@pytest.mark.parametrize("hi,H,W", [(0, 1, 1), (1, 1, 3), (2, 7, 9), (3, 8, 8), (4, 7, 73), (5, 16, 32), (6, 27, 19),
                                    (7, 32, 32), (8, 10, 103)])
def test_conv1x1_bx3_edges(ops, hi, H, W):
    """HW = 1, 3, 63, 64, 511, 512, 513, 1024, 1030 (scalar epilogue where HW % 4 != 0, the last partial 512-pixel tile)
    x Cin {32, 64, 512} x Cout {4, 64, 70, 128} x N {1, 3}; the option sets rotate so that each meets every HW.  Against
    float64 and against the exact-fp32 kernel on the same inputs (the sum of the two bounds).  Measured worst
    |err| / bound: 0.49 against float64 (HW = 511), 0.43 against the exact kernel."""
    idx = hi
    for Cin in (32, 64, 512):
        for Cout in (4, 64, 70, 128):
            for N in (1, 3):
                bias, res, silu = B1_OPTS[idx % len(B1_OPTS)]
                idx += 1
                x, w, b, r = _inputs3(N, Cin, Cout, H, W, 300 + idx, bias=bool(bias), res=bool(res), ksize=1, scale=2.0,
                                      shift=0.5)
                gn = None if silu is None else _mk_gn(ops, x, 8 if Cin == 32 else 32, silu, 310 + idx, beta_scale=0.5)
                what = f"1x1 HW={H * W} {N}x{Cin}->{Cout} bias={bias} res={res} gn={silu}"
                out = ops.conv1x1_bx3(x, ops.conv1x1_pack_bx3(w), b, resid=r, gn=gn)
                exact = ops.conv2d(x, w, b, resid=r, gn=gn, ksize=1)
                h, a = _prologue64(x, gn, False)
                ref, mag = _conv64(h, w, pad=(0, 0, 0, 0))
                amag = None if a is None else _conv64(a, w, pad=(0, 0, 0, 0))[1]
                if b is not None:
                    ref, mag = ref + b.double()[None, :, None, None], mag + b.double().abs()[None, :, None, None]
                if r is not None:
                    ref, mag = ref + r.double(), mag + r.double().abs()
                assert out.shape == ref.shape
                bound = _bx_bound(Cin, mag, amag)
                _within(out, ref, bound, what)
                _within(out, exact, bound + _exact_bound(Cin, mag, amag), what + " vs exact fp32")
                assert rel_l2(out, ref) < 3e-5, what


# ============================================================================================================
# C. exact-fp32 conv2d
# ============================================================================================================
def _exact_case(ops, N, Cin, Cout, H, W, mode, seed):
    k = 1 if mode == "1x1" else 3
    x, w, b, _ = _inputs3(N, Cin, Cout, H, W, seed, res=False, ksize=k)
    if mode == "3x3":
        out, (ref, mag) = ops.conv2d(x, w, b), _conv64(x, w)
    elif mode == "3x3s2":   # Downsample2D: zero pad (0, 1, 0, 1), stride 2; odd sizes follow from the same definition
        out, (ref, mag) = ops.conv2d(x, w, b, stride=2), _conv64(x, w, stride=2, pad=(0, 1, 0, 1))
    elif mode == "3x3up":
        out, (ref, mag) = ops.conv2d(x, w, b, upsample=True), _conv64(F.interpolate(x.double(), scale_factor=2.0), w)
    else:
        out, (ref, mag) = ops.conv2d(x, w, b, ksize=1), _conv64(x, w, pad=(0, 0, 0, 0))
    ref, mag = ref + b.double()[None, :, None, None], mag + b.double().abs()[None, :, None, None]
    what = f"conv2d {mode} {N}x{Cin}->{Cout} {H}x{W}"
    assert out.shape == ref.shape, what
    _within(out, ref, _exact_bound(Cin * k * k, mag), what)
    assert rel_l2(out, ref) < 2e-5, what


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 8, 64, 8, 32), (1, 3, 128, 16, 16), (3, 20, 70, 7, 37), (1, 128, 128, 32, 32),
                                            (2, 12, 40, 9, 8), (1, 5, 9, 3, 2)])
@pytest.mark.parametrize("mode", ["3x3", "3x3s2", "3x3up", "1x1"])
def test_conv2d_exact_elementwise(ops, N, Cin, Cout, H, W, mode):
    """The shapes of test_conv_variants plus odd sizes; stride 2 runs on odd H and / or W too (7x37, 9x8, 3x2).  Measured
    worst |err| / bound of (K + 4) 2^-24 mag: 0.30 (1x1, K = 3), 0.14 for the 3x3 modes."""
    _exact_case(ops, N, Cin, Cout, H, W, mode, 400)


@pytest.mark.parametrize("Cin", [4, 8])
def test_conv2d_exact_quant_convs(ops, Cin):
    """1x1 with 8 -> 8 and 4 -> 4 channels (quant_conv / post_quant_conv): a fraction of one 64-channel chunk."""
    _exact_case(ops, 2, Cin, Cin, 8, 12, "1x1", 410)


@pytest.mark.parametrize("HW", [40, 63, 65, 1024])
@pytest.mark.parametrize("Cin", [40, 64, 100])
@pytest.mark.parametrize("transposed", [False, True])
def test_conv2d_exact_batched_weights_padded_stride(ops, transposed, Cin, HW):
    """Per-image "weights" (the attention products' path) with a padded row stride ldw: (cout, ldw > Cin) rows, or stored
    [k][co] as (Cin, ldw > cout); the padding holds 1e3 so that reading it shows."""
    N, cout = 2, 70
    H, W = (HW // 8, 8) if HW % 8 == 0 else (1, HW)
    x = torch.randn(N, Cin, H, W, generator=g(420)).to(DEV)
    wt = torch.randn(N, cout, Cin, generator=g(421)).to(DEV) / Cin ** 0.5
    if transposed:
        ldw = cout + 3
        store = torch.full((N, Cin, ldw), 1e3, device=DEV)
        store[:, :, :cout] = wt.transpose(1, 2)
    else:
        ldw = Cin + 5
        store = torch.full((N, cout, ldw), 1e3, device=DEV)
        store[:, :, :Cin] = wt
    out = ops.conv2d(x, store, ksize=1, cout=cout, w_transposed=transposed, ldw=ldw, w_batch_stride=store[0].numel())
    xd = x.double().view(N, Cin, HW)
    ref, mag = wt.double() @ xd, wt.double().abs() @ xd.abs()
    what = f"conv2d batched weights transposed={int(transposed)} Cin={Cin} HW={HW}"
    _within(out.view(N, cout, HW), ref, _exact_bound(Cin, mag), what)
    assert rel_l2(out.view(N, cout, HW), ref) < 2e-5, what


# ============================================================================================================
# D. GroupNorm statistics
# ============================================================================================================
EPS = 1e-6


def _stats_check(ops, x, n, what):
    """x: (N, groups, n) fp32 on the GPU, one group per (N, groups) entry.  |mean - ref| <= (L + 22) 2^-24 (|ref| + std)
    and |rstd / ref - 1| <= 4 (L + 22) 2^-24: L = ceil(n / 4096) is the longest per-thread addition chain of the vector
    path, 22 the wave (6) and LDS (16) trees; the variance is a sum of squares (twice the relative error of a term) and
    rstd halves it again, the 4 leaves room for the shifted sum's (S/n)^2 correction.  At n = 262144 that is 2e-5, the
    budget of a whole convolution.  Measured worst |err| / bound over all cases: 0.028 (mean), 0.024 (rstd)."""
    st = ops.groupnorm_stats(x, x.shape[1], EPS)
    xd = x.double()
    mean = xd.mean(-1)
    var = (xd - mean[..., None]).pow(2).mean(-1)
    rstd = torch.rsqrt(var + float(np.float32(EPS)))
    rel = (math.ceil(n / 4096) + 22) * U32
    r_mean = float(((st[..., 0].double() - mean).abs() / (rel * (mean.abs() + var.sqrt()) + TINY)).max())
    r_rstd = float(((st[..., 1].double() / rstd - 1).abs() / (4 * rel)).max())
    print(f"MEASURE {what}: worst |err|/bound = {r_mean:.3g} (mean), {r_rstd:.3g} (rstd)")
    assert torch.isfinite(st).all() and r_mean <= 1.0 and r_rstd <= 1.0, f"{what}: worst |err|/bound = {r_mean:.3g} (mean), {r_rstd:.3g} (rstd)"
    return st


def _stats_data(kind, N, G, n, seed):
    z = torch.randn(N, G, n, generator=g(seed))
    if kind == "normal":
        x = z * 2 + 0.5
    elif kind == "offset":
        x = z * 0.1 + 100
    elif kind == "const":
        x = torch.tensor([3.25, -0.7, 100.1]).view(1, G, 1).expand(N, G, n).contiguous()   # var = 0: rstd = rsqrt(eps)
    else:   # "last": last element an outlier
        x = z.clone()
        x[..., -1] = 1000.0
    return x.to(DEV)


# 1, 3 (scalar path), 4 (one vector), 1023, 4096 (every thread one vector), 4100 (vector tail), 16384 + 4 (one pass of the
# unrolled loop plus tail), 20483 (% 4 = 3 above 16384), 65536, 262144 (a 128-channel 256^2 layer)
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4096, 4100, 16388, 20483, 65536, 262144])
@pytest.mark.parametrize("kind", ["normal", "offset", "const", "last"])
def test_groupnorm_stats_against_fp64(ops, kind, n):
    _stats_check(ops, _stats_data(kind, 2, 3, n, 500 + n % 97), n, f"gn_stats {kind} n={n}")


@pytest.mark.parametrize("n,first,std", [(262144, 1000.0, 1.0), (65536, 300.0, 0.5), (16384, -50.0, 0.2), (20483, 300.0, 0.5),
                                         (1023, 300.0, 0.5)])
def test_groupnorm_stats_first_element_outlier(ops, n, first, std):
    """The first element of a group is the top-left corner pixel of a channel, where zero padding makes outliers likely.
    With the group's first element as the shift K these cases missed the rstd bound 24- to 718-fold (worst |err| / bound
    n = 262144: 718, i.e. rstd 1.5e-2 off; 65536: 607; 16384: 288; 20483: 472; 1023: 24) and the mean bound 3- to 14-fold;
    with K the mean of the block's first loads they measure 0.004 to 0.024 (both in profiles/r10_vae_kernel_tests.log)."""
    x = torch.randn(2, 3, n, generator=g(520)) * std
    x[..., 0] = first
    _stats_check(ops, x.to(DEV), n, f"gn_stats first-outlier n={n} first={first:g}")


def test_groupnorm_stats_misaligned_group_base(ops):
    """A tensor that starts 4 bytes past a 16-byte boundary (n % 4 == 0: only the alignment test selects the scalar path),
    and odd HW * C/groups with N * groups > 1 (every other group base misaligned)."""
    buf = (torch.randn(1 + 2 * 3 * 4096, generator=g(530)) * 2 + 0.5).to(DEV)
    x = buf[1:].view(2, 3, 4096)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    _stats_check(ops, x, 4096, "gn_stats base + 4 bytes n=4096")
    x = (torch.randn(2, 6, 5, 9, generator=g(531)) * 2 + 0.5).to(DEV)   # C/groups = 3, HW = 45: 135 elements per group
    st = ops.groupnorm_stats(x, 2, EPS)
    st2 = _stats_check(ops, x.view(2, 2, 135), 135, "gn_stats odd group size 135")
    assert torch.equal(st, st2)


# ============================================================================================================
# E. column softmax
# ============================================================================================================
def _softmax_check(ops, s, scale, what):
    """|p - ref| <= (2 max|s scale| + keys/4 + 16) 2^-24 ref: the fp32 rounding of s * scale and of v - M moves the
    exponent's argument by up to 2^-24 max|s scale| each, the running sum of a key quarter is a chain of keys/4 additions,
    16 covers expf, the merge and the division; plus the smallest normal fp32, below which results may be flushed.
    Every column sums to 1 within keys * 2^-24.  Measured worst |err| / bound: 0.21 element-wise (63 keys), 0.58 for the
    column sums (3 keys), 0.05 / 0.008 at 1024 x 1024."""
    N, keys, queries = s.shape
    scale = float(np.float32(scale))
    ref = torch.softmax(s.double() * scale, dim=1)
    amax = float((s.double() * scale).abs().max())
    out = ops.col_softmax(s.clone(), scale)
    _within(out, ref, (2 * amax + keys / 4 + 16) * U32 * ref + TINY, what)
    _within(out.double().sum(1), torch.ones(N, queries, dtype=F64), torch.full((N, queries), keys * U32, dtype=F64),
            what + " column sums")
    return out, ref


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("keys,queries", [(1, 1), (2, 5), (3, 64), (5, 65), (40, 40), (63, 130), (1024, 1024), (1025, 100)])
def test_col_softmax_against_fp64(ops, keys, queries, N):
    """keys < 4 (empty key quarters: the -inf guard), keys % 4 != 0, one short of / past a 64-query block, the
    production size 1024 x 1024 with the mid-block's scale 1 / sqrt(512)."""
    s = (torch.randn(N, keys, queries, generator=g(600)) * 30).to(DEV)
    _softmax_check(ops, s, 1 / 512 ** 0.5, f"col_softmax {N}x{keys}x{queries}")


def test_col_softmax_large_scores_and_uniform(ops):
    s = (torch.randn(2, 37, 70, generator=g(610)) * 1e4).to(DEV)   # no max-subtraction would overflow expf
    out, ref = _softmax_check(ops, s, 1.0, "col_softmax scores ~1e4")
    assert torch.equal(out.argmax(1), ref.argmax(1).to(DEV)) and float(out.max(1).values.min()) > 0.5   # one-hot columns
    for keys in (3, 40, 1025):
        s = torch.full((1, keys, 70), 7.5, device=DEV)
        out = ops.col_softmax(s, 0.3)
        # all keys equal: every term is expf(0) = 1 exactly, the sum is the exact count: 1 / keys up to 2 ulp (measured 0.6
        # of that: the contracted s * scale - M leaves the product's rounding error in the exponent)
        ulp = float(np.spacing(np.float32(1.0 / keys)))
        _within(out, torch.full_like(out, 1.0 / keys, dtype=F64), torch.full_like(out, 2 * ulp, dtype=F64),
                f"col_softmax uniform keys={keys}")


# ============================================================================================================
# F. elementwise kernels
# ============================================================================================================
def test_vae_sample_clamps_and_layout(ops):
    """logvar columns at -40, -30, 0, 20, 30 (clamp to [-30, 20]) beside random ones, nonzero shift and scaling, N = 3,
    140 elements per image.  |z - ref| <= 6 * 2^-24 (|mean| + |exp(0.5 lv) noise| + |shift|) |scaling|: expf at 2 ulp plus
    four roundings, relative to the terms and not to a cancelled sum (measured worst |err| / bound 0.38)."""
    N, C, h, w = 3, 4, 5, 7
    mom = torch.randn(N, 2 * C, h, w, generator=g(700)) * 2
    for i, lv in enumerate((-40.0, -30.0, 0.0, 20.0, 30.0)):
        mom[:, C:, :, i] = lv
    noise = torch.randn(N, C, h, w, generator=g(701))
    shift, scaling = float(np.float32(0.0609)), float(np.float32(0.3611))
    z = ops.vae_sample(mom.to(DEV), noise.to(DEV), shift, scaling)
    mean, lv = mom[:, :C].double(), mom[:, C:].double().clamp(-30.0, 20.0)
    spread = torch.exp(0.5 * lv) * noise.double()
    ref = (mean + spread - shift) * scaling
    assert z.shape == ref.shape
    _within(z, ref, 6 * U32 * (mean.abs() + spread.abs() + abs(shift)) * abs(scaling), "vae_sample")


@pytest.mark.parametrize("C", [1, 3, 4])
def test_vae_postprocess_u8_bit_exact(ops, C):
    """Bit-exact against torch's fp32 (x * 0.5 + 0.5).clamp(0, 1).mul(255).to(uint8).permute(0, 2, 3, 1) on every exact
    integer boundary 2k/255 - 1 and its two fp32 neighbours, values outside [-1, 1], -0.0; N = 2, H != W."""
    N, H, W = 2, 19, 23
    k = torch.arange(256, dtype=F32) * 2 / 255 - 1
    special = torch.cat([k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-2.0)),
                         torch.tensor([-1.5, 1.5, -0.0, 0.0, 1.0, -1.0, 1e30, -1e30, 1.0000001, -1.0000001])])
    total = N * C * H * W
    x = torch.rand(total, generator=g(710)) * 2.4 - 1.2
    x[:special.numel()] = special
    x = x[torch.randperm(total, generator=g(711))].view(N, C, H, W)
    ref = (x * 0.5 + 0.5).clamp(0, 1).mul(255).to(torch.uint8).permute(0, 2, 3, 1)
    out = ops.vae_postprocess_u8(x.to(DEV)).cpu()
    assert out.shape == ref.shape and out.dtype == torch.uint8
    bad = (out != ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} pixels differ, first at {bad[0].tolist()}"


@pytest.mark.parametrize("dt", [F32, torch.bfloat16])
def test_affine_to_f32(ops, dt):
    """y = x * mul + add is one fp32 rounding of the float64 value (the compiler contracts it into one FMA; measured worst
    |err| / bound 0.96, half an ulp being at most 2^-24 |ref|); 1000 elements (not a multiple of the 256-thread block)."""
    x = (torch.randn(1000, generator=g(720)) * 3).to(dt).to(DEV)
    mul, add = float(np.float32(1 / 0.3611)), float(np.float32(0.0609))
    y = ops.affine_to_f32(x, mul, add)
    ref = x.double() * mul + add
    assert y.dtype == F32 and y.shape == x.shape
    _within(y, ref, U32 * ref.abs() + TINY, f"affine_to_f32 {dt}")
