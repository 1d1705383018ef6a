"""The three LoRA products (video-gpt_amd/ops_lora.py -> csrc/lora.hip) against an inline float64 restatement on the
bf16-rounded inputs, at the smallest shapes at which each kernel can go wrong: fewer rows than a tile, ragged row and
column tails, several k chunks / row passes / reduction slices, both orientations of the small operand, row strides wider
than the rows, every padded rank.

Tolerance style of tests/test_train_kernels_gpu.py:
  * bf16 outputs: <= 1 bf16 ulp of the reference plus an absolute floor (chain) * 2^-24 * sum|terms| where fp32 cancels;
    bf16 x bf16 products are exact in fp32, so the chain counts additions (any order of n terms makes at most n - 1) plus
    the roundings of the epilogue;
  * fp32 outputs: (chain) * 2^-24 * sum|terms| with the kernel's own longest chain of fp32 additions.
"""
import importlib
import math

import pytest
import torch

from tests.test_ops_gpu import bf, g
from tests.test_train_kernels_gpu import U32, _ulp, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("video-gpt_amd.ops_lora")


def _rand(shape, seed, scale=1.0):
    return bf(torch.randn(*shape, generator=g(seed)) * scale)


def _view(t, pad):
    """A bf16 GPU copy of t (rows, w) as a column view of a buffer `pad` columns wider on each side (row stride w + 2 pad);
    the surroundings are NaN: a kernel that reads past its columns shows it."""
    rows, w = t.shape
    wide = torch.full((rows, w + 2 * pad), float("nan"), dtype=BF, device=DEV)
    v = wide[:, pad:pad + w]
    v.copy_(t.to(DEV, BF))
    return wide, v


def _small(rows, cols, r, seed, rank_axis, scale=0.3):
    """A small operand whose ranks >= r along `rank_axis` are zero (the caller's padding)."""
    s = _rand((rows, cols), seed, scale)
    if rank_axis == 0:
        s[r:] = 0
    else:
        s[:, r:] = 0
    return s


# ============================================================================================================
# down: U (M, rp) = alpha X S
# ============================================================================================================
@pytest.mark.parametrize("k_by_rp", [False, True])
@pytest.mark.parametrize("M,K,rp", [(7, 64, 16), (300, 192, 16), (515, 576, 48), (1100, 3072, 64)])
def test_down(L, M, K, rp, k_by_rp):
    r = rp - 3
    x = _rand((M, K), 1)
    a = _small(rp, K, r, 2, 0)                                 # (rp, K), ranks >= r zero
    alpha = 1.75
    wide, xv = _view(x, 8)                                     # ldx = K + 16 > K
    s = (a.t().contiguous() if k_by_rp else a).to(DEV, BF)
    out = L.lora_down(xv, s, rp, s_is_k_by_rp=k_by_rp, alpha=alpha)
    xd, ad = x.to(DEV, F64), a.to(DEV, F64)
    ref = alpha * (xd @ ad.t())
    mag = alpha * (xd.abs() @ ad.abs().t())
    # chain: K - 1 additions of exact products (the two k halves of a chunk and the chunks, in whatever order), the
    # multiplication by alpha
    _within(out, ref, _ulp(ref) + (K + 1) * U32 * mag, f"lora_down M={M} K={K} rp={rp} k_by_rp={k_by_rp}")
    assert torch.equal(out[:, r:], torch.zeros_like(out[:, r:])), "padded ranks of U must stay exactly zero"


# ============================================================================================================
# up_add: Y = bf16(rope?(float(Y) + alpha U S))
# ============================================================================================================
@pytest.mark.parametrize("rp_by_n", [False, True])
@pytest.mark.parametrize("N", [192, 320, 3072])
@pytest.mark.parametrize("M", [1, 65, 300, 1031])
def test_up_add(L, M, N, rp_by_n):
    rp = (16, 32, 48, 64)[(M + N // 64) % 4]
    r = rp - 5
    y = _rand((M, N), 3, 2.0)
    u = _small(M, rp, r, 4, 1, 1.0)
    b = _small(N, rp, r, 5, 1)                                 # (N, rp)
    alpha = 0.5
    wide, yv = _view(y, 8)                                     # ldy = N + 16 > N
    s = (b.t().contiguous() if rp_by_n else b).to(DEV, BF)
    L.lora_up_add(yv, u.to(DEV, BF), s, s_is_rp_by_n=rp_by_n, alpha=alpha)
    yd, ud, bd = y.to(DEV, F64), u.to(DEV, F64), b.to(DEV, F64)
    ref = yd + alpha * (ud @ bd.t())
    mag = yd.abs() + alpha * (ud.abs() @ bd.abs().t())
    # chain: rp - 1 additions, alpha, the addition to Y
    _within(yv, ref, _ulp(ref) + (rp + 2) * U32 * mag, f"lora_up_add M={M} N={N} rp={rp} rp_by_n={rp_by_n}")
    assert torch.isnan(wide[:, :8]).all() and torch.isnan(wide[:, 8 + N:]).all(), "columns outside the view were written"


@pytest.mark.parametrize("rp_by_n", [False, True])
@pytest.mark.parametrize("nq,nk", [(2, 2), (3, 1)])
def test_up_add_rope(L, nq, nk, rp_by_n):
    ops = importlib.import_module("video-gpt_amd.ops")
    hd, M, rp = 96, 333, 32 if rp_by_n else 16
    N, half = (nq + 2 * nk) * hd, hd // 2
    pos = torch.randint(0, 4000, (M,), generator=g(6))         # non-monotone positions
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    cos, sin = ops.rope_table(pos.to(DEV), inv_freq.to(DEV), round_bf16=True)
    cos, sin = cos.view(M, half), sin.view(M, half)
    y = _rand((M, N), 7, 2.0)
    u = _small(M, rp, rp - 2, 8, 1, 1.0)
    b = _small(N, rp, rp - 2, 9, 1)
    alpha = 1.25
    yv = y.to(DEV, BF)
    s = (b.t().contiguous() if rp_by_n else b).to(DEV, BF)
    L.lora_up_add(yv, u.to(DEV, BF), s, s_is_rp_by_n=rp_by_n, alpha=alpha, rope=(cos, sin, nq, nk, hd))
    yd, ud, bd = y.to(DEV, F64), u.to(DEV, F64), b.to(DEV, F64)
    x = yd + alpha * (ud @ bd.t())
    xm = yd.abs() + alpha * (ud.abs() @ bd.abs().t())
    nrot = (nq + nk) * hd
    c = torch.cat([cos, cos], 1).double().repeat(1, nq + nk)
    sn = torch.cat([sin, sin], 1).double().repeat(1, nq + nk)
    xr = x[:, :nrot].view(M, nq + nk, 2, half)
    rot_half = torch.stack([-xr[:, :, 1], xr[:, :, 0]], 2).reshape(M, nrot)
    xmr = xm[:, :nrot].view(M, nq + nk, 2, half)
    partner = torch.stack([xmr[:, :, 1], xmr[:, :, 0]], 2).reshape(M, nrot)
    ref = torch.cat([x[:, :nrot] * c + rot_half * sn, x[:, nrot:]], 1)
    mag = torch.cat([xm[:, :nrot] * c.abs() + partner * sn.abs(), xm[:, nrot:]], 1)
    # chain: rp - 1 additions, alpha, the addition to Y, two products and the addition of the rotation
    _within(yv, ref, _ulp(ref) + (rp + 5) * U32 * mag, f"lora_up_add rope nq={nq} nk={nk} rp_by_n={rp_by_n}")
    # the v columns are the unrotated sum: same bound as without RoPE
    _within(yv[:, nrot:], x[:, nrot:], _ulp(x[:, nrot:]) + (rp + 2) * U32 * xm[:, nrot:], "lora_up_add rope: v columns")


def test_merge_use_of_up_add(L):
    """W (out, in) += s B A: Y = W, U = B (out, rp), S = A (rp, in)."""
    out_f, in_f, rp, r, s = 576, 192, 16, 8, 2.0
    w = _rand((out_f, in_f), 10, 0.05)
    bm = _small(out_f, rp, r, 11, 1, 0.05)
    am = _small(rp, in_f, r, 12, 0, 0.3)
    wd = w.to(DEV, BF)
    L.lora_up_add(wd, bm.to(DEV, BF), am.to(DEV, BF), s_is_rp_by_n=True, alpha=s)
    ref = w.to(DEV, F64) + s * (bm.to(DEV, F64) @ am.to(DEV, F64))
    mag = w.to(DEV, F64).abs() + s * (bm.to(DEV, F64).abs() @ am.to(DEV, F64).abs())
    _within(wd, ref, _ulp(ref) + (rp + 2) * U32 * mag, "merge W += s B A")


# ============================================================================================================
# grad: G (N, rp) fp32 = alpha Y^T U
# ============================================================================================================
def _grad_chain(M, N):
    """The kernel's longest chain of fp32 additions (csrc/lora.hip grad_plan): the rows of one slice one after the other
    (64-row chunks, 1024 workgroups wanted over ceil(N / 128) column blocks), then the slices in order, then alpha."""
    chunks, colblocks = -(-M // 64), -(-N // 128)
    want = min(max(1024 // colblocks, 1), chunks)
    cps = -(-chunks // want)
    slices = -(-chunks // cps)
    return min(M, 64 * cps) + slices + 1


@pytest.mark.parametrize("N", [192, 576, 3072])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000, 7740])
def test_grad(L, M, N):
    rp = (16, 32, 48, 64)[(M + N // 64) % 4]
    r = rp - 4
    y = _rand((M, N), 13)
    u = _small(M, rp, r, 14, 1, 1.0)
    alpha = 0.75
    _, yv = _view(y, 8)                                        # ldy > N
    _, uv = _view(u, 8)                                        # ldu > rp
    yd, ud = y.to(DEV, F64), u.to(DEV, F64)
    ref = alpha * (yd.t() @ ud)
    mag = alpha * (yd.abs().t() @ ud.abs())
    chain = _grad_chain(M, N)
    for tr in (False, True):
        out = torch.full((rp, N) if tr else (N, rp), float("nan"), dtype=F32, device=DEV)
        L.lora_grad(yv, uv, out, transposed=tr, alpha=alpha)
        again = torch.full_like(out, float("nan"))
        L.lora_grad(yv, uv, again, transposed=tr, alpha=alpha)
        assert torch.equal(out, again), "lora_grad must be bit-identical from run to run"
        got = out.t() if tr else out
        _within(got, ref, chain * U32 * mag + 1e-300, f"lora_grad M={M} N={N} rp={rp} transposed={tr}")
        assert torch.equal(got[:, r:], torch.zeros_like(got[:, r:])), "padded ranks of G must stay exactly zero"


# ============================================================================================================
# exact integer data: a swapped row / column, a permuted reduction index or a wrong fragment map cannot pass
# ============================================================================================================
def _ints(rows, cols, mul_r, mul_c, mod, off):
    i = torch.arange(rows)[:, None]
    j = torch.arange(cols)[None, :]
    return ((mul_r * i + mul_c * j) % mod - off).float()


@pytest.mark.parametrize("rp", [16, 32, 48, 64])
def test_exact_integer_data(L, rp):
    # down, both orientations: X in {-1, 0, 1}, asymmetric S in {-2..2}; |sums| <= 2 K = 128: exact in fp32 and in bf16
    M, K = 70, 64
    x = _ints(M, K, 1, 2, 3, 1)
    a = _ints(rp, K, 3, 5, 5, 2)
    ref = (x.double() @ a.double().t())
    for k_by_rp in (False, True):
        s = (a.t().contiguous() if k_by_rp else a).to(DEV, BF)
        out = L.lora_down(x.to(DEV, BF), s, rp, s_is_k_by_rp=k_by_rp)
        assert torch.equal(out.double().cpu(), ref), f"lora_down exact data, k_by_rp={k_by_rp}"
    # up_add, both orientations: U = I padded (rows >= rp repeat other integers), asymmetric S
    M, N = 70, 80
    u = torch.zeros(M, rp)
    u[:rp] = torch.eye(rp)
    u[rp:] = _ints(M - rp, rp, 2, 1, 3, 1)
    b = _ints(N, rp, 5, 3, 7, 3)
    y = _ints(M, N, 1, 3, 9, 4)
    ref = y.double() + u.double() @ b.double().t()
    assert torch.equal(ref[:rp], y.double()[:rp] + b.double().t()[:rp])          # U = I: row m of the sum is column m of S
    for rp_by_n in (False, True):
        s = (b.t().contiguous() if rp_by_n else b).to(DEV, BF)
        yd = y.to(DEV, BF)
        L.lora_up_add(yd, u.to(DEV, BF), s, s_is_rp_by_n=rp_by_n)
        assert torch.equal(yd.double().cpu(), ref), f"lora_up_add exact data, rp_by_n={rp_by_n}"
    # grad, both store orientations: |sums| <= 2 M = 260 < 2^24
    M, N = 130, 136
    y = _ints(M, N, 1, 2, 3, 1)
    u = _ints(M, rp, 3, 5, 5, 2)
    ref = y.double().t() @ u.double()
    for tr in (False, True):
        out = torch.empty((rp, N) if tr else (N, rp), dtype=F32, device=DEV)
        L.lora_grad(y.to(DEV, BF), u.to(DEV, BF), out, transposed=tr)
        got = out.t() if tr else out
        assert torch.equal(got.double().cpu(), ref), f"lora_grad exact data, transposed={tr}"


def test_padding_rank_4_in_16(L):
    """Rank 4 inside rp = 16: every padded row / column of every output is exactly zero, through the chain of calls a
    layer's backward makes (u = x A^T, dB = dy^T u, du = dy B, dA = du^T x)."""
    M, K, N, rp, r = 200, 192, 320, 16, 4
    x, dy = _rand((M, K), 20).to(DEV, BF), _rand((M, N), 21).to(DEV, BF)
    a = _small(rp, K, r, 22, 0).to(DEV, BF)
    b = _small(N, rp, r, 23, 1).to(DEV, BF)
    u = L.lora_down(x, a, rp)
    du = L.lora_down(dy, b, rp, s_is_k_by_rp=True)
    db = L.lora_grad(dy, u, torch.empty(N, rp, dtype=F32, device=DEV))
    da = L.lora_grad(x, du, torch.empty(rp, K, dtype=F32, device=DEV), transposed=True)
    for name, t in (("u", u[:, r:]), ("du", du[:, r:]), ("dB", db[:, r:]), ("dA", da[r:])):
        assert torch.equal(t, torch.zeros_like(t)), f"padded ranks of {name} are not exactly zero"
    for name, t in (("u", u[:, :r]), ("du", du[:, :r]), ("dB", db[:, :r]), ("dA", da[:r])):
        assert t.float().abs().max() > 0, f"{name} is all zero"
