"""The qkv + RoPE epilogue of the MX-fp8 GEMM at head dims 64 and 128 (video-gpt_amd/csrc/gemm_mx8.hip through
vgpt_gemm_mx8_hd; one head per wave, so column tiles of 128 and 256), and head dim 96 through the same entry against
vgpt_gemm_mx8.

Tolerances are those of tests/test_linear_fp8_gpu.py: against fp64 A_deq W_deq^T built from the kernel's own quantised bytes
with the same epilogue rel-L2 <= 4e-3 and every element within 2^-6 relative; against the unquantised fp64 product rel-L2
<= 6e-2.  Shapes: N = (3 + 2) head_dim -- the last column tile is partial, the two trailing heads (k, v of one kv head; the v
head un-rotated) -- M in {1, 70, 130} (one lane, a ragged row group, two row tiles), K in {64, 224} (one k tile; a k tail of
32).  The output has a padded row stride and sits between NaN guards.  Two exact probes with rstd = 1: cos = 1, sin = 0 is the
NONE epilogue's output bit for bit; cos = 0, sin = 1 is [-x2 | x1] of it on the rotated heads."""
import importlib

import numpy as np
import pytest
import torch

from tests import test_linear_fp8_gpu as T8

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
g, rel_l2 = T8.g, T8.rel_l2
HEAD_DIMS = [64, 128]
NQ, NKV = 3, 1
GUARD, PAD = 64, 8


@pytest.fixture(scope="module")
def L_():
    return importlib.import_module("video-gpt_amd._lib")


def rope_ref(y, cos, sin, n_rot, D):
    """y (M, N) float64 already rounded to bf16: rotate-half RoPE on the first n_rot heads of D columns."""
    out, h2 = y.copy(), D // 2
    for h in range(n_rot):
        a, b = y[:, D * h:D * h + h2], y[:, D * h + h2:D * (h + 1)]
        out[:, D * h:D * h + h2] = a * cos - b * sin
        out[:, D * h + h2:D * (h + 1)] = b * cos + a * sin
    return out


def gemm_hd(ops, L_, a8, w8, epi, D, n_rot=0, rstd=None, cos=None, sin=None, entry="vgpt_gemm_mx8_hd"):
    """One call through the C ABI into a guarded output with row stride N + PAD; returns the (M, N) result."""
    M, N, K = a8.rows, w8.rows, a8.K
    ldc = N + PAD
    buf = torch.full((2 * GUARD + M * ldc,), float("nan"), dtype=BF, device=DEV)
    out = buf[GUARD: GUARD + M * ldc].view(M, ldc)
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    L_.call(entry, a8.data_ptr(), w8.data_ptr(), out.data_ptr(), None, p(rstd), p(cos), p(sin), M, N, K, ldc, 0,
            {"none": L_.MX8_EPI_NONE, "rope": L_.MX8_EPI_ROPE}[epi], n_rot, D, 0, ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all() and torch.isnan(out[:, N:]).all()), \
        "a byte outside the output was written"
    return out[:, :N].clone()


def operands(ops, M, N, K, seed):
    a = torch.randn(M, K, generator=g(seed)).to(BF)
    w = (0.02 * torch.randn(N, K, generator=g(seed + 1))).to(BF)
    a8 = ops.Mx8Tensor(M, K, DEV)
    rstd = torch.empty(M, dtype=torch.float32, device=DEV)
    ops.mx8_quantize_rows(a.to(DEV), a8, rstd, eps=1e-5)
    w8 = ops.mx8_quantize_weight(w.to(DEV))
    return a, w, a8, w8, rstd


@pytest.mark.parametrize("K", [64, 224])
@pytest.mark.parametrize("M", [1, 70, 130])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_rope_epilogue_against_dequantised_and_exact(ops, L_, D, M, K):
    N, n_rot = (NQ + 2 * NKV) * D, NQ + NKV
    a, w, a8, w8, rstd = operands(ops, M, N, K, seed=M + N + K)
    ang = torch.rand(M, D // 2, generator=g(M + K + 3)).double() * 6.3
    cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    got = gemm_hd(ops, L_, a8, w8, "rope", D, n_rot, rstd, cos.to(DEV), sin.to(DEV)).float().cpu().numpy().astype(np.float64)
    qa, sa = T8.decode(a8, M, K)
    qw, sw = T8.decode(w8, N, K)
    rs = rstd.cpu().numpy().astype(np.float64)
    c64, s64 = cos.numpy().astype(np.float64), sin.numpy().astype(np.float64)
    epilogue = lambda p: rope_ref(T8.bf(p * rs[:, None]), c64, s64, n_rot, D)   # noqa: E731
    deq = epilogue(T8.dequant(qa, sa) @ T8.dequant(qw, sw).T)
    exact = epilogue(a.float().numpy().astype(np.float64) @ w.float().numpy().astype(np.float64).T)
    e_deq, worst = T8.ulp_check(got, deq)
    e_ex = rel_l2(got, exact)
    print(f"mx8 GEMM rope head_dim={D} M={M} N={N} K={K}: rel-L2 vs dequantised {e_deq:.2e} (worst elem {worst:.2e} rel), vs exact {e_ex:.3e}")
    assert np.isfinite(got).all()
    assert e_deq <= 4e-3 and worst <= 2.0 ** -6
    assert e_ex <= 6e-2


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_rows_do_not_depend_on_m_or_tile(ops, L_, D):
    """Rows [0, 64) and [128, 130) of an M = 130 call equal, bit for bit, the same rows computed by M = 64 and M = 2 calls."""
    M, K = 130, 224
    N, n_rot = (NQ + 2 * NKV) * D, NQ + NKV
    a = torch.randn(M, K, generator=g(5)).to(BF).to(DEV)
    w8 = ops.mx8_quantize_weight((0.02 * torch.randn(N, K, generator=g(6))).to(BF).to(DEV))
    ang = torch.rand(M, D // 2, generator=g(8)) * 6.3
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)

    def call(r0, r1):
        a8 = ops.Mx8Tensor(r1 - r0, K, DEV)
        rstd = torch.empty(r1 - r0, dtype=torch.float32, device=DEV)
        ops.mx8_quantize_rows(a[r0:r1].contiguous(), a8, rstd)
        return gemm_hd(ops, L_, a8, w8, "rope", D, n_rot, rstd, cos[r0:r1].contiguous(), sin[r0:r1].contiguous())
    full = call(0, M)
    assert torch.isfinite(full).all()
    assert torch.equal(full[:64], call(0, 64))
    assert torch.equal(full[128:], call(128, M))


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_exact_rotation_probes(ops, L_, D):
    M, K = 70, 224
    N, n_rot = (NQ + 2 * NKV) * D, NQ + NKV
    _, _, a8, w8, _ = operands(ops, M, N, K, seed=77)
    one = torch.ones(M, dtype=torch.float32, device=DEV)
    ones, zeros = torch.ones(M, D // 2, device=DEV), torch.zeros(M, D // 2, device=DEV)
    plain = gemm_hd(ops, L_, a8, w8, "none", D)
    assert torch.isfinite(plain).all() and bool((plain != 0).any())
    ident = gemm_hd(ops, L_, a8, w8, "rope", D, n_rot, one, ones, zeros)
    assert torch.equal(ident, plain)                            # x * 1 - other * 0
    quarter = gemm_hd(ops, L_, a8, w8, "rope", D, n_rot, one, zeros, ones)
    want = plain.clone()
    for h in range(n_rot):
        x1, x2 = plain[:, D * h:D * h + D // 2], plain[:, D * h + D // 2:D * (h + 1)]
        want[:, D * h:D * h + D // 2] = -x2                     # x1 * 0 - x2 * 1
        want[:, D * h + D // 2:D * (h + 1)] = x1                # x2 * 0 + x1 * 1
    assert torch.equal(quarter, want)
    assert torch.equal(quarter[:, n_rot * D:], plain[:, n_rot * D:])   # the v head is untouched


def test_head_dim_96_through_hd_equals_gemm_mx8(ops, L_):
    D, M, K = 96, 130, 224
    N, n_rot = (NQ + 2 * NKV) * D, NQ + NKV
    _, _, a8, w8, rstd = operands(ops, M, N, K, seed=96)
    ang = torch.rand(M, D // 2, generator=g(9)) * 6.3
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    old = gemm_hd(ops, L_, a8, w8, "rope", D, n_rot, rstd, cos, sin, entry="vgpt_gemm_mx8")
    new = gemm_hd(ops, L_, a8, w8, "rope", D, n_rot, rstd, cos, sin)
    assert torch.isfinite(old).all() and torch.equal(old, new)
    assert torch.equal(gemm_hd(ops, L_, a8, w8, "none", D, entry="vgpt_gemm_mx8"), gemm_hd(ops, L_, a8, w8, "none", D))
