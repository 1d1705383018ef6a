"""The head-grouped 256 x 288 tile of the four-wave qkv + RoPE kernel (csrc/gemm_bf16.hip, rope_grouped_col /
rope_store_grouped; include/vgpt.h vgpt_gemm_rope_grouped_col): where q, k and v have equally many 96-wide heads, column tile
t computes q head t, k head t and v head t.  Called through the C ABI with the helpers of tests/test_gemm_kernels_gpu.py:
NaN-filled allocations, padded strides, guard bands, the launch record asserted to be the four-wave kernel with NI 9.

Shapes: the smallest at which the launch decision itself picks 288-wide tiles and the grouped map applies -- M = 4096,
N = 4608 (16 + 16 + 16 heads) at K = 128 and K = 192 (an even and an odd k-tile count), and M = 2048, N = 9216 (32 + 32 + 32
heads, the sampler's width) at K = 128 -- each with and without the folded norm's rstd.  Every case checks
  * every element against float64 under the bound of test_qkv_rope_elementwise (its helpers, imported),
  * the quarter-turn probe: tables of 0 / +-1 and a one-hot A make every output +-(one weight), so a wrong partner, table
    row or head is a wrong integer,
  * bit-for-bit equality with the eight-wave family on the same operands (the k order of every element is unchanged),
  * inputs unchanged and guard bands intact (inside _rope_run).
One more case keeps the other map: N = 4608 with 36 rotated heads, which the query reports as not grouped, must still equal
the eight-wave family bit for bit.

MEASURED on one MI355X: worst |err| / bound 1.000 in all six cases (the bound is reached where the first rounding flips, as
in test_qkv_rope_elementwise); the quarter turns exact; 0 elements differ between the families; 19 tests in 3.5 s.
The family comparison needs general cos / sin tables: the quarter turns multiply by 0 and +-1 exactly and cannot tell
fma(own, cos, +-rn(other * sin)) from rn(own * cos) +- rn(other * sin).  Before the rotation was spelled out once for every
kernel (csrc/gemm_bf16.hip rope_rotate) hipcc gave the four-wave epilogues the first form and gemm_bf16_kernel's a mix of
both, and 151 - 209 of 18 874 368 elements were one bf16 step apart, on the old map and the new (profiles/README.md
round 13)."""
import pytest
import torch

from tests.test_gemm_kernels_gpu import (DEV, F32, ROPE, U32, Buf, L, _bf_bound, _expect, _family, _gamma, _launches,  # noqa: F401
                                         _one_hot, _randn, _rel, _rope_ref, _rope_run, _tables, _w_ints, _within)

pytestmark = pytest.mark.gpu
HD = 96

# id: (M, N, K, prenorm); a third of the heads each are q, k and v
CASES = {
    "n4608_k128": (4096, 4608, 128, False),
    "n4608_k128_norm": (4096, 4608, 128, True),
    "n4608_k192": (4096, 4608, 192, False),
    "n4608_k192_norm": (4096, 4608, 192, True),
    "n9216_k128": (2048, 9216, 128, False),
    "n9216_k128_norm": (2048, 9216, 128, True),
}


def _rstd(M, seed):
    """1 / rms per row over three orders of magnitude: another row's value cannot pass."""
    return (10.0 ** (torch.rand(M, device=DEV, generator=torch.Generator(DEV).manual_seed(seed)) * 3 - 1.5)).to(F32)


def _eight_wave(L, a, w, cos, sin, M, N, K, n_rot, what, rstd):
    """The same call in family 1, as _rope_run makes it; which of the eight-wave kernels takes the shape is that family's own
    plan (pinned in tests/test_gemm_kernels_gpu.py) -- here only that none of the launches is the four-wave kernel."""
    A, W, C = Buf(M, K, K + 24).set(a).freeze(), Buf(N, K, K + 40).set(w).freeze(), Buf(M, N, N + 20)
    Cs, Sn = Buf(M, HD // 2, HD // 2, F32).set(cos).freeze(), Buf(M, HD // 2, HD // 2, F32).set(sin).freeze()
    Rs = None if rstd is None else Buf(1, M, M, F32, guard=1).set(rstd[None]).freeze()
    with _family(L, 1):
        if rstd is None:
            L.call("vgpt_gemm_bf16_rope", A.ptr, W.ptr, C.ptr, Cs.ptr, Sn.ptr, M, N, K, A.ld, W.ld, C.ld, n_rot, HD, None)
        else:
            L.call("vgpt_gemm_bf16_rope_prenorm", A.ptr, W.ptr, C.ptr, Cs.ptr, Sn.ptr, Rs.ptr, M, N, K, A.ld, W.ld, C.ld, n_rot,
                   HD, None)
        got = _launches(L)
    print(f"LAUNCH {what}: {got}")
    assert got and all(r[0] >= 128 and r[1] == ROPE for r in got) and sum(r[5] for r in got) == M, f"{what}: launched {got}"
    torch.cuda.synchronize()
    return C.take(what)


def _grouped(L, N, n_rot):
    return L.load().vgpt_gemm_rope_grouped_col(N, n_rot * HD, HD, 0, 0) >= 0


_FOUR_WAVE = {}      # cid -> the four-wave kernel's output on the random operands, computed once


def _operands(cid):
    M, N, K, prenorm = CASES[cid]
    return _randn((M, K), 91), _randn((N, K), 92, 0.1), *_tables(M, HD, 93), (_rstd(M, 94) if prenorm else None)


def _four_wave(L, cid):
    if cid not in _FOUR_WAVE:
        M, N, K, _ = CASES[cid]
        a, w, cos, sin, rstd = _operands(cid)
        _FOUR_WAVE[cid] = _rope_run(L, 0, a, w, cos, sin, M, N, K, 2 * N // (3 * HD), HD, _expect(9, M, ROPE, N=N), cid, rstd)
    return _FOUR_WAVE[cid]


@pytest.mark.parametrize("cid", list(CASES))
def test_grouped_tile_elementwise(L, cid):
    M, N, K, prenorm = CASES[cid]
    n_rot = 2 * N // (3 * HD)
    assert _grouped(L, N, n_rot)
    a, w, cos, sin, rstd = _operands(cid)
    prod = a.double() @ w.double().t()
    d = _gamma(K) * (a.double().abs() @ w.double().abs().t())
    if prenorm:
        prod = prod * rstd.double()[:, None]
        d = d * rstd.double()[:, None] + U32 * prod.abs()       # one more fp32 rounding: acc * rstd
    out = _four_wave(L, cid)
    ref, e = _rope_ref(prod, d, cos, sin, n_rot, HD)
    _within(out, ref, _bf_bound(ref, e, spread=True), cid)
    assert _rel(out, ref) < 6e-3, cid


@pytest.mark.parametrize("cid", list(CASES))
def test_grouped_tile_equals_the_eight_wave_family_bit_for_bit(L, cid):
    M, N, K, _ = CASES[cid]
    a, w, cos, sin, rstd = _operands(cid)
    out = _four_wave(L, cid)
    other = _eight_wave(L, a, w, cos, sin, M, N, K, 2 * N // (3 * HD), f"{cid} eight-wave", rstd)
    diff = out.view(torch.int16) != other.view(torch.int16)
    print(f"MEASURE {cid}: {int(diff.sum())} of {diff.numel()} elements differ from the eight-wave family")
    assert not bool(diff.any()), f"{cid}: {int(diff.sum())} elements differ from the eight-wave family"


@pytest.mark.parametrize("cid", list(CASES))
def test_grouped_tile_quarter_turns_bit_for_bit(L, cid):
    M, N, K, prenorm = CASES[cid]
    n_rot = 2 * N // (3 * HD)
    w = _w_ints(N, K)
    q = (torch.arange(M, device=DEV)[:, None] + torch.arange(HD // 2, device=DEV)[None, :]) % 4
    cos, sin = (torch.tensor([1.0, 0.0, -1.0, 0.0], device=DEV)[q], torch.tensor([0.0, 1.0, 0.0, -1.0], device=DEV)[q])
    # with the folded norm: powers of two per row keep every output an exact +-(weight * 2^p)
    rstd = (2.0 ** ((torch.arange(M, device=DEV) % 5) - 2).to(F32)) if prenorm else None
    out = _rope_run(L, 0, _one_hot(M, K), w, cos, sin, M, N, K, n_rot, HD, _expect(9, M, ROPE, N=N), f"{cid} quarter turns", rstd)
    x = w.double().t()[(7 * torch.arange(M, device=DEV) + 3) % K]
    if prenorm:
        x = x * rstd.double()[:, None]
    ref, _ = _rope_ref(x, torch.zeros_like(x), cos, sin, n_rot, HD)
    assert torch.equal(out.double(), ref), f"{cid}: {int((out.double() != ref).sum())} wrong"


def test_other_head_split_keeps_the_consecutive_map(L):
    """36 rotated heads of N = 4608: not the 2 / 3 point, so three consecutive heads per tile as before."""
    M, N, K, n_rot = 4096, 4608, 128, 36
    assert not _grouped(L, N, n_rot)
    a, w = _randn((M, K), 95), _randn((N, K), 96, 0.1)
    cos, sin = _tables(M, HD, 97)
    rstd = _rstd(M, 98)
    out = _rope_run(L, 0, a, w, cos, sin, M, N, K, n_rot, HD, _expect(9, M, ROPE, N=N), "36 heads", rstd)
    other = _eight_wave(L, a, w, cos, sin, M, N, K, n_rot, "36 heads eight-wave", rstd)
    diff = out.view(torch.int16) != other.view(torch.int16)
    print(f"MEASURE 36 heads: {int(diff.sum())} of {diff.numel()} elements differ from the eight-wave family")
    assert not bool(diff.any()), f"36 heads: {int(diff.sum())} elements differ from the eight-wave family"
