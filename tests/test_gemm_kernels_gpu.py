"""Every bf16 GEMM kernel and epilogue (csrc/gemm_bf16.hip, csrc/gemm_w4_loop.inc) against an inline float64 restatement,
element by element, called through the C ABI (_lib.call) so that every row stride is the test's to choose.

  * WHICH KERNEL RAN is asserted by every case through vgpt_gemm_last_launches (kernel id, mode, transposed flags, first row,
    rows of every launch).  The grids below were found with that query on a 256-CU MI355X; when the launch plan moves, the
    case fails instead of quietly testing another kernel.  Kernel ids: 128 = the 128 x 128 kernel, 256 / 192 / 288 = the
    eight-wave 256-row kernels (four-, four- and six-phase loops), 8 / 6 / 9 = the four-wave kernel's NI (256- / 192- / 288-wide tiles);
    "split" = eight-wave 256 x 256 on the first 4096 rows, the 128 x 128 kernel on the rest through offset pointers.
  * GUARD BANDS AND STRIDES: every operand lives in an allocation with 256 guard rows before and after it (two in the one
    case whose output rows are 4 MiB each, test_output_stride_at_the_four_wave_limit) and a row stride
    larger than its width (pads that are no power of two, and for the outputs no multiple of 8 either, the ABI asking for a
    multiple of 4 only), all of it filled with a NaN bit pattern.  After the call every element outside [0, M) x [0, N) of
    an output must still hold that pattern, and inputs (guards included) must be bitwise unchanged.  An output element the
    kernel did not write is still NaN and fails the value check.
  * VALUES: random operands element-wise against fp64 under
        |out - ref| <= ulp_bf16(ref) / 2 + e + (one ulp where a bf16 rounding boundary lies within e of ref),
    e = gamma_K sum_k |a_k w_k| (+ |extra|), gamma_K = K u / (1 - K u), u = 2^-24: K exact bf16 products added in fp32 in any
    order, the residual / bias being one more addend of the same chain before the one rounding.  Integer-valued operands
    whose partial sums stay below 2^24 add exactly in any order: those outputs equal the correctly rounded fp64 value BIT
    FOR BIT.  Epilogues that qualify for the exact check: none / bias / residual (added in fp32 before the one rounding),
    the stored [gate | up] of the keep form, dX / dW, and RoPE with tables of 0 and +-1 (quarter turns); the activations and
    a general rotation do not.  A global rel-L2 (4e-3, as tests/test_ops_gpu.py) stands next to every element-wise bound.

Measured on one MI355X: the 85 value cases take 4.0 s together (the slowest, the first to touch the device, 1.0 s; the others 0.03
to 0.25 s).  Worst |err| / bound per group (MEASURE lines): plain epilogues 0.993 over 68 cases, dX 0.983, dW 0.993, stored
[gate | up] 0.991, activations 0.999, RoPE 1.000 (0.9995: the bound is reached where the first rounding flips), rstd 2.2e-7
relative under 3e-6.  The ratios sit just under 1 by construction: ulp / 2 is what a correct final rounding reaches among 16 M
outputs, and the accumulation term e is 1e-5 .. 1e-4 of it at these K -- there is no slack for a wrong element to hide in.
test_launch_decision_at_workload_shapes adds 22 calls that check the launch record alone, 2.3 s together."""
import contextlib
import ctypes
import importlib

import pytest
import torch

from tests.test_train_kernels_gpu import ACTS, U32, _ulp, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPI_NONE, EPI_RESID, EPI_BIAS = 0, 1, 2
PLAIN, GATED, ROPE = 0, 1, 2
GUARD = 256            # guard rows before and after every matrix: one full tile of the largest kernel
SENT16 = 0x7FC3        # a bf16 NaN
SENT32 = 0x7FC35A5A    # an fp32 NaN


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("video-gpt_amd._lib")


@contextlib.contextmanager
def _family(L, fam):
    lib = L.load()
    prev = lib.vgpt_gemm_set_family(fam)
    try:
        yield
    finally:
        lib.vgpt_gemm_set_family(prev)


def _launches(L):
    buf = (ctypes.c_int32 * 48)()
    n = L.load().vgpt_gemm_last_launches(buf, 8)
    assert 0 <= n <= 8
    return [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]


def _expect(kernel, M, mode=PLAIN, atr=0, wtr=0, N=4096):
    """The launch record a case is meant for.  "split" (20 row tiles, eight-wave family): N = 4096 gives 256 x 256 tiles up
    to row 4096; the ragged widths (21 column tiles of 192, 4032 included) give 256 x 192 tiles up to row 3072; the 128 x 128
    kernel takes the remaining rows in both."""
    if kernel == "split":
        big, m1 = (256, 4096) if N == 4096 or mode == GATED else (192, 3072)
        return [(big, mode, atr, wtr, 0, m1), (128, mode, atr, wtr, m1, M - m1)]
    return [(kernel, mode, atr, wtr, 0, M)]


def _ran(L, expect, what):
    got = _launches(L)
    print(f"LAUNCH {what}: {got}")
    assert got == expect, f"{what}: launched {got}, this case is meant for {expect}"


class Buf:
    """A (rows, width) matrix of row stride ld inside an allocation with `guard` rows of ld elements (or `pad` elements)
    before and after it; guard rows, gap columns and (until set) the matrix itself hold a NaN bit pattern."""

    def __init__(self, rows, width, ld, dtype=BF, guard=GUARD, pad=None):
        assert ld >= width
        self.rows, self.width, self.ld = rows, width, ld
        self.lead = guard * ld if pad is None else pad
        self.idt, self.sent = (torch.int16, SENT16) if dtype == BF else (torch.int32, SENT32)
        self.raw = torch.full((2 * self.lead + rows * ld,), self.sent, dtype=self.idt, device=DEV)
        self.m = self.raw.view(dtype)[self.lead:self.lead + rows * ld].view(rows, ld)[:, :width]
        self.ptr = self.m.data_ptr()
        self.snap = None

    def set(self, t):
        self.m.copy_(t.to(DEV))
        return self

    def freeze(self):
        self.snap = self.raw.clone()
        return self

    def unchanged(self, what):
        assert torch.equal(self.raw, self.snap), f"{what}: an input buffer or its guard band was written"

    def take(self, what):
        """The matrix as the kernel left it; everything around it must still be the fill pattern."""
        out = self.m.clone()
        self.m.view(self.idt).fill_(self.sent)
        bad = (self.raw != self.sent).nonzero()
        if bad.numel():
            r, c = divmod(int(bad[0]) - self.lead, self.ld)
            raise AssertionError(f"{what}: {bad.shape[0]} elements outside the {self.rows} x {self.width} output were written, "
                                 f"the first at row {r}, column {c} (row stride {self.ld})")
        return out


def _rbf(x):
    return x.to(F32).to(BF).double()


def _gamma(K):
    return K * U32 / (1 - K * U32)


def _bf_bound(ref, e, spread=False):
    """ulp(ref) / 2 + e, plus one ulp where a value within e of ref rounds to another bf16 than ref - e does.
    spread: e is an error the kernel really makes, not a worst case nobody reaches (the first rounding of the RoPE epilogue
    falling on the other side, an activation that cancels to zero), and may exceed |ref|: the value that is rounded lies
    within e of ref, so the ulp of the final rounding is taken at |ref| + e.  (With ulp(ref) the RoPE cases measured
    1.002 .. 1.003: a product of ~100 whose rounding flipped, rotated to a ref near zero -- the output's last bit is then
    2^-8 of e, not of ref.)"""
    near = _rbf(ref - e) != _rbf(ref + e)
    ulp = _ulp(ref.abs() + e) if spread else _ulp(ref)
    return ulp / 2 + e + near * ulp + 1e-30


def _rel(out, ref):
    return float((out.double() - ref).norm() / (ref.norm() + 1e-30))


def _randn(shape, seed, scale=1.0):
    gen = torch.Generator(DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=gen) * scale).to(BF)


def _ints(shape, seed, lo, hi):
    gen = torch.Generator(DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=gen).to(BF)


def _one_hot(M, K):
    """Row m selects k = (7 m + 3) mod K: the product is a gather of W's columns, so a swapped, dropped or repeated k-tile and
    a permuted row or column all give a wrong integer."""
    a = torch.zeros(M, K, dtype=BF, device=DEV)
    a[torch.arange(M, device=DEV), (7 * torch.arange(M, device=DEV) + 3) % K] = 1
    return a


def _w_ints(N, K):
    """Asymmetric integers in [-125, 125] (exact in bf16)."""
    n, k = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :]
    return ((n * 131 + k * 17) % 251 - 125).to(BF)


# ============================================================================================================
# the plain product: vgpt_gemm_bf16 and vgpt_gemm_bf16_tr
# ============================================================================================================
def _gemm(L, fam, a, w, M, N, K, expect, what, epi=EPI_NONE, extra=None, inplace=False, atr=0, wtr=0, ldc=None, guard=GUARD):
    """a, w: the operands as stored, (M, K) / (N, K) or, transposed, (K, M) / (K, N)."""
    A = Buf(a.shape[0], a.shape[1], a.shape[1] + 24).set(a).freeze()
    W = Buf(w.shape[0], w.shape[1], w.shape[1] + 40).set(w).freeze()
    C = Buf(M, N, ldc or N + 20, guard=guard)
    X, xptr, ldr = None, None, 0
    if epi == EPI_RESID and inplace:
        C.set(extra)
        xptr, ldr = C.ptr, C.ld
    elif epi == EPI_RESID:
        X = Buf(M, N, N + 36).set(extra).freeze()
        xptr, ldr = X.ptr, X.ld
    elif epi == EPI_BIAS:
        X = Buf(1, N, N + 12).set(extra[None]).freeze()
        xptr = X.ptr
    with _family(L, fam):
        if atr or wtr:
            L.call("vgpt_gemm_bf16_tr", A.ptr, W.ptr, C.ptr, xptr, M, N, K, A.ld, W.ld, C.ld, ldr, epi, atr, wtr, None)
        else:
            L.call("vgpt_gemm_bf16", A.ptr, W.ptr, C.ptr, xptr, M, N, K, A.ld, W.ld, C.ld, ldr, epi, None)
        _ran(L, expect, what)
    torch.cuda.synchronize()
    out = C.take(what)
    for b in (A, W, X):
        if b is not None:
            b.unchanged(what)
    return out


# kernel -> family, exact-fit grid, ragged M (one tail row in the first / second 128-row half of the last tile), ragged N
# (N % 8 == 4, N % 16 == 8: both sides of the four-wave epilogue's 16-byte switch, each a last column tile under one sub-tile
# wide; and a last column tile of exactly one 16-column sub-tile), K of the epilogue cases, k-tile counts of the sweep
PLAIN_KERNELS = {
    "k128": dict(kernel=128, fam=0, M0=256, Mr=(257, 385), N0=256, Nr=(268, 264, 272), K=128, nks=(1, 2, 3, 4, 5, 6, 7, 9, 13)),
    "w4_ni8": dict(kernel=8, fam=0, M0=4096, Mr=(3841, 3969), N0=4096, Nr=(3852, 3848, 3856), K=128,
                   nks=(2, 3, 4, 5, 6, 7, 9, 13)),
    "w4_ni6": dict(kernel=6, fam=0, M0=2048, Mr=(1793, 1921), N0=4096, Nr=(3852, 3848, 3856), K=128,
                   nks=(2, 3, 4, 5, 6, 7, 9, 13)),
    # NI = 9 takes whole tiles only (test_four_wave_288_takes_whole_tiles_only)
    "w4_ni9": dict(kernel=9, fam=0, M0=4096, Mr=(), N0=4608, Nr=(), K=128, nks=(2, 3, 4, 5, 6, 7, 9, 13)),
    "e8_256": dict(kernel=256, fam=1, M0=4096, Mr=(3841, 3969), N0=4096, Nr=(3852, 3848, 3856), K=128,
                   nks=(1, 2, 3, 4, 5, 6, 7, 9, 13)),
    "e8_192": dict(kernel=192, fam=1, M0=2048, Mr=(1793, 1921), N0=4096, Nr=(3852, 3848, 3856), K=128,
                   nks=(1, 2, 3, 4, 5, 6, 7, 9, 13)),
    # 256 x 288 tiles are taken where they save a round against an UNSPLIT plan of 192- / 256-wide tiles.  With several row
    # tiles that starts at 4096 x 9216 with 11 k-tiles (below, the split plan is cheaper, and a split plan never takes them);
    # with ONE row tile no plan can split, and 228 tiles of 288 columns (one round against two of 342 x 192 or 257 x 256) take
    # them at every k-tile count.  N must be a multiple of 288, M may be ragged: a tail in the second 128-row half, a single row
    "e8_288": dict(kernel=288, fam=1, M0=256, Mr=(129, 1), N0=65664, Nr=(), K=128, nks=(1, 2, 3, 4, 5, 6, 7, 9, 13)),
    "e8_split": dict(kernel="split", fam=1, M0=5120, Mr=(4865, 4993), N0=4096, Nr=(3852, 3848, 3856), K=128,
                     nks=(1, 2, 3, 4, 5, 6, 7, 9, 13)),
}


@pytest.mark.parametrize("kid", list(PLAIN_KERNELS))
def test_plain_epilogues_elementwise_with_guard_bands(L, kid):
    """a + d + e: none / bias / residual (out of place and in place), exact-fit and ragged, random values."""
    p = PLAIN_KERNELS[kid]
    M0, N0, K = p["M0"], max((p["N0"],) + p["Nr"]), p["K"]
    Mx = max((M0,) + p["Mr"])
    a, w = _randn((Mx, K), 11), _randn((N0, K), 12, 0.1)
    r, b = _randn((Mx, N0), 13), _randn((N0,), 14)
    prod = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    cases = [(M0, p["N0"], e) for e in ("none", "bias", "resid", "inplace")]
    if p["Nr"]:
        (m1, m2), (n1, n2, n3) = p["Mr"], p["Nr"]
        cases += [(m1, n1, "resid"), (m1, n1, "none"), (m2, n2, "bias"), (m2, n2, "inplace"), (M0, n3, "resid"), (m1, p["N0"], "inplace")]
    elif p["Mr"]:
        cases = [(M0, p["N0"], "resid"), (M0, p["N0"], "bias"), (p["Mr"][0], p["N0"], "inplace"), (p["Mr"][1], p["N0"], "none")]
    for M, N, e in cases:
        what = f"{kid} {M}x{N}x{K} {e}"
        epi = {"none": EPI_NONE, "bias": EPI_BIAS}.get(e, EPI_RESID)
        extra = None if e == "none" else (b[:N] if e == "bias" else r[:M, :N])
        out = _gemm(L, p["fam"], a[:M], w[:N], M, N, K, _expect(p["kernel"], M, N=N), what, epi, extra, inplace=e == "inplace")
        ref, s = prod[:M, :N], mag[:M, :N]
        if extra is not None:
            ref, s = ref + extra.double(), s + extra.double().abs()
        # measured worst |err| / bound over all kernels and cases: 0.993 (the formula of the module docstring, nothing fitted)
        _within(out, ref, _bf_bound(ref, _gamma(K) * s), what)
        assert _rel(out, ref) < 4e-3, what


def _exact_integer_products(L, kid):
    """b: a one-hot A (a gather of W's columns) plus an integer residual, in place, on the ragged grid; dense small integers
    plus an integer bias on the exact grid, where the output needs the one rounding (|sum| up to K * 2 * 125 < 2^24)."""
    p = PLAIN_KERNELS[kid]
    K = max(p["K"], 192)       # three k-tiles or more: a swap of two of them moves a row's k out of its tile
    M, N = (p["Mr"][0] if p["Mr"] else p["M0"]), (p["Nr"][0] if p["Nr"] else p["N0"])
    w = _w_ints(N, K)
    r = _ints((M, N), 21, -100, 100)
    out = _gemm(L, p["fam"], _one_hot(M, K), w, M, N, K, _expect(p["kernel"], M, N=N), f"{kid} one-hot", EPI_RESID, r, inplace=True)
    ref = w.double().t()[(7 * torch.arange(M, device=DEV) + 3) % K] + r.double()
    assert ref.abs().max() <= 256 and torch.equal(out.double(), ref), f"{kid} one-hot: {int((out.double() != ref).sum())} wrong"
    M, N = p["M0"], p["N0"]
    a, w, b = _ints((M, K), 22, -2, 2), _w_ints(N, K), _ints((N,), 23, -100, 100)
    out = _gemm(L, p["fam"], a, w, M, N, K, _expect(p["kernel"], M), f"{kid} dense integers", EPI_BIAS, b)
    ref = a.double() @ w.double().t() + b.double()
    assert ref.abs().max() < 2 ** 24
    assert torch.equal(out, ref.to(F32).to(BF)), f"{kid} dense integers: {int((out != ref.to(F32).to(BF)).sum())} wrong"


def test_gemm_is_not_transposed(L):
    """The 128 x 128 kernel's one-hot and integer cases (this name had a single A = I case in tests/test_ops_gpu.py): a
    swapped row / column map, a permuted column or a misplaced k-tile is a wrong integer."""
    _exact_integer_products(L, "k128")


@pytest.mark.parametrize("kid", [k for k in PLAIN_KERNELS if k != "k128"])
def test_exact_integer_products_bit_for_bit(L, kid):
    """The same on every 256-row kernel: eight-wave 256 / 192 / 288 / split, four-wave NI 8 / 6 / 9."""
    _exact_integer_products(L, kid)


@pytest.mark.parametrize("kid", list(PLAIN_KERNELS))
def test_k_tile_sweep(L, kid):
    """c: every k-tile count at and below the pipelines' depths and odd ones after, on the kernel's one-round grid, bit for
    bit on integers: a k-tile dropped in a prologue or read twice in a drain is a wrong integer."""
    p = PLAIN_KERNELS[kid]
    M, N, Kmax = p["M0"], p["N0"], 64 * max(p["nks"])
    a, w = _ints((M, Kmax), 31, -2, 2), _w_ints(N, Kmax)
    for nk in p["nks"]:
        K = 64 * nk
        out = _gemm(L, p["fam"], a[:, :K], w[:, :K], M, N, K, _expect(p["kernel"], M), f"{kid} nk={nk}")
        ref = (a[:, :K].double() @ w[:, :K].double().t()).to(F32).to(BF)
        assert torch.equal(out, ref), f"{kid} nk={nk}: {int((out != ref).sum())} wrong"


@pytest.mark.parametrize("kid,fallback", [("w4_ni8", [(256, 0, 0, 0, 0, 4096)]), ("w4_ni6", [(192, 0, 0, 0, 0, 2048)]),
                                          ("w4_ni9", [(192, 0, 0, 0, 0, 2560), (128, 0, 0, 0, 2560, 1536)])])
def test_one_k_tile_leaves_the_four_wave_kernel(L, kid, fallback):
    """The four-wave loop needs two k-tiles: at K = 64 its grids go to the eight-wave kernels (the NI = 9 grid to a split
    plan of 192-wide tiles), and are right."""
    p = PLAIN_KERNELS[kid]
    M, N, K = p["M0"], p["N0"], 64
    a, w = _ints((M, K), 32, -2, 2), _w_ints(N, K)
    out = _gemm(L, 0, a, w, M, N, K, fallback, f"{kid} nk=1")
    assert torch.equal(out, (a.double() @ w.double().t()).to(F32).to(BF))


@pytest.mark.parametrize("M,N,kernel", [(4095, 4608, 6), (4096, 4612, 6)])
def test_four_wave_288_takes_whole_tiles_only(L, M, N, kernel):
    """One row or four columns off its grid, the NI = 9 shape goes to another tile width, and is right."""
    K = 128
    a, w, r = _randn((M, K), 41), _randn((N, K), 42, 0.1), _randn((M, N), 43)
    out = _gemm(L, 0, a, w, M, N, K, _expect(kernel, M), f"ragged ni9 grid {M}x{N}", EPI_RESID, r)
    ref = a.double() @ w.double().t() + r.double()
    s = a.double().abs() @ w.double().abs().t() + r.double().abs()
    _within(out, ref, _bf_bound(ref, _gamma(K) * s), f"ragged ni9 grid {M}x{N}")


@pytest.mark.parametrize("ldc,kernel", [(2 ** 21 - 4, 6), (2 ** 21, 192)])
def test_output_stride_at_the_four_wave_limit(L, ldc, kernel):
    """The four-wave epilogue forms 32-bit byte offsets (row in tile * ldc + column) * 2 from the tile's origin: rows strides
    up to 2^21 - 4 stay on it, 2^21 goes to the eight-wave family.  Two guard rows here (a row is 4 MiB)."""
    M, N, K = 257, 16384, 128
    a, w = _ints((M, K), 51, -2, 2), _w_ints(N, K)
    out = _gemm(L, 0, a, w, M, N, K, _expect(kernel, M), f"ldc={ldc}", ldc=ldc, guard=2)
    assert torch.equal(out, (a.double() @ w.double().t()).to(F32).to(BF))


# ---- transposed operands: dX = dY W (W stored (K, N)), dW = dY^T X (both stored with the reduction index as the row) ----
TR_KERNELS = {"k128": (128, 0, 256, 264), "w4_ni8": (8, 0, 4096, 4096), "w4_ni6": (6, 0, 2048, 4096), "e8_256": (256, 1, 4096, 4096)}


@pytest.mark.parametrize("kid", list(TR_KERNELS))
def test_dx_transposed_weight(L, kid):
    """i: W as (K, N) row-major, with a residual; ragged rows, N a multiple of 8; random values and a one-hot gather."""
    kernel, fam, M0, N = TR_KERNELS[kid]
    K = 192
    for M in (M0, M0 - 127):
        what = f"dX {kid} {M}x{N}x{K}"
        a, wt, r = _randn((M, K), 61), _randn((K, N), 62, 0.1), _randn((M, N), 63)
        out = _gemm(L, fam, a, wt, M, N, K, _expect(kernel, M, wtr=1), what, EPI_RESID, r, wtr=1)
        ref = a.double() @ wt.double() + r.double()
        s = a.double().abs() @ wt.double().abs() + r.double().abs()
        _within(out, ref, _bf_bound(ref, _gamma(K) * s), what)       # measured worst ratio 0.983
        assert _rel(out, ref) < 4e-3
    wt = _w_ints(N, K).t().contiguous()
    out = _gemm(L, fam, _one_hot(M0, K), wt, M0, N, K, _expect(kernel, M0, wtr=1), f"dX {kid} one-hot", wtr=1)
    assert torch.equal(out.double(), wt.double()[(7 * torch.arange(M0, device=DEV) + 3) % K])


@pytest.mark.parametrize("kid", list(TR_KERNELS))
@pytest.mark.parametrize("Kred", [129, 191])
def test_dw_both_transposed(L, kid, Kred):
    """i: reduction lengths 64 k + 1 and 64 k + 63: the rows of the partial last reduction tile are the guard band's NaNs in
    memory and must be read as zeros.  Integers, bit for bit, and random values."""
    kernel, fam, M, N = TR_KERNELS[kid]
    what = f"dW {kid} {M}x{N} over {Kred}"
    at, wt = _ints((Kred, M), 71, -2, 2), _w_ints(N, Kred).t().contiguous()
    out = _gemm(L, fam, at, wt, M, N, Kred, _expect(kernel, M, atr=1, wtr=1), what + " integers", atr=1, wtr=1)
    assert torch.equal(out, (at.double().t() @ wt.double()).to(F32).to(BF)), what
    at, wt = _randn((Kred, M), 72), _randn((Kred, N), 73, 0.1)
    out = _gemm(L, fam, at, wt, M, N, Kred, _expect(kernel, M, atr=1, wtr=1), what, atr=1, wtr=1)
    ref, s = at.double().t() @ wt.double(), at.double().abs().t() @ wt.double().abs()
    _within(out, ref, _bf_bound(ref, _gamma(Kred) * s), what)
    assert _rel(out, ref) < 4e-3


# ============================================================================================================
# qkv + RoPE: vgpt_gemm_bf16_rope, vgpt_gemm_bf16_rope_prenorm
# ============================================================================================================
def _rope_run(L, fam, a, w, cos, sin, M, N, K, n_rot, hd, expect, what, rstd=None):
    A = Buf(M, K, K + 24).set(a).freeze()
    W = Buf(N, K, K + 40).set(w).freeze()
    C = Buf(M, N, N + 20)
    # the tables are dense (M, hd / 2) fp32; the rows before and after them are NaNs
    Cs, Sn = Buf(M, hd // 2, hd // 2, F32).set(cos).freeze(), Buf(M, hd // 2, hd // 2, F32).set(sin).freeze()
    Rs = None if rstd is None else Buf(1, M, M, F32, guard=1).set(rstd[None]).freeze()
    with _family(L, fam):
        if rstd is None:
            L.call("vgpt_gemm_bf16_rope", A.ptr, W.ptr, C.ptr, Cs.ptr, Sn.ptr, M, N, K, A.ld, W.ld, C.ld, n_rot, hd, None)
        else:
            L.call("vgpt_gemm_bf16_rope_prenorm", A.ptr, W.ptr, C.ptr, Cs.ptr, Sn.ptr, Rs.ptr, M, N, K, A.ld, W.ld, C.ld, n_rot,
                   hd, None)
        _ran(L, expect, what)
    torch.cuda.synchronize()
    out = C.take(what)
    for b in (A, W, Cs, Sn, Rs):
        if b is not None:
            b.unchanged(what)
    return out


def _tables(M, hd, seed):
    """cos / sin (M, hd / 2) fp32 of angles pos[m] * 10000^(-2 i / hd), every row its own position (a permutation)."""
    gen = torch.Generator(DEV).manual_seed(seed)
    pos = torch.randperm(M, device=DEV, generator=gen).double()
    ang = pos[:, None] * (10000.0 ** (-torch.arange(hd // 2, device=DEV).double() * 2 / hd))[None, :]
    return ang.cos().to(F32), ang.sin().to(F32)


def _rope_ref(prod, d, cos, sin, n_rot, hd):
    """fp64 restatement: the product (known to within d) rounded to bf16, rotated with the fp32 tables, rounded again.
    Returns (ref, e) for _bf_bound.  Where a rounding boundary lies within d of the product the kernel's first rounding may
    fall on either side: x is then known as the midpoint xm of the two candidates +- their half distance h (h = 0 elsewhere),
    and that ulp travels through the rotation as |c| h(own) + |s| h(partner).  The rotation itself is three fp32 operations
    (or one product and one fused multiply-add): 3 u (|x c| + |y s|).  The V columns are the product rounded once."""
    M, half, R = prod.shape[0], hd // 2, n_rot * hd
    lo, hi = _rbf(prod[:, :R] - d[:, :R]), _rbf(prod[:, :R] + d[:, :R])
    xm, h = ((lo + hi) / 2).view(M, n_rot, 2, half), ((hi - lo) / 2).view(M, n_rot, 2, half)
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    x, y, hx, hy = xm[:, :, 0], xm[:, :, 1], h[:, :, 0], h[:, :, 1]
    ref = torch.stack([x * c - y * s, y * c + x * s], 2).reshape(M, R)
    fl = 3 * U32 * ((x * c).abs() + (y * s).abs())
    fu = 3 * U32 * ((y * c).abs() + (x * s).abs())
    e = torch.stack([c.abs() * hx + s.abs() * hy + fl, c.abs() * hy + s.abs() * hx + fu], 2).reshape(M, R)
    return torch.cat([ref, prod[:, R:]], 1), torch.cat([e, d[:, R:]], 1)


# id: (family, kernel, M, N, K, head_dim, rotated heads, prenorm).  rope_cols = rotated heads * head_dim on / off a tile
# boundary of the kernel's tile width; M with a tail in the last tile wherever the kernel takes one; the two four-wave limits
# (tables of head dim 128 do not fit its LDS; 288-wide tiles are whole) asserted as what the query reports
ROPE_CASES = {
    "ni8_hd64_on": (0, 8, 3969, 4096, 128, 64, 56, False),        # 3584 = 14 * 256
    "ni8_hd64_off": (0, 8, 3841, 4096, 128, 64, 57, True),
    "ni8_hd96_off": (0, 8, 3969, 4032, 128, 96, 35, False),
    "ni6_hd64_on": (0, 6, 1921, 4096, 128, 64, 57, False),        # 3648 = 19 * 192
    "ni6_hd96_on": (0, 6, 1793, 4032, 128, 96, 32, True),         # 3072 = 16 * 192
    "ni6_hd96_off": (0, 6, 1921, 4032, 128, 96, 35, False),
    "ni9_hd96_on": (0, 9, 4096, 4608, 128, 96, 36, False),        # 3456 = 12 * 288
    "ni9_hd96_off": (0, 9, 4096, 4608, 128, 96, 40, True),
    "ni9_hd64_off": (0, 9, 4096, 4608, 128, 64, 58, False),
    "fam0_hd128": (0, 256, 3969, 4096, 128, 128, 25, False),      # head dim 128: not a four-wave shape
    "e256_hd128_on": (1, 256, 3841, 4096, 128, 128, 24, True),    # 3072 = 12 * 256
    "e256_hd64_off": (1, 256, 3969, 4096, 128, 64, 57, False),
    "e192_hd128_off": (1, 192, 1921, 4096, 128, 128, 25, False),  # tables read from global memory (no room in LDS)
    "e192_hd96_on": (1, 192, 1793, 4032, 128, 96, 32, True),
    "e288_hd96_off": (1, 288, 129, 65664, 128, 96, 601, False),   # one row tile (PLAIN_KERNELS); 57696 = 200.33 * 288
    "e288_hd96_on": (1, 288, 256, 65664, 128, 96, 600, True),     # 57600 = 200 * 288
    "e288_hd64_off": (1, 288, 200, 65664, 192, 64, 1001, False),
    "e288_hd128_on": (1, 288, 1, 65664, 128, 128, 450, True),     # 57600; a single row
    "split_hd64": (1, "split", 4865, 4096, 128, 64, 57, False),   # the remainder launch reads the tables from row 4096 on
    "split_hd96_norm": (1, "split", 4993, 4032, 128, 96, 35, True),   # 192-wide tiles, then the rstd too from row 3072 on
    "k128_hd64": (0, 128, 300, 320, 128, 64, 3, False),
    "k128_hd128_norm": (0, 128, 257, 384, 128, 128, 2, True),
}


@pytest.mark.parametrize("cid", list(ROPE_CASES))
def test_qkv_rope_elementwise(L, cid):
    fam, kernel, M, N, K, hd, n_rot, prenorm = ROPE_CASES[cid]
    a, w = _randn((M, K), 81), _randn((N, K), 82, 0.1)
    cos, sin = _tables(M, hd, 83)
    prod = a.double() @ w.double().t()
    d = _gamma(K) * (a.double().abs() @ w.double().abs().t())
    rstd = None
    if prenorm:      # rows of very different 1 / rms (three orders of magnitude): another row's value cannot pass
        rstd = (10.0 ** (torch.rand(M, device=DEV, generator=torch.Generator(DEV).manual_seed(84)) * 3 - 1.5)).to(F32)
        prod = prod * rstd.double()[:, None]
        d = d * rstd.double()[:, None] + U32 * prod.abs()       # one more fp32 rounding: acc * rstd
    out = _rope_run(L, fam, a, w, cos, sin, M, N, K, n_rot, hd, _expect(kernel, M, ROPE, N=N), cid, rstd)
    ref, e = _rope_ref(prod, d, cos, sin, n_rot, hd)
    _within(out, ref, _bf_bound(ref, e, spread=True), cid)
    assert _rel(out, ref) < 6e-3, cid


@pytest.mark.parametrize("kid", ["k128", "w4_ni8", "w4_ni6", "w4_ni9", "e8_256", "e8_192", "e8_split"])
def test_qkv_rope_quarter_turns_bit_for_bit(L, kid):
    """b for the rotation: tables of 0 and +-1 (the quarter turns, by (row + column) mod 4) and a one-hot A make every output
    +-(one weight): exact, so a wrong partner column, a wrong table row or a wrong head shows as a wrong integer."""
    p = PLAIN_KERNELS[kid]
    M, N, K, hd = (p["Mr"][1] if p["Mr"] else p["M0"]), p["N0"], 192, 64
    n_rot = N // hd - (7 if N > 1024 else 1)
    w = _w_ints(N, K)
    q = (torch.arange(M, device=DEV)[:, None] + torch.arange(hd // 2, device=DEV)[None, :]) % 4
    cos, sin = (torch.tensor([1.0, 0.0, -1.0, 0.0], device=DEV)[q], torch.tensor([0.0, 1.0, 0.0, -1.0], device=DEV)[q])
    out = _rope_run(L, p["fam"], _one_hot(M, K), w, cos, sin, M, N, K, n_rot, hd, _expect(p["kernel"], M, ROPE), f"{kid} quarter turns")
    x = w.double().t()[(7 * torch.arange(M, device=DEV) + 3) % K]
    ref, _ = _rope_ref(x, torch.zeros_like(x), cos, sin, n_rot, hd)
    assert torch.equal(out.double(), ref), f"{kid}: {int((out.double() != ref).sum())} wrong"


# ============================================================================================================
# gated MLP: vgpt_gated_mlp_act_fwd, _keep, _prenorm
# ============================================================================================================
def _gated_run(L, fam, form, a, w, M, I, K, act, expect, what, rstd=None):
    A = Buf(M, K, K + 24).set(a).freeze()
    W = Buf(2 * I, K, K + 40).set(w).freeze()
    O = Buf(M, I, I + 20)
    G = Buf(M, 2 * I, 2 * I + 12) if form == "keep" else None
    Rs = Buf(1, M, M, F32, guard=1).set(rstd[None]).freeze() if form == "prenorm" else None
    with _family(L, fam):
        if form == "keep":
            L.call("vgpt_gated_mlp_act_fwd_keep", A.ptr, W.ptr, O.ptr, G.ptr, M, I, K, A.ld, W.ld, O.ld, G.ld, act, None)
        elif form == "prenorm":
            L.call("vgpt_gated_mlp_act_fwd_prenorm", A.ptr, W.ptr, O.ptr, Rs.ptr, M, I, K, A.ld, W.ld, O.ld, act, None)
        else:
            L.call("vgpt_gated_mlp_act_fwd", A.ptr, W.ptr, O.ptr, M, I, K, A.ld, W.ld, O.ld, act, None)
        _ran(L, expect, what)
    torch.cuda.synchronize()
    out, gu = O.take(what), (G.take(what + " [gate | up]") if G is not None else None)
    for b in (A, W, Rs):
        if b is not None:
            b.unchanged(what)
    return out, gu


# kernel -> family, M exact / ragged, I: exact; one sub-tile in the last tile (I % 32 == 16: the paired 16-byte store's odd
# one out); three sub-tiles in the last tile (odd, I % 32 == 16)
GATED_KERNELS = {
    "k128": dict(kernel=128, fam=0, Ms=(256, 257), Is=(128, 144, 176)),
    "w4_ni8": dict(kernel=8, fam=0, Ms=(4096, 3969), Is=(2048, 1936, 1968)),
    "w4_ni6": dict(kernel=6, fam=0, Ms=(2048, 1793), Is=(2048, 1936, 1968)),
    "e8_256": dict(kernel=256, fam=1, Ms=(4096, 3841), Is=(2048, 1936, 1968)),
    "e8_split": dict(kernel="split", fam=1, Ms=(5120, 4993), Is=(2048, 1936, 1968)),
}


@pytest.mark.parametrize("kid", list(GATED_KERNELS))
def test_gated_mlp_elementwise(L, kid):
    """g: act(gate) * up of the fp32 accumulators.  gate and up are known to within dg, du = gamma_K sum |a w| (times rstd, plus
    one rounding, with the folded norm); through the activation (|act'| <= 1.13 for all three) and the product that is
    1.13 dg |up| + |act(gate)| du, plus the activation's own fp32 evaluation: 4 u |ref| and the 1e-6 |gate up| floor of
    tests/test_train_kernels_gpu.py section C (cancellation of 1 + erf / 1 + tanh in the tails).  Every 7th gate column has
    weights 30 times larger: saturated tails on both sides."""
    p = GATED_KERNELS[kid]
    K, (I0, I1, I2), (M0, M1) = 128, p["Is"], p["Ms"]
    a = _randn((max(M0, M1), K), 91)
    wg, wu = _randn((max(p["Is"]), K), 92, 0.05), _randn((max(p["Is"]), K), 93, 0.1)
    wg[3::7] = (wg[3::7].float() * 30).to(BF)
    a64 = a.double()
    gate, up = a64 @ wg.double().t(), a64 @ wu.double().t()
    dg, du = _gamma(K) * (a64.abs() @ wg.double().abs().t()), _gamma(K) * (a64.abs() @ wu.double().abs().t())
    assert gate.abs().max() > 20
    rstd = (10.0 ** (torch.rand(max(M0, M1), device=DEV, generator=torch.Generator(DEV).manual_seed(94)) * 3 - 1.5)).to(F32)
    cases = [("fwd", M0, I0, 0), ("fwd", M1, I1, 1), ("fwd", M1, I2, 2), ("prenorm", M1, I1, 0), ("prenorm", M0, I2, 0),
             ("keep", M1, I1, 0), ("keep", M0, I2, 1), ("keep", M1, I0, 2)]
    for form, M, I, act in cases:
        what = f"{kid} gated {form} {M}x{I}x{K} act {act}"
        w = torch.cat([wg[:I], wu[:I]], 0)
        out, gu = _gated_run(L, p["fam"], form, a[:M], w, M, I, K, act, _expect(p["kernel"], M, GATED), what, rstd[:M])
        g_, u_, dg_, du_ = gate[:M, :I], up[:M, :I], dg[:M, :I], du[:M, :I]
        if form == "prenorm":
            rs = rstd[:M].double()[:, None]
            g_, u_ = g_ * rs, u_ * rs
            dg_, du_ = dg_ * rs + U32 * g_.abs(), du_ * rs + U32 * u_.abs()
        if form == "keep":
            # the stored [gate | up] is the product rounded once; the activation is formed from those stored bits
            _within(gu[:, :I], g_, _bf_bound(g_, dg_), what + " stored gate")
            _within(gu[:, I:], u_, _bf_bound(u_, du_), what + " stored up")
            g_, u_ = gu[:, :I].double(), gu[:, I:].double()
            dg_, du_ = torch.zeros_like(g_), torch.zeros_like(u_)
        ref = ACTS[act](g_) * u_
        e = 1.13 * dg_ * u_.abs() + ACTS[act](g_).abs() * du_ + 4 * U32 * ref.abs() + 1e-6 * (g_ * u_).abs()
        _within(out, ref, _bf_bound(ref, e, spread=True), what)
        assert _rel(out, ref) < 4e-3, what


@pytest.mark.parametrize("kid", list(GATED_KERNELS))
def test_gated_keep_stores_exact_integers(L, kid):
    """b for the keep form: the stored [gate | up] of a one-hot A is W's gathered columns, bit for bit."""
    p = GATED_KERNELS[kid]
    M, I, K = p["Ms"][1], p["Is"][1], 192
    w = _w_ints(2 * I, K)
    _, gu = _gated_run(L, p["fam"], "keep", _one_hot(M, K), w, M, I, K, 0, _expect(p["kernel"], M, GATED), f"{kid} keep one-hot")
    assert torch.equal(gu.double(), w.double().t()[(7 * torch.arange(M, device=DEV) + 3) % K])


# ============================================================================================================
# the residual GEMM that also leaves 1 / rms of its output rows: vgpt_gemm_bf16_resid_rstd (four-wave kernel only)
# ============================================================================================================
@pytest.mark.parametrize("kernel,M,N,K", [(8, 3969, 4084, 128), (6, 1793, 3852, 192), (8, 4096, 4096, 128)])
def test_resid_rstd(L, kernel, M, N, K):
    """h: the output under the plain residual bound; rstd against fp64 on the ROUNDED output over exactly N columns (a ragged
    N: the clamped columns past N hold real products and must not count); the arrival counters back at zero; the same bits
    on a relaunch; a workspace of exactly the reported size with a NaN tail; in place on the residual stream.
    rstd tolerance 3e-6 relative (as tests/test_ops_gpu.py): the longest fp32 chain of a row's sum of squares is 8 squares
    of a lane's quad pair + 8 quads + 2 lane-group shuffles + 2 * 22 partials = 62 additions of non-negative terms,
    62 u = 3.7e-6 on the sum, half of it on its rsqrt, plus rsqrtf's own 2 u."""
    lib, eps, what = L.load(), 1e-5, f"resid_rstd {M}x{N}x{K}"
    need = int(lib.vgpt_gemm_norm_workspace_bytes(M, N, K))
    n_cnt = -(-M // 256)
    assert need > n_cnt * 4 and need % 4 == 0
    a, w, r = _randn((M, K), 101), _randn((N, K), 102, 0.1), _randn((M, N), 103)
    A, W = Buf(M, K, K + 24).set(a).freeze(), Buf(N, K, K + 40).set(w).freeze()
    ws = Buf(1, need // 4, need // 4, F32, pad=4096)      # the workspace, zeroed once; NaNs on both sides of it
    ws.m.zero_()
    runs = []
    for inplace in (True, False, False):
        C = Buf(M, N, N + 20)
        Rs = Buf(1, M, M, F32, guard=1)
        if inplace:
            C.set(r)
            X, xptr, ldr = None, C.ptr, C.ld
        else:
            X = Buf(M, N, N + 36).set(r).freeze()
            xptr, ldr = X.ptr, X.ld
        L.call("vgpt_gemm_bf16_resid_rstd", A.ptr, W.ptr, C.ptr, xptr, Rs.ptr, ws.ptr, need, eps, M, N, K, A.ld, W.ld, C.ld, ldr,
               None)
        _ran(L, _expect(kernel, M), what)
        torch.cuda.synchronize()
        assert int(ws.m.view(torch.int32)[0, :n_cnt].abs().sum()) == 0, "an arrival counter was left non-zero"
        runs.append((C.take(what), Rs.take(what + " rstd")[0]))
        for b in (A, W, X):
            if b is not None:
                b.unchanged(what)
    part = ws.take(what + " workspace")
    assert torch.isfinite(part).all()
    out, rstd = runs[0]
    for o2, r2 in runs[1:]:
        assert torch.equal(o2, out) and torch.equal(r2, rstd), "not the same bits on a relaunch"
    ref = a.double() @ w.double().t() + r.double()
    s = a.double().abs() @ w.double().abs().t() + r.double().abs()
    _within(out, ref, _bf_bound(ref, _gamma(K) * s), what)
    want = torch.rsqrt(out.double().pow(2).mean(-1) + eps)
    worst = float(((rstd.double() - want).abs() / want).max())
    print(f"MEASURE {what}: worst relative rstd error = {worst:.3g} (bound 3e-6)")      # measured 1.9e-7 .. 2.2e-7
    assert worst <= 3e-6
    # the plain residual GEMM on the same kernel gives the same output bits
    same = _gemm(L, 0, a, w, M, N, K, _expect(kernel, M), what + " plain", EPI_RESID, r)
    assert torch.equal(same, out)
    # a workspace one byte short is refused, and launches nothing
    with pytest.raises(L.VgptError, match="workspace too small"):
        L.call("vgpt_gemm_bf16_resid_rstd", A.ptr, W.ptr, C.ptr, xptr, Rs.ptr, ws.ptr, need - 1, eps, M, N, K, A.ld, W.ld, C.ld, ldr,
               None)
    assert _launches(L) == []


# ============================================================================================================
# the launch decision at the workload's own shapes
# ============================================================================================================
# id: (entry, M, N or I, K, expected records in family 0, in family 1).  The small-shape cases above reach every kernel; these
# reach what only the workload's sizes do: round splits of the eight-wave plan (7740 rows), the 288-wide choice (qkv_proj), the
# 192 / 256 choice of both families' cost models at 48 and 128 k-tiles, the 128-tile threshold.  The records are those of
# commit 04b49a6 on a 256-CU MI355X.  dW = dY^T X is called as the trainer calls it, with the 7740 tokens as the reduction
# length (a transposed A's width, here the weight's rows, must be a multiple of 8, which 7740 is not).
WORKLOAD_LAUNCHES = {
    "qkv_rope": ("rope", 4096, 9216, 3072, [(9, ROPE, 0, 0, 0, 4096)], [(288, ROPE, 0, 0, 0, 4096)]),
    "o_proj_resid": ("resid", 4096, 3072, 3072, [(6, PLAIN, 0, 0, 0, 4096)], [(192, PLAIN, 0, 0, 0, 4096)]),
    "gate_up_gated": ("gated", 4096, 8192, 3072, [(8, GATED, 0, 0, 0, 4096)], [(256, GATED, 0, 0, 0, 4096)]),
    "down_proj": ("resid", 4096, 3072, 8192, [(6, PLAIN, 0, 0, 0, 4096)], [(192, PLAIN, 0, 0, 0, 4096)]),
    "nt_7740x9216": ("nt", 7740, 9216, 3072, [(8, PLAIN, 0, 0, 0, 7740)],
                     [(256, PLAIN, 0, 0, 0, 7168), (128, PLAIN, 0, 0, 7168, 572)]),
    "nt_7740x3072": ("nt", 7740, 3072, 3072, [(6, PLAIN, 0, 0, 0, 7740)],
                     [(256, PLAIN, 0, 0, 0, 5376), (128, PLAIN, 0, 0, 5376, 2364)]),
    "dx_7740x9216": ("dx", 7740, 9216, 3072, [(8, PLAIN, 0, 1, 0, 7740)],
                     [(256, PLAIN, 0, 1, 0, 7168), (128, PLAIN, 0, 1, 7168, 572)]),
    "dx_7740x3072": ("dx", 7740, 3072, 3072, [(6, PLAIN, 0, 1, 0, 7740)],
                     [(256, PLAIN, 0, 1, 0, 5376), (128, PLAIN, 0, 1, 5376, 2364)]),
    "dw_9216x3072_over_7740": ("dw", 9216, 3072, 7740, [(8, PLAIN, 1, 1, 0, 9216)], [(256, PLAIN, 1, 1, 0, 9216)]),
    "dw_3072x3072_over_7740": ("dw", 3072, 3072, 7740, [(6, PLAIN, 1, 1, 0, 3072)], [(256, PLAIN, 1, 1, 0, 3072)]),
    "nt_below_the_128_tile_threshold": ("nt", 544, 3072, 3072, [(128, PLAIN, 0, 0, 0, 544)], [(128, PLAIN, 0, 0, 0, 544)]),
}


@pytest.mark.parametrize("fam", [0, 1])
@pytest.mark.parametrize("cid", list(WORKLOAD_LAUNCHES))
def test_launch_decision_at_workload_shapes(L, cid, fam):
    """One call on dense zero operands; only the launch record is under test (the kernels are pinned above)."""
    entry, M, N, K, *expect = WORKLOAD_LAUNCHES[cid]
    z = lambda *shape, dtype=BF: torch.zeros(shape, dtype=dtype, device=DEV)
    with _family(L, fam):
        if entry == "rope":
            hd, n_rot = 96, 64
            a, w, c, cs, sn = z(M, K), z(N, K), z(M, N), z(M, hd // 2, dtype=F32), z(M, hd // 2, dtype=F32)
            L.call("vgpt_gemm_bf16_rope", a.data_ptr(), w.data_ptr(), c.data_ptr(), cs.data_ptr(), sn.data_ptr(), M, N, K, K, K, N,
                   n_rot, hd, None)
        elif entry == "gated":
            a, w, c = z(M, K), z(2 * N, K), z(M, N)
            L.call("vgpt_gated_mlp_act_fwd", a.data_ptr(), w.data_ptr(), c.data_ptr(), M, N, K, K, K, N, 0, None)
        elif entry in ("nt", "resid"):
            a, w, c = z(M, K), z(N, K), z(M, N)
            epi, xptr, ldr = (EPI_RESID, c.data_ptr(), N) if entry == "resid" else (EPI_NONE, None, 0)
            L.call("vgpt_gemm_bf16", a.data_ptr(), w.data_ptr(), c.data_ptr(), xptr, M, N, K, K, K, N, ldr, epi, None)
        else:
            atr = int(entry == "dw")
            a, w, c = (z(K, M) if atr else z(M, K)), z(K, N), z(M, N)
            L.call("vgpt_gemm_bf16_tr", a.data_ptr(), w.data_ptr(), c.data_ptr(), None, M, N, K, a.shape[1], N, N, 0, EPI_NONE, atr, 1,
                   None)
        _ran(L, expect[fam], f"{cid} family {fam}")
    torch.cuda.synchronize()
