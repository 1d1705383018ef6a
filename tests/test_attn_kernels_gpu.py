"""Every path of the inference attention forward (csrc/attn_fwd.hip, csrc/attn_p2_loop.inc, csrc/attn_fp8.hip) against an
inline float64 restatement, element by element, called through the C ABI (_lib.call) so that every pointer and stride is the
test's own.  tests/test_ops_gpu.py holds these kernels to a whole-tensor rel-L2 and ties the paths to each other bit for bit;
here a wrong row, a key counted twice at a mask seam or a key read past L fails by itself, and says where.

PATHS (the first field of every case id; the selector is set by the case, never left to a default)
  A  vgpt_attn_blockmask_fwd, variant 0, head dim 96: once with vgpt_attn_set_hand_scheduled(1), once with (0)
  B  the same, head dims 64 / 128 (register-staged K / V, transposed LDS reads)
  C  the same, variant 1 (the [d][key] V image), head dims 64 / 96 / 128
  D  vgpt_attn_blockmask_fwd_qrange, q_start 128 / 256, with the order of vgpt_attn_qblock_order and with NULL
  E  vgpt_attn_fwd_plan, 128-row items, head dims 64 / 96 / 128, with lse and with lse = NULL (96: both tile bodies)
  F  vgpt_attn_fwd_plan, 256-row items (eight waves), head dim 96, with lse
  G  vgpt_attn_fp8_quantize + vgpt_attn_fwd_plan_fp8, head dim 96

GUARD BANDS AND STRIDES (Arena / Field: tests/test_gemm_kernels_gpu.py's Buf with three strides).  Q, K, V and O live in
allocations filled with a NaN bit pattern, GUARD rows before and after them and NaN in every gap column; three layouts:
"fused" (one (B, L, width + 8) row buffer: a row stride that is a multiple of 8 but not of 16 elements), "bhsd" (separate
(B, heads, S, d) tensors, three NaN rows between heads) and "pad4" (head stride hd + 8; output strides that are multiples of
4 but not of 8).  After every call each element outside the rows x n_heads x hd the call owns still holds the pattern (rows
below q_start and rows no plan item covers included), every owned element was written, the inputs with their guards are
bitwise unchanged (the mask words too, which the launches read from a guarded copy), and the same holds for lse.  The NaN rows directly behind key row L - 1 check the tail clamp of
attn_fwd.hip (glds_tile / gload / the tail branch of the pipelined bodies): a kernel that read them and weighted them by
zero would still produce NaN.

CHECK 1, the key-map probe (exact).  Q = 0: every visible key of row i gets weight exactly 1 / n_i.  V is zero except for a
window of hd consecutive keys where kv head g holds V[w0 + (d + 5 g) % hd, g, d] = 1; one launch per window covers all keys.
O[i, head, d] must be exactly 0 where that key is masked for row i or lies at or beyond L, within one bf16 ulp of 1 / n_i
elsewhere (the fp32 quotient rounded once more) and bit-equal to it where n_i is a power of two; wholly masked rows are exact
zeros; lse = log2(n_i), +inf on empty rows.  This pins the mask-bit-to-key map, item row offsets, the GQA head map and the
tail handling per key.  For G the same values are required: 2^8 (the stored probability) and 1 (the one-hot V) are exact in
e4m3, so nothing of the fp8 rounding is left in this probe.

CHECK 2, random values, element-wise: attn_fwd_bound (its docstring lists every term with its source line) for A-F,
attn_fp8_bound for G (against the dequantised-operand reference of tests/test_attn_fp8_gpu.py), _per_row beside both.
tests/test_attn_kernels_cabi.py runs a CPU model of the kernel's rounding points against the same bounds.

CHECK 3, relations, on the same cases: planned (E) == aligned (A / B) bit for bit on the rows both compute, eight-wave (F)
== four-wave (E), hand-scheduled == compiler-scheduled (outputs and lse), a second launch gives the same bits.

The second mask word of a row with an odd word count (L = 33, 96, 160: attn_fwd.hip:342, :466) is read under a clamp and
then discarded, so a missing clamp changes no value; those lengths are in the set all the same, with the mask words in a
guarded allocation.

MEASURED on one MI355X (the MEASURE lines of a full run): the 91 cases take 4.7 s together under pytest (the first, which
touches the device, 1.4 s; every other 0.01 to 0.10 s).  Worst |err| / bound of check 2 per path: A 0.788, B 0.792, C 0.785,
D 0.552, E 0.785, F 0.747 (the CPU model of tests/test_attn_kernels_cabi.py reaches 0.788 on the same data: the kernels sit
where an implementation with these rounding points and no others sits); worst row error 2.9e-3 under 3e-2 on every bf16
path; lse on live rows 4.3e-6 (E) and 1.2e-5 (F, whose cases include the spike with scale 0.25) under 5e-5.
fp8 (G): worst |err| / bound 0.782 against attn_fp8_bound; worst row error against the dequantised-operand reference
measured 3.6e-2 on one MI355X, bound 6.25e-2 = 2^-4 derived (FP8_ROW_TOL below): a margin of 1.7.  The rel-L2 asserts of
tests/test_attn_fp8_gpu.py (3e-2 / 8e-2) stay as they are.
With the reference's mask shifted by one key (a throwaway edit of probe_expect, never of a kernel) check 1 fails on every
path, at the first window, for every mask kind but "dense".
"""
import contextlib
import importlib
import math

import numpy as np
import pytest
import torch

from tests.test_attn_fp8_gpu import quantise_blocks
from tests.test_gemm_kernels_gpu import SENT16, SENT32, Buf
from tests.test_ops_gpu import g
from tests.test_train_kernels_gpu import U32, _mask, _per_row, _ulp, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64              # guard rows before and after every operand: one key tile, the most a missing tail clamp could reach
LOG2E = 1.4426950408889634
LSE_TOL = 5e-5          # log2 units on live rows: the figure of tests/test_train_kernels_gpu.py (measured there 4.2e-6)


@pytest.fixture(scope="module")
def LIB():
    return importlib.import_module("video-gpt_amd._lib")


# ============================================================================================================
# operands with guard bands
# ============================================================================================================
class Arena:
    """One allocation of bf16 elements filled with the NaN pattern, `lead` guard elements before and after the payload."""

    def __init__(self, n, lead):
        self.lead = lead
        self.raw = torch.full((2 * lead + n,), SENT16, dtype=torch.int16, device=DEV)
        self.snap = None

    def freeze(self):
        self.snap = self.raw.clone()
        return self

    def unchanged(self, what):
        assert torch.equal(self.raw, self.snap), f"{what}: an input buffer or its guard band was written"


class Field:
    """A (B, S, heads, d) operand inside an Arena at element offset `off` with strides (sb, sh, ss): Buf with three strides."""

    def __init__(self, arena, off, shape, sb, sh, ss):
        B, S, H, d = shape
        ar = lambda n: torch.arange(n, device=DEV)   # noqa: E731
        self.idx = (arena.lead + off + ar(B)[:, None, None, None] * sb + ar(S)[None, :, None, None] * ss +
                    ar(H)[None, None, :, None] * sh + ar(d))
        assert int(self.idx.max()) < arena.raw.numel() - arena.lead
        self.arena, self.shape, self.sb, self.sh, self.ss = arena, shape, sb, sh, ss
        self.ptr = arena.raw.data_ptr() + 2 * (arena.lead + off)

    def set(self, t):
        self.arena.raw[self.idx] = t.to(DEV, BF).contiguous().view(torch.int16)
        return self

    def take(self, rows, what):
        """The operand as the kernel left it (rows it did not own still NaN); everything outside `rows` (B, S) x heads x d
        must still hold the fill pattern.  The arena is refilled for the next launch."""
        raw = self.arena.raw
        own = torch.zeros(raw.shape, dtype=torch.bool, device=DEV)
        own[self.idx[rows.to(DEV)]] = True
        bad = ((raw != SENT16) & ~own).nonzero()
        if bad.numel():
            raise AssertionError(f"{what}: {bad.shape[0]} elements outside the rows the call owns were written, the first at "
                                 f"element {int(bad[0]) - self.arena.lead} (strides {self.sb}, {self.sh}, {self.ss})")
        assert bool((raw[own] != SENT16).all()), f"{what}: an element the call owns was not written"
        out = raw[self.idx].view(BF)
        raw.fill_(SENT16)
        return out


def _operands(layout, B, L, nh, nkv, hd):
    """(input arena, q, k, v, o) in one of the three layouts of the module docstring."""
    if layout == "fused":
        ld, lo = (nh + 2 * nkv) * hd + 8, nh * hd + 8
        a = Arena(B * L * ld, GUARD * ld)
        q, k, v = (Field(a, off, (B, L, H, hd), L * ld, hd, ld) for off, H in ((0, nh), (nh * hd, nkv), ((nh + nkv) * hd, nkv)))
        o = Field(Arena(B * L * lo, GUARD * lo), 0, (B, L, nh, hd), L * lo, hd, lo)
    elif layout == "bhsd":
        sh = (L + 3) * hd
        a = Arena(B * (nh + 2 * nkv) * sh, GUARD * hd)
        q = Field(a, 0, (B, L, nh, hd), nh * sh, sh, hd)
        k = Field(a, B * nh * sh, (B, L, nkv, hd), nkv * sh, sh, hd)
        v = Field(a, B * (nh + nkv) * sh, (B, L, nkv, hd), nkv * sh, sh, hd)
        o = Field(Arena(B * nh * sh, GUARD * hd), 0, (B, L, nh, hd), nh * sh, sh, hd)
    elif layout == "pad4":
        hs = hd + 8
        ld = (nh + 2 * nkv) * hs
        a = Arena(B * L * ld, GUARD * ld)
        q, k, v = (Field(a, off, (B, L, H, hd), L * ld, hs, ld) for off, H in ((0, nh), (nh * hs, nkv), ((nh + nkv) * hs, nkv)))
        odd4 = lambda n: n + 4 if n % 8 == 0 else n   # noqa: E731  a multiple of 4 that is no multiple of 8
        osh = hd + 4
        oss = odd4(nh * osh)
        osb = odd4(L * oss)
        o = Field(Arena(B * osb, odd4(GUARD * oss)), 0, (B, L, nh, hd), osb, osh, oss)
        assert osh % 8 == 4 and oss % 8 == 4 and osb % 8 == 4 and o.ptr % 16 == 8
    else:
        raise ValueError(layout)
    return a, q, k, v, o


def _lse_buf(B, L, nh):
    return Buf(B * nh, L, L, dtype=F32, guard=4)


def _take_lse(buf, rows, nh, what):
    """(B, nh, L) lse as the kernel left it; rows the call does not own, and the guards, still hold the fp32 NaN pattern."""
    B, L = rows.shape
    got = buf.m.clone().view(B, nh, L)
    own = rows.to(DEV)[:, None, :].expand(B, nh, L)
    assert bool((got.view(torch.int32)[~own] == SENT32).all()), f"{what}: lse of a row the call does not own was written"
    buf.m.view(buf.idt).fill_(buf.sent)
    assert bool((buf.raw == buf.sent).all()), f"{what}: the guard band of lse was written"
    return got


# ============================================================================================================
# float64 reference and the element-wise bounds (device-agnostic: the CPU model test imports them)
# ============================================================================================================
def attn_reference(q, k, v, m, scale):
    """Masked softmax attention in fp64 on q (B, L, nh, hd), k / v (B, L, nkv, hd), m (B, L, L) bool (True = visible).
    Returns o (B, L, nh, hd), the probabilities P (B, nh, L, L), the raw scores s = q.k and sabs = |q|.|k|, |v| per query
    head, lse (B, nh, L) in log2 units (+inf on rows without a visible key) and the mask broadcast over heads."""
    q, k, v = q.double(), k.double(), v.double()
    grp = q.shape[2] // k.shape[2]
    qh = q.permute(0, 2, 1, 3)
    kh = k.permute(0, 2, 1, 3).repeat_interleave(grp, 1)
    vh = v.permute(0, 2, 1, 3).repeat_interleave(grp, 1)
    mm = m.to(q.device)[:, None]
    s = qh @ kh.transpose(2, 3)
    t = (s * scale).masked_fill(~mm, float("-inf"))
    mx = t.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(t - mx)
    l = e.sum(-1, keepdim=True)
    P = e / torch.where(l > 0, l, torch.ones_like(l))
    lse = torch.where(l > 0, (mx + torch.log(l.clamp_min(1e-300))) / math.log(2), torch.full_like(l, float("inf")))
    return dict(o=(P @ vh).permute(0, 2, 1, 3), P=P, s=s, sabs=qh.abs() @ kh.abs().transpose(2, 3), vabs=vh.abs(),
                lse=lse.squeeze(-1), mask=mm.expand_as(P))


def _fp32_terms(r, scale, hd):
    """eps' of attn_fwd_bound: the relative error of one key's weight that the numerator and the denominator share or that
    is made in fp32, (B, nh, L, L)."""
    u, ln2 = U32, math.log(2)
    L = r["P"].shape[-1]
    T = (L + 63) // 64
    c = scale * LOG2E
    gam = lambda n: n * u / (1 - n * u)   # noqa: E731
    smax = (r["s"].abs() * r["mask"]).amax(-1, keepdim=True)
    score = ln2 * c * (gam(hd) * r["sabs"] + 4 * u * (r["s"].abs() + smax))
    chain = T * (2.0 ** -23 + u + ln2 * 2 * u * c * smax)
    return 2.0 ** -23 + score + chain + gam(L + T)


def attn_fwd_bound(r, scale, hd):
    """Element-wise bound on |out - ref| of the bf16 kernels (paths A-F), from the rounding points of attn_fwd_kernel.  With
    u = 2^-24 and c = scale * log2(e), the weight the kernel gives key j in row i differs from the exact exp2(c s_ij - m) by
    the relative eps'_ij, the sum of
      * 2^-23: v_exp_f32 is accurate to one fp32 ulp (attn_fwd.hip:531-532, __builtin_amdgcn_exp2f);
      * ln2 * c * (gamma_hd sum_d |q_d k_d| + 4 u (|s_ij| + max_j |s_ij|)): the score is the fp32 sum of hd exact bf16
        products (the MFMA chain of :428-431), c carries three roundings (the float argument, the constant, their product,
        :849) and the FMA one more on |c s - m| <= c (|s| + max |s|) (:530); an error dt of the exponent is ln2 dt of the
        weight -- the term that matters in the spike case.  The row maximum itself needs no term: any m cancels in O / l;
      * T (2^-23 + u + ln2 2 u c max_j |s_ij|), T = ceil(L / 64) tiles: what a tile's rescale alpha = exp2(m_old - m_new)
        (:519, one subtraction, one v_exp_f32) and the products l alpha, O alpha (:538, :544) add to the weights of earlier
        tiles;
      * gamma_(L + T): the fp32 addition chain of the row sum l (:535-538, taken from the UNROUNDED p) and of the P V
        accumulators (:560).
    The numerator's weight is rounded to bf16 for the P V MFMA (:554, round to nearest even) and the quotient costs 1 / l
    and one product (:734, :742): eps_ij = eps'_ij + 2^-8 + 2 u.  (bf16 keeps 8 significant bits: the spacing in [1, 2) is
    2^-7 and round-to-nearest errs by up to half of it, 2^-8 of the value.  2^-9, the figure this test was first asked to
    use, is not the unit roundoff of the format: with it the CPU model of tests/test_attn_kernels_cabi.py, which has exactly
    these rounding points and nothing else, reaches 1.33.)  To first order
        e_id = sum_j P_ij |V_jd| eps_ij + |ref_id| max_j eps'_ij,
    times (1 + 2^-6) for the products of two such errors (each below 2^-7), and the result is rounded once to bf16 (:742):
        |out - ref| <= e + ulp_bf16(|ref| + e) / 2.
    At the test's shapes everything but 2^-8 sum_j P |V| and the final half ulp is below 1e-3 of the bound."""
    epsd = _fp32_terms(r, scale, hd)
    epsn = epsd + 2.0 ** -8 + 2 * U32
    first = (r["P"] * epsn) @ r["vabs"] + r["o"].permute(0, 2, 1, 3).abs() * (epsd * r["mask"]).amax(-1, keepdim=True)
    e = (first * (1 + 2.0 ** -6)).permute(0, 2, 1, 3)
    return e + _ulp(r["o"].abs() + e) / 2 + 1e-30


def attn_fp8_bound(r, scale, hd):
    """Element-wise bound on |out - ref| of attn_fwd_fp8_kernel against attention on the DEQUANTISED operands (r is
    attn_reference of those; the MFMA multiplies e4m3 values exactly, so Q, K, V contribute nothing further).  What is
    left (attn_fp8.hip:277-309): p' = exp2(s - (m - 8)) in (0, 256] is computed in fp32 and the row sum is taken from that
    unrounded p' (:292-293, :297); the P^T operand is p' rounded to e4m3 with the fixed block scale 2^-8 (:295, :309), NOT
    re-scaled per block: three mantissa bits, relative error <= 2^-4 for p' >= 2^-6, and below that the subnormal spacing
    2^-9, i.e. an absolute 2^-10 in p', 2^-18 in units of the row's largest weight at that tile (later rescales only shrink
    it).  With l_i = sum_j w_ij in those units (1 / l_i = max_j P_ij):
        e_id = 2^-4 sum_j P_ij |V_jd| + 2^-18 max_j P_ij sum_(j visible) |V_jd| + the fp32 terms of attn_fwd_bound
    (eps' there: fp32 scores, v_exp_f32, rescale chain, addition chains; the roundings of c are not made here, which only
    makes that term generous), times (1 + 2^-3) for products of two relative errors below 2^-4, and one rounding to bf16
    (:325):  |out - ref| <= e + ulp_bf16(|ref| + e) / 2.  A worst case nobody reaches: it assumes every probability of a
    row rounds the same way, so the measured ratio is expected well below 1 wherever a row sees many keys."""
    epsd = _fp32_terms(r, scale, hd)
    pmax = r["P"].amax(-1, keepdim=True)
    first = ((r["P"] * (epsd + 2.0 ** -4 + 2 * U32)) @ r["vabs"] + 2.0 ** -18 * pmax * (r["mask"].double() @ r["vabs"]) +
             r["o"].permute(0, 2, 1, 3).abs() * (epsd * r["mask"]).amax(-1, keepdim=True))
    e = (first * (1 + 2.0 ** -3)).permute(0, 2, 1, 3)
    return e + _ulp(r["o"].abs() + e) / 2 + 1e-30


# per-row tolerance of the fp8 kernel against the dequantised-operand reference.  Row error / row norm: the P roundings
# are relative errors of at most 2^-4 each, so ||dO_i|| <= 2^-4 || sum_j P_ij |V_j| ||; where the signs of V do not cancel
# in the reference (a row that sees few keys) that is 2^-4 of the row norm, and where they do (many keys) the roundings
# average as well: for independent roundings uniform in +-2^-4 the expectation is 2^-4 / sqrt(3) = 3.6e-2 of the row norm
# whatever the number of keys.  Bound = 2^-4, the value no row exceeds without its roundings being correlated.
FP8_ROW_TOL = 2.0 ** -4


def dequantised_operands(q, k, v, scale):
    """The values the fp8 kernel multiplies, as tests/test_attn_fp8_gpu.py restates them: Q * (scale * log2 e) (fp32) in
    e4m3 blocks of 32 along d, divided by that factor again; K in blocks along d; V in blocks of 32 keys of a tile.
    q / k / v: (B, L, heads, hd) CPU tensors of bf16 values; returns fp64 CPU tensors of the same shapes."""
    B, L, nh, hd = q.shape
    nkv = k.shape[2]
    qmul = np.float32(np.float32(scale) * np.float32(LOG2E))
    qx = (q.float().numpy() * qmul).astype(np.float64).reshape(B, L, nh, hd // 32, 32)
    qd = quantise_blocks(qx)[0].reshape(B, L, nh, hd) / (scale * LOG2E)
    kd = quantise_blocks(k.double().numpy().reshape(B, L, nkv, hd // 32, 32))[0].reshape(B, L, nkv, hd)
    Lp = (L + 31) // 32 * 32
    vp = np.zeros((B, Lp, nkv, hd))
    vp[:, :L] = v.double().numpy()
    vd = quantise_blocks(vp.reshape(B, Lp // 32, 32, nkv, hd).transpose(0, 1, 3, 4, 2))[0].transpose(0, 1, 4, 2, 3)
    return torch.from_numpy(qd), torch.from_numpy(kd), torch.from_numpy(vd.reshape(B, Lp, nkv, hd)[:, :L].copy())


# ============================================================================================================
# cases
# ============================================================================================================
def attn_mask(kind, B, L, seed):
    """The kinds of tests/test_train_kernels_gpu.py::_mask, plus "packed2": two sequences packed into one row of tokens, the
    first dense, the second causal, meeting at an odd row inside a mask word."""
    if kind != "packed2":
        return _mask(kind, B, L, seed)
    s = max(1, (3 * L // 7) | 1) if L > 1 else 1
    m = torch.zeros(B, L, L, dtype=torch.bool)
    m[:, :s, :s] = True
    m[:, s:, s:] = torch.ones(L - s, L - s, dtype=torch.bool).tril()
    return m


def attn_inputs(kind, B, L, nh, nkv, hd):
    """mask (B, L, L) bool and bf16-valued q (B, L, nh, hd), k, v (B, L, nkv, hd) of a case, on the CPU.  "stage1" brings
    its own B = 2, L = 330; "spike" makes one key 8x longer, so the rows that see it get a nearly one-hot P."""
    m = attn_mask(kind, B, L, 31 + L)
    B, L = m.shape[0], m.shape[-1]
    gen = g(1000 * hd + 7 * L + nh + nkv)
    q, k, v = (torch.randn(B, L, H, hd, generator=gen).to(BF).float() for H in (nh, nkv, nkv))
    if kind == "spike":
        k[:, L // 3] = (k[:, L // 3] * 8.0).to(BF).float()
    return m, q, k, v


def _ragged(L):
    """Plan segments out of row order, with gaps: 128 rows from 261 (cut short by L), ONE row at 37 (no multiple of 32),
    33 rows from 70, 31 rows from 200, the rest from 389."""
    segs = [(0, 261, min(389, L)), (0, 37, 38), (0, 70, 103), (0, 200, 231)]
    return tuple(segs + ([(0, 389, L)] if L > 389 else []))


# eight-wave items of 256 rows starting at 37, 129 rows, 255 rows (batch 1) and one row; rows between them stay untouched
_BIG = ((0, 300, 429), (1, 5, 260), (0, 37, 293), (1, 300, 301))


def _c(path, hd, kind, B, L, nh, nkv, layout, **kw):
    ident = f"{path}-hd{hd}-{kind}-B{B}-L{L}-h{nh}x{nkv}-{layout}" + "".join(f"-{a}{b}" for a, b in kw.items() if a != "segs")
    if "segs" in kw:
        ident += "-ragged" if kw["segs"] != _BIG else "-big"
    return pytest.param(path, hd, kind, B, L, nh, nkv, layout, kw, id=ident)


# covering set: every L of {1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 191, 257, 383, 449} (+ 330, the stage-1
# mask), every (n_heads, n_kv) of {(1,1), (3,3), (4,2), (8,1), (8,8)}, every mask kind and every layout meet every path
CASES = [
    _c("A", 96, "dense", 1, 1, 1, 1, "fused"), _c("A", 96, "causal", 1, 33, 3, 3, "bhsd"),
    _c("A", 96, "holes", 2, 65, 4, 2, "pad4"), _c("A", 96, "unseen", 1, 96, 8, 1, "fused", scale=0.25),
    _c("A", 96, "packed2", 1, 129, 8, 8, "bhsd"), _c("A", 96, "spike", 1, 257, 4, 2, "pad4"),
    _c("A", 96, "holes", 1, 383, 1, 1, "fused"), _c("A", 96, "causal", 1, 449, 3, 3, "fused", scale=0.03),
    _c("A", 96, "stage1", 2, 330, 4, 2, "bhsd"), _c("A", 96, "dense", 1, 160, 8, 8, "fused"),
    _c("A", 96, "unseen", 1, 64, 4, 2, "pad4"), _c("A", 96, "holes", 1, 128, 3, 3, "bhsd"),
    _c("B", 64, "causal", 1, 31, 1, 1, "fused"), _c("B", 128, "holes", 1, 63, 3, 3, "bhsd"),
    _c("B", 64, "unseen", 1, 127, 4, 2, "pad4"), _c("B", 128, "dense", 1, 128, 8, 1, "fused"),
    _c("B", 64, "packed2", 1, 191, 8, 8, "bhsd"), _c("B", 128, "spike", 2, 257, 4, 2, "pad4"),
    _c("B", 64, "holes", 1, 449, 3, 3, "fused", scale=0.25), _c("B", 128, "causal", 1, 160, 1, 1, "pad4", scale=0.03),
    _c("B", 128, "unseen", 1, 65, 4, 2, "fused"), _c("B", 64, "dense", 1, 33, 8, 8, "bhsd"),
    _c("B", 64, "stage1", 2, 330, 4, 2, "bhsd"), _c("C", 128, "stage1", 2, 330, 8, 1, "fused"),
    _c("C", 64, "holes", 1, 32, 1, 1, "fused"), _c("C", 96, "causal", 1, 64, 3, 3, "bhsd"),
    _c("C", 128, "unseen", 1, 129, 4, 2, "pad4"), _c("C", 64, "dense", 1, 65, 8, 1, "bhsd"),
    _c("C", 96, "packed2", 1, 257, 8, 8, "pad4", scale=0.25), _c("C", 128, "holes", 1, 383, 4, 2, "fused"),
    _c("C", 96, "spike", 1, 160, 1, 1, "fused"), _c("C", 64, "causal", 2, 96, 4, 2, "pad4", scale=0.03),
    _c("D", 96, "packed2", 1, 129, 1, 1, "fused", q0=128, order=1), _c("D", 96, "holes", 2, 257, 4, 2, "bhsd", q0=128, order=0),
    _c("D", 96, "unseen", 1, 257, 8, 1, "pad4", q0=256, order=1), _c("D", 96, "causal", 1, 449, 3, 3, "fused", q0=256, order=0),
    _c("D", 128, "dense", 1, 160, 8, 8, "pad4", q0=128, order=1), _c("D", 128, "spike", 1, 383, 4, 2, "bhsd", q0=256, order=0),
    _c("D", 128, "holes", 1, 191, 3, 3, "fused", q0=128, order=0, scale=0.25),
    _c("D", 96, "stage1", 2, 330, 8, 8, "bhsd", q0=256, order=1),
    _c("E", 96, "dense", 1, 1, 1, 1, "fused", lse=1), _c("E", 96, "causal", 1, 31, 3, 3, "bhsd", lse=0),
    _c("E", 64, "holes", 2, 33, 4, 2, "pad4", lse=1), _c("E", 128, "unseen", 1, 63, 8, 1, "fused", lse=0),
    _c("E", 96, "packed2", 1, 127, 8, 8, "pad4", lse=1), _c("E", 64, "spike", 1, 129, 4, 2, "bhsd", lse=1),
    _c("E", 128, "holes", 1, 191, 3, 3, "pad4", lse=1), _c("E", 96, "holes", 1, 449, 8, 8, "fused", lse=1, segs=_ragged(449)),
    _c("E", 64, "causal", 1, 449, 4, 2, "bhsd", lse=0, segs=_ragged(449)),
    _c("E", 128, "unseen", 1, 449, 8, 1, "fused", lse=1, segs=_ragged(449), scale=0.25),
    _c("E", 96, "stage1", 2, 330, 4, 2, "bhsd", lse=1), _c("E", 96, "packed2", 1, 383, 1, 1, "pad4", lse=0, segs=_ragged(383)),
    _c("E", 96, "dense", 1, 96, 1, 1, "bhsd", lse=1, scale=0.03), _c("E", 96, "causal", 1, 64, 3, 3, "fused", lse=1),
    _c("E", 96, "unseen", 2, 128, 4, 2, "fused", lse=1), _c("E", 96, "spike", 1, 257, 8, 1, "pad4", lse=1),
    _c("E", 128, "dense", 1, 32, 1, 1, "bhsd", lse=1), _c("E", 64, "unseen", 1, 65, 3, 3, "fused", lse=1),
    _c("E", 96, "holes", 1, 160, 4, 2, "bhsd", lse=0),
    _c("F", 96, "dense", 1, 257, 1, 1, "fused", lse=1), _c("F", 96, "causal", 1, 129, 3, 3, "bhsd", lse=1),
    _c("F", 96, "holes", 2, 449, 8, 8, "pad4", lse=1, segs=_BIG), _c("F", 96, "unseen", 1, 383, 4, 2, "fused", lse=1),
    _c("F", 96, "spike", 1, 257, 8, 1, "pad4", lse=1, scale=0.25), _c("F", 96, "stage1", 2, 330, 4, 2, "bhsd", lse=1),
    _c("F", 96, "holes", 1, 33, 4, 2, "fused", lse=1), _c("F", 96, "packed2", 1, 449, 3, 3, "bhsd", lse=1, scale=0.03),
    _c("F", 96, "dense", 1, 1, 8, 8, "pad4", lse=1), _c("F", 96, "packed2", 1, 191, 8, 1, "fused", lse=1),
    _c("G", 96, "dense", 1, 1, 1, 1, "fused"), _c("G", 96, "causal", 1, 33, 3, 3, "bhsd"),
    _c("G", 96, "holes", 2, 65, 4, 2, "pad4"), _c("G", 96, "unseen", 1, 129, 8, 1, "fused"),
    _c("G", 96, "packed2", 1, 449, 8, 8, "bhsd", segs=_ragged(449)), _c("G", 96, "holes", 1, 257, 4, 2, "pad4", q0=128),
    _c("G", 96, "spike", 1, 160, 1, 1, "fused", scale=0.25), _c("G", 96, "causal", 1, 383, 8, 8, "fused", scale=0.03),
    _c("G", 96, "stage1", 2, 330, 4, 2, "bhsd"), _c("G", 96, "unseen", 1, 96, 3, 3, "pad4"),
]

# path A runs whole in both tile bodies (the other paths compare the two bit for bit in check 3)
CASES = [pytest.param(*c.values[:8], dict(c.values[8], hand=h), id=f"{c.id}-hand{h}") if c.values[0] == "A" else c
         for c in CASES for h in ((1, 0) if c.values[0] == "A" else (1,))]


# ============================================================================================================
# launching
# ============================================================================================================
class _Run:
    """One case's operands, mask, plan and fp8 workspace, and the launches of every path on them."""

    def __init__(self, ops, LIB, path, hd, kind, B, L, nh, nkv, layout, kw):
        self.ops, self.LIB, self.path, self.hd, self.kind, self.kw = ops, LIB, path, hd, kind, kw
        self.m, self.q, self.k, self.v = attn_inputs(kind, B, L, nh, nkv, hd)
        self.B, self.L, self.nh, self.nkv = self.m.shape[0], self.m.shape[-1], nh, nkv
        B, L = self.B, self.L
        self.scale = float(kw.get("scale", 1 / math.sqrt(hd)))
        self.pm = ops.pack_mask(self.m.to(DEV))
        W = self.pm.bits.shape[-1]                  # the launches read the mask words from a guarded copy
        self.bits = Buf(B * L, W, W, dtype=F32, guard=8)
        self.bits.m.view(torch.int32).copy_(self.pm.bits.view(B * L, W))
        self.bits.freeze()
        self.arena, self.fq, self.fk, self.fv, self.fo = _operands(layout, B, L, nh, nkv, hd)
        self.q0 = int(kw.get("q0", 0))
        segs = kw.get("segs")
        if segs is None:
            segs = tuple((b, self.q0, L) for b in range(B))
        self.segs = segs
        self.rows = torch.zeros(B, L, dtype=torch.bool)        # the rows this case's path writes
        for b, r0, r1 in segs:
            self.rows[b, r0:r1] = True
        self.all_rows = torch.ones(B, L, dtype=torch.bool)
        self.lse = _lse_buf(B, L, nh)
        self.ws = None

    def st(self):
        f = (self.fq, self.fk, self.fv, self.fo)
        return [x for t in f for x in (t.sb, t.sh, t.ss)]

    def set(self, q, k, v):
        self.fq.set(q), self.fk.set(k), self.fv.set(v)
        self.arena.freeze()

    @contextlib.contextmanager
    def hand(self, on):
        """The tile body of the head-dim-96 four-wave kernels (1 = hand-scheduled), asserted to be the one asked for."""
        lib = self.LIB.load()
        prev = lib.vgpt_attn_set_hand_scheduled(on)
        try:
            assert lib.vgpt_attn_set_hand_scheduled(on) == on
            yield self
        finally:
            lib.vgpt_attn_set_hand_scheduled(prev)

    def aligned(self, variant=0, what="aligned"):
        self.LIB.call("vgpt_attn_blockmask_fwd", self.fq.ptr, self.fk.ptr, self.fv.ptr, self.fo.ptr, self.bits.ptr,
                      self.pm.summary.data_ptr(), self.B, self.L, self.nh, self.nkv, self.hd, *self.st(), self.scale, variant,
                      self.ops._stream())
        return self.done(self.all_rows, None, what)

    def qrange(self, q0, order, what="qrange"):
        optr = self.pm.order(q0).data_ptr() if order else None
        self.LIB.call("vgpt_attn_blockmask_fwd_qrange", self.fq.ptr, self.fk.ptr, self.fv.ptr, self.fo.ptr, q0,
                      self.bits.ptr, self.pm.summary.data_ptr(), optr, self.B, self.L, self.nh, self.nkv, self.hd,
                      *self.st(), self.scale, self.ops._stream())
        rows = self.all_rows.clone()
        rows[:, :q0] = False
        return self.done(rows, None, what)

    def planned(self, item_rows, lse, what="planned"):
        plan = self.pm.plan(self.segs, item_rows)
        assert plan.item_rows == item_rows and plan.n_items == sum(-(-(r1 - r0) // item_rows) for _, r0, r1 in self.segs)
        self.LIB.call("vgpt_attn_fwd_plan", self.fq.ptr, self.fk.ptr, self.fv.ptr, self.fo.ptr, self.lse.ptr if lse else None,
                      self.bits.ptr, plan.items.data_ptr(), plan.summary.data_ptr(), plan.order.data_ptr(),
                      plan.n_items, self.B, self.L, self.nh, self.nkv, self.hd, *self.st(), self.scale, item_rows,
                      self.ops._stream())
        return self.done(self.rows, self.rows if lse else None, what)

    def fp8(self, what="fp8"):
        """Caller-owned workspace; with q_start > 0 the rows below it were quantised by an earlier call (the engine's cached
        prefix) from a buffer whose later rows held other values, and this call re-quantises from q_start on."""
        B, L, nh, nkv, hd = self.B, self.L, self.nh, self.nkv, self.hd
        if self.ws is None:
            self.ws = self.ops.attention_fp8_workspace(B, L, nh, nkv, hd, DEV)
        self.ws.fill_(0x5A)
        quant = lambda row_begin: self.LIB.call(   # noqa: E731
            "vgpt_attn_fp8_quantize", self.fq.ptr, self.fk.ptr, self.fv.ptr, self.ws.data_ptr(), B, L, row_begin, nh, nkv, hd,
            *self.st()[:9], self.scale, self.ops._stream())
        if self.q0:
            keep = self.arena.raw.clone()
            for f in (self.fq, self.fk, self.fv):
                junk = torch.zeros(f.shape)
                junk[:, :self.q0] = self.arena.raw[f.idx].view(BF).float().cpu()[:, :self.q0]
                f.set(junk)
            quant(0)
            torch.cuda.synchronize()
            self.arena.raw.copy_(keep)
        quant(self.q0)
        plan = self.pm.plan(self.segs, 128)
        self.LIB.call("vgpt_attn_fwd_plan_fp8", self.ws.data_ptr(), self.fo.ptr, self.bits.ptr, plan.items.data_ptr(),
                      plan.summary.data_ptr(), plan.order.data_ptr(), plan.n_items, B, L, nh, nkv, hd, *self.st()[9:],
                      self.ops._stream())
        return self.done(self.rows, None, what)

    def done(self, rows, lse_rows, what):
        torch.cuda.synchronize()
        out = self.fo.take(rows, what)
        self.arena.unchanged(what)
        self.bits.unchanged(what)
        lse = _take_lse(self.lse, lse_rows if lse_rows is not None else torch.zeros_like(self.all_rows), self.nh, what)
        return out, (lse if lse_rows is not None else None), rows

    def main(self, what):
        """The launch of the case's own path: (out (B, L, nh, hd) bf16, lse or None, rows it owns)."""
        p, kw = self.path, self.kw
        if p in ("A", "B"):
            return self.aligned(0, what)
        if p == "C":
            return self.aligned(1, what)
        if p == "D":
            return self.qrange(self.q0, kw["order"], what)
        if p == "E":
            return self.planned(128, kw["lse"], what)
        if p == "F":
            return self.planned(256, kw["lse"], what)
        return self.fp8(what)


def _same(a, b, rows, what):
    if a is None or b is None:
        return
    r = rows.to(DEV)
    x, y = (a[r] if a.dim() == 4 else a.transpose(1, 2)[r]), (b[r] if b.dim() == 4 else b.transpose(1, 2)[r])
    it = torch.int16 if x.dtype == BF else torch.int32
    assert torch.equal(x.contiguous().view(it), y.contiguous().view(it)), f"{what}: not bit-identical"


def _relations(run, out, lse, rows, what):
    """Check 3 on the operands the run currently holds."""
    o2, l2, _ = run.main(what + " again")
    _same(out, o2, rows, what + ": second launch")
    _same(lse, l2, rows, what + ": second launch, lse")
    p = run.path
    if run.hd == 96 and p in ("A", "D", "E"):          # the other tile body
        with run.hand(1 - int(run.kw.get("hand", 1))):
            o3, l3, _ = run.main(what + " other tile body")
        _same(out, o3, rows, what + ": hand-scheduled == compiler-scheduled")
        _same(lse, l3, rows, what + ": hand-scheduled == compiler-scheduled, lse")
    if p == "E":                                       # planned == aligned on the rows both compute
        o4, _, _ = run.aligned(0, what + " aligned")
        _same(out, o4, rows, what + ": planned == aligned")
    if p == "D":
        o4, _, _ = run.aligned(0, what + " aligned")
        _same(out, o4, rows, what + ": q range == full launch")
    if p == "F":                                       # eight waves == four waves
        o4, l4, _ = run.planned(128, run.kw["lse"], what + " four-wave")
        _same(out, o4, rows, what + ": eight-wave == four-wave")
        _same(lse, l4, rows, what + ": eight-wave == four-wave, lse")


# ============================================================================================================
# the test
# ============================================================================================================
def probe_expect(m, w0, L, nh, nkv, hd):
    """Check 1's required output (B, L, nh, hd) in fp64 for the window at w0, and n (B, L), on m's device."""
    B = m.shape[0]
    n = m.sum(-1).double()
    d, grp = torch.arange(hd, device=m.device), nh // nkv
    want = torch.zeros(B, L, nh, hd, dtype=F64, device=m.device)
    for head in range(nh):
        key = w0 + (d + 5 * (head // grp)) % hd
        ok = key < L
        vis = m[:, :, key.clamp_max(L - 1)] & ok
        want[:, :, head] = torch.where(vis, 1.0 / n.clamp_min(1)[..., None], torch.zeros((), dtype=F64, device=m.device))
    return want, n


def probe_v(w0, B, L, nkv, hd):
    v = torch.zeros(B, L, nkv, hd)
    for gk in range(nkv):
        key = w0 + (torch.arange(hd) + 5 * gk) % hd
        ok = key < L
        v[:, key[ok], gk, torch.arange(hd)[ok]] = 1.0
    return v


@pytest.mark.parametrize("path,hd,kind,B,L,nh,nkv,layout,kw", CASES)
def test_attention_forward_paths_against_fp64(ops, LIB, path, hd, kind, B, L, nh, nkv, layout, kw):
    run = _Run(ops, LIB, path, hd, kind, B, L, nh, nkv, layout, kw)
    with run.hand(int(kw.get("hand", 1))):
        _check_case(run)


def _check_case(run):
    B, L, nh, nkv, hd, path = run.B, run.L, run.nh, run.nkv, run.hd, run.path
    mdev = run.m.to(DEV)
    tag = f"{path} hd{hd} {run.kind} L{L}"

    # ---- check 1: the key-map probe ----
    for w0 in range(0, L, hd):
        run.set(torch.zeros_like(run.q), run.k, probe_v(w0, B, L, nkv, hd))
        out, lse, rows = run.main(f"{tag} probe w0={w0}")
        want, n = probe_expect(mdev, w0, L, nh, nkv, hd)
        r = rows.to(DEV)
        got, want = out.double()[r], want[r]
        zero = want == 0
        bad = (zero & (got != 0)).nonzero()
        assert not bad.numel(), (f"{tag} probe w0={w0}: a masked or out-of-range key has weight: {bad.shape[0]} elements, the "
                                 f"first (row among owned, head, d) = {bad[0].tolist()}, value {float(got[tuple(bad[0])])}")
        err = (got - want).abs()
        assert bool((err <= _ulp(want)).all()), f"{tag} probe w0={w0}: a visible key's weight is not 1 / n within one bf16 ulp"
        pow2 = (torch.frexp(n)[0] == 0.5)[r][:, None, None].expand_as(want) & ~zero
        assert bool((got[pow2] == want[pow2]).all()), f"{tag} probe w0={w0}: 1 / n is not exact where n is a power of two"
        if lse is not None:
            lg, nr = lse.transpose(1, 2)[r].double(), n[r][:, None].expand(-1, nh)
            live = nr > 0
            assert bool((lg[~live] == float("inf")).all()), f"{tag} probe: lse of an empty row is not +inf"
            assert not live.any() or float((lg[live] - torch.log2(nr[live])).abs().max()) < LSE_TOL, f"{tag} probe: lse != log2 n"

    # ---- check 2: random values, element-wise; check 3 on the same operands ----
    run.set(run.q, run.k, run.v)
    out, lse, rows = run.main(tag)
    r = rows.to(DEV)
    if path == "G":
        qd, kd, vd = dequantised_operands(run.q, run.k, run.v, run.scale)
        ref = attn_reference(qd.to(DEV), kd.to(DEV), vd.to(DEV), mdev, run.scale)
        bound, row_tol = attn_fp8_bound(ref, run.scale, hd), FP8_ROW_TOL
    else:
        ref = attn_reference(run.q.to(DEV), run.k.to(DEV), run.v.to(DEV), mdev, run.scale)
        bound, row_tol = attn_fwd_bound(ref, run.scale, hd), 3e-2
    if run.kind == "spike":
        assert float(ref["P"].amax(-1).max()) > 0.99   # the spike does make some rows one-hot
    _within(out[r], ref["o"][r], bound[r], f"attn {path} O")
    _per_row(out[r], ref["o"][r], row_tol, f"attn {path} O rows")
    empty = ~mdev.any(-1)
    assert bool((out[empty & r] == 0).all()), f"{tag}: a wholly masked row is not exact zeros"
    if run.kind == "holes":
        assert bool(empty.any())
    if lse is not None:
        lg, lr = lse.transpose(1, 2)[r].double(), ref["lse"].transpose(1, 2)[r]
        live = torch.isfinite(lr)
        lerr = (lg - lr)[live].abs()
        print(f"MEASURE attn {path} lse: max |err| = {float(lerr.max()) if lerr.numel() else 0.0:.3g} (log2 units)")
        assert lerr.numel() == 0 or float(lerr.max()) < LSE_TOL
        assert bool((lg[~live] == float("inf")).all())
    _relations(run, out, lse, rows, tag)
