"""csrc/norm_rope.hip on the device, one entry point at a time: vgpt_rmsnorm_fwd (templated and generic kernel),
vgpt_rms_rstd, vgpt_fold_norm_gain, vgpt_rope_table and vgpt_rope_qk_inplace.  Every operand sits in a tests/kernel_guards.py
Guarded allocation (sentinel bands, sentinel stride padding) that is checked after each launch; exact probes pin the index
maps with torch.equal; random data is held element by element against float64 under bounds read from the kernels' rounding
points.  e = 2^-24; one rounding to bf16 costs half an ulp, hu(v) = tests/kernel_guards.py half_ulp(v), between 2^-9 |v| and
2^-8 |v|; u = 2^-8 is its relative worst case, used where two roundings follow each other:

  rmsnorm     |y - y64| <= |y64| (2u + u^2 + (H/64 + 16) e)      fp32 sum of squares, rsqrtf, bf16(x rstd), bf16(w n)
  rms_rstd    the same statistics, fp32 out: the running bound of that computation, rounding by rounding (half an fp32 ulp
              of every partial sum of the squares in the kernel's order, of ss / H and of ss / H + eps, carried through
              d rsqrt = r / (2a), plus one ulp for rsqrtf), never more than r64 (H/64 + 16) e
  fold gain   torch.equal with bf16(w * g)                        the fp32 product of two bf16 is exact: one rounding
  rope_table  fp32 angle = fp32(pos) * inv_freq reproduced on the host, cos / sin of THAT angle in fp64, TAU = 2^-22 absolute
              (twice the 2 ulp the ROCm math library documents for sinf / cosf at |result| <= 1); unrounded outputs within
              TAU |scale|, bf16-rounded outputs one of bf16((c64 - TAU) scale), bf16(c64 scale), bf16((c64 + TAU) scale)
              (the MI355X stays inside it: largest deviation of an unrounded entry 1.08e-7 against TAU = 2.38e-7)
  rope_qk     |o - o64| <= hu(o64) + 4e (|a c| + |b s|)           bf16(a c - b s), bf16(b c + a s) in fp32

The input generators, references and bounds are plain CPU functions: tests/test_glue_kernels_cabi.py runs a CPU model of each
kernel's rounding points through the same ones."""
import importlib
import math

import pytest
import torch

from tests.kernel_guards import BF, E, U, Guarded, all_intact, half_ulp, half_ulp32, running_row_sum, to_bf16

pytestmark = pytest.mark.gpu

F32 = torch.float32
TAU = 2.0 ** -22
WIDTHS = [8, 504, 512, 520, 3072, 4096, 4104, 8192]
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("video-gpt_amd.ops")


def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _sync(*bufs):
    torch.cuda.synchronize()
    assert all_intact(*bufs)


# ---- rmsnorm / rms_rstd --------------------------------------------------------------------------------------------------

def rms_inputs(rows, H, seed=11):
    g = _gen(seed + 7 * rows + H)
    x = (torch.randn(rows, H, generator=g) * torch.exp2(torch.randint(-2, 3, (rows, 1), generator=g).float())).to(BF)
    w = (1.0 + 0.25 * torch.randn(H, generator=g)).to(BF)
    return x, w


def rstd_reference(x, eps=EPS):
    return torch.rsqrt(x.double().pow(2).mean(-1) + float(torch.tensor(eps, dtype=F32)))


def rmsnorm_reference(x, w, eps=EPS):
    return w.double() * x.double() * rstd_reference(x, eps)[:, None]


def rmsnorm_bound(y64, H):
    return y64.abs() * (2 * U + U * U + (H / 64 + 16) * E)


def rstd_bound(x, eps=EPS):
    """The closed form r64 (H/64 + 16) e counts every addition at its worst and is never filled beyond a fifth; the running
    bound below follows the same rounding points with the ulp each of them actually has."""
    H = x.shape[-1]
    ss, e_ss = running_row_sum(x.double().pow(2))           # the squares of bf16 values are exact in fp32
    m = ss / H
    e_m = e_ss / H + half_ulp32(m)
    a = m + float(torch.tensor(eps, dtype=F32))
    e_a = e_m + half_ulp32(a)
    r = torch.rsqrt(a)
    running = (0.5 * r * e_a / a + 2 * half_ulp32(r)) * (1 + 2.0 ** -10)
    return torch.minimum(running, r * (H / 64 + 16) * E)


def power_of_two_probe(rows, H, seed=5):
    """x[r, c] = +-2^(k_r): the mean square of row r is 4^(k_r) exactly in fp32 (H 4^k has at most 14 significant bits), so
    rstd is 2^-k within fp32 ulps and x rstd rounds to +-1 exactly."""
    g = _gen(seed + rows + H)
    k = (torch.arange(rows) * 5 % 7 - 3).float()
    sign = torch.randint(0, 2, (rows, H), generator=g).float() * 2 - 1
    return (sign * torch.exp2(k)[:, None]).to(BF), sign, k


RMS_CASES = [(r, H) for H in WIDTHS for r in (1, 3, 5)] + [(8192 + 5, 8)]


def _rmsnorm(ops, x, w, eps):
    rows, H = x.shape
    xg, wg, yg = Guarded.of(x), Guarded.of(w), Guarded(rows, H, BF)
    ops.rmsnorm(xg.t, wg.t.view(-1), eps, out=yg.t)
    _sync(xg, wg, yg)
    assert torch.equal(xg.t.cpu(), x) and torch.equal(wg.t.cpu().view(-1), w)
    return yg.t.cpu()


@pytest.mark.parametrize("rows,H", RMS_CASES)
def test_rmsnorm_random_against_fp64(ops, rows, H):
    x, w = rms_inputs(rows, H)
    y = _rmsnorm(ops, x, w, EPS)
    y64 = rmsnorm_reference(x, w)
    err, bound = (y.double() - y64).abs(), rmsnorm_bound(y64, H)
    print(f"MEASURE rmsnorm {rows}x{H}: worst |err|/bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("rows,H", RMS_CASES)
def test_rmsnorm_exact_probe(ops, rows, H):
    """eps = 0, x = +-2^(k_row): y = sign(x) w for every element.  A row normalised with another row's statistics, or a
    column multiplied by another column's gain, changes bits."""
    x, sign, _ = power_of_two_probe(rows, H)
    w = rms_inputs(rows, H)[1]
    y = _rmsnorm(ops, x, w, 0.0)
    assert torch.equal(y, (sign * w.float()).to(BF))


RSTD_CASES = [(r, H, pad) for H in WIDTHS for r in (1, 5) for pad in (8, 64)] + [(16384 + 3, 8, 8)]


def _rms_rstd(x, pad, eps):
    rows, H = x.shape
    xg, og = Guarded.of(x, ld=H + pad), Guarded(1, rows, F32)
    _lib = importlib.import_module("video-gpt_amd._lib")
    _lib.call("vgpt_rms_rstd", xg.t.data_ptr(), og.t.data_ptr(), rows, H, H + pad, float(eps), torch.cuda.current_stream().cuda_stream)
    _sync(xg, og)
    return og.t.cpu().view(-1)


@pytest.mark.parametrize("rows,H,pad", RSTD_CASES)
def test_rms_rstd_padded_rows_against_fp64(ops, rows, H, pad):
    x, _ = rms_inputs(rows, H)
    r = _rms_rstd(x, pad, EPS)
    r64 = rstd_reference(x)
    err, bound = (r.double() - r64).abs(), rstd_bound(x)
    print(f"MEASURE rms_rstd {rows}x{H} ldx={H + pad}: worst |err|/bound = {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("rows,H,pad", RSTD_CASES)
def test_rms_rstd_exact_probe(ops, rows, H, pad):
    x, _, k = power_of_two_probe(rows, H)
    r = _rms_rstd(x, pad, 0.0)
    want = torch.exp2(-k)
    # 2 fp32 ulps of a power of two: the spacing is 2^-24 relative below it and 2^-23 above
    assert bool(((r >= want * (1 - 2 * 2.0 ** -24)) & (r <= want * (1 + 2 * 2.0 ** -23))).all())


# ---- fold_norm_gain ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(1, 8), (3, 24), (257, 8), (5, 3072)])
def test_fold_norm_gain_is_one_rounding(ops, N, K):
    g = _gen(N * 31 + K)
    w, gain = torch.randn(N, K, generator=g).to(BF), (1 + 0.5 * torch.randn(K, generator=g)).to(BF)
    wg, gg, og = Guarded.of(w), Guarded.of(gain), Guarded(N, K, BF)
    ops.fold_norm_gain(wg.t, gg.t.view(-1), out=og.t)
    _sync(wg, gg, og)
    assert torch.equal(og.t.cpu(), (w.float() * gain.float()).to(BF))
    assert torch.equal(wg.t.cpu(), w)


# ---- rope_table ----------------------------------------------------------------------------------------------------------

LONGROPE_SCALE = math.sqrt(1 + math.log(32) / math.log(4096))   # the attention factor of tests/test_rope_scaling.py
LONGROPE_MAX_POS = 299 * 20                                     # the largest position that file's longrope path forms
TABLE_POSITIONS = {1: [LONGROPE_MAX_POS], 7: [0, 1, 3100, LONGROPE_MAX_POS, 2, 4095, 77]}
TABLE_CASES = [(half, tokens, scale, rnd) for half in (8, 32, 48, 64) for tokens in (1, 7) for scale in (1.0, LONGROPE_SCALE)
               for rnd in (False, True)]


def rope_table_inputs(half, tokens):
    pos = torch.tensor(TABLE_POSITIONS[tokens], dtype=torch.int64)
    inv = 1.0 / (10000.0 ** (torch.arange(0, 2 * half, 2, dtype=torch.int64).float() / (2 * half)))
    return pos, inv


def rope_table_reference(pos, inv):
    """cos / sin in fp64 of the fp32 angle the kernel forms (one fp32 multiply)."""
    ang = (pos.float()[:, None] * inv[None, :]).double()
    return torch.cos(ang), torch.sin(ang)


def trig_table_ok(out, ref64, scale, round_bf16, tau=TAU):
    """(ok, largest deviation of the unrounded comparison or nan).  `scale` as the fp32 value the kernel multiplies by."""
    if not round_bf16:
        dev = (out.double() - ref64 * scale).abs()
        return bool((dev <= tau * abs(scale)).all()), dev
    cands = [to_bf16((ref64 + d) * scale).float() for d in (-tau, 0.0, tau)]
    hit = (out == cands[0]) | (out == cands[1]) | (out == cands[2])
    return bool(hit.all() and torch.equal(out, out.to(BF).float())), (out.double() - ref64 * scale).abs()


@pytest.mark.parametrize("half,tokens,scale,rnd", TABLE_CASES,
                         ids=[f"half{h}-t{t}-{'longrope' if s != 1 else 'plain'}-{'bf16' if r else 'fp32'}" for h, t, s, r in TABLE_CASES])
def test_rope_table(ops, half, tokens, scale, rnd):
    pos, inv = rope_table_inputs(half, tokens)
    pg, ig = Guarded.of(pos), Guarded.of(inv)
    cg, sg = Guarded(tokens, half, F32), Guarded(tokens, half, F32)
    _lib = importlib.import_module("video-gpt_amd._lib")
    _lib.call("vgpt_rope_table", pg.t.data_ptr(), ig.t.data_ptr(), cg.t.data_ptr(), sg.t.data_ptr(), tokens, half, int(rnd),
              float(scale), torch.cuda.current_stream().cuda_stream)
    _sync(pg, ig, cg, sg)
    c, s = cg.t.cpu(), sg.t.cpu()
    c64, s64 = rope_table_reference(pos, inv)
    s32 = float(torch.tensor(scale, dtype=F32))
    for name, out, ref in (("cos", c, c64), ("sin", s, s64)):
        ok, dev = trig_table_ok(out, ref, s32, rnd)
        print(f"MEASURE rope_table {name}: largest |out - ref| = {float(dev.max()):.3g} (tau |scale| = {TAU * s32:.3g})")
        assert ok, name
    zero = [i for i, p in enumerate(pos.tolist()) if p == 0]
    for i in zero:                                                       # position 0: cos = 1, sin = 0, exactly
        one = torch.tensor(s32, dtype=F32)
        one = one.to(BF).float() if rnd else one
        assert bool((c[i] == one).all()) and bool((s[i] == 0).all())


# ---- rope_qk -------------------------------------------------------------------------------------------------------------

ROPE_SHAPES = [(16, 1, 1), (32, 2, 1), (64, 3, 1), (96, 2, 2), (128, 4, 2)]
ROPE_CASES = [(hd, nq, nkv, t) for hd, nq, nkv in ROPE_SHAPES for t in (1, 77)]


def rope_qk_inputs(hd, nq, nkv, tokens, seed=23):
    g = _gen(seed + hd + 3 * tokens)
    qkv = torch.randn(tokens, (nq + 2 * nkv) * hd, generator=g).to(BF)
    ang = torch.rand(tokens, hd // 2, generator=g) * 6.2831853
    return qkv, torch.cos(ang), torch.sin(ang)


def rope_qk_reference(qkv, cos, sin, hd, nq, nkv):
    """(o64, magnitude) with magnitude = |a c| + |b s| per output element; v columns pass through with magnitude 0."""
    tokens, half, n_rot = qkv.shape[0], hd // 2, nq + nkv
    x = qkv.double()[:, :n_rot * hd].view(tokens, n_rot, 2, half)
    a, b = x[:, :, 0], x[:, :, 1]
    c, s = cos.double()[:, None], sin.double()[:, None]
    o = torch.stack([a * c - b * s, b * c + a * s], 2).reshape(tokens, n_rot * hd)
    mag = torch.stack([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], 2).reshape(tokens, n_rot * hd)
    v = qkv.double()[:, n_rot * hd:]
    return torch.cat([o, v], 1), torch.cat([mag, torch.zeros_like(v)], 1)


def rope_qk_bound(o64, mag):
    return half_ulp(o64) + 4 * E * mag


def _rope_qk(ops, qkv, cos, sin, hd, nq, nkv):
    qg, cg, sg = Guarded.of(qkv), Guarded.of(cos), Guarded.of(sin)
    ops.rope_qk_inplace(qg.t, cg.t, sg.t, nq, nkv, hd)
    _sync(qg, cg, sg)
    assert torch.equal(cg.t.cpu(), cos) and torch.equal(sg.t.cpu(), sin)
    out = qg.t.cpu()
    assert torch.equal(out[:, (nq + nkv) * hd:], qkv[:, (nq + nkv) * hd:])          # v columns: bit-identical
    return out


def _rotated(qkv, pick, hd, nq, nkv):
    """The exact result for tables of zeros and ones: pick[t, i] = 0 -> (cos, sin) = (1, 0), 1 -> (0, 1)."""
    tokens, half, n_rot = qkv.shape[0], hd // 2, nq + nkv
    x = qkv[:, :n_rot * hd].view(tokens, n_rot, 2, half)
    a, b, p = x[:, :, 0], x[:, :, 1], pick[:, None].bool()
    o = torch.stack([torch.where(p, -b, a), torch.where(p, a, b)], 2).reshape(tokens, n_rot * hd)
    return torch.cat([o, qkv[:, n_rot * hd:]], 1)


@pytest.mark.parametrize("hd,nq,nkv,tokens", ROPE_CASES)
def test_rope_qk_exact_probes(ops, hd, nq, nkv, tokens):
    qkv = rope_qk_inputs(hd, nq, nkv, tokens)[0]
    half = hd // 2
    picks = {"identity": torch.zeros(tokens, half, dtype=torch.int64), "quarter turn": torch.ones(tokens, half, dtype=torch.int64),
             "pattern": torch.randint(0, 2, (tokens, half), generator=_gen(hd + tokens))}
    for name, pick in picks.items():
        out = _rope_qk(ops, qkv, (1 - pick).float(), pick.float(), hd, nq, nkv)
        assert torch.equal(out, _rotated(qkv, pick, hd, nq, nkv)), name


@pytest.mark.parametrize("hd,nq,nkv,tokens", ROPE_CASES)
def test_rope_qk_random_against_fp64(ops, hd, nq, nkv, tokens):
    qkv, cos, sin = rope_qk_inputs(hd, nq, nkv, tokens)
    out = _rope_qk(ops, qkv, cos, sin, hd, nq, nkv)
    o64, mag = rope_qk_reference(qkv, cos, sin, hd, nq, nkv)
    err, bound = (out.double() - o64).abs(), rope_qk_bound(o64, mag)
    n_rot = (nq + nkv) * hd
    print(f"MEASURE rope_qk hd{hd} {nq}+{nkv} heads {tokens} tokens: worst |err|/bound = "
          f"{float((err[:, :n_rot] / bound[:, :n_rot].clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bound).all())
