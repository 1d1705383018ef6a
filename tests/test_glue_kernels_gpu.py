"""csrc/glue.hip on the device, one entry point at a time: vgpt_embed_gather, vgpt_patch_embed_fwd, vgpt_timestep_sinusoid,
vgpt_linear_small, vgpt_final_layer_fwd, vgpt_sampler_set_timesteps, vgpt_euler_cfg_update, vgpt_sampler_copy_step_rows,
vgpt_cast_f32_to_bf16 and vgpt_sampler_advance.  Every operand sits in a tests/kernel_guards.py Guarded allocation (sentinel
bands, sentinel stride padding) checked after each launch; rows and columns a call must not write are compared bit for bit
with what they held before; exact probes pin every index map with torch.equal; random data is held element by element
against float64 under bounds read from the kernels' rounding points (e = 2^-24; hu(v) = tests/kernel_guards.py half_ulp(v),
what one rounding of v to bf16 costs, between 2^-9 |v| and 2^-8 |v|; EPS_ACT = 2^-14 for activation inputs in [-8, 8]):

  patch_embed   |o - o64| <= hu(o64) + 20 e sum|terms|                        16 fp32 products + bias + pos, one rounding
  linear_small  hu(o64) + (K/64 + 16) e sum|w a|  (+ sum|w| (hu(a64) + EPS_ACT |a64|) with pre_act, + EPS_ACT |o64| with
                post_act)                                                     bf16(act(x)), fp32 dot, bias, act, one rounding
  final_layer   hu(o64) + (H/64 + 32) e sum_k |v64_k W_ok|                    fp32 mean, variance, rsqrtf, modulate, dots
  euler_cfg     fp32 throughout: the running bound of the update, rounding by rounding (half an fp32 ulp of dt, 1 - sigma, its
                reciprocal, pred - z, the velocity, the CFG combination, dt v and the new z, each carried through the operations
                behind it), never more than 8 e (|z0| + |dt| (|v_c| + |v_u|) (1 + |scale|)); z_model == bf16(z) exactly
  timestep_sinusoid  the trigonometric rule of tests/test_norm_rope_kernels_gpu.py (TAU = 2^-22) on bf16-rounded outputs

The input generators, references and bounds are plain CPU functions: tests/test_glue_kernels_cabi.py runs a CPU model of each
kernel's rounding points through the same ones."""
import importlib
import math

import pytest
import torch

from tests.kernel_guards import BAND, BF, DEV, E, Guarded, all_intact, half_ulp, half_ulp32, sentinel
from tests.test_norm_rope_kernels_gpu import trig_table_ok

pytestmark = pytest.mark.gpu

F32 = torch.float32
EPS_ACT = 2.0 ** -14
ACT_SILU, ACT_GELU, ACT_GELU_TANH, ACT_NONE = 0, 1, 2, 3      # include/vgpt.h
PRED_V, PRED_X1 = 0, 1


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("video-gpt_amd.ops")


def _call(name, *args):
    importlib.import_module("video-gpt_amd._lib").call(name, *args, torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _sync(*bufs):
    torch.cuda.synchronize()
    assert all_intact(*bufs)


def _ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


# ---- embed_gather --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("H", [8, 200, 3072])
def test_embed_gather_copies_rows_and_clamps_ids(ops, H, rows):
    """out[r] = table[ids[r]] bit for bit; an id outside [0, vocab) reads the nearest valid row (include/vgpt.h)."""
    vocab = 11
    g = _gen(H + rows)
    table = torch.randn(vocab, H, generator=g).to(BF)
    ids = torch.randint(0, vocab, (rows,), generator=g)
    special = torch.tensor([vocab - 1, 0, -1, vocab, 1 << 40, -(1 << 40), vocab + 5])
    ids[:min(rows, special.numel())] = special[:rows]
    tg, ig, og = Guarded.of(table), Guarded.of(ids), Guarded(rows, H, BF)
    ops.embed_gather(ig.t.view(-1), tg.t, out=og.t)
    _sync(tg, ig, og)
    assert torch.equal(og.t.cpu(), table[ids.clamp(0, vocab - 1)])
    assert torch.equal(tg.t.cpu(), table) and torch.equal(ig.t.cpu().view(-1), ids)


# ---- patch_embed ---------------------------------------------------------------------------------------------------------

# (h, w) -> pos_max: 1, 15, 16 and 17 tokens.  pos_max - h/2 is odd at (2, 2) and (6, 10), even at (8, 8) and (2, 34);
# (top, left) = (1, 1), (2, 1), (1, 1), (8, 0)
PATCH_GRIDS = {(2, 2): 4, (6, 10): 8, (8, 8): 6, (2, 34): 17}
PATCH_CASES = [(h, w, H) for (h, w) in PATCH_GRIDS for H in (4, 192, 1028)]
NF = 3


def frame_rows(ntok):
    """Three frames out of order with gaps: (dst_row per frame, rows of the buffer, rows no frame owns)."""
    rows = [2 * ntok + 3, 1, ntok + 2]
    total = 3 * ntok + 5
    owned = {r + t for r in rows for t in range(ntok)}
    return rows, total, sorted(set(range(total)) - owned)


def patches_of(x):
    """(nf, 4, h, w) -> (nf, tokens, 16) with element e = ci * 4 + p * 2 + q of token t = i * (w / 2) + j."""
    nf, C, h, w = x.shape
    return x.reshape(nf, C, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(nf, (h // 2) * (w // 2), 16)


def cropped_pos(pos, pos_max, h, w):
    h2, w2 = h // 2, w // 2
    top, left = (pos_max - h2) // 2, (pos_max - w2) // 2
    return pos.view(pos_max, pos_max, -1)[top:top + h2, left:left + w2].reshape(h2 * w2, -1)


def patch_inputs(h, w, H, seed=41):
    g = _gen(seed + h * 100 + w + H)
    pm = PATCH_GRIDS[(h, w)]
    return (torch.randn(NF, 4, h, w, generator=g).to(BF), (0.25 * torch.randn(H, 16, generator=g)).to(BF),
            torch.randn(H, generator=g).to(BF), torch.randn(pm * pm, H, generator=g).to(BF))


def patch_reference(x, W, bias, pos, pos_max):
    """(o64, sum of |terms|), both (nf, tokens, H)."""
    _, _, h, w = x.shape
    p, W64 = patches_of(x).double(), W.double()
    prod = p[:, :, None, :] * W64[None, None]
    cp = cropped_pos(pos, pos_max, h, w).double()[None]
    return prod.sum(-1) + bias.double() + cp, prod.abs().sum(-1) + bias.double().abs() + cp.abs()


def patch_bound(o64, terms):
    return half_ulp(o64) + 20 * E * terms


def _patch_embed(ops, x, W, bias, pos, pos_max):
    nf, _, h, w = x.shape
    H, ntok = W.shape[0], (h // 2) * (w // 2)
    rows, total, free = frame_rows(ntok)
    fill = torch.randn(total, H, generator=_gen(3)).to(BF)
    xg, wg, bg, pg = Guarded.of(x.reshape(nf, -1)), Guarded.of(W), Guarded.of(bias), Guarded.of(pos)
    dg, sg = Guarded.of(torch.tensor(rows, dtype=torch.int32)), Guarded.of(fill)
    ops.patch_embed(xg.t.view(nf, 4, h, w), wg.t, bg.t.view(-1), pg.t, dg.t.view(-1), sg.t, pos_max)
    _sync(xg, wg, bg, pg, dg, sg)
    seq = sg.t.cpu()
    assert torch.equal(seq[free].view(torch.int16), fill[free].view(torch.int16))         # rows outside every frame
    return torch.stack([seq[r:r + ntok] for r in rows])


@pytest.mark.parametrize("h,w,H", PATCH_CASES)
def test_patch_embed_exact_probes(ops, h, w, H):
    x, W, bias, pos = patch_inputs(h, w, H)
    pm = PATCH_GRIDS[(h, w)]
    zero = torch.zeros_like
    # nothing but the position table: the crop window (top, left) and the row stride of the table
    out = _patch_embed(ops, zero(x), zero(W), zero(bias), pos, pm)
    assert torch.equal(out, cropped_pos(pos, pm, h, w)[None].expand(NF, -1, -1))
    # channel c selects patch element c mod 16: token -> (i, j), element -> (ci, p, q), frame -> dst_row
    sel = torch.zeros(H, 16)
    sel[torch.arange(H), torch.arange(H) % 16] = 1
    out = _patch_embed(ops, x, sel.to(BF), zero(bias), zero(pos), pm)
    assert torch.equal(out, patches_of(x)[:, :, torch.arange(H) % 16])


@pytest.mark.parametrize("h,w,H", PATCH_CASES)
def test_patch_embed_random_against_fp64(ops, h, w, H):
    x, W, bias, pos = patch_inputs(h, w, H)
    pm = PATCH_GRIDS[(h, w)]
    out = _patch_embed(ops, x, W, bias, pos, pm)
    o64, terms = patch_reference(x, W, bias, pos, pm)
    err, bound = (out.double() - o64).abs(), patch_bound(o64, terms)
    print(f"MEASURE patch_embed {h}x{w} H={H}: worst |err|/bound = {_ratio(err, bound):.3g}")
    assert bool((err <= bound).all())


# ---- timestep_sinusoid ---------------------------------------------------------------------------------------------------

def sampler_sigma(n_steps=5, shift=3.0):
    t = torch.linspace(0, 1, n_steps + 1)
    return (t / (t + shift - shift * t)).float()


def timestep_inputs(n, half=128):
    """t in [0, 1] as the sampler forms it (sigma values); freqs[0] = 1, so t = 1 gives the largest angle of the product path."""
    sg = sampler_sigma()
    t = {1: sg[2:3], 3: torch.stack([sg[0], sg[5], sg[3]]), 6: sg}[n].clone()
    freqs = torch.exp(-math.log(10000.0) * torch.arange(0, half, dtype=F32) / half)
    return t, freqs


@pytest.mark.parametrize("n", [1, 3, 6])
def test_timestep_sinusoid(ops, n):
    half = 128
    t, freqs = timestep_inputs(n, half)
    tg, fg, og = Guarded.of(t), Guarded.of(freqs), Guarded(n, 2 * half, BF)
    ops.timestep_sinusoid(tg.t.view(-1), fg.t.view(-1), out=og.t)
    _sync(tg, fg, og)
    out = og.t.cpu().float()
    ang = (t[:, None] * freqs[None, :]).double()                      # the kernel's fp32 product, then fp64
    for name, got, ref in (("cos", out[:, :half], torch.cos(ang)), ("sin", out[:, half:], torch.sin(ang))):
        ok, dev = trig_table_ok(got, ref, 1.0, True)
        print(f"MEASURE timestep_sinusoid {name} n={n}: largest |out - ref| = {float(dev.max()):.3g}")
        assert ok, name
    for i in (t == 0).nonzero().flatten().tolist():
        assert bool((out[i, :half] == 1).all()) and bool((out[i, half:] == 0).all())


# ---- linear_small --------------------------------------------------------------------------------------------------------

# (M, N, K, pre_act, post_act, bias, out_row)
_N_, _S_, _G_, _T_ = ACT_NONE, ACT_SILU, ACT_GELU, ACT_GELU_TANH
LINEAR_CASES = [(M, 5, 520, _N_, _N_, True, True) for M in (1, 8, 9, 16, 17, 32)] + [
    (9, 1, 8, _N_, _N_, True, True), (8, 3, 504, _N_, _N_, True, False), (17, 3, 512, _N_, _N_, False, True),
    (16, 1, 3072, _N_, _N_, True, True), (32, 3, 3072, _S_, _N_, True, True), (9, 8192 + 5, 8, _N_, _N_, True, True),
    (1, 3, 8, _N_, _S_, False, False)] + [(9, 5, 504, a, _N_, True, True) for a in (_S_, _G_, _T_)] + [
    (9, 5, 504, _N_, a, True, True) for a in (_S_, _G_, _T_)] + [(3, 3, 520, _G_, _T_, True, True)]
LINEAR_IDS = [f"M{M}-N{N}-K{K}-pre{a}-post{b}-{'bias' if bi else 'nobias'}-{'rows' if r else 'inorder'}"
              for M, N, K, a, b, bi, r in LINEAR_CASES]


def act64(x, act):
    if act == ACT_SILU:
        return x * torch.sigmoid(x)
    if act == ACT_GELU:
        return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))
    if act == ACT_GELU_TANH:
        return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return x


def linear_inputs(M, N, K, bias, seed=61):
    """x and the pre-activation outputs stay well inside [-8, 8]: W ~ N(0, 1/K)."""
    g = _gen(seed + M + 7 * N + K)
    x = (1.5 * torch.randn(M, K, generator=g)).clamp(-8, 8).to(BF)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    b = (0.5 * torch.randn(N, generator=g)).to(BF) if bias else None
    return x, W, b


def linear_reference(x, W, b, pre, post):
    """(o64, sum|w a64|, sum|w| (hu(a64) + EPS_ACT |a64|)) with a64 = act(x) unrounded; the last is what rounding the
    activated input to bf16 can move the dot by."""
    a = act64(x.double(), pre)
    W64 = W.double()
    v = a @ W64.T + (b.double() if b is not None else 0.0)
    return act64(v, post), (a.abs() @ W64.abs().T, (half_ulp(a) + EPS_ACT * a.abs()) @ W64.abs().T)


def linear_bound(o64, mags, K, pre, post):
    mag, mag_pre = mags
    bound = half_ulp(o64) + (K / 64 + 16) * E * mag
    if pre != ACT_NONE:
        bound = bound + mag_pre
    if post != ACT_NONE:
        bound = bound + EPS_ACT * o64.abs()
    return bound


def out_rows(M, use):
    """A permutation of the M result rows into a buffer 3 rows taller."""
    tall = M + 3
    rows = [(5 * m + 2) % tall for m in range(M)] if use else list(range(M))
    if len(set(rows)) != M:
        rows = list(range(tall - 1, tall - 1 - M, -1))
    return rows, tall


def _linear_small(x, W, b, pre, post, use_rows):
    M, K = x.shape
    N = W.shape[0]
    rows, tall = out_rows(M, use_rows)
    fill = torch.randn(tall, N, generator=_gen(9)).to(BF)
    xg, wg, og = Guarded.of(x, ld=K + 8), Guarded.of(W), Guarded.of(fill, ld=N + 3)
    bg = Guarded.of(b) if b is not None else None
    rg = Guarded.of(torch.tensor(rows, dtype=torch.int32)) if use_rows else None
    _call("vgpt_linear_small", xg.t.data_ptr(), wg.t.data_ptr(), bg.t.data_ptr() if bg else None, og.t.data_ptr(),
          rg.t.data_ptr() if rg else None, M, N, K, K + 8, N + 3, pre, post)
    _sync(*[g for g in (xg, wg, og, bg, rg) if g is not None])
    out = og.t.cpu()
    free = sorted(set(range(tall)) - set(rows))
    assert torch.equal(out[free].view(torch.int16), fill[free].view(torch.int16))           # rows no result row maps to
    assert torch.equal(xg.t.cpu(), x)
    return out[rows]


@pytest.mark.parametrize("M,N,K,pre,post,bias,use_rows", LINEAR_CASES, ids=LINEAR_IDS)
def test_linear_small_random_against_fp64(ops, M, N, K, pre, post, bias, use_rows):
    x, W, b = linear_inputs(M, N, K, bias)
    out = _linear_small(x, W, b, pre, post, use_rows)
    o64, mag = linear_reference(x, W, b, pre, post)
    err, bound = (out.double() - o64).abs(), linear_bound(o64, mag, K, pre, post)
    print(f"MEASURE linear_small M{M} N{N} K{K} pre{pre} post{post}: worst |err|/bound = {_ratio(err, bound):.3g}")
    assert bool((err <= bound).all())


def linear_integer_probe(M, N, K, seed=71):
    """x in -2..2, 16 (8 at K = 8) weights of +-1 per output column at seeded places, bias in -4..4: |sum| <= 36, exact."""
    g = _gen(seed + M + N + K)
    x = torch.randint(-2, 3, (M, K), generator=g)
    W = torch.zeros(N, K, dtype=torch.int64)
    nz = min(16, K)
    for n in range(min(N, 64)):
        cols = torch.randperm(K, generator=g)[:nz]
        W[n, cols] = torch.randint(0, 2, (nz,), generator=g) * 2 - 1
    if N > 64:                                     # the wide case: one weight per column, at a column-dependent place
        idx = torch.arange(64, N)
        W[idx, idx % K] = 1 - 2 * (idx % 2)
    b = torch.randint(-4, 5, (N,), generator=g)
    return x, W, b


@pytest.mark.parametrize("M,N,K", sorted({(M, N, K) for M, N, K, *_ in LINEAR_CASES}))
def test_linear_small_exact_probe(ops, M, N, K):
    x, W, b = linear_integer_probe(M, N, K)
    want = (x @ W.T + b).to(BF)
    assert torch.equal(want.long(), x @ W.T + b)
    out = _linear_small(x.to(BF), W.to(BF), b.to(BF), ACT_NONE, ACT_NONE, True)
    assert torch.equal(out, want)
    out = _linear_small(x.to(BF), W.to(BF), None, ACT_NONE, ACT_NONE, False)
    assert torch.equal(out, (x @ W.T).to(BF))


# ---- final_layer ---------------------------------------------------------------------------------------------------------

FINAL_GRIDS = [(2, 2), (2, 6), (4, 4), (2, 10)]           # 1, 3, 4 and 5 tokens
FINAL_WIDTHS = [8, 504, 512, 520, 3072, 4096]
FINAL_CASES = [(h, w, H) for (h, w) in FINAL_GRIDS for H in FINAL_WIDTHS]
FINAL_EPS = 1e-6


def final_rows(ntok):
    """src_row of three frames, out of order: (rows, rows of the hidden buffer)."""
    return [2 * ntok + 2, 0, ntok + 1], 3 * ntok + 2


def unpatchify(y, h, w):
    """(nf, tokens, 16) with y[.., (p * 2 + q) * 4 + c] -> (nf, 4, h, w)."""
    nf = y.shape[0]
    return y.reshape(nf, h // 2, w // 2, 2, 2, 4).permute(0, 5, 1, 3, 2, 4).reshape(nf, 4, h, w)


def final_inputs(h, w, H, seed=83):
    g = _gen(seed + 10 * h + w + H)
    ntok = (h // 2) * (w // 2)
    _, total = final_rows(ntok)
    hidden = (torch.randn(total, H, generator=g) * 2 + 0.5).to(BF)
    mod = torch.cat([torch.randn(NF, H, generator=g), 0.3 * torch.randn(NF, H, generator=g)], 1).to(BF)
    Wf = (torch.randn(16, H, generator=g) / math.sqrt(H)).to(BF)
    b = torch.randn(16, generator=g).to(BF)
    return hidden, mod, Wf, b


def final_reference(hidden, mod, Wf, b, h, w, eps=FINAL_EPS):
    """(o64, sum_k |v64_k W_ok|), both (nf, 4, h, w)."""
    ntok, H = (h // 2) * (w // 2), hidden.shape[1]
    rows, _ = final_rows(ntok)
    x = torch.stack([hidden[r:r + ntok] for r in rows]).double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    shift, scale = mod.double()[:, None, :H], mod.double()[:, None, H:]
    v = (x - mean) * torch.rsqrt(var + float(torch.tensor(eps, dtype=F32))) * (1 + scale) + shift
    W64 = Wf.double()
    return unpatchify(v @ W64.T + b.double(), h, w), unpatchify(v.abs() @ W64.abs().T, h, w)


def final_bound(o64, mag, H):
    return half_ulp(o64) + (H / 64 + 32) * E * mag


def _final_layer(ops, hidden, mod, Wf, b, h, w, eps=FINAL_EPS):
    ntok = (h // 2) * (w // 2)
    rows, _ = final_rows(ntok)
    hg, mg, wg, bg = Guarded.of(hidden), Guarded.of(mod), Guarded.of(Wf), Guarded.of(b)
    rg, og = Guarded.of(torch.tensor(rows, dtype=torch.int32)), Guarded(NF, 4 * h * w, BF)
    ops.final_layer(hg.t, rg.t.view(-1), mg.t, wg.t, bg.t.view(-1), og.t.view(NF, 4, h, w), eps)
    _sync(hg, mg, wg, bg, rg, og)
    assert torch.equal(hg.t.cpu().view(torch.int16), hidden.view(torch.int16))
    return og.t.cpu().view(NF, 4, h, w)


@pytest.mark.parametrize("h,w,H", FINAL_CASES)
def test_final_layer_exact_probes(ops, h, w, H):
    hidden, mod, Wf, b = final_inputs(h, w, H)
    ntok = (h // 2) * (w // 2)
    ramp = torch.arange(16).float().to(BF)
    # W = 0, b[o] = o: the unpatchify map alone
    out = _final_layer(ops, hidden, mod, torch.zeros_like(Wf), ramp, h, w)
    p, q, c = torch.arange(h)[None, :, None] % 2, torch.arange(w)[None, None, :] % 2, torch.arange(4)[:, None, None]
    assert torch.equal(out, ((2 * p + q) * 4 + c).float().to(BF)[None].expand(NF, -1, -1, -1))
    # a constant hidden row normalises to exactly 0, so v = shift: small-integer shifts distinct per frame and sparse
    # integer weights pin frame -> modulation row and the column map of the 16 dots (|sum| <= 3 * 2 * 16 + 15, exact)
    g = _gen(h + w + H)
    const = torch.full_like(hidden, 3.0)
    shift = torch.randint(-2, 3, (1, H), generator=g) * torch.tensor([[1], [2], [3]])
    imod = torch.cat([shift.float(), mod[:, H:].float()], 1).to(BF)
    iW = torch.zeros(16, H, dtype=torch.int64)
    for o in range(16):
        cols = torch.randperm(H, generator=g)[:min(16, H)]
        iW[o, cols] = torch.randint(0, 2, (cols.numel(),), generator=g) * 2 - 1
    y = (shift @ iW.T + torch.arange(16))[:, None, :].expand(NF, ntok, 16)
    out = _final_layer(ops, const, imod, iW.to(BF), ramp, h, w)
    assert torch.equal(out, unpatchify(y.float(), h, w).to(BF))


@pytest.mark.parametrize("h,w,H", FINAL_CASES)
def test_final_layer_random_against_fp64(ops, h, w, H):
    hidden, mod, Wf, b = final_inputs(h, w, H)
    out = _final_layer(ops, hidden, mod, Wf, b, h, w)
    o64, mag = final_reference(hidden, mod, Wf, b, h, w)
    err, bound = (out.double() - o64).abs(), final_bound(o64, mag, H)
    print(f"MEASURE final_layer {h}x{w} H={H}: worst |err|/bound = {_ratio(err, bound):.3g}")
    assert bool((err <= bound).all())


# ---- sampler: set_timesteps, euler_cfg, copy_step_rows, cast, advance -------------------------------------------------------

def _step(value):
    return Guarded.of(torch.tensor([value], dtype=torch.int32))


@pytest.mark.parametrize("n", [1, 64, 65])
def test_sampler_set_timesteps(ops, n):
    sigma = sampler_sigma()
    n_steps = sigma.numel() - 1
    sg = Guarded.of(sigma)
    for step in (-1, 0, n_steps - 1, n_steps, n_steps + 1):
        st, ts = _step(step), Guarded(1, n, F32)
        before = ts.bits()
        ops.sampler_set_timesteps(sg.t.view(-1), st.t.view(-1), ts.t.view(-1))
        _sync(sg, st, ts)
        if 0 <= step <= n_steps:                   # the table has n_steps + 1 entries
            assert torch.equal(ts.t.cpu().view(-1), sigma[step].expand(n)), step
        else:
            assert torch.equal(ts.bits(), before), step
        assert int(st.t.item()) == step


class EulerState:
    def __init__(self, z0, pred, sigma, step):
        self.z, self.zm, self.pred = Guarded.of(z0), Guarded(z0.shape[0], z0.shape[1], BF), Guarded.of(pred)
        self.zm.t.copy_(z0)
        self.sigma, self.step = Guarded.of(sigma), _step(step)

    def buffers(self):
        return (self.z, self.zm, self.pred, self.sigma, self.step)

    def update(self, ops, pred_type, use_cfg, scale):
        ops.euler_cfg_update(self.z.t, self.zm.t, self.pred.t, self.sigma.t.view(-1), self.step.t.view(-1), pred_type, use_cfg, scale)
        _sync(*self.buffers())


def euler_inputs(nf, elems, seed=97):
    g = _gen(seed + nf + elems)
    z0 = torch.randn(nf, elems, generator=g)
    return z0, torch.randn(nf, elems, generator=g).to(BF)


def euler_reference(z0, pred, sigma, step, pred_type, use_cfg, scale):
    """One step in fp64 from the fp32 inputs: (z64, bound).  With CFG both halves advance with the guided velocity.  The
    closed form 8 e (...) counts every rounding at its worst and is never filled beyond a quarter; the running bound follows
    euler_cfg_kernel's rounding points with the ulp each of them actually has (first order in 2^-24; a contraction to fma
    only removes one of them)."""
    hu = half_ulp32
    sg, sg_next = sigma[step].double(), sigma[step + 1].double()
    dt = sg_next - sg
    e_dt = hu(dt)
    z, p = z0.double(), pred.double()
    if pred_type == PRED_X1:
        inv = 1 / (1 - sg)
        e_inv = hu(1 - sg) * inv * inv + hu(inv)
        d = p - z
        v = d * inv
        e_v = hu(d) * inv + d.abs() * e_inv + hu(v)
    else:
        v, e_v = p, torch.zeros_like(p)
    if use_cfg:
        half = z.shape[0] // 2
        vc, vu, e_vc, e_vu = v[:half], v[half:], e_v[:half], e_v[half:]
        diff = vc - vu
        e_diff = e_vc + e_vu + hu(diff)
        e_prod = abs(scale) * e_diff + hu(scale * diff)
        guided = vu + scale * diff
        e_g = e_vu + e_prod + hu(guided)
        v, e_v = torch.cat([guided, guided]), torch.cat([e_g, e_g])
        mag = (vc.abs() + vu.abs()) * (1 + abs(scale))
        mag = torch.cat([mag, mag])
    else:
        mag = v.abs()
    z64 = z + dt * v
    running = (v.abs() * e_dt + abs(dt) * e_v + hu(dt * v) + hu(z64)) * (1 + 2.0 ** -10)
    return z64, torch.minimum(running, 8 * E * (z.abs() + abs(dt) * mag))


EULER_CASES = [(pt, cfg, scale) for pt in (PRED_X1, PRED_V) for cfg, scale in ((False, 1.6), (True, 0.0), (True, 1.0), (True, 1.6))]


def _euler_step(ops, nf, elems, pred_type, use_cfg, scale, step=2):
    z0, pred = euler_inputs(nf, elems)
    sigma = sampler_sigma()
    st = EulerState(z0, pred, sigma, step)
    st.update(ops, pred_type, use_cfg, scale)
    z, zm = st.z.t.cpu(), st.zm.t.cpu()
    z64, bound = euler_reference(z0, pred, sigma, step, pred_type, use_cfg, float(torch.tensor(scale, dtype=F32)))
    err = (z.double() - z64).abs()
    print(f"MEASURE euler_cfg {nf}x{elems} pred{pred_type} cfg={use_cfg} scale={scale}: worst |err|/bound = {_ratio(err, bound):.3g}")
    assert bool((err <= bound).all())
    assert torch.equal(zm, z.to(BF))
    assert torch.equal(st.pred.t.cpu(), pred) and int(st.step.t.item()) == step


@pytest.mark.parametrize("pred_type,use_cfg,scale", EULER_CASES)
def test_euler_cfg_one_step_against_fp64(ops, pred_type, use_cfg, scale):
    _euler_step(ops, 4, 250, pred_type, use_cfg, scale)


def test_euler_cfg_second_trip_of_the_grid_stride_loop(ops):
    _euler_step(ops, 2, 524288 + 37, PRED_X1, True, 1.6)


@pytest.mark.parametrize("use_cfg", [False, True], ids=["nocfg", "cfg"])
def test_euler_cfg_exact_probe_and_steps_outside_the_table(ops, use_cfg):
    """Dyadic sigma (0, 1/4, 1/2, 1), z = 0, v = 1 (with CFG: cond 1, uncond 0, scale 1): z = dt exactly at every step.  A
    step of -1 or n_steps leaves every buffer bit-identical."""
    sigma = torch.tensor([0.0, 0.25, 0.5, 1.0])
    nf, elems = 4, 250
    pred = torch.ones(nf, elems).to(BF)
    if use_cfg:
        pred[nf // 2:] = 0
    for step in (0, 1, 2):
        st = EulerState(torch.zeros(nf, elems), pred, sigma, step)
        st.update(ops, PRED_V, use_cfg, 1.0)
        dt = float(sigma[step + 1] - sigma[step])
        assert torch.equal(st.z.t.cpu(), torch.full((nf, elems), dt)), step
        assert torch.equal(st.zm.t.cpu(), torch.full((nf, elems), dt).to(BF)), step
    z0, rnd = euler_inputs(nf, elems)
    for step in (-1, 3):
        st = EulerState(z0, rnd, sigma, step)
        before = [b.bits() for b in st.buffers()]
        st.update(ops, PRED_X1, use_cfg, 1.6)
        assert all(torch.equal(b.bits(), a) for b, a in zip(st.buffers(), before)), step


@pytest.mark.parametrize("slab,n_layers", [(16, 2), (86 * 16, 3)], ids=["16B-2layers", "86vec-3layers"])
def test_sampler_copy_step_rows(ops, slab, n_layers):
    """dst[l][0:slab] = src[clamp(*step)][l][0:slab] in bytes; every stride is larger than the slab and the gaps hold the
    sentinel: the whole destination allocation is compared with its expected image, the whole source with its own."""
    n_steps = 4
    src_layer, dst_layer = slab + 32, slab + 80
    src_step = n_layers * src_layer + 48
    src, dst = Guarded(1, n_steps * src_step, torch.uint8), Guarded(1, n_layers * dst_layer, torch.uint8)
    data = torch.randint(0, 256, (n_steps, n_layers, slab), generator=_gen(slab), dtype=torch.uint8)
    sv = src.t.view(n_steps, src_step)[:, :n_layers * src_layer].view(n_steps, n_layers, src_layer)
    sv[:, :, :slab] = data.to(DEV)
    src_before = src.bits()
    for step in (-1, 0, n_steps - 1, n_steps + 3):
        dst.full.fill_(sentinel(torch.uint8))
        want = dst.bits()
        want[BAND:BAND + n_layers * dst_layer].view(n_layers, dst_layer)[:, :slab] = data[min(max(step, 0), n_steps - 1)].to(DEV)
        st = _step(step)
        _call("vgpt_sampler_copy_step_rows", src.t.data_ptr(), dst.t.data_ptr(), st.t.data_ptr(), n_steps, n_layers, slab,
              src_step, src_layer, dst_layer)
        _sync(src, dst, st)
        assert torch.equal(dst.bits(), want), step
        assert torch.equal(src.bits(), src_before), step


def cast_inputs(n, seed=101):
    g = _gen(seed + n)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())
    fmax = torch.finfo(F32).max
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, float("inf"),
                            float("-inf"), 1e-40, -1e-40, 2.0 ** -149, fmax, -fmax, float("nan"), 1 + 2.0 ** -8 + 2.0 ** -23,
                            1 + 2.0 ** -8 - 2.0 ** -24, 2.0 ** -133 * 1.5, 3.3895314e38], dtype=F32)
    x[:min(n, special.numel())] = special[:n]
    return x


@pytest.mark.parametrize("n", [1, 255, 524288 + 37])
def test_cast_f32_to_bf16_rounds_to_nearest_even(ops, n):
    x = cast_inputs(n)
    sg, dg = Guarded.of(x), Guarded(1, n, BF)
    ops.cast_f32_to_bf16(sg.t.view(-1), dg.t.view(-1))
    _sync(sg, dg)
    out, want = dg.t.cpu().view(-1), x.to(BF)
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(out), nan)                                            # NaN stays NaN, nothing else becomes one
    assert torch.equal(out[~nan].view(torch.int16), want[~nan].view(torch.int16))       # bits: -0 stays -0
    if n > 16:
        assert math.isinf(float(out[11])) and float(out[0]) == 1.0 and float(out[1]) == 1 + 2.0 ** -6


def test_sampler_advance_moves_the_counter_only(ops):
    st = _step(4)
    for _ in range(3):
        ops.sampler_advance(st.t.view(-1))
    _sync(st)
    assert int(st.t.item()) == 7
