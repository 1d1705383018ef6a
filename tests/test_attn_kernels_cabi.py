"""The attention forward entry points (include/vgpt.h: vgpt_attn_blockmask_fwd, _fwd_lse, _fwd_qrange, vgpt_attn_fwd_plan,
vgpt_attn_plan_build, vgpt_attn_plan_workspace_bytes, vgpt_attn_fp8_workspace_bytes, vgpt_attn_fp8_quantize,
vgpt_attn_fwd_plan_fp8, vgpt_attn_supported) without a GPU: host-side argument checks refuse bad calls before any launch,
with the documented return code and a message in vgpt_last_error().  EVERY call in this file either fails a host check or
returns early (B = 0, L = 0, q_start >= L, n_items = 0): the pointers are fake, a launch would fault.

And a CPU model of the forward kernel's rounding points (64-key tiles, fp32 statistics, bf16-rounded P, fp32 accumulation,
one final rounding) held against the element-wise bound of tests/test_attn_kernels_gpu.py on every case of that file with
L <= 257: the bound is attainable by an honest implementation, and the model fills a good part of it."""
import importlib
import math
import os

import pytest
import torch

from tests import test_attn_kernels_gpu as G

FAKE = 1 << 20   # a non-null, 256-byte aligned address that is never dereferenced: every call below fails its checks first
INVALID, UNSUPPORTED = -1, -2
S96 = dict(q_sb=300 * 288, q_sh=96, q_ss=288, k_sb=300 * 288, k_sh=96, k_ss=288, v_sb=300 * 288, v_sh=96, v_ss=288,
           o_sb=300 * 96, o_sh=96, o_ss=96)
STRIDE_NAMES = list(S96)


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


def _strides(kw):
    st = dict(S96)
    for n in STRIDE_NAMES:
        if n in kw:
            st[n] = kw.pop(n)
    return [st[n] for n in STRIDE_NAMES]


def _fwd(lib, entry="fwd", q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=FAKE, bits=FAKE, summary=FAKE, order=None, items=FAKE, isum=FAKE,
         iorder=FAKE, n_items=3, q_start=0, B=1, L=300, nh=1, nkv=1, hd=96, scale=0.1, variant=0, item_rows=128, **kw):
    st = _strides(kw)
    assert not kw, kw
    if entry == "fwd":
        return lib.vgpt_attn_blockmask_fwd(q, k, v, o, bits, summary, B, L, nh, nkv, hd, *st, scale, variant, None)
    if entry == "lse":
        return lib.vgpt_attn_blockmask_fwd_lse(q, k, v, o, lse, bits, summary, order, B, L, nh, nkv, hd, *st, scale, None)
    if entry == "qrange":
        return lib.vgpt_attn_blockmask_fwd_qrange(q, k, v, o, q_start, bits, summary, order, B, L, nh, nkv, hd, *st, scale, None)
    assert entry == "plan"
    return lib.vgpt_attn_fwd_plan(q, k, v, o, lse, bits, items, isum, iorder, n_items, B, L, nh, nkv, hd, *st, scale, item_rows, None)


ENTRIES = ["fwd", "lse", "qrange", "plan"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_forward_entry_points_refuse_bad_calls(lib, entry):
    """attn_fwd_impl's checks (csrc/attn_fwd.hip), reached through each of the four entry points."""
    f = lambda **kw: _fwd(lib, entry, **kw)   # noqa: E731
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(bits=None)):
        _refused(lib, f(**kw), INVALID, b"null pointer")
    if entry != "plan":
        _refused(lib, f(summary=None), INVALID, b"null pointer")
    for kw in (dict(B=-1), dict(L=-1), dict(nh=0), dict(nkv=0), dict(nh=-2)):
        _refused(lib, f(**kw), INVALID, b"bad shape")
    for nh, nkv in ((4, 3), (3, 2), (1, 2)):
        _refused(lib, f(nh=nh, nkv=nkv), INVALID, b"n_kv_heads must divide n_heads")
    for hd in (80, 32, 0, 192):
        _refused(lib, f(hd=hd), UNSUPPORTED, b"unsupported (64, 96, 128)")
    for scale in (0.0, -0.1):
        _refused(lib, f(scale=scale), INVALID, b"scale must be positive")
    for n in STRIDE_NAMES[:9]:
        _refused(lib, f(**{n: S96[n] + 4}), UNSUPPORTED, b"q/k/v strides must be multiples of 8 elements")
    for n in STRIDE_NAMES[9:]:
        _refused(lib, f(**{n: S96[n] + 2}), UNSUPPORTED, b"o strides must be multiples of 4 elements")
    for kw in (dict(q=FAKE + 8), dict(k=FAKE + 8), dict(v=FAKE + 8), dict(o=FAKE + 4), dict(q=FAKE + 2)):
        _refused(lib, f(**kw), UNSUPPORTED, b"must be 16-byte aligned")
    for L in (1 << 24, 1 << 26):
        _refused(lib, f(L=L), UNSUPPORTED, b"problem too large")
    _refused(lib, f(B=1 << 20, L=1 << 20, nh=64, nkv=64), UNSUPPORTED, b"problem too large")
    for kw in (dict(k_ss=0), dict(v_ss=0), dict(k_ss=-8), dict(v_ss=-288), dict(k_ss=1 << 24), dict(v_ss=1 << 24)):
        _refused(lib, f(**kw), UNSUPPORTED, b"key/value row strides must be in (0, 2^24) elements")
    # nothing to do: OK before anything is read or launched
    assert f(B=0) == 0 and f(L=0) == 0
    assert f(o_ss=100, o_sh=4, o_sb=36, L=0) == 0        # output strides need multiples of 4 only


def test_variant_and_lse_are_checked(lib):
    for variant in (2, -1, 7):
        _refused(lib, _fwd(lib, "fwd", variant=variant), INVALID, b"unknown variant")
    _refused(lib, _fwd(lib, "lse", lse=None), INVALID, b"null lse")


def test_q_range_refuses_bad_starts(lib):
    for q_start in (100, 64, 129, -128, 384, 512):
        _refused(lib, _fwd(lib, "qrange", q_start=q_start), INVALID, b"q_start must be a multiple of 128 in [0, L]")
    assert _fwd(lib, "qrange", q_start=256, L=256) == 0       # q_start == L: no rows, OK without a launch
    assert _fwd(lib, "qrange", q_start=128, L=128, order=FAKE) == 0


def test_planned_launch_refuses_bad_plans(lib):
    for kw in (dict(items=None), dict(isum=None), dict(iorder=None)):
        _refused(lib, _fwd(lib, "plan", **kw), INVALID, b"vgpt_attn_fwd_plan: null pointer")
    for item_rows in (0, 64, 127, 129, 192, 512, -128):
        _refused(lib, _fwd(lib, "plan", item_rows=item_rows), INVALID, b"item_rows must be 128 or 256")
    for hd in (64, 128):                                       # the eight-wave kernel exists for head dim 96 only
        st = {n: v * hd // 96 for n, v in S96.items()}
        _refused(lib, _fwd(lib, "plan", item_rows=256, hd=hd, **st), UNSUPPORTED, b"256-row items need head_dim 96")
    assert _fwd(lib, "plan", n_items=0) == 0 and _fwd(lib, "plan", n_items=0, item_rows=256) == 0
    assert _fwd(lib, "plan", lse=None, n_items=0) == 0        # lse is optional


def test_plan_build_and_workspace_sizes(lib):
    build = lambda bits=FAKE, B=1, L=300, items=FAKE, n=3, isum=FAKE, order=FAKE: lib.vgpt_attn_plan_build(   # noqa: E731
        bits, B, L, items, n, isum, order, None)
    for kw in (dict(bits=None), dict(items=None), dict(isum=None), dict(order=None)):
        _refused(lib, build(**kw), INVALID, b"vgpt_attn_plan_build: null pointer")
    for kw in (dict(n=0), dict(n=65536), dict(n=-1), dict(L=(1 << 22) + 1), dict(L=0), dict(B=0)):
        _refused(lib, build(**kw), INVALID, b"vgpt_attn_plan_build: bad shape")
    ws = lib.vgpt_attn_plan_workspace_bytes
    assert ws(0, 3) == -1 and ws(-5, 3) == -1 and ws(300, -1) == -1
    a256 = lambda n: (n + 255) // 256 * 256   # noqa: E731
    assert ws(300, 3) == a256(3 * 5 * 2) + a256(3 * 4) and ws(300, 0) == 0 and ws(64, 1000) == a256(2000) + a256(4000)
    w8 = lib.vgpt_attn_fp8_workspace_bytes
    for args in ((0, 300, 2, 2, 96), (1, 0, 2, 2, 96), (1, 300, 0, 2, 96), (1, 300, 2, 0, 96), (1, 300, 2, 2, 128), (1, 300, 2, 2, 64),
                 (1, 300, 2, 2, 80), (-1, 300, 2, 2, 96)):
        assert w8(*args) == -1, args
    assert w8(2, 300, 4, 2, 96) == a256(2 * 4 * 300 * 96) + a256(2 * 4 * 300 * 4) + 2 * 2 * 5 * 13 * 1024


def test_supported_head_dims(lib):
    assert [lib.vgpt_attn_supported(hd) for hd in (64, 96, 128, 80, 0, 32, 256)] == [1, 1, 1, 0, 0, 0, 0]


def _quant(lib, q=FAKE, k=FAKE, v=FAKE, ws=FAKE, B=1, L=300, row_begin=0, nh=2, nkv=2, hd=96, scale=0.1, **kw):
    st = _strides(kw)[:9]
    assert not kw, kw
    return lib.vgpt_attn_fp8_quantize(q, k, v, ws, B, L, row_begin, nh, nkv, hd, *st, scale, None)


def _plan8(lib, ws=FAKE, o=FAKE, bits=FAKE, items=FAKE, isum=FAKE, order=FAKE, n_items=3, B=1, L=300, nh=2, nkv=2, hd=96, **kw):
    st = _strides(kw)[9:]
    assert not kw, kw
    return lib.vgpt_attn_fwd_plan_fp8(ws, o, bits, items, isum, order, n_items, B, L, nh, nkv, hd, *st, None)


def test_fp8_pair_refuses_bad_calls(lib):
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(ws=None)):
        _refused(lib, _quant(lib, **kw), INVALID, b"vgpt_attn_fp8_quantize: null pointer")
    for hd in (64, 128, 80):
        _refused(lib, _quant(lib, hd=hd), UNSUPPORTED, b"vgpt_attn_fp8_quantize: head_dim must be 96")
    for kw in (dict(B=0), dict(L=0), dict(L=(1 << 22) + 1), dict(nh=0), dict(nkv=0), dict(nh=4, nkv=3)):
        _refused(lib, _quant(lib, **kw), INVALID, b"vgpt_attn_fp8_quantize: bad shape")
    for scale in (0.0, -1.0):
        _refused(lib, _quant(lib, scale=scale), INVALID, b"scale must be positive")
    for row_begin in (100, 32, 65, -64, 320, 384):
        _refused(lib, _quant(lib, row_begin=row_begin), INVALID, b"row_begin must be a multiple of 64 in [0, L]")
    assert _quant(lib, row_begin=256, L=256) == 0              # nothing left to quantise: OK without a launch
    for n in STRIDE_NAMES[:9]:
        _refused(lib, _quant(lib, **{n: S96[n] + 4}), UNSUPPORTED, b"q/k/v strides must be multiples of 8 elements")
    for kw in (dict(q=FAKE + 8), dict(k=FAKE + 8), dict(v=FAKE + 8), dict(ws=FAKE + 8)):
        _refused(lib, _quant(lib, **kw), UNSUPPORTED, b"must be 16-byte aligned")
    _refused(lib, _quant(lib, B=4096, L=1 << 22, nh=8, nkv=8), UNSUPPORTED, b"problem too large")

    for kw in (dict(ws=None), dict(o=None), dict(bits=None), dict(items=None), dict(isum=None), dict(order=None)):
        _refused(lib, _plan8(lib, **kw), INVALID, b"vgpt_attn_fwd_plan_fp8: null pointer")
    for hd in (64, 128, 80):
        _refused(lib, _plan8(lib, hd=hd), UNSUPPORTED, b"vgpt_attn_fwd_plan_fp8: head_dim must be 96")
    for kw in (dict(B=0), dict(L=0), dict(L=(1 << 22) + 1), dict(n_items=-1), dict(n_items=65536), dict(nh=0), dict(nkv=0),
               dict(nh=4, nkv=3)):
        _refused(lib, _plan8(lib, **kw), INVALID, b"vgpt_attn_fwd_plan_fp8: bad shape")
    for kw in (dict(o_sb=S96["o_sb"] + 2), dict(o_sh=98), dict(o_ss=194), dict(o=FAKE + 4), dict(o=FAKE + 2)):
        _refused(lib, _plan8(lib, **kw), UNSUPPORTED, b"o strides must be multiples of 4 elements, o 8-byte aligned")
    assert _plan8(lib, n_items=0) == 0 and _plan8(lib, n_items=0, o_ss=100, o=FAKE + 8) == 0


# ============================================================================================================
# the CPU model of the forward kernel against the element-wise bound of the GPU test
# ============================================================================================================
def _model_forward(q, k, v, m, scale):
    """attn_fwd_kernel's arithmetic in plain torch on the CPU: per 64-key tile fp32 scores of the bf16 values, the row
    maximum, p = exp2(s c - m) in fp32, the row sum from the unrounded p, p rounded to bf16 for the fp32 P V product,
    rescales of l and O by exp2(m_old - m_new); at the end O / l rounded once to bf16.  q (B, L, nh, hd), k / v (B, L, nkv, hd)."""
    B, L, nh, hd = q.shape
    grp = nh // k.shape[2]
    qh = q.float().permute(0, 2, 1, 3)
    kh = k.float().permute(0, 2, 1, 3).repeat_interleave(grp, 1)
    vh = v.float().permute(0, 2, 1, 3).repeat_interleave(grp, 1)
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(G.LOG2E, dtype=torch.float32)
    m_i = torch.full((B, nh, L, 1), float("-inf"))
    l_i = torch.zeros(B, nh, L, 1)
    O = torch.zeros(B, nh, L, hd)
    for k0 in range(0, L, 64):
        k1 = min(k0 + 64, L)
        s = (qh @ kh[:, :, k0:k1].transpose(2, 3)).masked_fill(~m[:, None, :, k0:k1], float("-inf"))
        m_new = torch.maximum(m_i, s.amax(-1, keepdim=True) * c)
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m_i - m_use)
        p = torch.exp2(s * c - m_use)
        l_i = l_i * alpha + p.sum(-1, keepdim=True)
        O = O * alpha + p.to(torch.bfloat16).float() @ vh[:, :, k0:k1]
        m_i = m_new
    inv = torch.where(l_i > 0, 1.0 / l_i, torch.zeros_like(l_i))
    return (O * inv).to(torch.bfloat16).permute(0, 2, 1, 3)


def _model_cases():
    seen, out = set(), []
    for c in G.CASES:
        path, hd, kind, B, L, nh, nkv, _, kw = c.values
        key = (hd, kind, B, L, nh, nkv, kw.get("scale"))
        if path != "G" and L <= 257 and key not in seen:
            seen.add(key)
            out.append(pytest.param(*key, id=f"hd{hd}-{kind}-B{B}-L{L}-h{nh}x{nkv}" + (f"-scale{key[-1]}" if key[-1] else "")))
    return out


def _model_ratio(hd, kind, B, L, nh, nkv, scale):
    m, q, k, v = G.attn_inputs(kind, B, L, nh, nkv, hd)
    scale = float(scale or 1 / math.sqrt(hd))
    ref = G.attn_reference(q, k, v, m, scale)
    bound = G.attn_fwd_bound(ref, scale, hd)
    out = _model_forward(q, k, v, m, scale)
    assert torch.isfinite(out.float()).all()
    assert bool((out[~m.any(-1)] == 0).all())          # wholly masked rows: exact zeros
    return float(((out.double() - ref["o"]).abs() / bound).max())


@pytest.fixture(scope="module")
def model_ratios():
    """Worst |err| / bound of the model per case, computed once for both tests below."""
    return {c.id: _model_ratio(*c.values) for c in _model_cases()}


@pytest.mark.parametrize("case", [c.id for c in _model_cases()])
def test_cpu_model_stays_within_the_elementwise_bound(model_ratios, case):
    print(f"MEASURE cpu model {case}: worst |err|/bound = {model_ratios[case]:.3g}")
    assert model_ratios[case] <= 1.0


def test_cpu_model_fills_the_bound(model_ratios):
    """A bound the honest model fills to a few percent only would hide errors.  The final rounding alone reaches half an ulp
    on some element of every larger case, and the bound there is that half ulp plus 2^-8 sum_j P |V| >= 2^-8 |ref|, half an
    ulp to an ulp more where the signs of V do not cancel (a row that sees few keys): a third of the bound from the final
    rounding alone, the rounding of P on top of it.  The worst ratio over the cases must come out above 1/2."""
    worst = list(model_ratios.values())
    print(f"MEASURE cpu model: worst |err|/bound over {len(worst)} cases = {max(worst):.3g}, smallest per-case worst {min(worst):.3g}")
    assert max(worst) > 0.5
