"""The attention backward at head dims 64 and 128 (csrc/attn_bwd.hip, vgpt_attn_blockmask_bwd_hd) against fp64 autograd:
section A of tests/test_train_kernels_gpu.py restated with the head dim as a parameter, on the same covering set, the
same single-row probes and the same limits.  The only figure that moves with the head dim is the cancellation term of the
element-wise bound, 2 * hd * u (192 u there is 2 * 96 u), and the length of the delta dot product, hd.  Added here: the
C entry point on padded, separately allocated buffers between NaN guards, and the bit-for-bit relations (B = 2 against
two B = 1 launches, head dim 96 through the new entry point against the old one).

The bounds are derived (see _attn_bwd_explicit), not measured; the worst measured |err| / bound is 0.46 at head dim 64 and
0.46 at head dim 128 (covering set), 0.53 / 0.48 on the single-row probes."""
import ctypes
import importlib
import math

import pytest
import torch

from oracle import restate as R
from tests.test_ops_gpu import bf, g, rel_l2
from tests.test_train_kernels_gpu import ATTN_CASES, U32, _mask, _per_row, _ulp, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
HEAD_DIMS = [64, 128]


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("video-gpt_amd.ops_train")


def _attn_ref(qkv, m, nh, nkv, dout, hd):
    """fp64 autograd of masked softmax attention on the fused qkv rows; wholly masked rows give O = 0 and no gradient.
    Returns O (B, L, nh*hd), lse (B, nh, L) in log2 units (-inf on empty rows), P (B, nh, L, L) and dqkv."""
    B, L, width = qkv.shape
    x = qkv.detach().to(DEV, F64).requires_grad_()
    q = x[..., : nh * hd].view(B, L, nh, hd).transpose(1, 2)
    k = x[..., nh * hd:(nh + nkv) * hd].view(B, L, nkv, hd).transpose(1, 2).repeat_interleave(nh // nkv, 1)
    v = x[..., (nh + nkv) * hd:].view(B, L, nkv, hd).transpose(1, 2).repeat_interleave(nh // nkv, 1)
    mm = m.to(DEV)[:, None]
    s = (q @ k.transpose(2, 3) / math.sqrt(hd)).masked_fill(~mm, float("-inf"))
    mx = s.amax(-1, keepdim=True).detach()
    e = torch.exp(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(l > 0, l, torch.ones_like(l))
    o = (p @ v).transpose(1, 2).reshape(B, L, nh * hd)
    o.backward(dout.to(DEV, F64))
    lse = torch.logsumexp(s.detach(), -1) / math.log(2)
    return o.detach(), lse, p.detach(), x.grad


def _attn_fwd(T, ops, qkv, m, nh, nkv, hd):
    B, L, width = qkv.shape
    pm = ops.pack_mask(m.to(DEV))
    qd = qkv.to(DEV, BF)
    out = torch.empty(B, L, nh * hd, dtype=BF, device=DEV)
    lse = torch.empty(B, nh, L, dtype=F32, device=DEV)
    T.attention_qkv_train(qd, pm, nh, nkv, hd, out, lse)
    return pm, qd, out, lse


def _attn_run(T, ops, qkv, m, nh, nkv, dout, hd):
    B, L, width = qkv.shape
    pm, qd, out, lse = _attn_fwd(T, ops, qkv, m, nh, nkv, hd)
    dqkv = torch.full((B, L, width), float("nan"), dtype=BF, device=DEV)   # every element must be written
    delta = torch.empty(B, nh, L, dtype=F32, device=DEV)
    T.attention_qkv_bwd(qd, out, dout.to(DEV, BF), lse, delta, dqkv, pm, nh, nkv, hd)
    return pm, qd, out, lse, dqkv, delta


def _split(t, nh, nkv, hd):
    """(B, L, width) -> per-head views dq (B, L, nh, hd), dk, dv (B, L, nkv, hd)."""
    B, L, _ = t.shape
    a, b = nh * hd, (nh + nkv) * hd
    return t[..., :a].reshape(B, L, nh, hd), t[..., a:b].reshape(B, L, nkv, hd), t[..., b:].reshape(B, L, nkv, hd)


def _attn_bwd_explicit(qkv, p, nh, nkv, dout, out, hd):
    """dQ, dK, dV (B, L, heads, hd) in fp64 from the fp64 probabilities p (B, nh, L, L) with delta = rowsum(dO o O) on the
    kernel's own bf16 O (the value the backward reads), and element-wise bounds for each.  The backward rounds P and
    dS = P (dP - delta) to bf16 before its MFMAs (relative 2^-8 at most, the bf16 unit roundoff; the fp32 accumulation of
    <= L products adds L u << 2^-8), and dP - delta cancels in fp32 (two hd-term sums of the same products:
    2 * hd u sum_d |dO| (|V| + |O|)).  With twice that rounding per score,
        e_ij = P_ij (2^-7 |dP_ij - delta_i| + 2 hd u sum_d |dO_id| (|V_jd| + |O_id|)) / sqrt(hd)
    and  |dQ - ref| <= ulp + e |K|,  |dK - ref| <= ulp + e^T |Q|,  |dV - ref| <= ulp + 2^-7 P^T |dO|  (GQA: summed over
    the heads of a group)."""
    B, L, _ = qkv.shape
    grp = nh // nkv
    x = qkv.to(DEV, F64)
    q = x[..., : nh * hd].view(B, L, nh, hd).transpose(1, 2)
    k = x[..., nh * hd:(nh + nkv) * hd].view(B, L, nkv, hd).transpose(1, 2).repeat_interleave(grp, 1)
    v = x[..., (nh + nkv) * hd:].view(B, L, nkv, hd).transpose(1, 2).repeat_interleave(grp, 1)
    do = dout.to(DEV, F64).view(B, L, nh, hd).transpose(1, 2)
    o = out.double().view(B, L, nh, hd).transpose(1, 2)
    dp = do @ v.transpose(2, 3)
    dlt = (do * o).sum(-1, keepdim=True)
    c = 1 / math.sqrt(hd)
    ds = p * (dp - dlt) * c
    cancel = 2 * hd * U32 * (do.abs() @ v.abs().transpose(2, 3) + (do * o).abs().sum(-1, keepdim=True))
    err = p * (2.0 ** -7 * (dp - dlt).abs() + cancel) * c
    group = lambda t: t.view(B, nkv, grp, L, hd).sum(2).transpose(1, 2)   # noqa: E731  (B, nh, L, hd) -> (B, L, nkv, hd)
    dq, dk, dv = (ds @ k).transpose(1, 2), group(ds.transpose(2, 3) @ q), group(p.transpose(2, 3) @ do)
    dq_b = _ulp(dq) + (err @ k.abs()).transpose(1, 2)
    dk_b = _ulp(dk) + group(err.transpose(2, 3) @ q.abs())
    dv_b = _ulp(dv) + group(2.0 ** -7 * p.transpose(2, 3) @ do.abs())
    return (dq, dk, dv), (dq_b, dk_b, dv_b)


def _case_inputs(kind, B, L, nh, nkv, hd):
    m = _mask(kind, B, L, 31 + L)
    L = m.shape[-1]
    width = (nh + 2 * nkv) * hd
    x = torch.randn(B, L, width, generator=g(40 + L + hd))
    if kind == "spike":   # one key 8x longer: rows that see it get a nearly one-hot P
        x[:, L // 3, nh * hd:(nh + nkv) * hd] *= 8.0
    return m, bf(x), bf(torch.randn(B, L, nh * hd, generator=g(41 + L + hd)))


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("kind,B,L,nh,nkv", ATTN_CASES, ids=[f"{c[0]}-B{c[1]}-L{c[2]}-h{c[3]}x{c[4]}" for c in ATTN_CASES])
def test_attention_train_forward_and_backward_against_fp64(ops, T, kind, B, L, nh, nkv, hd):
    m, qkv, dout = _case_inputs(kind, B, L, nh, nkv, hd)
    L = m.shape[-1]
    o_ref, lse_ref, p_ref, gref = _attn_ref(qkv, m, nh, nkv, dout, hd)
    pm, qd, out, lse, dqkv, delta = _attn_run(T, ops, qkv, m, nh, nkv, dout, hd)
    if kind == "spike":
        assert float(p_ref.amax(-1).max()) > 0.99   # the spike does make some rows one-hot

    mdev = m.to(DEV)
    empty_q = ~mdev.any(-1)          # (B, L) query rows with no visible key
    unseen_k = ~mdev.any(-2)         # (B, L) keys no query row sees
    if kind in ("holes", "unseen"):
        assert bool(empty_q.any() if kind == "holes" else unseen_k.any())
    live = ~empty_q[:, None, :].expand(B, nh, L)

    # forward: O rows; empty rows write exact zeros (the backward's delta relies on it)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out, o_ref) < 1e-2
    _per_row(out.view(B, L, nh, hd), o_ref.view(B, L, nh, hd), 3e-2, "attn O rows")
    assert bool((out.view(B, L, -1)[empty_q] == 0).all())
    lerr = (lse.double() - lse_ref)[live].abs()
    print(f"MEASURE attn lse: max |err| = {float(lerr.max()) if lerr.numel() else 0.0:.3g} (log2 units)")
    assert lerr.numel() == 0 or float(lerr.max()) < 5e-5
    assert bool((lse[~live] == float("inf")).all())        # empty rows: +inf exactly, so exp2(c S - lse) == 0

    # delta workspace == rowsum(dO o O) on the same bf16 values (hd-term fp32 dot: hd u sum|terms| worst case)
    o64 = out.double().view(B, L, nh, hd)
    d64 = dout.to(DEV, F64).view(B, L, nh, hd)
    dref = (o64 * d64).sum(-1).transpose(1, 2)
    dabs = (o64 * d64).abs().sum(-1).transpose(1, 2)
    _within(delta, dref, hd * U32 * dabs + 1e-30, f"attn delta hd{hd}")

    dq, dk, dv = _split(dqkv.float(), nh, nkv, hd)
    gq, gk, gv = _split(gref, nh, nkv, hd)
    assert torch.isfinite(dqkv.float()).all()        # the NaN prefill is gone: every element was written
    refs, bounds = _attn_bwd_explicit(qkv, p_ref, nh, nkv, dout, out, hd)
    for name, a, b, e, eb in zip(("dq", "dk", "dv"), (dq, dk, dv), (gq, gk, gv), refs, bounds):
        # against fp64 autograd (exact O).  With a single visible key everywhere (L = 1) softmax is constant and the exact dq
        # and dk are identically 0: a relative error is undefined there, and what the fp32 cancellation dP - delta leaves
        # is held by the element-wise bound below
        assert float(b.norm()) == 0 or rel_l2(a, b) < 2e-2, name
        _within(a, e, eb, f"attn {name} hd{hd}")   # every element; the bound is derived in _attn_bwd_explicit
    if float(gk.norm()) > 0:          # L = 1: the exact dk is identically 0 (above), a relative row error is undefined
        _per_row(dk, gk, 4e-2, "attn dk rows")
    _per_row(dv, gv, 2e-2, "attn dv rows")
    # exact zeros: dQ of empty query rows, dK / dV of keys no row sees
    assert bool((dq[empty_q] == 0).all())
    assert bool((dk[unseen_k] == 0).all()) and bool((dv[unseen_k] == 0).all())

    # a second launch of the backward gives the same bits (gradient checkpointing recomputes and compares)
    dqkv2 = torch.empty_like(dqkv)
    delta2 = torch.empty_like(delta)
    T.attention_qkv_bwd(qd, out, dout.to(DEV, BF), lse, delta2, dqkv2, pm, nh, nkv, hd)
    assert torch.equal(dqkv2.view(torch.int16), dqkv.view(torch.int16))
    assert torch.equal(delta2.view(torch.int32), delta.view(torch.int32))


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", [(4, 2), (8, 1)])
def test_attention_backward_single_row_probes(ops, T, nh, nkv, hd):
    """dO non-zero on one query row only: dV / dK must be that row's fp64 outer-product contribution (element-wise, the
    bounds of _attn_bwd_explicit), every other dQ row and every key the row does not see exactly 0.  A wrong row map,
    tile map or GQA head map shows up as a gradient on the wrong key or row."""
    batch = R.collate_stage1([3, 2], 64)
    m = batch["attention_mask"]
    B, L = m.shape[0], m.shape[-1]
    width = (nh + 2 * nkv) * hd
    qkv = bf(torch.randn(B, L, width, generator=g(50 + hd)))
    pm, qd, out, lse = _attn_fwd(T, ops, qkv, m, nh, nkv, hd)
    dfull = bf(torch.randn(B, L, nh * hd, generator=g(51 + hd)))
    # seams of item 0: the first denoise block ends at 66 and the first input block starts at 67 ([2, 66], [67, 131]);
    # item 1 is left-padded (its first block starts at 134)
    seams = batch["denoise_image_sizes"][0][0][1]
    rows = [(0, 0), (0, seams - 1), (0, seams), (0, seams + 1), (1, 133), (1, 134), (0, L - 1), (1, L - 1)]
    _, _, p_ref, _ = _attn_ref(qkv, m, nh, nkv, dfull, hd)
    for b, r in rows:
        dout = torch.zeros(B, L, nh * hd)
        dout[b, r] = dfull[b, r]
        dqkv = torch.empty(B, L, width, dtype=BF, device=DEV)
        delta = torch.empty(B, nh, L, dtype=F32, device=DEV)
        T.attention_qkv_bwd(qd, out, dout.to(DEV, BF), lse, delta, dqkv, pm, nh, nkv, hd)
        dq, dk, dv = _split(dqkv.float(), nh, nkv, hd)
        vis = m[b, r].to(DEV)
        other = torch.ones(B, L, dtype=torch.bool, device=DEV)
        other[b, r] = False
        assert bool((dq[other] == 0).all()), f"row {(b, r)}: dQ on other rows"
        assert bool((dk[1 - b] == 0).all()) and bool((dv[1 - b] == 0).all()), f"row {(b, r)}: dK/dV in the other item"
        assert bool((dk[b][~vis] == 0).all()) and bool((dv[b][~vis] == 0).all()), f"row {(b, r)}: dK/dV on unseen keys"
        refs, bounds = _attn_bwd_explicit(qkv, p_ref, nh, nkv, dout, out, hd)
        for name, a, e, eb in zip(("dq", "dk", "dv"), (dq, dk, dv), refs, bounds):
            _within(a, e, eb, f"probe {name} hd{hd} row {(b, r)}")
        assert rel_l2(dv, refs[2]) < 1e-2, f"row {(b, r)}: dv"   # no cancellation in P^T dO: bf16 rounding of P only


# ============================================================================================================
# the C entry points themselves
# ============================================================================================================
def _bwd_entry(ops, entry, q, k, v, o, do, lse, delta, dq, dk, dv, pm, B, L, nh, nkv, hd, strides):
    """The C call of ops_train.attention_qkv_bwd with every pointer and stride spelled out (element offsets are the
    caller's: each argument is (tensor, element offset))."""
    arr = (ctypes.c_int64 * 24)(*strides)
    ptr = lambda t: t[0].data_ptr() + 2 * t[1]   # noqa: E731  bf16
    ops.call(entry, ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), lse.data_ptr(), delta.data_ptr(), ptr(dq), ptr(dk), ptr(dv),
             pm.bits.data_ptr(), pm.summary.data_ptr(), B, L, nh, nkv, hd, arr, 1.0 / math.sqrt(hd), ops._stream())


def _fused_strides(L, nh, nkv, hd):
    width = (nh + 2 * nkv) * hd
    return [L * width, hd, width] * 3 + [L * nh * hd, hd, nh * hd] * 2 + [L * width, hd, width] * 3


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_c_abi_padded_separate_buffers_between_nan_guards(ops, T, hd):
    """q, k, v, o, dout in buffers of their own whose rows are 8 elements longer than the data, dq / dk / dv in buffers of
    their own whose rows are 4 elements longer, one NaN guard row before and after every item: the values equal the fused
    contiguous run bit for bit, pads and guards stay NaN (nothing is written outside the rows, nothing read from the pads
    reaches a result)."""
    kind, B, L, nh, nkv = "holes", 2, 191, 4, 2
    m, qkv, dout = _case_inputs(kind, B, L, nh, nkv, hd)
    pm, qd, out, lse, dqkv, delta = _attn_run(T, ops, qkv, m, nh, nkv, dout, hd)
    nan = float("nan")

    def padded(src, pad):   # (B, L, w) -> NaN buffer (B, L + 2, w + pad) with the data in rows 1 .. L
        w = src.shape[-1]
        buf = torch.full((B, L + 2, w + pad), nan, dtype=BF, device=DEV)
        buf[:, 1:L + 1, :w] = src
        return buf

    hq, hk = nh * hd, nkv * hd
    ins = [padded(t, 8) for t in (qd[..., :hq], qd[..., hq:hq + hk], qd[..., hq + hk:], out, dout.to(DEV, BF))]
    outs = [torch.full((B, L + 2, w + 4), nan, dtype=BF, device=DEV) for w in (hq, hk, hk)]
    st = []
    for t in ins + outs:
        st += [t.stride(0), hd, t.stride(1)]
    delta2 = torch.empty_like(delta)
    args = [(t, t.stride(1)) for t in ins]   # skip the guard row
    oargs = [(t, t.stride(1)) for t in outs]
    _bwd_entry(ops, "vgpt_attn_blockmask_bwd_hd", *args, lse, delta2, *oargs, pm, B, L, nh, nkv, hd, st)
    torch.cuda.synchronize()
    ref = (dqkv[..., :hq], dqkv[..., hq:hq + hk], dqkv[..., hq + hk:])
    for name, t, r in zip(("dq", "dk", "dv"), outs, ref):
        w = r.shape[-1]
        assert torch.equal(t[:, 1:L + 1, :w].contiguous().view(torch.int16), r.contiguous().view(torch.int16)), name
        assert bool(torch.isnan(t[:, 1:L + 1, w:].float()).all()), f"{name}: row pad written"
        assert bool(torch.isnan(t[:, 0].float()).all()) and bool(torch.isnan(t[:, L + 1].float()).all()), f"{name}: guard row"
    assert torch.equal(delta2.view(torch.int32), delta.view(torch.int32))


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_batch_of_two_equals_two_single_launches(ops, T, hd):
    kind, B, L, nh, nkv = "stage1", 2, 330, 4, 2
    m, qkv, dout = _case_inputs(kind, B, L, nh, nkv, hd)
    _, _, out, lse, dqkv, delta = _attn_run(T, ops, qkv, m, nh, nkv, dout, hd)
    for b in range(2):
        _, _, out1, lse1, dqkv1, delta1 = _attn_run(T, ops, qkv[b:b + 1], m[b:b + 1], nh, nkv, dout[b:b + 1], hd)
        assert torch.equal(out1.view(torch.int16), out[b:b + 1].view(torch.int16))
        assert torch.equal(dqkv1.view(torch.int16), dqkv[b:b + 1].view(torch.int16)), f"item {b}"
        assert torch.equal(delta1.view(torch.int32), delta[b:b + 1].view(torch.int32))


@pytest.mark.parametrize("kind,B,L,nh,nkv", [ATTN_CASES[11], ATTN_CASES[13], ATTN_CASES[15]],
                         ids=["holes-B2-L383-h8x2", "stage1-B2-L330-h4x2", "spike-B1-L257-h4x2"])
def test_head_dim_96_through_the_new_entry_point_equals_the_old_one(ops, T, kind, B, L, nh, nkv):
    hd = 96
    m, qkv, dout = _case_inputs(kind, B, L, nh, nkv, hd)
    L = m.shape[-1]
    pm, qd, out, lse = _attn_fwd(T, ops, qkv, m, nh, nkv, hd)
    dd = dout.to(DEV, BF)
    hq, hk = nh * hd, nkv * hd
    res = []
    for entry in ("vgpt_attn_blockmask_bwd", "vgpt_attn_blockmask_bwd_hd"):
        dqkv = torch.full_like(qd, float("nan"))
        delta = torch.empty(B, nh, L, dtype=F32, device=DEV)
        _bwd_entry(ops, entry, (qd, 0), (qd, hq), (qd, hq + hk), (out, 0), (dd, 0), lse, delta, (dqkv, 0), (dqkv, hq),
                   (dqkv, hq + hk), pm, B, L, nh, nkv, hd, _fused_strides(L, nh, nkv, hd))
        res.append((dqkv, delta))
    assert torch.isfinite(res[0][0].float()).all()
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
