"""vgpt_vae_attn_fwd (csrc/vae_attn.hip through ops.vae_attention), the fused mid-block attention of the VAE, at the shapes
where such a kernel goes wrong: one key, key and query tiles one short of / exactly / one past full, several tiles with a
ragged end, the 176 x 320 frame (880 positions), 1024 positions; C = 64, 128, 512; 1 and 3 images; contiguous and padded
channel / image strides (16-byte and scalar staging).

Harness: every tensor lives in a NaN-filled buffer with a guard band in front and behind; with a padded ld the pad columns of
q, k, v are NaN too and those of o start as NaN.  After every launch the output is finite, and every float outside the
(N, C, HW) view of every buffer, inputs included, still holds its bits.

TQ / TK below are VGPT_VAE_ATTN_TQ / VGPT_VAE_ATTN_TK of include/vgpt.h."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_train_kernels_gpu import _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24
TINY = 2.0 ** -126
BAND = 64          # guard floats in front of and behind every tensor (256 bytes: the view keeps the buffer's alignment)

_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vgpt.h")).read()
TQ = int(re.search(r"#define VGPT_VAE_ATTN_TQ (\d+)", _HDR).group(1))
TK = int(re.search(r"#define VGPT_VAE_ATTN_TK (\d+)", _HDR).group(1))
HWS = sorted({1, 2, TK - 1, TK, TK + 1, TQ - 1, TQ, TQ + 1, 2 * TQ + TK - 1, 880, 1024})
CS = [64, 128, 512]


def g(seed):
    return torch.Generator("cpu").manual_seed(seed)


class _Banded:
    """(N, C, HW) fp32 view with strides (bs, ld, 1) inside a NaN buffer: [BAND | N * bs | BAND]."""

    def __init__(self, N, C, HW, ld, bs, values=None):
        self.buf = torch.full((2 * BAND + N * bs,), float("nan"), dtype=F32, device=DEV)
        self.view = torch.as_strided(self.buf, (N, C, HW), (bs, ld, 1), BAND)
        if values is not None:
            self.view.copy_(values)
        inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        torch.as_strided(inside, (N, C, HW), (bs, ld, 1), BAND).fill_(True)
        self.outside = ~inside
        self.before = self.buf.view(torch.int32).clone()

    def assert_untouched(self, what, whole=False):
        now = self.buf.view(torch.int32)
        if whole:
            assert torch.equal(now, self.before), f"{what}: an input buffer changed"
        else:
            assert torch.equal(now[self.outside], self.before[self.outside]), f"{what}: written outside the (N, C, HW) view"


def fused(ops, q, k, v, scale, ld_pad=False, bs_pad=0, what="fused"):
    """One launch on guard-banded buffers; q, k, v: (N, C, HW) values.  Returns the contiguous (N, C, HW) output."""
    N, C, HW = q.shape
    ld = HW + 3 if ld_pad else HW
    bs = C * ld + bs_pad
    bq, bk, bv = (_Banded(N, C, HW, ld, bs, t.to(DEV)) for t in (q, k, v))
    bo = _Banded(N, C, HW, ld, bs)
    ret = ops.vae_attention(bq.view, bk.view, bv.view, scale, out=bo.view)
    assert ret.data_ptr() == bo.view.data_ptr()
    torch.cuda.synchronize()
    out = bo.view.contiguous()
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    for b in (bq, bk, bv):
        b.assert_untouched(what, whole=True)
    bo.assert_untouched(what)
    return out


def materialised(ops, q, k, v, scale):
    """The existing path on the same values: K^T Q through the conv kernel, column softmax, P V through the conv kernel."""
    N, C, HW = q.shape
    q4, k4, v4 = (t.to(DEV).contiguous().view(N, C, 1, HW) for t in (q, k, v))
    st = ops.conv2d(q4, k4, ksize=1, cout=HW, w_transposed=True, ldw=HW, w_batch_stride=C * HW)
    ops.col_softmax(st.view(N, HW, HW), scale)
    return ops.conv2d(st, v4, ksize=1, cout=C, ldw=HW, w_batch_stride=C * HW).view(N, C, HW)


def attn_ref_and_bound(q, k, v, scale, queries=None):
    """float64 attention of the fp32 values and the element-wise bound of fp32 attention, u = 2^-24.

    With S_j = sum_c k_cj q_ci, A_j = sum_c |k_cj| |q_ci|, x_j = scale S_j, X = max |x|, T = ceil(HW / TK) key tiles:
      - a score is an fp32 FMA chain of at most C terms (the fused kernel: four chains of C/4 and three adds; the conv
        kernel: one chain of C): |s^ - S_j| <= (C + 4) u A_j, i.e. scale (C + 4) u A_j in the exponent;
      - x = fl(s scale): u |x_j|; fl(x - m) with any running maximum m: u |x_j - m| <= 2 u X; the exponential's own
        argument product (v_exp_f32((x - m) log2 e), or expf's reduction): another 2 u X; its result: 2 u;
      - one rescale a = exp(m_old - m_new) per key tile, applied by one multiply: (|m_old - m_new| + 3) u each; the rises
        of m telescope to at most 2 X: rho = (2 X + 3 T + 8) u in all, 8 covering the materialised path's merge of its four
        key quarters and its division before the product;
      so every weight is p_j (1 + e_j) with e_j <= expm1(scale (C + 4) u A_j + u |x_j| + 4 u X + 2 u + rho);
      - numerator and denominator are accumulations of HW terms: HW u on top of e_j for each term, weighted by
        p_j |v_cj| and by p_j;
      - with w_j = p_j (e_j + HW u) / l and eta = sum_j w_j:
            |o^ - o| <= (sum_j w_j |v_cj| + |o| eta) / (1 - eta) + 2 u |o|     (the last term: the division)
        plus the smallest normal fp32.  Where eta >= 1 the bound says nothing and is infinite (the output must still be
        finite); the share of such elements is printed, and it is 0 for randn inputs (asserted: eta < 0.01 there).
    The bound describes fp32 attention, not one kernel: test_random_against_float64 holds the materialised path
    (conv2d -> col_softmax -> conv2d) to it on the same inputs.  It is a worst-case bound: at C = 512 with inputs * 30 the
    first term alone reaches e_j ~ 0.4, and there it mostly shows that nothing overflowed."""
    q, k, v = (t.to(DEV).double() for t in (q, k, v))
    if queries is not None:
        q = q[:, :, queries]
    N, C, HW = k.shape
    T = -(-HW // TK)
    x = torch.einsum("ncj,nci->nji", k, q) * scale
    A = torch.einsum("ncj,nci->nji", k.abs(), q.abs())
    X = x.abs().amax(dim=(1, 2), keepdim=True)
    rho = (2 * X + 3 * T + 8) * U32
    e = torch.expm1(scale * (C + 4) * U32 * A + U32 * x.abs() + 4 * U32 * X + 2 * U32 + rho)
    p = torch.exp(x - x.amax(dim=1, keepdim=True))
    l = p.sum(1, keepdim=True)
    ref = torch.einsum("ncj,nji->nci", v, p / l)
    w = p * (e + HW * U32) / l
    eta = w.sum(1, keepdim=True)
    bound = (torch.einsum("ncj,nji->nci", v.abs(), w) + ref.abs() * eta) / (1 - eta) + 2 * U32 * ref.abs() + TINY
    bound = torch.where(eta < 1, bound, torch.full_like(bound, float("inf")))
    print(f"MEASURE attention bound: max eta = {float(eta.max()):.3g}, void share = {float((eta >= 1).double().mean()):.3g}")
    return ref, bound, float(eta.max())


# ============================================================================================================
# 1. one key: softmax over a single key is 1, o == v
# ============================================================================================================
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N,ld_pad,bs_pad", [(1, False, 0), (3, True, 8), (3, False, 5)])
def test_single_position_returns_v(ops, C, N, ld_pad, bs_pad):
    q, k, v = (torch.randn(N, C, 1, generator=g(700 + i)) * 3 for i in range(3))
    out = fused(ops, q, k, v, 1 / C ** 0.5, ld_pad, bs_pad, f"HW=1 C={C} N={N}")
    assert torch.equal(out.cpu().view(torch.int32), v.view(torch.int32))


# ============================================================================================================
# 2. uniform probe: q = 0 makes every weight 1 / HW; one-hot V rows count the keys that took part
# ============================================================================================================
def _probe_keys(HW):
    """First and last key of every key tile, and every key of the ragged last tile."""
    keys = []
    for t0 in range(0, HW, TK):
        keys += [t0, min(t0 + TK - 1, HW - 1)]
    keys += list(range((HW // TK) * TK, HW)) + [HW - 1]
    return sorted(set(keys))


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C,N,ld_pad,bs_pad", [(64, 1, False, 0), (128, 3, True, 8), (512, 1, True, 0), (64, 3, False, 5)])
def test_uniform_probe_counts_every_key_once(ops, HW, C, N, ld_pad, bs_pad):
    """o[c][i] = 1 / HW where channel c marks a key, 0 elsewhere.  A masked key that should count, an unmasked pad column
    (NaN in k and v) or a tail key dropped changes the denominator or the numerator."""
    keys = _probe_keys(HW)[-C:]   # 880 positions have 70 such keys: C = 64 keeps the ragged tile and the last tiles' ends
    q = torch.zeros(N, C, HW)
    k = torch.randn(N, C, HW, generator=g(710)) * 5
    v = torch.zeros(N, C, HW)
    for c, j in enumerate(keys):
        v[:, c, j] = 1.0
    out = fused(ops, q, k, v, 1 / C ** 0.5, ld_pad, bs_pad, f"uniform HW={HW} C={C} N={N}").cpu()
    assert torch.equal(out[:, len(keys):], torch.zeros(N, C - len(keys), HW)), "a channel without a marked key is not 0"
    want = np.float32(1.0) / np.float32(HW)
    ulp = float(np.spacing(want))
    err = (out[:, :len(keys)].double() - float(want)).abs().max().item()
    print(f"MEASURE uniform HW={HW} C={C}: worst error {err / ulp:.3g} ulp of 1/HW")
    assert err <= 2 * ulp


# ============================================================================================================
# 3. one-hot probe: the index map key -> query
# ============================================================================================================
@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("N,ld_pad,bs_pad", [(1, False, 0), (3, True, 8)])
def test_one_hot_probe_moves_v_columns(ops, HW, N, ld_pad, bs_pad):
    """k = random signs, q[:, i] = 5 k[:, pi(i)], scale 1/2, C = 128: the score of key pi(i) is 320 and every other key's is
    2.5 * (a sum of 128 signs), so it leads by at least 64 (asserted in float64 before the launch); exp(-64) = 1.6e-28 is
    far below half an ulp of 1 and of any v, so l == 1 and o[:, i] == v[:, pi(i)] bit for bit.  pi is a random permutation
    (it crosses tiles) and differs per image."""
    C, scale = 128, 0.5
    k = torch.randint(0, 2, (N, C, HW), generator=g(720 + HW)).float() * 2 - 1
    pi = torch.stack([torch.randperm(HW, generator=g(730 + HW + n)) for n in range(N)])
    q = 5 * torch.stack([k[n][:, pi[n]] for n in range(N)])
    v = torch.randn(N, C, HW, generator=g(740))
    s = torch.einsum("ncj,nci->nji", k.double(), q.double()) * scale            # [n][key][query]
    chosen = s.gather(1, pi[:, None, :]).squeeze(1)
    others = s.scatter(1, pi[:, None, :], float("-inf")).amax(1)
    assert HW == 1 or float((chosen - others).min()) >= 64, float((chosen - others).min())
    out = fused(ops, q, k, v, scale, ld_pad, bs_pad, f"one-hot HW={HW} N={N}").cpu()
    want = torch.stack([v[n][:, pi[n]] for n in range(N)])
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ============================================================================================================
# 4. random values against float64, element-wise, the materialised path held to the same bound
# ============================================================================================================
@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_random_against_float64(ops, HW, C):
    """Bound: attn_ref_and_bound.  randn inputs, and randn * 30: scaled scores in the thousands, so a missing maximum
    subtraction overflows the exponential.  Measured worst |err| / bound over all cases of this test
    (profiles/vae_attn_tests.log): 0.010 for the fused kernel, 0.030 for the materialised path, both at HW = 880, C = 64
    with inputs * 30; with randn inputs 0.009 and 0.019.  Largest eta: 0.65 (C = 512, inputs * 30), so no element's bound
    was void."""
    for N, ld_pad, bs_pad, amp in ((1, False, 0, 1.0), (3, True, 8, 30.0), (3, False, 5, 1.0), (1, True, 0, 30.0)):
        q, k, v = (torch.randn(N, C, HW, generator=g(750 + i)) * amp for i in range(3))
        scale = 1 / C ** 0.5
        ref, bound, eta = attn_ref_and_bound(q, k, v, scale)
        assert amp != 1.0 or eta < 0.01
        what = f"HW={HW} C={C} N={N} x{amp:g} ld_pad={ld_pad} bs_pad={bs_pad}"
        _within(fused(ops, q, k, v, scale, ld_pad, bs_pad, what), ref, bound, "fused " + what)
        _within(materialised(ops, q, k, v, scale), ref, bound, "materialised " + what)


@pytest.mark.parametrize("C", [192, 256, 320, 384, 448])
def test_other_channel_counts_against_float64(ops, C):
    """Every other supported C is an instantiation of its own: where C / 32 is no multiple of 4 the waves own unequal
    numbers of output tiles, and the K register ring wraps at another length."""
    HW = 2 * TQ + TK - 1
    for N, ld_pad, bs_pad, amp in ((2, False, 0, 1.0), (1, True, 5, 30.0)):
        q, k, v = (torch.randn(N, C, HW, generator=g(755 + i)) * amp for i in range(3))
        ref, bound, _ = attn_ref_and_bound(q, k, v, 1 / C ** 0.5)
        what = f"HW={HW} C={C} N={N} x{amp:g} ld_pad={ld_pad} bs_pad={bs_pad}"
        _within(fused(ops, q, k, v, 1 / C ** 0.5, ld_pad, bs_pad, what), ref, bound, "fused " + what)


def test_production_shape_against_float64(ops):
    """The mid-block of a 256 x 256 frame: C = 512, HW = 1024, two images, scale 1 / sqrt(512)."""
    q, k, v = (torch.randn(2, 512, 1024, generator=g(760 + i)) for i in range(3))
    scale = 1 / 512 ** 0.5
    ref, bound, eta = attn_ref_and_bound(q, k, v, scale)
    assert eta < 0.01
    _within(fused(ops, q, k, v, scale, what="production"), ref, bound, "fused production 2x512x1024")
    _within(materialised(ops, q, k, v, scale), ref, bound, "materialised production 2x512x1024")


# ============================================================================================================
# 5. bit-for-bit relations
# ============================================================================================================
@pytest.mark.parametrize("HW", [TK + 1, 2 * TQ + TK - 1, 880])
@pytest.mark.parametrize("C", [64, 512])
def test_bit_for_bit_relations(ops, HW, C):
    N, scale = 3, 1 / C ** 0.5
    q, k, v = (torch.randn(N, C, HW, generator=g(770 + i)) * 2 for i in range(3))
    base = fused(ops, q, k, v, scale, what="first launch")
    bits = base.view(torch.int32)
    assert torch.equal(fused(ops, q, k, v, scale, what="second launch").view(torch.int32), bits), "two launches differ"
    single = torch.cat([fused(ops, q[n:n + 1], k[n:n + 1], v[n:n + 1], scale, what="single image") for n in range(N)])
    assert torch.equal(single.view(torch.int32), bits), "a batch of 3 differs from three single launches"
    for ld_pad, bs_pad in ((True, 0), (True, 8), (False, 5), (False, 8)):
        out = fused(ops, q, k, v, scale, ld_pad, bs_pad, what="padded")
        assert torch.equal(out.view(torch.int32), bits), f"ld_pad={ld_pad} bs_pad={bs_pad} differs from contiguous"
    # beside a busy second stream
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(8):
            a = (a @ a).clamp_(-1, 1)
    out = fused(ops, q, k, v, scale, what="beside a busy stream")
    side.synchronize()
    assert torch.equal(out.view(torch.int32), bits), "a launch beside a busy stream differs"


def test_wrapper_refuses_mismatched_tensors(ops):
    from importlib import import_module
    VgptError = import_module("video-gpt_amd._lib").VgptError
    q = torch.randn(1, 64, 5, 5, device=DEV)
    with pytest.raises(VgptError):
        ops.vae_attention(q, q.double(), q, 0.125)
    with pytest.raises(VgptError):
        ops.vae_attention(q, q.cpu(), q, 0.125)
    with pytest.raises(VgptError):
        ops.vae_attention(q, q[:, :, :4], q, 0.125)
    with pytest.raises(VgptError):
        ops.vae_attention(q, q, q.transpose(2, 3), 0.125)
    with pytest.raises(VgptError):
        ops.vae_attention(torch.randn(1, 96, 5, 5, device=DEV), *([torch.randn(1, 96, 5, 5, device=DEV)] * 2), 0.125)
    out = ops.vae_attention(q, q, q, 0.125)
    q3 = q.view(1, 64, 25)
    assert out.shape == q.shape and torch.equal(out, ops.vae_attention(q3, q3, q3, 0.125).view_as(q))
