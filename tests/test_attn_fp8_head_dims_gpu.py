"""MX-fp8 attention at head dims 64 and 128 (video-gpt_amd/csrc/attn_fp8.hip through vgpt_attn_fp8_quantize_hd +
vgpt_attn_fwd_plan_fp8_hd), and head dim 96 through the same entries against the head_dim 96 ones.

  * the quantiser byte for byte against the numpy model of tests/test_attn_fp8_gpu.py (quantise_blocks) in the record layout
    include/vgpt.h documents per head dim, pad scale bytes included;
  * an exact probe of the key maps: with Q = 0 every visible probability is 2^8 in e4m3 and the row sum is exact in fp32, so
    with a one-hot V (key i -> column (i + 5 kv head) % D) every output element is bf16(c / n) -- c visible keys mapped to the
    column, n visible keys of the row.  (bf16(c / n) does not depend on how c / n is formed in fp32: a bf16 rounding tie
    needs a dyadic c / n with a 9-bit numerator, which n <= 330 cannot give, and every other c / n is at least 2^-18
    relative away from a tie.)  This pins the V record's key order, the d tile -> column map, the GQA head map, the tail tile;
  * random values per 32-column d tile against fp64 attention on the dequantised operands (rel-L2 < 3e-2) and on the
    unquantised inputs (rel-L2 < 8e-2): the bounds of tests/test_attn_fp8_gpu.py, which follow from e4m3 rounding and do not
    depend on D.  d block j of q is scaled by 2^j, of k by 2^-j, of v by 2^j: the ideal result per d tile is unchanged up to
    the tile's factor, a scale byte paired with the wrong block is a gross error;
  * bit-for-bit relations: D = 96 through the _hd entries equals the head_dim 96 entries (workspace and output), B = 2
    equals two B = 1 launches, a launch beside a busy stream equals a launch alone.
"""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import test_attn_fp8_gpu as T96

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
g, rel_l2, quantise_blocks, ref_attention, random_block_mask = T96.g, T96.rel_l2, T96.quantise_blocks, T96.ref_attention, T96.random_block_mask
HEAD_DIMS = [64, 128]


def a256(n):
    return (n + 255) // 256 * 256


def rec_layout(D):
    nb = D // 32
    ks, v8 = 64 * D, 64 * D + 256
    vs = v8 + nb * 2048
    return ks, v8, vs, (vs + nb * 64 + 1023) // 1024 * 1024


def split_qkv(qkv, nh, nkv, D):
    B, L, _ = qkv.shape
    q = qkv[..., : nh * D].view(B, L, nh, D).transpose(1, 2)
    k = qkv[..., nh * D:(nh + nkv) * D].view(B, L, nkv, D).transpose(1, 2)
    v = qkv[..., (nh + nkv) * D:].view(B, L, nkv, D).transpose(1, 2)
    return q, k, v


def fuse_qkv(q, k, v):
    """(B, heads, L, D) x 3 -> the fused (B, L, (nh + 2 nkv) D) buffer."""
    B, _, L, _ = q.shape
    return torch.cat([t.transpose(1, 2).reshape(B, L, -1) for t in (q, k, v)], dim=-1)


@pytest.fixture(scope="module")
def L_():
    return importlib.import_module("video-gpt_amd._lib")


# ---- 1. the quantiser, byte for byte -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_quantiser_layout_and_rounding(ops, L_, D):
    NB = D // 32
    KS_OFF, V8_OFF, VS_OFF, REC = rec_layout(D)
    B, L, nh, nkv = 1, 150, 2, 1
    scale = 1 / math.sqrt(D)
    width = (nh + 2 * nkv) * D
    qkv = (torch.randn(B, L, width, generator=g(5)) * torch.logspace(-2, 1.5, width)).to(BF)
    nkt = (L + 63) // 64
    nbytes = int(L_.load().vgpt_attn_fp8_workspace_bytes_hd(B, L, nh, nkv, D))
    assert nbytes == a256(B * nh * L * D) + a256(B * nh * L * 4) + B * nkv * nkt * REC
    ws = ops.attention_fp8_workspace_hd(B, L, nh, nkv, D, DEV).zero_()
    assert ws.numel() == nbytes
    ops.attention_fp8_quantize_hd(qkv.to(DEV), ws, nh, nkv, D, scale)
    raw = ws.cpu().numpy()
    tab = T96.e4m3_table()
    q, k, v = [t.float().numpy().astype(np.float64) for t in split_qkv(qkv, nh, nkv, D)]
    # Q (pre-multiplied by scale * log2 e in fp32, as the kernel does)
    qmul = np.float32(np.float32(scale) * np.float32(1.4426950408889634))
    qx = (q.astype(np.float32) * qmul).astype(np.float64).reshape(B, nh, L, NB, 32)
    want, sc = quantise_blocks(qx)
    q8 = raw[: B * nh * L * D].reshape(B, nh, L, NB, 32)
    qs = raw[a256(B * nh * L * D): a256(B * nh * L * D) + B * nh * L * 4].reshape(B, nh, L, 4)
    assert np.array_equal(qs[..., :NB], sc)
    assert (qs[..., NB:] == 127).all()                                # the scale bytes no d block owns
    assert np.array_equal(tab[q8] * 2.0 ** (qs[..., :NB, None].astype(np.float64) - 127), want)
    # K / V records
    recs = raw[a256(B * nh * L * D) + a256(B * nh * L * 4):].reshape(B, nkv, nkt, REC)
    kp = np.zeros((B, nkv, nkt * 64, D)); kp[:, :, :L] = k
    vp = np.zeros((B, nkv, nkt * 64, D)); vp[:, :, :L] = v
    for kt in range(nkt):
        rec = recs[0, 0, kt]
        want, sc = quantise_blocks(kp[0, 0, kt * 64:(kt + 1) * 64].reshape(64, NB, 32))
        ks = rec[KS_OFF: KS_OFF + 256].reshape(64, 4)
        assert np.array_equal(ks[:, :NB], sc)
        assert (ks[:, NB:] == 127).all()
        k8 = rec[: 64 * D].reshape(64, NB, 32)
        assert np.array_equal(tab[k8] * 2.0 ** (ks[:, :NB, None].astype(np.float64) - 127), want)
        vt = vp[0, 0, kt * 64:(kt + 1) * 64]                         # (64 keys, D)
        blocks = vt.reshape(2, 32, NB, 32).transpose(2, 0, 3, 1)      # (dt, key half, d, 32 keys)
        want, sc = quantise_blocks(blocks)
        vs = rec[VS_OFF: VS_OFF + NB * 64].reshape(NB, 2, 32)
        assert np.array_equal(vs, sc)
        v8 = rec[V8_OFF: V8_OFF + NB * 2048].reshape(NB, 2, 32, 32)   # (dt, lane half h, d, byte)
        got = np.zeros((NB, 2, 32, 32))                               # back to (dt, key half, d, key in half)
        for kb in range(2):
            for kk in range(32):
                h, j = (kk >> 2) & 1, kb * 16 + (kk & 3) + 4 * (kk >> 3)
                got[:, kb, :, kk] = tab[v8[:, h, :, j]] * 2.0 ** (vs[:, kb, :].astype(np.float64) - 127)
        assert np.array_equal(got, want)
        assert not rec[VS_OFF + NB * 64:].any()                       # the pad to whole KiB is never written


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_quantiser_row_begin_keeps_earlier_rows(ops, D):
    B, L, nh, nkv = 1, 150, 2, 1
    width = (nh + 2 * nkv) * D
    qkv = torch.randn(B, L, width, generator=g(31)).to(BF).to(DEV)
    full = ops.attention_fp8_workspace_hd(B, L, nh, nkv, D, DEV).zero_()
    ops.attention_fp8_quantize_hd(qkv, full, nh, nkv, D)
    part = full.clone()
    qkv2 = qkv.clone()
    qkv2[:, 128:] = torch.randn(B, L - 128, width, generator=g(32)).to(BF).to(DEV)   # rows >= 128 change
    ops.attention_fp8_quantize_hd(qkv2, part, nh, nkv, D, row_begin=128)
    want = ops.attention_fp8_workspace_hd(B, L, nh, nkv, D, DEV).zero_()
    ops.attention_fp8_quantize_hd(qkv2, want, nh, nkv, D)
    assert torch.equal(part, want) and not torch.equal(part, full)
    with pytest.raises(Exception, match="multiple of 64"):
        ops.attention_fp8_quantize_hd(qkv, full, nh, nkv, D, row_begin=100)


# ---- the forward through the C ABI on a guarded, padded output -------------------------------------------------------
GUARD, SENTINEL = 64, 7.0


def run_padded(ops, L_, qkv, pm, nh, nkv, D, q_start=0, segs=None, pad=4):
    """vgpt_attn_fp8_quantize_hd + vgpt_attn_fwd_plan_fp8_hd with `out` rows of nh D + pad elements between NaN guards.
    Returns (out view (B, L - q_start, nh D), the whole buffer, a bool map of the bytes `out` owns)."""
    B, L, _ = qkv.shape
    hq, rows = nh * D, L - q_start
    ld = hq + pad
    assert ld % 4 == 0 and GUARD % 4 == 0
    buf = torch.full((2 * GUARD + B * rows * ld,), float("nan"), dtype=BF, device=DEV)
    out = buf[GUARD: GUARD + B * rows * ld].view(B, rows, ld)[:, :, :hq]
    out.fill_(SENTINEL)
    own = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    own[GUARD: GUARD + B * rows * ld].view(B, rows, ld)[:, :, :hq] = True
    ws = ops.attention_fp8_workspace_hd(B, L, nh, nkv, D, DEV)
    ops.attention_fp8_quantize_hd(qkv, ws, nh, nkv, D)
    plan = pm.plan(segs if segs is not None else tuple((b, q_start, L) for b in range(B)))
    L_.call("vgpt_attn_fwd_plan_fp8_hd", ws.data_ptr(), out.data_ptr() - q_start * ld * 2, pm.bits.data_ptr(), plan.items.data_ptr(),
            plan.summary.data_ptr(), plan.order.data_ptr(), plan.n_items, B, L, nh, nkv, D, rows * ld, D, ld, ops._stream())
    torch.cuda.synchronize()
    return out, buf, own


def check_guards(out, buf, own, B, L, q_start, segs):
    assert bool(torch.isnan(buf[~own]).all()), "a byte outside `out` was written"
    seen = torch.zeros(B, L - q_start, dtype=torch.bool)
    for b, r0, r1 in (segs if segs is not None else [(b, q_start, L) for b in range(B)]):
        seen[b, r0 - q_start:r1 - q_start] = True
    o = out.float().cpu()
    assert bool((o[~seen] == SENTINEL).all()), "a row outside the segments was written"
    assert bool(torch.isfinite(o[seen]).all())
    return seen


# ---- 2. the exact key-map probe ---------------------------------------------------------------------------------------
PROBE = [(1, 1, 2, 1, 0, None), (1, 64, 2, 1, 0, None), (1, 150, 2, 1, 0, None), (2, 330, 4, 2, 0, None),
         (1, 330, 4, 2, 128, ((0, 128, 200), (0, 264, 330)))]


@pytest.mark.parametrize("B,L,nh,nkv,q_start,segs", PROBE, ids=[f"B{c[0]}-L{c[1]}-h{c[2]}x{c[3]}-q{c[4]}" for c in PROBE])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_exact_key_map_probe(ops, L_, D, B, L, nh, nkv, q_start, segs):
    m = random_block_mask(B, L, 3 + L) if L > 1 else np.ones((B, 1, 1), dtype=np.uint8)
    pm = ops.pack_mask(torch.from_numpy(m).to(DEV))
    q = torch.zeros(B, nh, L, D)
    k = torch.randn(B, nkv, L, D, generator=g(7))
    v = torch.zeros(B, nkv, L, D)
    for kvh in range(nkv):
        v[:, kvh, torch.arange(L), (torch.arange(L) + 5 * kvh) % D] = 1.0
    out, buf, own = run_padded(ops, L_, fuse_qkv(q, k, v).to(DEV, BF), pm, nh, nkv, D, q_start, segs)
    seen = check_guards(out, buf, own, B, L, q_start, segs)
    mask = torch.from_numpy(m).double()
    n = mask.sum(-1, keepdim=True)                                           # (B, L, 1) visible keys of a row
    assert bool((n >= 1).all())
    c = torch.einsum("blj,bhjd->bhld", mask, v.double())                     # (B, nkv, L, D) visible keys per column
    want = (c / n[:, None]).float().to(BF).repeat_interleave(nh // nkv, 1)   # head -> kv head head // group
    want = want.transpose(1, 2).reshape(B, L, nh * D)[:, q_start:]
    got = out.cpu()
    assert torch.equal(got[seen], want[seen]), f"{int((got[seen] != want[seen]).sum())} elements differ"


# ---- 3. random values ---------------------------------------------------------------------------------------------------
def scaled_inputs(B, L, nh, nkv, D, seed):
    """Unit-normal bf16 q / k / v with d block j of q times 2^j, of k times 2^-j, of v times 2^j (exact in bf16)."""
    f = (2.0 ** torch.arange(D // 32).float()).repeat_interleave(32)
    q = (torch.randn(B, nh, L, D, generator=g(seed)).to(BF).float() * f)
    k = (torch.randn(B, nkv, L, D, generator=g(seed + 1)).to(BF).float() / f)
    v = (torch.randn(B, nkv, L, D, generator=g(seed + 2)).to(BF).float() * f)
    return q, k, v


def references(q, k, v, m, D):
    """fp64 attention on the unquantised inputs and on the dequantised operands (Q and K in blocks of 32 along d, V in blocks
    of 32 keys), both (B, L, nh D)."""
    B, nh, L, _ = q.shape
    nkv, NB, rep = k.shape[1], D // 32, nh // k.shape[1]
    scale = 1 / math.sqrt(D)
    mask = torch.from_numpy(m)
    exact = ref_attention(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1), mask, scale)
    qmul = np.float32(np.float32(scale) * np.float32(1.4426950408889634))
    qd = torch.from_numpy(quantise_blocks((q.numpy().astype(np.float32) * qmul).astype(np.float64).reshape(B, nh, L, NB, 32))[0])
    qd = qd.reshape(B, nh, L, D) / float(qmul)
    kd = torch.from_numpy(quantise_blocks(k.numpy().astype(np.float64).reshape(B, nkv, L, NB, 32))[0]).reshape(B, nkv, L, D)
    Lp = (L + 31) // 32 * 32
    vpad = np.zeros((B, nkv, Lp, D)); vpad[:, :, :L] = v.numpy()
    vd = quantise_blocks(vpad.reshape(B, nkv, Lp // 32, 32, D).transpose(0, 1, 2, 4, 3))[0].transpose(0, 1, 2, 4, 3)
    vd = torch.from_numpy(vd.reshape(B, nkv, Lp, D)[:, :, :L])
    deq = ref_attention(qd, kd.repeat_interleave(rep, 1), vd.repeat_interleave(rep, 1), mask, scale)
    to_rows = lambda t: t.transpose(1, 2).reshape(B, L, nh * D)   # noqa: E731
    return to_rows(exact), to_rows(deq)


RANDOM = [(1, 150, 2, 1, 0, None), (2, 330, 4, 2, 0, None), (1, 330, 4, 2, 128, ((0, 128, 200), (0, 264, 330)))]


@pytest.mark.parametrize("B,L,nh,nkv,q_start,segs", RANDOM, ids=[f"B{c[0]}-L{c[1]}-h{c[2]}x{c[3]}-q{c[4]}" for c in RANDOM])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_attention_against_references_per_d_tile(ops, L_, D, B, L, nh, nkv, q_start, segs):
    m = random_block_mask(B, L, 3)
    m[:, : L // 3, L // 2:] = 0
    pm = ops.pack_mask(torch.from_numpy(m).to(DEV))
    q, k, v = scaled_inputs(B, L, nh, nkv, D, 13)
    out, buf, own = run_padded(ops, L_, fuse_qkv(q, k, v).to(DEV, BF), pm, nh, nkv, D, q_start, segs)
    seen = check_guards(out, buf, own, B, L, q_start, segs)
    exact, deq = references(q, k, v, m, D)
    got = out.double().cpu()
    tile = lambda t, dt: t.reshape(*t.shape[:2], nh, D)[..., dt * 32:(dt + 1) * 32][seen]   # noqa: E731
    worst_deq = worst_exact = 0.0
    for dt in range(D // 32):
        e_deq = rel_l2(tile(got, dt), tile(deq[:, q_start:], dt))
        e_exact = rel_l2(tile(got, dt), tile(exact[:, q_start:], dt))
        print(f"fp8 attention D={D} L={L} d tile {dt}: rel-L2 vs dequantised-operand reference {e_deq:.3e}, vs exact {e_exact:.3e}")
        worst_deq, worst_exact = max(worst_deq, e_deq), max(worst_exact, e_exact)
    assert worst_deq < 3e-2
    assert worst_exact < 8e-2


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_late_spike_and_masked_first_tile(ops, D):
    """Running-maximum moves in the middle of the tile loop; first tile mixed for every row and wholly masked for some."""
    B, L, nh = 1, 330, 2
    q = torch.randn(B, nh, L, D, generator=g(44)).to(BF).float()
    k = torch.randn(B, nh, L, D, generator=g(45)).to(BF).float()
    v = torch.randn(B, nh, L, D, generator=g(46)).to(BF).float()
    k[:, :, 100] = (q[:, :, 150] * 8.0).to(BF).float()
    k[:, :, 300] = (q[:, :, 260] * 3.0).to(BF).float()
    m = np.ones((B, L, L), dtype=np.uint8)
    m[:, :, :17] = 0
    m[:, 200:, 17:64] = 0
    pm = ops.pack_mask(torch.from_numpy(m).to(DEV))
    out = ops.attention_qkv_fp8_hd(fuse_qkv(q, k, v).to(DEV, BF), pm, nh, nh, D)
    ref = ref_attention(q, k, v, torch.from_numpy(m), 1 / math.sqrt(D)).transpose(1, 2).reshape(B, L, -1)
    assert torch.isfinite(out).all()
    e = rel_l2(out, ref)
    print(f"fp8 attention D={D} late spike: rel-L2 vs exact {e:.3e}")
    assert e < 8e-2


# ---- 4. / 5. bit-for-bit relations -----------------------------------------------------------------------------------
def test_head_dim_96_through_hd_equals_the_96_entries(ops):
    D, B, L, nh, nkv = 96, 2, 330, 4, 2
    m = random_block_mask(B, L, 3)
    pm = ops.pack_mask(torch.from_numpy(m).to(DEV))
    qkv = torch.randn(B, L, (nh + 2 * nkv) * D, generator=g(13)).to(BF).to(DEV)
    old_ws = ops.attention_fp8_workspace(B, L, nh, nkv, D, DEV).zero_()
    new_ws = ops.attention_fp8_workspace_hd(B, L, nh, nkv, D, DEV).zero_()
    assert old_ws.numel() == new_ws.numel()
    ops.attention_fp8_quantize(qkv, old_ws, nh, nkv, D)
    ops.attention_fp8_quantize_hd(qkv, new_ws, nh, nkv, D)
    assert torch.equal(old_ws, new_ws)
    old = ops.attention_qkv_fp8(qkv, pm, nh, nkv, D, workspace=old_ws.clone())
    new = ops.attention_qkv_fp8_hd(qkv, pm, nh, nkv, D, workspace=new_ws.clone())
    assert torch.isfinite(old).all() and torch.equal(old, new)


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_batch_and_busy_stream_are_bit_for_bit(ops, L_, D):
    B, L, nh, nkv = 2, 330, 4, 2
    m = random_block_mask(B, L, 9)
    qkv = torch.randn(B, L, (nh + 2 * nkv) * D, generator=g(17)).to(BF).to(DEV)
    pm = ops.pack_mask(torch.from_numpy(m).to(DEV))
    both = ops.attention_qkv_fp8_hd(qkv, pm, nh, nkv, D).clone()
    for b in range(B):
        pm1 = ops.pack_mask(torch.from_numpy(m[b:b + 1]).to(DEV))
        one = ops.attention_qkv_fp8_hd(qkv[b:b + 1].contiguous(), pm1, nh, nkv, D)
        assert torch.equal(one[0], both[b]), f"batch item {b} of a B = 2 launch differs from its own launch"
    n = 256 << 20
    src = torch.zeros(n, dtype=torch.uint8, device=DEV)
    dst = torch.empty(n, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    L_.call("vgpt_calib_copy", src.data_ptr(), dst.data_ptr(), n, side.cuda_stream)
    beside = ops.attention_qkv_fp8_hd(qkv, pm, nh, nkv, D).clone()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(beside, both), "a launch beside a busy stream differs"
