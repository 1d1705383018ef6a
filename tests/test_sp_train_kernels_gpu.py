"""The two re-layout kernels of the sharded training step's backward (include/vgpt.h, vgpt_sp_pack_ctx /
vgpt_sp_unpack_qkv_rope), the inverses of vgpt_sp_pack_qkv / vgpt_sp_unpack_ctx (tests/test_sp_engine_gpu.py).

Without tables both move bytes: compared byte for byte against torch index operations on arbitrary 16-bit patterns (NaN /
Inf patterns included), with NaN guard rows around every output.  With cos / sin tables the unpack also rotates the q and k
heads: it must equal the unfused pair -- unpack, then ops.rope_qk_inplace -- bit for bit (same bf16 inputs, same fp32
expressions, one rounding), and two exact-data probes pin the half mapping and the sign on their own."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GUARD = 3                   # NaN rows before and after every output
HEADS = [(32, 32), (2, 2), (32, 8)]
HEAD_IDS = ["32x96", "tiny-2x96", "gqa-32q8kv"]
ROWS = [1, 37, 255, 1001]
RANKS = [1, 2, 4, 8]


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("video-gpt_amd.ops")


def _bits(shape, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16)


def _guarded(rows, width):
    """(whole, out): `out` is rows [GUARD, GUARD + rows) of a NaN-filled (rows + 2 GUARD, width) buffer."""
    whole = torch.full((rows + 2 * GUARD, width), float("nan"), dtype=BF, device=DEV)
    return whole, whole[GUARD:GUARD + rows]


def _guards_untouched(whole, rows):
    g = torch.cat([whole[:GUARD], whole[GUARD + rows:]]).view(torch.int16)
    return bool((g == torch.full((1,), float("nan"), dtype=BF).view(torch.int16).item()).all())


def _ref_unpack_qkv(chunks, P, nq, nk, hd):
    """(P, rows, (nq/P + 2 nk/P) hd) -> (rows, (nq + 2 nk) hd) as [q heads | k heads | v heads], by index operations."""
    rows = chunks.shape[1]
    qw, kw = nq // P * hd, nk // P * hd
    part = lambda a, b: chunks[:, :, a:b].permute(1, 0, 2).reshape(rows, -1)
    return torch.cat([part(0, qw), part(qw, qw + kw), part(qw + kw, qw + 2 * kw)], dim=1).contiguous()


def _tables(rows, half, seed):
    ang = torch.rand(rows, half, generator=torch.Generator("cpu").manual_seed(seed)) * 6.2831853
    return ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()


def _chunks_with_values(rows, P, nq, nk, hd, seed):
    """Chunks whose q and k columns hold ordinary values and whose v columns hold arbitrary bit patterns (NaN included)."""
    Wl = (nq + 2 * nk) // P * hd
    g = torch.Generator("cpu").manual_seed(seed)
    vals = (torch.randn(P, rows, Wl, generator=g) * 3).to(BF).view(torch.int16)
    vals[:, :, (nq + nk) // P * hd:] = _bits((P, rows, nk // P * hd), seed + 1)
    return vals


# ---- bytes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("P", RANKS)
@pytest.mark.parametrize("rows", ROWS)
def test_pack_ctx_and_unpack_qkv_move_bytes(ops, P, heads, rows):
    nq, nk = heads
    hd = 96
    W = (nq + 2 * nk) * hd
    if nq % P or nk % P:
        with pytest.raises(ops.VgptError, match="multiples of n_ranks"):
            ops.sp_unpack_qkv_rope(torch.zeros(P, rows, 8, dtype=BF, device=DEV), P, nq, nk, hd)
        return
    # pack_ctx: (rows, P Dc) -> (P, rows, Dc)
    Dc = nq // P * hd
    cb = _bits((rows, P * Dc), rows * 31 + P)
    whole, out = _guarded(P * rows, Dc)
    ops.sp_pack_ctx(cb.to(DEV).view(BF), P, out=out.view(P, rows, Dc))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16).cpu().view(P, rows, Dc), cb.view(rows, P, Dc).permute(1, 0, 2))
    assert _guards_untouched(whole, P * rows)
    # ... and it is the inverse of unpack_ctx
    blocks = _bits((P, rows, Dc), rows * 37 + P).to(DEV).view(BF)
    back = ops.sp_pack_ctx(ops.sp_unpack_ctx(blocks, P), P)
    torch.cuda.synchronize()
    assert torch.equal(back.view(torch.int16), blocks.view(torch.int16))
    # unpack_qkv without tables: (P, rows, Wl) -> (rows, W)
    ch = _bits((P, rows, W // P), rows * 41 + P)
    whole, out = _guarded(rows, W)
    ops.sp_unpack_qkv_rope(ch.to(DEV).view(BF), P, nq, nk, hd, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16).cpu(), _ref_unpack_qkv(ch, P, nq, nk, hd))
    assert _guards_untouched(whole, rows)
    # ... and it is the inverse of pack_qkv (under GQA too)
    x = _bits((rows, W), rows * 43 + P).to(DEV).view(BF)
    back = ops.sp_unpack_qkv_rope(ops.sp_pack_qkv(x, P, nq, nk, hd), P, nq, nk, hd)
    torch.cuda.synchronize()
    assert torch.equal(back.view(torch.int16), x.view(torch.int16))


# ---- tables: exact-data probes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,P", [((2, 2), 2), ((32, 8), 4)], ids=["tiny-2x96-P2", "gqa-32q8kv-P4"])
def test_unpack_with_tables_exact_probes(ops, heads, P):
    nq, nk = heads
    hd, rows = 96, 37
    half, W = hd // 2, (nq + 2 * nk) * hd
    ch = _chunks_with_values(rows, P, nq, nk, hd, 5)
    plain = _ref_unpack_qkv(ch, P, nq, nk, hd)
    one, zero = torch.ones(rows, half, device=DEV), torch.zeros(rows, half, device=DEV)
    # cos = 1, sin = 0: the plain unpack
    whole, out = _guarded(rows, W)
    ops.sp_unpack_qkv_rope(ch.to(DEV).view(BF), P, nq, nk, hd, one, zero, out=out)
    torch.cuda.synchronize()
    rot = (nq + nk) * hd
    assert torch.equal(out[:, :rot].float().cpu(), plain.view(BF)[:, :rot].float())
    assert torch.equal(out[:, rot:].view(torch.int16).cpu(), plain[:, rot:])          # v: bytes, NaN patterns and all
    assert _guards_untouched(whole, rows)
    # cos = 0, sin = 1: every q / k head becomes [-x2 | x1] exactly
    whole, out = _guarded(rows, W)
    ops.sp_unpack_qkv_rope(ch.to(DEV).view(BF), P, nq, nk, hd, zero, one, out=out)
    torch.cuda.synchronize()
    x = plain.view(BF)[:, :rot].float().view(rows, nq + nk, 2, half)
    want = torch.stack([-x[:, :, 1], x[:, :, 0]], dim=2).reshape(rows, rot)
    assert torch.equal(out[:, :rot].float().cpu(), want)
    assert torch.equal(out[:, rot:].view(torch.int16).cpu(), plain[:, rot:])
    assert _guards_untouched(whole, rows)


# ---- tables: the unfused pair, bit for bit --------------------------------------------------------------------------

def _fused_equals_unfused(ops, rows, P, nq, nk, hd, negate=False):
    W = (nq + 2 * nk) * hd
    ch = _chunks_with_values(rows, P, nq, nk, hd, rows * 13 + P + hd).to(DEV).view(BF)
    cos, sin = _tables(rows, hd // 2, rows + hd)
    if negate:
        sin = (-sin).contiguous()                    # what the trainer passes: the inverse rotation
    ref = ops.rope_qk_inplace(ops.sp_unpack_qkv_rope(ch, P, nq, nk, hd), cos, sin, nq, nk, hd)
    whole, out = _guarded(rows, W)
    ops.sp_unpack_qkv_rope(ch, P, nq, nk, hd, cos, sin, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert _guards_untouched(whole, rows)
    return out


@pytest.mark.parametrize("hd", [64, 96, 128])
def test_unpack_with_tables_is_unpack_then_rope_at_every_head_dim(ops, hd):
    for nq, nk, P in ((4, 4, 2), (8, 2, 2), (2, 2, 1)):
        out = _fused_equals_unfused(ops, 133, P, nq, nk, hd, negate=True)
        # the rotation really happened: the q columns differ from the plain unpack
        plain = ops.sp_unpack_qkv_rope(_chunks_with_values(133, P, nq, nk, hd, 133 * 13 + P + hd).to(DEV).view(BF), P, nq, nk, hd)
        assert not torch.equal(out[:, :nq * hd].view(torch.int16), plain[:, :nq * hd].view(torch.int16))


@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("P", RANKS)
@pytest.mark.parametrize("rows", ROWS)
def test_unpack_with_tables_is_unpack_then_rope(ops, P, heads, rows):
    nq, nk = heads
    if nq % P or nk % P:         # refused with tables as without
        with pytest.raises(ops.VgptError, match="multiples of n_ranks"):
            ops.sp_unpack_qkv_rope(torch.zeros(P, rows, 8, dtype=BF, device=DEV), P, nq, nk, 96,
                                   torch.zeros(rows, 48, device=DEV), torch.zeros(rows, 48, device=DEV))
        return
    _fused_equals_unfused(ops, rows, P, nq, nk, 96)


def test_zero_rows_and_refusals(ops):
    z = ops.sp_pack_ctx(torch.zeros(0, 2 * 96, dtype=BF, device=DEV), 2)
    assert z.shape == (2, 0, 96)
    z = ops.sp_unpack_qkv_rope(torch.zeros(2, 0, 3 * 96, dtype=BF, device=DEV), 2, 2, 2, 96)
    assert z.shape == (0, 6 * 96)
    ch = torch.zeros(2, 8, 3 * 96, dtype=BF, device=DEV)
    cos = torch.zeros(8, 48, device=DEV)
    with pytest.raises(ops.VgptError, match="together"):
        ops.sp_unpack_qkv_rope(ch, 2, 2, 2, 96, cos=cos)
    with pytest.raises(ops.VgptError, match="tables"):
        ops.sp_unpack_qkv_rope(ch, 2, 2, 2, 96, cos[:7], cos[:7])
    with pytest.raises(ops.VgptError, match="are not"):
        ops.sp_unpack_qkv_rope(ch, 2, 2, 4, 96)
    with pytest.raises(ops.VgptError, match="dtype"):
        ops.sp_unpack_qkv_rope(ch.float(), 2, 2, 2, 96)
    with pytest.raises(ops.VgptError, match="out"):
        ops.sp_unpack_qkv_rope(ch, 2, 2, 2, 96, out=torch.empty(7, 6 * 96, dtype=BF, device=DEV))
    with pytest.raises(ops.VgptError, match="tables"):           # hd 8: copies, but cannot rotate (hd / 2 % 8 != 0)
        ops.sp_unpack_qkv_rope(torch.zeros(2, 8, 3 * 8, dtype=BF, device=DEV), 2, 2, 2, 8, torch.zeros(8, 4, device=DEV),
                               torch.zeros(8, 4, device=DEV))
    with pytest.raises(ops.VgptError, match="is not"):
        ops.sp_pack_ctx(torch.zeros(8, 2 * 96 + 1, dtype=BF, device=DEV), 2)
    with pytest.raises(ops.VgptError, match="multiple of 8"):
        ops.sp_pack_ctx(torch.zeros(8, 2 * 12, dtype=BF, device=DEV), 2)
    with pytest.raises(ops.VgptError, match="out is"):
        ops.sp_pack_ctx(torch.zeros(8, 2 * 96, dtype=BF, device=DEV), 2, out=torch.empty(8, 2 * 96, dtype=BF, device=DEV))
