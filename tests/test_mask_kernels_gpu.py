"""csrc/mask.hip on the device, one entry point at a time: vgpt_mask_pack_bool, vgpt_mask_pack_additive,
vgpt_mask_tile_summary, vgpt_mask_count_empty_rows and vgpt_attn_qblock_order.  Every result is an integer and is compared
with torch.equal against a restatement written with numpy from the DENSE mask and the definitions of include/vgpt.h and
mask.hip's header (it never looks at packed words the device produced):

  bits[b][q][w], w < W = ceil(L / 32): bit j = visible(b, q, 32 w + j), bits of keys >= L are 0
  summary[b][qb][kt]: 2 bits per 32-row sub-block s of the 128-row q block qb against the 64-key tile kt:
      0 = no live row (q < L) of the sub-block sees a key of the tile, 1 = every live row sees all 64 keys and the tile lies
      inside L, 2 = anything else (so a wholly visible TAIL tile is 2: the attention kernel must still mask keys >= L)
  order[b]: the q blocks from q_start / 128 on, most non-empty key tiles first, stable

Operands sit in tests/kernel_guards.py Guarded allocations (0xDEADBEEF around int32 words, 0xA5 around bytes, NaN around
additive masks); the bands are checked after every launch."""
import importlib

import numpy as np
import pytest
import torch

from tests.kernel_guards import BF, Guarded, all_intact

pytestmark = pytest.mark.gpu

LENGTHS = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128]


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("video-gpt_amd.ops")


def _call(name, *args):
    importlib.import_module("video-gpt_amd._lib").call(name, *args, torch.cuda.current_stream().cuda_stream)


def _sync(*bufs):
    torch.cuda.synchronize()
    assert all_intact(*bufs)


def _rng(seed):
    return np.random.default_rng(seed)


# ---- the dense restatement -----------------------------------------------------------------------------------------------

def dense_pack(vis):
    """(B, L, L) bool -> (B, L, W) words as int32 (the bit pattern of the uint32 words)."""
    B, L, _ = vis.shape
    W = (L + 31) // 32
    padded = np.zeros((B, L, W * 32), dtype=np.uint64)
    padded[:, :, :L] = vis
    words = (padded.reshape(B, L, W, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def dense_summary(vis):
    B, L, _ = vis.shape
    nqb, nkt = (L + 127) // 128, (L + 63) // 64
    out = np.zeros((B, nqb, nkt), dtype=np.uint8)
    for b in range(B):
        for qb in range(nqb):
            for kt in range(nkt):
                for s in range(4):
                    q0 = qb * 128 + s * 32
                    blk = vis[b, q0:min(q0 + 32, L), kt * 64:min(kt * 64 + 64, L)]
                    if blk.shape[0] == 0 or not blk.any():
                        code = 0
                    elif blk.all() and kt * 64 + 64 <= L:
                        code = 1
                    else:
                        code = 2
                    out[b, qb, kt] |= code << (2 * s)
    return out


def random_visibility(B, L, seed):
    return _rng(seed).random((B, L, L)) < 0.5


# ---- pack ----------------------------------------------------------------------------------------------------------------

def _pack(kind, vis, seed=0):
    """Pack a dense visibility through one of the three input formats; returns the (B, L, W) int32 words."""
    B, L, _ = vis.shape
    W = (L + 31) // 32
    r = _rng(seed + L)
    if kind == "bool":
        m = np.where(vis, r.choice(np.array([1, 2, 255], dtype=np.uint8), size=vis.shape), 0).astype(np.uint8)
        mg = Guarded.of(torch.from_numpy(m).reshape(B * L, L))
    else:
        dtype = torch.float32 if kind == "f32" else BF
        lo = torch.finfo(dtype).min
        seen = torch.tensor([0.0, -0.0], dtype=dtype)[torch.from_numpy(r.integers(0, 2, vis.shape))]
        hidden = torch.tensor([lo, float("-inf")], dtype=dtype)[torch.from_numpy(r.integers(0, 2, vis.shape))]
        mg = Guarded.of(torch.where(torch.from_numpy(vis), seen, hidden).reshape(B * L, L))
    bg = Guarded(B * L, W, torch.int32)
    if kind == "bool":
        _call("vgpt_mask_pack_bool", mg.t.data_ptr(), bg.t.data_ptr(), B, L)
    else:
        _call("vgpt_mask_pack_additive", mg.t.data_ptr(), int(kind == "f32"), bg.t.data_ptr(), B, L)
    _sync(mg, bg)
    return bg.t.cpu().view(B, L, W)


@pytest.mark.parametrize("kind", ["bool", "bf16", "f32"])
@pytest.mark.parametrize("L", LENGTHS)
def test_mask_pack(ops, L, kind):
    """Bool bytes 1, 2 and 255 are all visible; additive 0 and -0.0 are visible, finfo.min and -inf are masked."""
    vis = random_visibility(2, L, 5)
    vis[1, :, -1] = True                      # the last key of every row of the second item: the top bit of the last word
    vis[1, L // 2] = False                    # and one empty row
    assert torch.equal(_pack(kind, vis), torch.from_numpy(dense_pack(vis)))


def test_mask_pack_second_trip_of_the_wave_loop(ops):
    """L = 1100: 1100 rows x 18 chunks = 19800 wave-iterations, more than the 16384 one grid pass covers."""
    vis = random_visibility(1, 1100, 7)
    assert torch.equal(_pack("bool", vis), torch.from_numpy(dense_pack(vis)))


# ---- tile summary --------------------------------------------------------------------------------------------------------

def _summary(words, B, L):
    W = (L + 31) // 32
    nqb, nkt = (L + 127) // 128, (L + 63) // 64
    bg, sg = Guarded.of(words.reshape(B * L, W)), Guarded(B * nqb, nkt, torch.uint8)
    _call("vgpt_mask_tile_summary", bg.t.data_ptr(), sg.t.data_ptr(), B, L)
    _sync(bg, sg)
    assert torch.equal(bg.t.cpu().view(B, L, W), words)
    return sg.t.cpu().view(B, nqb, nkt)


def constructed_visibility(L):
    """Item 0: random, then every (q block, key tile, sub-block) in turn is made all zero, all visible, left mixed, left
    mixed.  Item 1: everything visible.  Item 2: nothing.  Returns the mask and the kind chosen per sub-block."""
    vis = np.zeros((3, L, L), dtype=bool)
    vis[0] = random_visibility(1, L, 11)[0]
    vis[1] = True
    kinds, n = {}, 0
    for qb in range((L + 127) // 128):
        for kt in range((L + 63) // 64):
            for s in range(4):
                q0 = qb * 128 + s * 32
                if q0 >= L:
                    continue
                kind = ("zero", "full", "mixed", "mixed")[n % 4]
                n += 1
                blk = vis[0, q0:q0 + 32, kt * 64:kt * 64 + 64]
                if kind == "zero":
                    blk[:] = False
                elif kind == "full":
                    blk[:] = True
                elif blk.size > 1:
                    blk.flat[0], blk.flat[-1] = True, False
                else:
                    kind = "full" if blk.all() else "zero"
                kinds[(qb, kt, s)] = kind
    return vis, kinds


@pytest.mark.parametrize("L", LENGTHS + [129, 257])
def test_mask_tile_summary(ops, L):
    vis, kinds = constructed_visibility(L)
    got = _summary(torch.from_numpy(dense_pack(vis)), 3, L)
    assert torch.equal(got, torch.from_numpy(dense_summary(vis)))
    # and the named sub-blocks by hand, without the restatement
    g = got.numpy()
    code = lambda b, qb, kt, s: (int(g[b, qb, kt]) >> (2 * s)) & 3   # noqa: E731
    for (qb, kt, s), kind in kinds.items():
        inside = kt * 64 + 64 <= L
        assert code(0, qb, kt, s) == {"zero": 0, "full": 1 if inside else 2, "mixed": 2}[kind], (qb, kt, s, kind)
        assert code(1, qb, kt, s) == (1 if inside else 2) and code(2, qb, kt, s) == 0
    for qb in range(g.shape[1]):                                      # sub-blocks without a live row: 0 whatever the mask
        for s in range(4):
            if qb * 128 + s * 32 >= L:
                assert all(code(b, qb, kt, s) == 0 for b in range(3) for kt in range(g.shape[2])), (qb, s)


@pytest.mark.parametrize("L", [33, 65, 96, 127])
def test_mask_tile_summary_tail_tile_with_bits_set_past_the_row(ops, L):
    """Words whose bits past L are set (no packer of this library writes them): the tail tile still is 2, never 1; the
    attention kernel reads a 1 as "skip the mask words", which would let it attend to keys past the row."""
    W = (L + 31) // 32
    words = torch.full((1, L, W), -1, dtype=torch.int32)
    g = _summary(words, 1, L).numpy()
    nkt = (L + 63) // 64
    for s in range(4):
        if s * 32 < L:
            assert (int(g[0, 0, nkt - 1]) >> (2 * s)) & 3 == 2, s
            assert all((int(g[0, 0, kt]) >> (2 * s)) & 3 == 1 for kt in range(nkt - 1)), s


# ---- empty rows ----------------------------------------------------------------------------------------------------------

def test_mask_count_empty_rows(ops):
    """513 rows (one past two 256-thread blocks): rows 0, 255, 256 and 512 see nothing; row 1 sees the first key only, row
    2 the last key only; the counter starts from garbage."""
    L = 513
    vis = random_visibility(1, L, 13)
    vis[0, np.arange(L), np.arange(L)] = True
    vis[0, [0, 255, 256, 512]] = False
    vis[0, 1] = False
    vis[0, 1, 0] = True
    vis[0, 2] = False
    vis[0, 2, L - 1] = True
    bg = Guarded.of(torch.from_numpy(dense_pack(vis)).reshape(L, -1))
    cg = Guarded.of(torch.tensor([123456789], dtype=torch.int32))
    _call("vgpt_mask_count_empty_rows", bg.t.data_ptr(), cg.t.data_ptr(), 1, L)
    _sync(bg, cg)
    assert int(cg.t.item()) == 4
    assert int((~vis[0].any(-1)).sum()) == 4


# ---- q block order -------------------------------------------------------------------------------------------------------

def hand_made_summary(B, nqb, nkt, seed):
    """Rows with costs in 0..11 (ties and zero-cost rows everywhere): `cost` bytes of the row are non-zero codes, the rest 0."""
    r = _rng(seed)
    rows = B * nqb
    cost = r.integers(0, 12, rows)
    cost[r.integers(0, rows, max(rows // 8, 1))] = 0
    cost = np.minimum(cost, nkt)
    idx = (r.integers(0, nkt, rows)[:, None] + np.arange(12)[None]) % nkt     # a run of `cost` tiles from a random start
    summ = np.zeros((rows, nkt), dtype=np.uint8)
    live = np.arange(12)[None] < cost[:, None]
    rr = np.broadcast_to(np.arange(rows)[:, None], idx.shape)
    summ[rr[live], idx[live]] = r.integers(1, 256, int(live.sum()))
    assert np.array_equal((summ != 0).sum(-1), cost)
    return summ, cost.reshape(B, nqb)


def _order(summ, B, L, q_start):
    nqb, nkt = (L + 127) // 128, (L + 63) // 64
    n = nqb - q_start // 128
    sg, og = Guarded.of(torch.from_numpy(summ).reshape(B * nqb, nkt)), Guarded(B, n, torch.int32)
    _call("vgpt_attn_qblock_order", sg.t.data_ptr(), B, L, q_start, og.t.data_ptr())
    _sync(sg, og)
    return og.t.cpu().numpy()


@pytest.mark.parametrize("q_start", [0, 256])
@pytest.mark.parametrize("L", [1280, 1300, 385])
def test_qblock_order_is_the_stable_sort_by_cost(ops, L, q_start):
    B, nqb, nkt = 2, (L + 127) // 128, (L + 63) // 64
    summ, cost = hand_made_summary(B, nqb, nkt, L)
    qb0 = q_start // 128
    want = np.stack([np.argsort(-cost[b, qb0:], kind="stable") + qb0 for b in range(B)]).astype(np.int32)
    assert np.array_equal(_order(summ, B, L, q_start), want)


def test_qblock_order_sorts_2048_blocks_and_keeps_2049_in_natural_order(ops):
    """2049 q blocks: all of them (q_start = 0) are more than the kernel ranks in shared memory and keep their natural
    order; from q_start = 128 on there are 2048, which are sorted."""
    B, nqb = 2, 2049
    L = nqb * 128
    summ, cost = hand_made_summary(B, nqb, L // 64, 3)
    assert np.array_equal(_order(summ, B, L, 0), np.broadcast_to(np.arange(nqb, dtype=np.int32), (B, nqb)))
    want = np.stack([np.argsort(-cost[b, 1:], kind="stable") + 1 for b in range(B)]).astype(np.int32)
    assert np.array_equal(_order(summ, B, L, 128), want)
