"""The head-grouped slot map of the four-wave qkv + RoPE kernel's 256 x 288 tile, without a GPU: vgpt_gemm_rope_grouped_col
(include/vgpt.h) answers from the function the kernel itself uses (csrc/gemm_bf16.hip, rope_grouped_col), so the properties
the kernel's loop and epilogue rely on are pinned here:
  * a tile's 288 slots are 288 distinct columns and all tiles together cover 0 .. N - 1 exactly once,
  * every aligned group of 8 slots is 8 consecutive columns (= rows of W: the loop stages W in 8-row pieces at one scalar
    offset each),
  * in a rotated sub-tile slot w and slot w ^ 8 are d and d + 48 of one head (the partner sits in lane ^ 32),
  * sub-tiles i and i + 3 of a wave column have equal d (one cos / sin quad serves both),
  * tile t holds only head t of q, k and v,
and -1 is the answer wherever the map does not apply."""
import importlib

import pytest

HD, TILE, WCOL = 96, 288, 144
SHAPES = [(9216, 6144), (4608, 3072)]       # (N, rope_cols): the sampler's qkv_proj, and half of it


@pytest.fixture(scope="module")
def col():
    fn = importlib.import_module("video-gpt_amd._lib").load().vgpt_gemm_rope_grouped_col
    return lambda N, rope_cols, hd, tile, slot: int(fn(N, rope_cols, hd, tile, slot))


def _tile(col, N, rc, t):
    return [col(N, rc, HD, t, s) for s in range(TILE)]


@pytest.mark.parametrize("N,rc", SHAPES)
def test_tiles_partition_the_columns(col, N, rc):
    seen = []
    for t in range(N // TILE):
        cols = _tile(col, N, rc, t)
        assert len(set(cols)) == TILE and min(cols) >= 0
        seen += cols
    assert sorted(seen) == list(range(N))


@pytest.mark.parametrize("N,rc", SHAPES)
def test_every_staging_piece_is_eight_consecutive_columns(col, N, rc):
    for t in range(N // TILE):
        cols = _tile(col, N, rc, t)
        for s in range(0, TILE, 8):
            assert cols[s:s + 8] == list(range(cols[s], cols[s] + 8)), (t, s)


@pytest.mark.parametrize("N,rc", SHAPES)
def test_rotation_partners_table_columns_and_heads(col, N, rc):
    n_heads = rc // (2 * HD)                      # q heads = k heads = v heads
    assert n_heads == N // TILE
    for t in range(n_heads):
        cols = _tile(col, N, rc, t)
        for wn in range(2):
            sub = [cols[wn * WCOL + i * 16: wn * WCOL + (i + 1) * 16] for i in range(9)]
            for i in range(6):                    # q (0-2) and k (3-5): rotated, pair group 3 wn + i % 3
                base = (i // 3) * (rc // 2) + t * HD
                for w in range(8):
                    d = sub[i][w] - base
                    assert d == (3 * wn + i % 3) * 8 + w, (t, wn, i, w)
                    assert sub[i][w ^ 8] == sub[i][w] + HD // 2
            for i in range(3):                    # sub-tiles i and i + 3: the same d, one head of q and one of k apart
                assert [c + rc // 2 for c in sub[i]] == sub[i + 3]
            for i in range(6, 9):                 # v: 48 plain columns of head t per wave column
                assert sub[i] == list(range(rc + t * HD + wn * 48 + (i - 6) * 16, rc + t * HD + wn * 48 + (i - 5) * 16))
        heads = {(0 if c < rc // 2 else 1 if c < rc else 2, (c % (rc // 2)) // HD) for c in cols}
        assert heads == {(0, t), (1, t), (2, t)}


@pytest.mark.parametrize("N,rc,hd", [
    (9216, 6144 + 96, 96), (9216, 6144 - 96, 96),     # one head off the 2 / 3 point
    (4608, 3072 + 96, 96), (4608, 3456, 96),
    (9216, 6144, 64), (9216, 6144, 128),             # other head dims
    (4608, 3072, 64), (4608, 3072, 128),
    (9216 + 96, 6208, 96), (4608 - 96, 3008, 96), (4096, 2688, 96),   # N no multiple of 288
])
def test_other_shapes_are_not_grouped(col, N, rc, hd):
    assert col(N, rc, hd, 0, 0) == -1


def test_out_of_range_tile_or_slot(col):
    assert col(9216, 6144, 96, 31, 287) == 9215 and col(9216, 6144, 96, 0, 0) == 0
    for tile, slot in [(32, 0), (-1, 0), (0, 288), (0, -1)]:
        assert col(9216, 6144, 96, tile, slot) == -1
