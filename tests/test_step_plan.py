"""step_plan (video-gpt_amd/step_plan.py): the row plan of a sampler step, on CPU tensors.

A wrong row gives a plausible picture, not a fault, so the plan is checked twice.  By properties, against the collator's
own batch: the original-to-new row map r(b, s) is injective, carries every token's id and position with it, and carries
the mask with it -- M1[r(b, q), r(b, k)] == M0[b, q, k] inside one original row, nothing across rows, nothing to or from
a gap row; the first live row S is a multiple of 128 and nothing below it sees anything at or behind it; the frame and
time rows are r of the collator's index dicts; the attention-plan segments tile the computed rows without straddling two
sequences.  And for equality, field by field, with tests/golden/engine_step_plans.npz, recorded once by running the
constructor lines of StaticDenoiser as they stood before the plan was a function of its own, unchanged, on these inputs."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from tests.test_collator import GOLD, product_inference

LY = importlib.import_module("video-gpt_amd.layout")
SP = importlib.import_module("video-gpt_amd.step_plan")

BL = 18   # tokens of one frame block at N = 16


def _cases():
    out = {}
    for C, G, N in ((2, 3, 16), (8, 3, 16)):   # prefix of 36 rows: too short to reuse; of 144 rows: reused
        for fmt in ("bool", "layout"):
            for reuse in (False, True):
                for hoist in (False, True):
                    out[f"c{C}g{G}n{N}_{fmt}_reuse{int(reuse)}_hoist{int(hoist)}"] = (
                        (C, G, N, fmt), dict(pack_padding=True, reuse_condition_prefix=reuse, hoist_special_rows=hoist), False)
    out["c2g3n16_bool_nopack"] = ((2, 3, 16, "bool"), dict(pack_padding=False, reuse_condition_prefix=True,
                                                           hoist_special_rows=True), False)
    # the tail cut as in test_layout.test_hoist_plan_permutation_matches_dense_permutation: no hoisting, the gap path
    out["c8g3n16_layout_badtail"] = ((8, 3, 16, "layout"), dict(pack_padding=True, reuse_condition_prefix=True,
                                                                hoist_special_rows=True), True)
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _batch(C, G, N, fmt):
    return product_inference(C, G, N, 1, fmt)


@functools.lru_cache(maxsize=None)
def _planned(name):
    (C, G, N, fmt), opts, badtail = CASES[name]
    batch = dict(_batch(C, G, N, fmt))
    if badtail:
        d = batch["denoise_image_sizes"]
        batch["denoise_image_sizes"] = {0: d[0][:-1], 1: d[1]}
    plan = SP.plan_step_rows(batch["input_ids"], batch["position_ids"], batch["attention_mask"], batch["input_image_sizes"],
                             batch["denoise_image_sizes"], batch["time_emb_inx"], **opts)
    return batch, plan


def _dense(mask):
    return mask.to_bool() if isinstance(mask, LY.TokenLayout) else mask.numpy().astype(bool)


def _flat_mask(plan):
    """The plan's mask over rows flattened as b * L + s: the batch rows' masks on the diagonal."""
    m = _dense(plan.attention_mask)
    B, L = plan.B, plan.L
    assert m.shape == (B, L, L)
    out = np.zeros((B * L, B * L), dtype=bool)
    for b in range(B):
        out[b * L:(b + 1) * L, b * L:(b + 1) * L] = m[b]
    return out


def _of_dict(r, sizes, span):
    return [int(r[b, it[0] if span else it]) for b in sizes.keys() for it in sizes[b]]


@pytest.mark.parametrize("name", list(CASES))
def test_plan_properties(name):
    (C, G, N, fmt), opts, badtail = CASES[name]
    batch, plan = _planned(name)
    ids0, pos0 = batch["input_ids"].numpy(), batch["position_ids"].numpy()
    M0 = _batch(C, G, N, "bool")["attention_mask"].numpy()                          # the collator's dense mask
    pad0 = _batch(C, G, N, "layout")["attention_mask"].kind == LY.PAD               # its left pads, from the block plan
    B0, L0 = ids0.shape
    assert pad0.any() and pad0.shape == (B0, L0)

    # ---- which path the plan took ----
    reused = opts["pack_padding"] and opts["reuse_condition_prefix"] and C * BL >= 128
    hoisted = reused and opts["hoist_special_rows"] and fmt == "layout" and not badtail
    assert plan.packed == opts["pack_padding"] and plan.B == (1 if plan.packed else B0)
    assert plan.S == (256 if reused else 0) and plan.S % 128 == 0
    assert bool(plan.hoist) == hoisted
    assert plan.S0 == (C * BL if hoisted else plan.S)
    B, L, S = plan.B, plan.L, plan.S
    assert tuple(plan.input_ids.shape) == (B, L) == tuple(plan.position_ids.shape)

    # ---- the row map: injective over the tokens that are kept, -1 exactly on the dropped pads ----
    r = np.stack(plan.row_map)
    assert r.shape == (B0, L0)
    tok = r >= 0
    assert np.array_equal(~tok, pad0 if plan.packed else np.zeros_like(pad0)) and (r[~tok] == -1).all()
    rows = r[tok]
    assert rows.max() < B * L and np.unique(rows).size == rows.size
    assert all(plan.row(b, s) == r[b, s] for b in range(B0) for s in (0, L0 // 2, L0 - 1))
    # every new row is the image of exactly one token or a gap row; the gap rows are the alignment rows in front of S
    owner = np.full(B * L, -1)
    for b in range(B0):
        owner[r[b][tok[b]]] = b
    gap = np.nonzero(owner < 0)[0]
    assert gap.size + rows.size == B * L
    assert np.array_equal(gap, np.arange(S - gap.size, S))
    assert (gap.size > 0) == reused

    # ---- ids, positions and the mask move with the tokens ----
    assert np.array_equal(plan.input_ids.numpy().reshape(-1)[rows], ids0[tok])
    assert np.array_equal(plan.position_ids.numpy().reshape(-1)[rows], pos0[tok])
    M1 = _flat_mask(plan)
    for b in range(B0):
        mine = r[b][tok[b]]
        assert np.array_equal(M1[np.ix_(mine, mine)], M0[b][np.ix_(tok[b], tok[b])])
        for b2 in range(B0):
            if b2 != b:
                assert not M1[np.ix_(mine, r[b2][tok[b2]])].any()
    assert not M1[:, gap].any()        # no row sees a gap column
    assert not M1[gap].any()           # gap rows see nothing
    assert not M1[:S, S:].any()        # the reused rows see nothing a step rewrites

    # ---- the collator's index dicts ----
    assert plan.cond_rows == _of_dict(r, batch["input_image_sizes"], True)
    assert plan.x_rows == _of_dict(r, batch["denoise_image_sizes"], True)
    assert plan.t_rows == _of_dict(r, batch["time_emb_inx"], False)
    assert all(type(v) is int for v in plan.cond_rows + plan.x_rows + plan.t_rows)

    # ---- the attention-plan segments of the rows a step computes ----
    seg = plan.seg_live if S else plan.seg_all
    if not plan.packed:
        assert seg is None                                     # one segment per batch row, the kernel's default
    else:
        assert seg[0][1] == S and seg[-1][2] == L              # covers exactly [S, L) ...
        for i, (b, a, e) in enumerate(seg):
            assert b == 0 and a < e and (i == 0 or a == seg[i - 1][2])   # ... disjoint and in order
            assert np.unique(owner[a:e][owner[a:e] >= 0]).size == 1      # rows of one original sequence
        assert len(seg) == B0

    if hoisted:
        nf = len(plan.x_rows)
        assert plan.hoist["nf"] == nf == 2 * G and plan.hoist["ntok"] == N
        assert B * L - S == nf * N                             # Ma: a step computes the image rows and nothing else
        t_old = [(b, t) for b, v in batch["time_emb_inx"].items() for t in v]
        special = [int(r[b, t]) for b, t in t_old] + [int(r[b, t - 1]) for b, t in t_old]   # time and <|diffusion|> rows
        assert len(special) == 2 * nf and max(special) < S
        assert not M1[special][:, S:].any()                    # the special rows see no image column
        assert sorted(plan.x_rows + [x + j for x in plan.x_rows for j in range(1, N)]) == list(range(S, L))


@pytest.mark.parametrize("name", list(CASES))
def test_plan_equals_the_recorded_constructor(name):
    _, plan = _planned(name)
    gold = np.load(os.path.join(GOLD, "engine_step_plans.npz"))
    g = lambda k: gold[f"{name}/{k}"]
    assert np.array_equal(plan.input_ids.numpy(), g("input_ids")) and plan.input_ids.numpy().dtype == g("input_ids").dtype
    assert np.array_equal(plan.position_ids.numpy(), g("position_ids"))
    assert plan.position_ids.numpy().dtype == g("position_ids").dtype
    for k in ("B", "L", "S", "S0"):
        assert getattr(plan, k) == int(g(k)), k
    assert plan.packed == bool(g("packed"))
    for k in ("x_rows", "t_rows", "cond_rows"):
        assert getattr(plan, k) == g(k).tolist(), k
    for k in ("seg_all", "seg_live"):
        want = None if g(k).tolist() == [-1] else tuple(tuple(s) for s in g(k).reshape(-1, 3).tolist())
        assert getattr(plan, k) == want, k
    assert (list(plan.hoist["perm"]) if plan.hoist else []) == g("perm").tolist()
    dense = _dense(plan.attention_mask)
    assert list(dense.shape) == g("mask_shape").tolist()
    assert np.array_equal(np.packbits(dense.astype(np.uint8).reshape(-1)), g("mask_bits"))


def test_plan_leaves_its_inputs_alone():
    for fmt in ("bool", "layout"):
        batch = _batch(8, 3, 16, fmt)
        ids, pos = batch["input_ids"].clone(), batch["position_ids"].clone()
        before = _dense(batch["attention_mask"]).copy()
        for hoist in (False, True):
            SP.plan_step_rows(batch["input_ids"], batch["position_ids"], batch["attention_mask"], batch["input_image_sizes"],
                              batch["denoise_image_sizes"], batch["time_emb_inx"], pack_padding=True,
                              reuse_condition_prefix=True, hoist_special_rows=hoist)
        assert torch.equal(batch["input_ids"], ids) and torch.equal(batch["position_ids"], pos)
        assert np.array_equal(_dense(batch["attention_mask"]), before)


def test_packed_mask_passes_through_untouched():
    """A mask that is already bit-packed cannot be re-laid out: the sequence stays as it came, whatever the options ask."""
    ops = importlib.import_module("video-gpt_amd.ops")
    batch = _batch(8, 3, 16, "bool")
    B, L = batch["input_ids"].shape
    pm = ops.PackedMask(torch.zeros(1), torch.zeros(1), B, L)
    plan = SP.plan_step_rows(batch["input_ids"], batch["position_ids"], pm, batch["input_image_sizes"],
                             batch["denoise_image_sizes"], batch["time_emb_inx"], pack_padding=True,
                             reuse_condition_prefix=True, hoist_special_rows=True)
    assert plan.attention_mask is pm and plan.input_ids is batch["input_ids"] and plan.position_ids is batch["position_ids"]
    assert (plan.B, plan.L, plan.S, plan.S0, plan.packed, plan.hoist, plan.seg_all, plan.seg_live) == \
           (B, L, 0, 0, False, None, None, None)
    assert np.array_equal(np.stack(plan.row_map), np.arange(B * L).reshape(B, L))
    assert plan.x_rows == [b * L + it[0] for b, v in batch["denoise_image_sizes"].items() for it in v]


@pytest.mark.parametrize("T", [1, 4])
def test_clip_pass_rows(T):
    S0, nf = 36, 6
    Sc = S0 + nf
    idx, sub_tail = SP.clip_pass_rows(S0, nf, T)
    want_idx, want_sub = list(range(Sc)), []
    for s in range(T):
        for f in range(nf):
            want_idx.append(Sc + f)
            want_sub.append(s + 1)
    assert idx.tolist() == want_idx and sub_tail.tolist() == want_sub
    assert len(idx) == Sc + T * nf == Sc + len(sub_tail)


@pytest.mark.parametrize("M,P,x_rows", [(256, 2, [100, 116, 132, 148]),      # frame 1 straddles the cut at 128
                                        (260, 3, [88, 104, 184, 200])])      # frames 0 and 2 straddle 96 and 192
def test_sp_final_layer_owners(M, P, x_rows):
    h = w = 8
    nf, ntok = len(x_rows), (h // 2) * (w // 2)
    shares, _ = SP.sp_shares(M, P)
    assert x_rows[-1] + ntok <= M
    want = np.full((nf, h, w), -1)
    touched = [set() for _ in range(P)]
    for f in range(nf):
        for y in range(h):
            for x in range(w):
                row = x_rows[f] + (y // 2) * (w // 2) + x // 2
                holders = [i for i, (a, b) in enumerate(shares) if a <= row < b]
                assert len(holders) == 1                                    # every element has exactly one owner
                want[f, y, x] = holders[0]
                touched[holders[0]].add(f)
    assert any(len({int(v) for v in want[f].reshape(-1)}) == 2 for f in range(nf))   # a frame cut between two ranks
    for rank in range(P):
        (f0, f1), owner = SP.sp_final_layer_owners(x_rows, h, w, shares, rank)
        assert owner.dtype == torch.int64 and owner.device.type == "cpu" and tuple(owner.shape) == (nf, h, w)
        assert np.array_equal(owner.numpy(), want)                          # the owner's share contains the element's row
        assert set(range(f0, f1)) == touched[rank]                          # exactly the frames intersecting the share
