"""TokenLayout (video-gpt_amd/layout.py): the per-token form of the attention mask.

CPU: its dense expansion equals, bit for bit, the masks dumped from the REFERENCE'S OWN collator
(tests/golden/ref_collator_*.npz) for all three layouts, and its re-layouts (dropping left pads and concatenating the
rows; the alignment gap behind the condition prefix) equal the same operations done on the dense tensors
(step_plan.pack_left_padded / plan_step_rows).  GPU: the device expansion (vgpt_mask_build_tokens) equals the packed
rows of the dense mask, bit for bit, and the sampler gives the same latents from either form."""
import glob
import importlib
import os

import numpy as np
import pytest
import torch

from tests.test_collator import GOLD, load, product_fbtrain, product_inference, product_stage1

LY = importlib.import_module("video-gpt_amd.layout")
E = importlib.import_module("video-gpt_amd.engine")
SP = importlib.import_module("video-gpt_amd.step_plan")


def names(pat):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, pat)))


def fb_lists(d):
    flat = d["frame_blocks_flat"].tolist()
    cut = flat.index(-1)
    vals, lens = flat[:cut], flat[cut + 1:]
    out, o = [], 0
    for n in lens:
        out.append(vals[o:o + n]); o += n
    return out


def golden_layouts():
    for name in names("ref_collator_infer_*.npz"):
        d, mask = load(name)
        yield name, product_inference(int(d["C"]), int(d["G"]), int(d["N"]), int(d["sp"]), mask_format="layout")["attention_mask"], mask
    for name in names("ref_collator_stage1_*.npz"):
        d, mask = load(name)
        yield name, product_stage1(d["F"].tolist(), int(d["N"]), mask_format="layout")["attention_mask"], mask
    for name in names("ref_collator_fbtrain_*.npz"):
        d, mask = load(name)
        yield name, product_fbtrain(fb_lists(d), int(d["N"]), mask_format="layout")[2], mask


CASES = list(golden_layouts())


@pytest.mark.parametrize("name,lay,mask", CASES, ids=[c[0] for c in CASES])
def test_dense_expansion_matches_reference_masks(name, lay, mask):
    assert isinstance(lay, LY.TokenLayout) and lay.shape == mask.shape
    assert np.array_equal(lay.to_bool(), mask)
    a = lay.attr()
    assert a.dtype == np.int32 and a.shape == (lay.B, lay.L, 2)


@pytest.mark.parametrize("name,lay,mask", CASES, ids=[c[0] for c in CASES])
def test_packing_matches_dense_packing(name, lay, mask):
    m = torch.from_numpy(mask)
    pads = E.count_left_pads(m)
    assert lay.left_pads() == pads
    B, L, _ = mask.shape
    ids = torch.arange(B * L).view(B, L)
    i1, p1, m1, o1 = E.pack_left_padded(ids, ids, m, pads)
    i2, p2, l2, o2 = E.pack_left_padded(ids, ids, lay, pads)
    assert torch.equal(i1, i2) and torch.equal(p1, p2) and o1 == o2
    assert np.array_equal(l2.to_bool(), m1.numpy())


def test_prefix_gap_matches_dense_insertion():
    """cfg-2-shaped case at N=16: C=4 condition blocks, G=8 clip blocks, CFG row packed behind."""
    lay = product_inference(4, 8, 16, 1, mask_format="layout")["attention_mask"]
    pads = lay.left_pads()
    packed, _ = lay.pack(pads)
    dense = packed.to_bool()[0]
    S0 = 4 * 18
    assert packed.prefix_is_static(S0) and not bool(dense[:S0, S0:].any())
    assert not packed.prefix_is_static(S0 + 5)       # rows of the clip see the rest of the clip
    npad = 128 - S0
    g = packed.insert_gap(S0, npad)
    S, L2 = S0 + npad, packed.L + npad
    want = np.zeros((L2, L2), dtype=bool)
    want[:S0, :S0] = dense[:S0, :S0]
    want[S:, :S0] = dense[S0:, :S0]
    want[S:, S:] = dense[S0:, S0:]
    assert np.array_equal(g.to_bool()[0], want)
    assert not lay.prefix_is_static(S0, row=1)       # the CFG row's pad rows see everything


def test_from_plans_rejects_bad_plans():
    P = importlib.import_module("video-gpt_amd.processor")
    kinds, _ = P.plan_inference([1, 1])
    with pytest.raises(AssertionError):
        LY.TokenLayout.from_plans([(kinds, 6, 0)], 13)
    with pytest.raises(ValueError):
        P.LVMCollator(mask_format="dense")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,lay,mask", CASES, ids=[c[0] for c in CASES])
def test_device_expansion_is_bit_exact(ops, name, lay, mask):
    dev = "cuda:0"
    ref = ops.pack_mask(torch.from_numpy(mask).to(dev))
    pm = lay.packed_mask(dev)
    assert torch.equal(pm.bits, ref.bits) and torch.equal(pm.summary, ref.summary)
    packed, _ = lay.pack()
    ref2 = ops.pack_mask(torch.from_numpy(packed.to_bool()).to(dev))
    pm2 = packed.packed_mask(dev)
    assert torch.equal(pm2.bits, ref2.bits) and torch.equal(pm2.summary, ref2.summary)


@pytest.mark.gpu
def test_device_expansion_cfg4_shape_properties(ops):
    """512^2, F=16 stage-1 layout (L = 31 806): the dense mask would be 1 GB per row, so the
    check is by properties of the packed rows — visible-pair count against the closed form of the layout, no empty
    row, nothing visible past L — and by exact comparison on a band of rows expanded on the host."""
    P = importlib.import_module("video-gpt_amd.processor")
    F, N = 16, 1024
    bl = N + 2
    kinds, _ = P.plan_stage1(2 * F - 1)
    L = (2 * F - 1) * bl
    lay = LY.TokenLayout.from_plans([(kinds, bl, 0)], L)
    pm = lay.packed_mask("cuda:0")
    assert pm.count_empty_rows() == 0
    bits = pm.bits[0]                                                   # (L, W) int32
    W = bits.shape[1]
    if L % 32:
        assert int((bits[:, W - 1].to(torch.int64) & 0xffffffff).max()) < (1 << (L % 32))
    # closed form: a clean block is seen by itself (1 + (bl-1)*(bl-2) + 1 ... counted per key) and fully by later rows
    clean_self = bl + (bl - 1) * (bl - 2) + 1                           # <img>: bl rows, slots: bl-1 rows each, </img>: 1
    noisy_self = bl + (bl - 1) + (bl - 2) * (bl - 2)                    # <|diffusion|>, time, image slots
    total = 0
    for i, (kd, _) in enumerate(kinds):
        later = L - (i + 1) * bl
        total += (clean_self + bl * later) if kd == P.CLEAN else noisy_self
    # (`later` counts every row behind a clean block, clean or noisy: both see it)
    pop = 0
    for r0 in range(0, L, 4096):
        chunk = bits[r0:r0 + 4096].contiguous().view(torch.uint8)
        pop += int(torch.from_numpy(np.unpackbits(chunk.cpu().numpy())).sum())
    assert pop == total
    band = slice(5 * bl - 3, 5 * bl + 5)                                # rows around a block boundary
    q = np.arange(L)[:, None]
    kq, kk = lay.kind[0][band, None], lay.kind[0][None, :]
    vis = ((kk == LY.CLEAN) & (q[band] >= lay.thr[0][None, :])) | \
          ((kk == LY.NOISY) & (kq == LY.NOISY) & (lay.grp[0][band, None] == lay.grp[0][None, :]) &
           (lay.oc[0][band, None] >= lay.oc[0][None, :]))
    got = np.unpackbits(bits[band].contiguous().view(torch.uint8).cpu().numpy(), axis=-1, bitorder="little")[:, :L]
    assert np.array_equal(got.astype(bool), vis)


def test_hoist_plan_permutation_matches_dense_permutation():
    """step_plan._hoist_plan: the re-ordering [prefix | <|diffusion|> rows | time rows | gap | image rows] of
    a packed next-clip sequence is a pure permutation of tokens: the permuted layout expands to the dense mask with
    rows and columns permuted (gap rows / columns empty), and every frame's rows land where the plan says."""
    C, G, N = 2, 3, 16
    bl = N + 2
    batch = product_inference(C, G, N, 1, mask_format="layout")
    lay, offs = batch["attention_mask"].pack()
    pads = batch["attention_mask"].left_pads()
    row_of = lambda b, s: offs[b] + s - pads[b]
    S0 = C * bl
    plan = SP._hoist_plan(lay, S0, lay.L, row_of, batch["denoise_image_sizes"], batch["time_emb_inx"])
    assert plan is not None and plan["nf"] == 2 * G and plan["ntok"] == N and plan["S"] == 128
    perm = np.array(plan["perm"])
    assert sorted(perm[perm >= 0].tolist()) == list(range(lay.L))          # a permutation (plus gap rows)
    dense = lay.to_bool()[0]
    got = lay.permute(perm).to_bool()[0]
    keep = perm >= 0
    assert np.array_equal(got[np.ix_(keep, keep)], dense[np.ix_(perm[keep], perm[keep])])
    assert not got[~keep].any() and not got[:, ~keep].any()
    # special rows never see an image column; image rows see their clip's special columns
    nf, S = plan["nf"], plan["S"]
    assert not got[S0:S0 + 2 * nf, S:].any()
    assert got[S:S + N, S0:S0 + G].all() and got[S:S + N, S0 + nf:S0 + nf + G].all()
    # the plan's segments: one per sequence, covering the image rows
    assert plan["segments"] == ((0, S, S + G * N), (0, S + G * N, S + 2 * G * N))
    # a layout whose tail is not whole noisy frames is refused
    bad = {0: batch["denoise_image_sizes"][0][:-1], 1: batch["denoise_image_sizes"][1]}
    assert SP._hoist_plan(lay, S0, lay.L, row_of, bad, batch["time_emb_inx"]) is None


def test_left_pads_are_not_inferred_from_rows_that_merely_see_everything():
    """Leading all-ones rows are padding only in the collator's pattern (the first real row masks the pad columns,
    LVM/processor.py:722-727): a caller's full bidirectional mask, or a mask whose first real rows see everything, keeps
    every token."""
    L = 6
    assert E.count_left_pads(torch.ones(2, L, L, dtype=torch.bool)) == [0, 0]
    m = torch.ones(1, L, L, dtype=torch.bool)
    m[0, 3:, :] = torch.tril(torch.ones(3, L, dtype=torch.bool), diagonal=3)   # rows 0..2 all ones, row 3 still sees cols 0..2
    assert E.count_left_pads(m) == [0]
    ref = torch.zeros(1, L, L, dtype=torch.bool)                               # the collator's pattern: 2 pad rows
    ref[0, :2] = True
    ref[0, 2:, 2:] = torch.tril(torch.ones(4, 4, dtype=torch.bool))
    assert E.count_left_pads(ref) == [2]


def _clip_pass_layout(C=2, G=3, N=16, T=4):
    """The sequence engine.StaticDenoiser._clip_pass lays out: [prefix | <|diffusion|> rows | T x time rows]."""
    bl = N + 2
    batch = product_inference(C, G, N, 1, mask_format="layout")
    lay, offs = batch["attention_mask"].pack()
    pads = batch["attention_mask"].left_pads()
    row_of = lambda b, s: offs[b] + s - pads[b]
    S0 = C * bl
    plan = SP._hoist_plan(lay, S0, lay.L, row_of, batch["denoise_image_sizes"], batch["time_emb_inx"])
    hoisted = lay.permute(np.array(plan["perm"]))
    nf = plan["nf"]
    Sc = S0 + nf
    idx, sub_tail = SP.clip_pass_rows(S0, nf, T)
    lp = hoisted.permute(idx)
    sub = lp.sub.copy()
    sub[0, Sc:] = sub_tail
    return hoisted, lp.with_subgroups(sub), S0, nf, T


def test_time_rows_of_all_steps_in_one_sequence():
    """Sub-groups (layout.TokenLayout.sub): with the time rows of step s numbered s + 1, the one-sequence clip pass gives
    every time row exactly the keys it has in the sampler's own sequence -- the prefix, its clip's <|diffusion|> columns,
    the time columns of ITS step -- and nothing of any other step; prefix and <|diffusion|> rows are unchanged."""
    hoisted, lp, S0, nf, T = _clip_pass_layout()
    Sc = S0 + nf
    ref = hoisted.to_bool()[0]                  # rows / columns [0, Sc + nf) = prefix, diffusion rows, time rows
    got = lp.to_bool()[0]
    assert np.array_equal(got[:Sc, :Sc], ref[:Sc, :Sc]) and not got[:Sc, Sc:].any()
    for s in range(T):
        rows = slice(Sc + s * nf, Sc + (s + 1) * nf)
        assert np.array_equal(got[rows, :Sc], ref[Sc:Sc + nf, :Sc])            # prefix + diffusion columns
        assert np.array_equal(got[rows, rows], ref[Sc:Sc + nf, Sc:Sc + nf])    # own step's time columns
        other = np.ones(lp.L, dtype=bool)
        other[:Sc] = False
        other[rows] = False
        assert not got[rows][:, other].any()                                   # no other step
    with pytest.raises(ValueError):
        LY.TokenLayout(lp.thr, lp.seq, lp.kind, lp.oc, lp.grp, np.ones_like(lp.sub))   # sub on a CLEAN token


@pytest.mark.gpu
def test_device_expansion_with_subgroups_is_bit_exact(ops):
    _, lp, _, _, _ = _clip_pass_layout(C=2, G=3, N=16, T=5)
    ref = ops.pack_mask(torch.from_numpy(lp.to_bool()).to("cuda:0"))
    pm = lp.packed_mask("cuda:0")
    assert torch.equal(pm.bits, ref.bits) and torch.equal(pm.summary, ref.summary)
