"""The row plan of a sampler step: which row of the engine's sequence every token of the collator's batch lands on.

Integer arithmetic on token positions only -- nothing here launches a kernel or needs a device, and everything runs on
CPU tensors and device tensors alike (tests/test_step_plan.py).  `plan_step_rows` rewrites the collator's batch the way
`engine.StaticDenoiser` runs it:
  1. left pads dropped and the rows packed into ONE sequence with a block-diagonal mask (pack_left_padded);
  2. the step-invariant condition prefix found (rows in front of the first `<|diffusion|>` token that see nothing behind it);
  3. behind a reusable prefix, either the sequence re-ordered to [prefix | `<|diffusion|>` rows | time rows | gap | image
     rows] (special-row hoisting, _hoist_plan) or an alignment gap inserted so that the first computed row is a multiple
     of 128;
  4. the query-row segments of the attention plan cut where two packed sequences meet;
  5. the collator's `input_image_sizes` / `denoise_image_sizes` / `time_emb_inx` mapped to rows of the rewritten sequence.
The smaller functions are the row arithmetic of the per-clip pass (clip_pass_rows) and of the sharded engine (sp_shares,
sp_final_layer_owners).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ._lib import VgptError
from .layout import NOISY, TokenLayout


def _rows(sizes: Dict[int, list], row_of, span: bool):
    out = []
    for b in sizes.keys():
        for item in sizes[b]:
            out.append(row_of(b, item[0] if span else item))
    return out


def count_left_pads(attention_mask) -> List[int]:
    """Left-pad length of every row, read off the mask itself: pad rows are the leading all-ones rows
    (LVM/processor.py:726-727); a real first token only sees itself."""
    if isinstance(attention_mask, TokenLayout):
        return attention_mask.left_pads()
    B, L, _ = attention_mask.shape
    if L <= 1:
        return [0] * B
    mb = attention_mask.to(torch.bool)
    lead = [int(v) for v in torch.cumprod(mb.all(-1).to(torch.int64), dim=1).sum(1).tolist()]
    # leading all-ones rows are padding only in the collator's pattern, where the first real row does not see the pad
    # columns (LVM/processor.py:722-727).  A mask whose first rows simply see everything (a caller's full bidirectional
    # mask) has no padding: packing it would drop real tokens.
    for b, n in enumerate(lead):
        if n and (n >= L or bool(mb[b, n, :n].any())):
            lead[b] = 0
    return lead


def pack_left_padded(input_ids, position_ids, attention_mask, pads: List[int]):
    """Drop the left-pad tokens of every batch row and lay the real tokens of all rows out as ONE
    sequence with a block-diagonal mask (row b's real-token sub-mask on the diagonal, everything
    between different rows masked).  Pad rows never influence real rows (pad columns are masked,
    LVM/processor.py:722-727) and the model only reads real positions, so the outputs are unchanged;
    the attention kernel skips the off-diagonal tiles through its tile summary.
    Returns (ids (1,M), positions (1,M), mask (1,M,M) bool, offsets, pads)."""
    B, L = input_ids.shape
    lens = [L - p for p in pads]
    offsets = [0]
    for n in lens[:-1]:
        offsets.append(offsets[-1] + n)
    M = sum(lens)
    ids = torch.cat([input_ids[b, pads[b]:] for b in range(B)]).view(1, M)
    pos = torch.cat([position_ids[b, pads[b]:] for b in range(B)]).view(1, M)
    if isinstance(attention_mask, TokenLayout):   # tokens keep their sequence id: block-diagonal by construction
        return ids.contiguous(), pos.contiguous(), attention_mask.pack(pads)[0], offsets
    mask = torch.zeros(1, M, M, dtype=torch.bool, device=attention_mask.device)
    for b in range(B):
        o, n, p = offsets[b], lens[b], pads[b]
        mask[0, o:o + n, o:o + n] = attention_mask[b, p:, p:].to(torch.bool)
    return ids.contiguous(), pos.contiguous(), mask, offsets


def sp_shares(M: int, P: int):
    """Contiguous shares [(begin, end)] of M rows over P ranks, in rank order, and the cut granularity: shares of a
    multiple of 256 rows (full GEMM tiles) where that keeps the largest share within 1/8 of an even split and leaves every
    rank rows, else of 64 or 16 rows, else an even split (ragged shares differ by at most one row)."""
    if M < P:
        raise VgptError(f"sequence parallelism: {M} rows cannot be shared by {P} ranks")
    even = -(-M // P)
    for g in (256, 64, 16):
        c = -(-even // g) * g
        if c <= even + even // 8 and (P - 1) * c < M:
            return [(min(r * c, M), min((r + 1) * c, M)) for r in range(P)], g
    q, rem = divmod(M, P)
    b = [0]
    for r in range(P):
        b.append(b[-1] + q + (r < rem))
    return list(zip(b[:-1], b[1:])), 1


def _hoist_plan(layout: TokenLayout, S0: int, L: int, row_of, denoise_image_sizes, time_emb_inx):
    """Re-ordering [prefix | diffusion rows | time rows | gap | image rows] of a packed next-clip sequence, or None
    when the rows behind the prefix are not exactly whole noisy frames (then only the prefix is reused)."""
    x_old = _rows(denoise_image_sizes, row_of, True)
    t_old = _rows(time_emb_inx, row_of, False)
    ntoks = {it[1] - it[0] for b in denoise_image_sizes.keys() for it in denoise_image_sizes[b]}
    nf = len(x_old)
    if nf == 0 or len(t_old) != nf or len(ntoks) != 1:
        return None
    ntok = ntoks.pop()
    if any(t != x - 1 for t, x in zip(t_old, x_old)):
        return None
    d_old = [t - 1 for t in t_old]
    rows = sorted(d_old + t_old + [x + j for x in x_old for j in range(ntok)])
    if rows != list(range(S0, L)) or not bool((layout.kind[0, S0:] == NOISY).all()):
        return None
    # the special rows must really be the offset-0 / offset-1 tokens of their frames (what makes them image-blind)
    if not (bool((layout.oc[0, d_old] == 0).all()) and bool((layout.oc[0, t_old] == 1).all())
            and bool((layout.oc[0, [x + j for x in x_old for j in range(ntok)]] == 2).all())):
        return None
    S = (S0 + 2 * nf + 127) // 128 * 128
    perm = list(range(S0)) + d_old + t_old + [-1] * (S - S0 - 2 * nf) + [x + j for x in x_old for j in range(ntok)]
    inv = {o: i for i, o in enumerate(perm) if o >= 0}
    # image rows of one sequence form one segment of the attention plan
    seqs = [int(layout.seq[0, x]) for x in x_old]
    segs, f0 = [], 0
    for f in range(1, nf + 1):
        if f == nf or seqs[f] != seqs[f0]:
            segs.append((0, S + f0 * ntok, S + f * ntok))
            f0 = f
    return dict(perm=perm, inv=inv, S=S, nf=nf, ntok=ntok, segments=tuple(segs))


@dataclass(frozen=True)
class StepPlan:
    """What plan_step_rows decided.  Rows are indices into the rewritten sequence, flattened over the batch (b * L + s)."""
    input_ids: torch.Tensor          # (B, L), rewritten
    position_ids: torch.Tensor       # (B, L), rewritten
    attention_mask: object           # (B, L, L) bool | TokenLayout, rewritten; a PackedMask as it came
    B: int
    L: int
    S: int                           # first row a step computes: 0, or the (aligned) end of the step-invariant rows
    S0: int                          # rows of the reused prefix the prefill computes: its own length when hoisted, else == S
    packed: bool                     # left pads were dropped and the batch rows laid out as one sequence
    hoist: Optional[dict]            # _hoist_plan's dict when the special rows left the per-step row set
    seg_all: Optional[tuple]         # attention-plan segments (batch, begin, end) over every row, None = one per batch row
    seg_live: Optional[tuple]        # ... over the rows [S, L) a step computes behind a reused prefix
    cond_rows: List[int]             # first row of every condition frame (input_image_sizes)
    x_rows: List[int]                # first row of every noisy frame (denoise_image_sizes)
    t_rows: List[int]                # row of every time token (time_emb_inx)
    row_map: Tuple[np.ndarray, ...]  # row_map[b][s]: row of token s of the ORIGINAL batch row b, -1 for a dropped pad

    def row(self, b: int, s: int) -> int:
        return int(self.row_map[b][s])


def _moved(row_map, new_of_old: np.ndarray):
    """row_map after one more rewrite of the sequence that puts old row i at new_of_old[i]."""
    return tuple(np.where(m >= 0, new_of_old[np.maximum(m, 0)], -1) for m in row_map)


def plan_step_rows(input_ids, position_ids, attention_mask, input_image_sizes, denoise_image_sizes, time_emb_inx, *,
                   pack_padding: bool, reuse_condition_prefix: bool, hoist_special_rows: bool) -> StepPlan:
    """The batch as the collator laid it out -> the sequence a sampler step runs (module docstring).  attention_mask: a
    dense (B, L, L) bool tensor, a TokenLayout, or an already bit-packed mask (anything else), which is passed through with
    the sequence untouched."""
    prepacked = not isinstance(attention_mask, (TokenLayout, torch.Tensor))
    B, L = input_ids.shape
    row_map = tuple(b * L + np.arange(L, dtype=np.int64) for b in range(B))
    row_of = lambda b, s: int(row_map[b][int(s)])   # reads the row_map of the moment it is called
    packed = False
    seq_bounds = None   # packed layout: row range of every original batch row, for the attention plan
    pads = count_left_pads(attention_mask) if pack_padding and not prepacked else []
    if any(pads):
        input_ids, position_ids, attention_mask, offs = pack_left_padded(input_ids, position_ids, attention_mask, pads)
        row_map = tuple(np.where(np.arange(L) >= pads[b], offs[b] + np.arange(L, dtype=np.int64) - pads[b], -1)
                        for b in range(B))
        seq_bounds = [(offs[b], offs[b] + (L - pads[b])) for b in range(B)]
        B, L = input_ids.shape
        packed = True
    # ---- condition-prefix reuse: rows before the first <|diffusion|> token never see a
    #      noisy / time token (LVM/processor.py:682-731), so their activations are identical at every denoise
    #      step; the reference recomputes them 50x (LVM/scheduler.py:174).  They are computed ONCE (prefill),
    #      their per-layer K/V stay in a full-length qkv buffer, and a step only runs the remaining rows. ----
    S = S0 = 0
    hoist = None
    if reuse_condition_prefix and B == 1 and not prepacked:
        t_first = min(row_of(b, t) for b in time_emb_inx.keys() for t in time_emb_inx[b]) - 1
        is_layout = isinstance(attention_mask, TokenLayout)
        m2 = None if is_layout else attention_mask[0].to(torch.bool)
        static = t_first >= 128 and (attention_mask.prefix_is_static(t_first) if is_layout
                                     else not bool(m2[:t_first, t_first:].any()))
        if static and hoist_special_rows and is_layout:
            hoist = _hoist_plan(attention_mask, t_first, L, row_of, denoise_image_sizes, time_emb_inx)
        dev = input_ids.device
        if hoist is not None:
            # ---- special-row hoisting: the `<|diffusion|>` row of a noisy frame sees only `<|diffusion|>` columns
            #      and the condition prefix, its time row only those and the time columns — never an image column
            #      (LVM/processor.py:682-731) — so the first is step-invariant and the second a function of the step
            #      index alone.  Both leave the per-step row set: the sequence is re-ordered to
            #      [prefix | diffusion rows | time rows | gap | image rows], the image rows (n_frames x N: whole
            #      GEMM / attention tiles) are all a step computes, and the time rows' q/k/v of EVERY step come
            #      from the per-clip pass (StaticDenoiser._clip_pass) and are dropped in by vgpt_sampler_copy_step_rows. ----
            perm = np.asarray(hoist["perm"], dtype=np.int64)
            pt = torch.from_numpy(np.maximum(perm, 0)).to(dev)
            gapm = torch.from_numpy(perm < 0).to(dev)
            input_ids = torch.where(gapm, input_ids[0, 0], input_ids[0, pt]).view(1, -1)
            position_ids = torch.where(gapm, torch.zeros_like(position_ids[0, pt]), position_ids[0, pt]).view(1, -1)
            attention_mask = attention_mask.permute(perm)
            new_of_old = np.full(L, -1, dtype=np.int64)
            new_of_old[perm[perm >= 0]] = np.nonzero(perm >= 0)[0]
            row_map = _moved(row_map, new_of_old)
            L = len(perm)
            S, S0 = hoist["S"], t_first
            seq_bounds = None   # the plan cut its own segments
        elif static:
            # ---- no hoisting: a gap behind the prefix aligns the first computed row to the kernels' 128-row blocks ----
            P0 = t_first
            S = S0 = (P0 + 127) // 128 * 128   # S0 == S: the alignment rows ride along with the prefix
            npad = S - P0
            pad_ids = torch.full((1, npad), int(input_ids[0, 0]), dtype=input_ids.dtype, device=dev)
            input_ids = torch.cat([input_ids[:, :P0], pad_ids, input_ids[:, P0:]], dim=1)
            position_ids = torch.cat([position_ids[:, :P0], torch.zeros(1, npad, dtype=position_ids.dtype, device=dev),
                                      position_ids[:, P0:]], dim=1)
            if is_layout:
                attention_mask = attention_mask.insert_gap(P0, npad)
            else:
                mask2 = torch.zeros(1, L + npad, L + npad, dtype=torch.bool, device=m2.device)
                mask2[0, :P0, :P0] = m2[:P0, :P0]
                mask2[0, S:, :P0] = m2[P0:, :P0]
                mask2[0, S:, S:] = m2[P0:, P0:]
                attention_mask = mask2
            new_of_old = np.arange(L, dtype=np.int64)
            new_of_old[P0:] += npad
            row_map = _moved(row_map, new_of_old)
            if seq_bounds is not None:
                seq_bounds = [(int(new_of_old[a]), int(new_of_old[e - 1]) + 1) for a, e in seq_bounds]
            L += npad
    # query-row segments of the attention plan: cut where two packed sequences meet (their key sets differ) so
    # that no work item of the kernel straddles them; `seg_live` covers the rows computed at every step
    seg_all = seg_live = None
    if seq_bounds is not None and B == 1:
        cuts = sorted({0, L, *[a for a, _ in seq_bounds]})
        seg_all = tuple((0, a, e) for a, e in zip(cuts[:-1], cuts[1:]) if e > a)
        if S:
            cl = sorted({S, L, *[a for a, _ in seq_bounds if a > S]})
            seg_live = tuple((0, a, e) for a, e in zip(cl[:-1], cl[1:]) if e > a)
    if hoist is not None:
        seg_live = hoist["segments"]
    return StepPlan(input_ids=input_ids, position_ids=position_ids, attention_mask=attention_mask, B=B, L=L, S=S, S0=S0,
                    packed=packed, hoist=hoist, seg_all=seg_all, seg_live=seg_live,
                    cond_rows=_rows(input_image_sizes or {}, row_of, True), x_rows=_rows(denoise_image_sizes, row_of, True),
                    t_rows=_rows(time_emb_inx, row_of, False), row_map=row_map)


def _sees(mask, q0: int, q1: int, k0: int, k1: int) -> bool:
    """Whether any row of [q0, q1) sees a column of [k0, k1) of batch row 0: from a TokenLayout's attributes
    (TokenLayout.visible_block: its rule on that block alone) or from a dense mask."""
    if q1 <= q0 or k1 <= k0:
        return False
    if not isinstance(mask, TokenLayout):
        return bool(mask[0, q0:q1, k0:k1].to(torch.bool).any())
    return bool(mask.visible_block(q0, q1, k0, k1).any())


def conditional_live_rows(plan: StepPlan, layout_or_mask, n_frames: int):
    """The rows a step computes for the FIRST packed sequence alone (with image CFG: the conditional one), or None.

    Returns (row_begin, row_end, n_cond_frames, segments): the leading range [S, S + Mc) of the live rows [S, L) that
    belongs to the first packed sequence, the number of (leading) noisy frames whose rows lie in it, and the attention-plan
    segments restricted to it.  A step that needs the first sequence's prediction only (an unguided step of a guidance
    schedule, engine.py) may run these rows and nothing else: it is checked HERE, from the mask's attributes, that no row of
    the range sees a live row outside it -- the rows below S it sees are cached, step-invariant ones.
    None when the live rows of sequence 0 are no such range: an unpacked batch, a pre-packed mask (nothing is known about
    it), one sequence, frames or time rows that do not split into a leading group inside the range and a rest outside it, or
    a range that sees out."""
    if not plan.packed or plan.B != 1 or not isinstance(layout_or_mask, (TokenLayout, torch.Tensor)):
        return None
    seg = plan.seg_live if plan.S else plan.seg_all
    if seg is None or len(seg) < 2:
        return None
    S, L = plan.S, plan.L
    _, a, e = seg[0]
    if a != S or not (S < e < L) or len(plan.x_rows) != n_frames:
        return None
    inside = [a <= x < e for x in plan.x_rows]
    nc = sum(inside)
    if nc == 0 or nc == n_frames or not all(inside[:nc]):
        return None
    # the time rows of a layout that keeps them live go with their frames (hoisted: they sit below S, written for every frame)
    if not plan.hoist and [a <= t < e for t in plan.t_rows] != inside:
        return None
    if any(x < S for x in plan.x_rows) or (not plan.hoist and any(t < S for t in plan.t_rows)):
        return None
    if _sees(layout_or_mask, a, e, e, L):
        return None
    return a, e, nc, (seg[0],)


def clip_pass_rows(S0: int, nf: int, T: int):
    """The one-sequence per-clip pass of a hoisted layout (StaticDenoiser._clip_pass),
        [prefix 0..S0) | nf `<|diffusion|>` rows | step 0's nf time rows | step 1's | ... | step T-1's],
    as rows of the hoisted sequence: (idx, sub_tail).  idx[i]: the hoisted row at position i of the pass -- the cached rows
    [0, S0 + nf) once, then the nf time rows behind them T times; sub_tail: the sub-group of every position from S0 + nf
    on, s + 1 for the time rows of step s (layout.TokenLayout)."""
    Sc = S0 + nf
    idx = np.concatenate([np.arange(Sc), np.tile(np.arange(Sc, Sc + nf), T)])
    return idx, 1 + np.repeat(np.arange(T), nf)


def sp_final_layer_owners(x_rows_live, h: int, w: int, shares, rank: int):
    """Final layer of the sharded engine.  x_rows_live: first live row of every frame (h/2 * w/2 rows each); shares: the
    ranks' row ranges (sp_shares).  Returns ((f0, f1), owner): the frames with a row in `rank`'s share, and for every
    (frame, y, x) of the latent the index of the share that computed its row, a CPU int64 tensor."""
    a, b = shares[rank]
    ntok = (h // 2) * (w // 2)
    mine = [f for f, x0 in enumerate(x_rows_live) if x0 < b and x0 + ntok > a]
    frames = (mine[0], mine[-1] + 1) if mine else (0, 0)
    bounds = torch.tensor([e for _, e in shares], dtype=torch.int64)
    tok = (torch.arange(h)[:, None] // 2) * (w // 2) + torch.arange(w)[None, :] // 2
    rows = torch.tensor(x_rows_live, dtype=torch.int64)[:, None, None] + tok[None]          # (nf, h, w) live row
    return frames, torch.bucketize(rows, bounds, right=True)
