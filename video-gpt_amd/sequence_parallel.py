"""Ulysses sequence parallelism behind the reference's seam.

Reference: `LVM.frame_block_forward` gives every rank of the sequence-parallel group a contiguous L/P slice of the
token sequence (LVM/model.py:457-463) and all-gathers the last hidden state (:466-473); every attention module's
`dist_attn` (DeepSpeed `DistributedAttention`, rebound to `new_attn_forward`, LVM/transform/sdpa_transform.py:94-159,
168) turns (B, L/P, heads, d) into (B, L, heads/P, d) with one all-to-all per q / k / v, runs `local_attn` on the full
sequence for its heads and returns with a fourth all-to-all.

Here the exchange is `torch.distributed.all_to_all_single` over RCCL (one process per GPU, xGMI links); the data
re-layout around it is tensor copies, the attention itself is the block-masked HIP kernel on the full-length mask.
Transports without an all-to-all for device tensors (gloo, used by the 2-rank test on a single GPU) fall back to an
all-gather through host memory -- same result, test-only bandwidth.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

_GROUP = None


def initialize_sequence_parallel_state(sequence_parallel_size: Optional[int] = None, group=None):
    """LVM/parallel_states.py:40-53: the sequence-parallel group (default: all ranks)."""
    global _GROUP
    if not dist.is_initialized():
        raise RuntimeError("initialize torch.distributed before the sequence-parallel state")
    world = dist.get_world_size()
    if group is not None:
        _GROUP = group
    elif sequence_parallel_size in (None, world):
        _GROUP = dist.group.WORLD
    else:
        if world % sequence_parallel_size:
            raise ValueError("world size must be a multiple of the sequence-parallel size")
        rank = dist.get_rank()
        for g0 in range(0, world, sequence_parallel_size):
            ranks = list(range(g0, g0 + sequence_parallel_size))
            g = dist.new_group(ranks)
            if rank in ranks:
                _GROUP = g
    return _GROUP


def get_sequence_parallel_group():
    return _GROUP


def sp_world(group=None) -> int:
    group = group if group is not None else _GROUP
    return 1 if group is None else dist.get_world_size(group)


def sp_rank(group=None) -> int:
    group = group if group is not None else _GROUP
    return 0 if group is None else dist.get_rank(group)


def _exchange(chunks: torch.Tensor, group) -> torch.Tensor:
    """chunks (P, ...): chunk j goes to rank j; returns (P, ...) with chunk i received from rank i."""
    if dist.get_backend(group) == "nccl":
        out = torch.empty_like(chunks)
        dist.all_to_all_single(out, chunks.contiguous(), group=group)
        return out
    P, me = dist.get_world_size(group), dist.get_rank(group)
    host = chunks.contiguous().cpu()
    gathered = [torch.empty_like(host) for _ in range(P)]
    dist.all_gather(gathered, host, group=group)
    return torch.stack([gathered[src][me] for src in range(P)]).to(chunks.device)


def seq_all_to_all(x: torch.Tensor, scatter_idx: int, gather_idx: int, group) -> torch.Tensor:
    """DeepSpeed `_SeqAllToAll` on a (B, S, heads, d) tensor: split dim `scatter_idx` over the P ranks, concatenate the
    received pieces along dim `gather_idx` (rank order)."""
    P = dist.get_world_size(group)
    if P == 1:
        return x
    if x.shape[scatter_idx] % P:
        raise ValueError(f"dimension {scatter_idx} ({x.shape[scatter_idx]}) is not divisible by the group size {P}")
    parts = torch.stack(torch.chunk(x, P, dim=scatter_idx))      # (P, ..., scatter/P, ...)
    recv = _exchange(parts, group)                               # recv[i] = what rank i held for me
    return torch.cat(list(recv.unbind(0)), dim=gather_idx)


class DistributedAttention:
    """`module.dist_attn` of the reference: called as dist_attn(q, k, v, batch_dim_idx, **kw) on (B, L/P, heads, d)
    tensors, returns (B, L/P, heads, d).  `local_attn` gets (B, heads/P, L, d) like SDPA."""

    def __init__(self, local_attn, group=None, scatter_idx: int = 2, gather_idx: int = 1):
        self.local_attn, self.spg = local_attn, group
        self.scatter_idx, self.gather_idx = scatter_idx, gather_idx

    def __call__(self, query, key, value, batch_dim_idx: int = 0, *args, **kwargs):
        g = self.spg if self.spg is not None else _GROUP
        if batch_dim_idx != 0:
            raise ValueError("batch must be dimension 0")
        q = seq_all_to_all(query, self.scatter_idx, self.gather_idx, g).transpose(1, 2)
        k = seq_all_to_all(key, self.scatter_idx, self.gather_idx, g).transpose(1, 2)
        v = seq_all_to_all(value, self.scatter_idx, self.gather_idx, g).transpose(1, 2)
        ctx = self.local_attn(q, k, v, *args, **kwargs).transpose(1, 2)          # (B, L, heads/P, d)
        return seq_all_to_all(ctx.contiguous(), self.gather_idx, self.scatter_idx, g)

    forward = __call__


def shard_sequence(input_emb: torch.Tensor, position_ids: torch.Tensor, group=None):
    """LVM/model.py:457-463: this rank's contiguous L/P slice of the embeddings and positions."""
    P, r = sp_world(group), sp_rank(group)
    L = input_emb.shape[1]
    assert L % P == 0, "sequence length must be divisible by the sequence-parallel size"
    c = L // P
    return input_emb[:, r * c:(r + 1) * c].contiguous(), position_ids[:, r * c:(r + 1) * c].contiguous()


def gather_sequence(hidden: torch.Tensor, group=None) -> torch.Tensor:
    """LVM/model.py:466-473: all-gather of the last hidden state along the sequence."""
    group = group if group is not None else _GROUP
    P = sp_world(group)
    if P == 1:
        return hidden
    if dist.get_backend(group) == "nccl":
        parts = [torch.empty_like(hidden) for _ in range(P)]
        dist.all_gather(parts, hidden.contiguous(), group=group)
    else:
        host = hidden.contiguous().cpu()
        hp = [torch.empty_like(host) for _ in range(P)]
        dist.all_gather(hp, host, group=group)
        parts = [t.to(hidden.device) for t in hp]
    return torch.cat(parts, dim=1)


def broadcast_batch(obj, src: int, group=None, device=None):
    """`broadcast_data` of the reference's sequence-parallel scripts (train_x1_stage2_noiseinput_frameblock.py:370-373,
    LVM/train_helper/loss.py:150,168-172): every rank of `group` returns rank `src`'s `obj` (`src` is a GLOBAL rank, as in
    torch.distributed.broadcast) -- any nesting of dicts, lists, tuples, tensors and plain values.  Tensors travel through
    host memory and come back on `device` (default: the CPU).  Host side, once per batch: not on the step's hot path."""
    group = group if group is not None else _GROUP
    if group is None or dist.get_world_size(group) == 1:
        return obj

    def walk(o, fn):
        if torch.is_tensor(o):
            return fn(o)
        if isinstance(o, dict):
            return {k: walk(v, fn) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return type(o)(walk(v, fn) for v in o)
        return o
    box = [walk(obj, lambda t: t.detach().cpu()) if dist.get_rank() == src else None]
    dist.broadcast_object_list(box, src=src, group=group)
    return box[0] if device is None else walk(box[0], lambda t: t.to(device))


# ---- flat exchanges: the sharded sampler engine (engine.StaticDenoiser with sequence_parallel=True) and the trainer's
#      sharded optimizer (train.Stage1Trainer with dp_sharding="optimizer") ----

def exchange_split(send: torch.Tensor, recv: torch.Tensor, counts, group=None) -> torch.Tensor:
    """All-to-all with per-rank split sizes, in place: counts[i][j] = elements rank i sends to rank j (every rank passes
    the same matrix); `send` holds this rank's chunks in destination order, `recv` (contiguous) receives the chunks of
    ranks 0..P-1 in rank order.  RCCL: one all_to_all_single on the current stream.  Other transports (gloo, the tests'
    two ranks on one GPU): an all-gather of padded buffers through host memory -- test-only bandwidth."""
    group = group if group is not None else _GROUP
    P, me = dist.get_world_size(group), dist.get_rank(group)
    if len(counts) != P or any(len(row) != P for row in counts):
        raise ValueError(f"exchange_split: counts must be a {P} x {P} matrix")
    rs = [int(counts[i][me]) for i in range(P)]
    if send.numel() != sum(counts[me]) or recv.numel() != sum(rs) or not recv.is_contiguous():
        raise ValueError("exchange_split: send / recv sizes disagree with counts (recv must be contiguous)")
    if dist.get_backend(group) == "nccl":
        dist.all_to_all_single(recv.view(-1), send.contiguous().view(-1), output_split_sizes=rs,
                               input_split_sizes=[int(c) for c in counts[me]], group=group)
        return recv
    es = send.element_size()                      # moved as bytes: any dtype, whatever the transport supports
    n = max(sum(row) for row in counts) * es
    host = torch.zeros(n, dtype=torch.uint8)
    host[:send.numel() * es] = send.reshape(-1).cpu().view(torch.uint8)
    gathered = [torch.empty_like(host) for _ in range(P)]
    dist.all_gather(gathered, host, group=group)
    parts = []
    for i in range(P):
        off = sum(counts[i][:me]) * es
        parts.append(gathered[i][off:off + rs[i] * es])
    recv.view(-1).copy_(torch.cat(parts).view(recv.dtype).to(recv.device))
    return recv


def _flat_collective(fn, out: torch.Tensor, inp: torch.Tensor, group, async_op: bool):
    """fn(out, inp) -- dist.all_gather_into_tensor or dist.reduce_scatter_tensor -- on the device tensors over RCCL (`inp`
    may be this rank's slice of `out`: in place; with async_op the work handle is returned).  Other transports (gloo, the
    tests' ranks sharing one GPU) have no device-tensor version: the collective runs on host copies and the result is
    copied back on the current stream before returning (None) -- test-only bandwidth."""
    if dist.get_backend(group) == "nccl":
        return fn(out, inp, group=group, async_op=async_op)
    host = torch.empty(out.shape, dtype=out.dtype)
    fn(host, inp.cpu(), group=group)
    out.copy_(host)
    return None


def all_gather_flat(x: torch.Tensor, group=None, out: Optional[torch.Tensor] = None, async_op: bool = False):
    """(P, x.numel()) stack of every rank's `x` (same size on every rank), row i from rank i.  `out` (contiguous, P x
    x.numel() elements) receives it instead of a new tensor; `x` may be row `rank` of `out` (in place).  async_op: the
    RCCL work handle is returned instead (None on host-staged transports, which finish before returning)."""
    group = group if group is not None else _GROUP
    P = dist.get_world_size(group)
    flat = x.contiguous().view(-1)
    if out is None:
        out = torch.empty(P, flat.numel(), dtype=x.dtype, device=x.device)
    if out.numel() != P * flat.numel() or not out.is_contiguous():
        raise ValueError("all_gather_flat: out must be contiguous with P x x.numel() elements")
    work = _flat_collective(dist.all_gather_into_tensor, out.view(-1), flat, group, async_op)
    return work if async_op else out.view(P, flat.numel())


def reduce_scatter_flat(buf: torch.Tensor, group=None, async_op: bool = False):
    """In place on the contiguous flat `buf` (numel a multiple of P): rank r's slice [r*s, (r+1)*s), s = numel / P,
    receives the sum over the ranks of that slice; the rest of `buf` keeps this rank's values.  Returns the slice, or
    with async_op the RCCL work handle (None on host-staged transports, which finish before returning)."""
    group = group if group is not None else _GROUP
    P, me = dist.get_world_size(group), dist.get_rank(group)
    if buf.dim() != 1 or not buf.is_contiguous() or buf.numel() % P:
        raise ValueError(f"reduce_scatter_flat: need a contiguous 1-D buffer whose length is a multiple of {P}")
    s = buf.numel() // P
    mine = buf[me * s:(me + 1) * s]
    work = _flat_collective(dist.reduce_scatter_tensor, mine, buf, group, async_op)
    return work if async_op else mine
