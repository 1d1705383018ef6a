"""Tensor-level wrappers of the LoRA entry points of the C ABI (include/vgpt.h, "LoRA adapters"; csrc/lora.hip).
Same rules as ops_train.py: GPU tensors only, no torch arithmetic.

Every small operand carries a padded rank rp in {16, 32, 48, 64}; the caller owns the padding (ranks r..rp-1 are zero and
stay zero).  The big operand may be a column view of a wider buffer (row stride a multiple of 8, unit column stride)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .ops import BF16, VgptError, _chk, _ptr, _stream, call

F32 = torch.float32
PADDED_RANKS = (16, 32, 48, 64)


def padded_rank(r: int) -> int:
    """Smallest padded rank that holds a true rank r (1 <= r <= 64)."""
    if not 1 <= int(r) <= 64:
        raise VgptError(f"LoRA rank {r}: 1 <= r <= 64 is built")
    return -(-int(r) // 16) * 16


def _rows(t, name):
    """(rows, width, row stride) of a 2-D bf16 GPU tensor whose rows are contiguous."""
    _chk(t, BF16, name, contiguous=False)
    if t.dim() != 2 or t.stride(1) != 1:
        raise VgptError(f"{name}: expected a 2-D tensor with contiguous rows")
    return t.shape[0], t.shape[1], t.stride(0)


def lora_down(x, s, rp: int, s_is_k_by_rp: bool = False, alpha: float = 1.0, out=None):
    """U (M, rp) = alpha * x (M, K) @ S, S stored (rp, K) (default: u = x A^T) or (K, rp) (du = dy B)."""
    M, K, ldx = _rows(x, "lora_down.x")
    _chk(s, BF16, "lora_down.s")
    if tuple(s.shape) != ((K, rp) if s_is_k_by_rp else (rp, K)):
        raise VgptError(f"lora_down: small operand {tuple(s.shape)} does not match K={K}, rp={rp}")
    if out is None:
        out = torch.empty(M, rp, dtype=BF16, device=x.device)
    _chk(out, BF16, "lora_down.out")
    if tuple(out.shape) != (M, rp):
        raise VgptError("lora_down: output shape mismatch")
    call("vgpt_lora_down", x.data_ptr(), s.data_ptr(), out.data_ptr(), M, K, rp, ldx, int(s_is_k_by_rp), float(alpha),
         _stream())
    return out


def lora_up_add(y, u, s, s_is_rp_by_n: bool = False, alpha: float = 1.0, rope=None):
    """In place y (M, N) = bf16(rope?(float(y) + alpha * u (M, rp) @ S)), S stored (N, rp) (default) or (rp, N).
    rope = (cos, sin, n_heads, n_kv_heads, head_dim): rotate the q and k heads as ops.linear_qkv_rope does."""
    M, N, ldy = _rows(y, "lora_up_add.y")
    _chk(u, BF16, "lora_up_add.u"); _chk(s, BF16, "lora_up_add.s")
    if u.dim() != 2 or u.shape[0] != M:
        raise VgptError("lora_up_add: u must be (M, rp)")
    rp = u.shape[1]
    if tuple(s.shape) != ((rp, N) if s_is_rp_by_n else (N, rp)):
        raise VgptError(f"lora_up_add: small operand {tuple(s.shape)} does not match N={N}, rp={rp}")
    cos = sin = None
    nq = nk = hd = 0
    if rope is not None:
        cos, sin, nq, nk, hd = rope
        _chk(cos, F32, "lora_up_add.cos"); _chk(sin, F32, "lora_up_add.sin")
        if cos.numel() != M * (hd // 2) or sin.numel() != cos.numel():
            raise VgptError("lora_up_add: cos / sin tables must be (M, head_dim / 2)")
    call("vgpt_lora_up_add", y.data_ptr(), u.data_ptr(), s.data_ptr(), _ptr(cos), _ptr(sin), M, N, rp, ldy,
         int(s_is_rp_by_n), int(nq), int(nk), int(hd), float(alpha), _stream())
    return y


_grad_ws = {}


def lora_grad(y, u, out, transposed: bool = False, alpha: float = 1.0):
    """out (N, rp) fp32 (or (rp, N) with transposed) = alpha * y (M, N)^T @ u (M, rp); bit-identical from run to run."""
    M, N, ldy = _rows(y, "lora_grad.y")
    Mu, rp, ldu = _rows(u, "lora_grad.u")
    if Mu != M:
        raise VgptError("lora_grad: row counts disagree")
    _chk(out, F32, "lora_grad.out")
    if tuple(out.shape) != ((rp, N) if transposed else (N, rp)):
        raise VgptError(f"lora_grad: output {tuple(out.shape)} does not match N={N}, rp={rp}")
    need = int(_lib.load().vgpt_lora_grad_workspace_bytes(M, N, rp)) // 4
    ws = _grad_ws.get(y.device)
    if ws is None or ws.numel() < need:
        ws = _grad_ws[y.device] = torch.empty(max(need, 1 << 18), dtype=F32, device=y.device)
    call("vgpt_lora_grad", y.data_ptr(), u.data_ptr(), out.data_ptr(), M, N, rp, ldy, ldu, int(transposed), float(alpha),
         ws.data_ptr(), ws.numel() * 4, _stream())
    return out
