"""Tensor-level wrappers of the frame-preprocessing entry points of the C ABI (include/vgpt.h, "frame
preprocessing").  Same rules as ops.py: GPU tensors only, no torch arithmetic.  Frames are (N, H, W, 3) uint8,
contiguous; the resampler is Pillow's 8-bit one bit for bit."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import FILTER_BICUBIC, FILTER_BOX
from .ops import VgptError, _chk, _stream, call

U8, F32 = torch.uint8, torch.float32

_TABLES = {}      # (in, out, filter, device) -> (bounds, coeffs, ksize): device copies of vgpt_resample_coeffs
_WORKSPACE = {}   # device -> grow-only uint8 buffer for the image between the two passes of a resize


def resample_ksize(n_in: int, n_out: int, filter: int) -> int:
    lib = _lib.load()
    ksize = lib.vgpt_resample_ksize(n_in, n_out, filter)
    if ksize < 0:
        raise VgptError(f"vgpt_resample_ksize failed (rc={ksize}): {lib.vgpt_last_error().decode()}")
    return ksize


def resample_table_host(n_in: int, n_out: int, filter: int):
    """(bounds (out, 2) int32, coeffs (out, ksize) int32) of one pass, as numpy arrays (no GPU needed)."""
    ksize = resample_ksize(n_in, n_out, filter)
    bounds = np.empty((n_out, 2), np.int32)
    coeffs = np.empty((n_out, ksize), np.int32)
    call("vgpt_resample_coeffs", n_in, n_out, filter, bounds.ctypes.data, coeffs.ctypes.data)
    return bounds, coeffs


def resample_table(n_in: int, n_out: int, filter: int, device):
    """Device copy of one pass's table, built once per (in, out, filter, device)."""
    device = torch.device(device)
    key = (n_in, n_out, filter, device)
    if key not in _TABLES:
        bounds, coeffs = resample_table_host(n_in, n_out, filter)
        _TABLES[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device), coeffs.shape[1])
    return _TABLES[key]


def _workspace(nbytes: int, device) -> torch.Tensor:
    ws = _WORKSPACE.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _WORKSPACE[device] = torch.empty(nbytes, dtype=U8, device=device)
    return ws[:nbytes]


def _chk_frames(frames: torch.Tensor, name: str):
    _chk(frames, U8, name)
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise VgptError(f"{name}: expected (N, H, W, 3) uint8 frames, got shape {tuple(frames.shape)}")


def _chk_out(out: Optional[torch.Tensor], shape, dtype, device, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _chk(out, dtype, name)
    if tuple(out.shape) != tuple(shape):
        raise VgptError(f"{name}: expected shape {tuple(shape)}, got {tuple(out.shape)}")
    return out


def resample_pass(frames: torch.Tensor, out_len: int, filter: int, axis: int, out: Optional[torch.Tensor] = None):
    """One pass of the resampler: axis 1 resizes the width, axis 0 the height."""
    _chk_frames(frames, "resample_pass.frames")
    if axis not in (0, 1):
        raise VgptError(f"resample_pass: axis = {axis} (0 = vertical, 1 = horizontal)")
    N, H, W, _ = frames.shape
    bounds, coeffs, ksize = resample_table(W if axis == 1 else H, out_len, filter, frames.device)
    shape = (N, H, out_len, 3) if axis == 1 else (N, out_len, W, 3)
    out = _chk_out(out, shape, U8, frames.device, "resample_pass.out")
    call("vgpt_resample_u8", frames.data_ptr(), out.data_ptr(), bounds.data_ptr(), coeffs.data_ptr(), ksize, N, H, W,
         out_len, axis, _stream())
    return out


def _horizontal(frames: torch.Tensor, w: int, filter: int, workspace: Optional[torch.Tensor]) -> torch.Tensor:
    """The first pass of a two-pass resize, into the (cached) workspace."""
    N, H = frames.shape[:2]
    need = N * H * w * 3
    if workspace is None:
        workspace = _workspace(need, frames.device)
    else:
        _chk(workspace, U8, "resample.workspace")
        if workspace.numel() < need:
            raise VgptError(f"resample: workspace of {workspace.numel()} bytes, {need} needed")
    return resample_pass(frames, w, filter, 1, out=workspace.view(-1)[:need].view(N, H, w, 3))


def resample_u8(frames: torch.Tensor, size: Tuple[int, int], filter: int, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PIL.Image.resize(size=(w, h), resample=BOX | BICUBIC) on every frame: the horizontal pass if the width changes, then
    the vertical pass if the height changes; the image between two passes lives in a cached per-device workspace (or in
    `workspace`), which the next resize on that device overwrites.  Nothing to do: a copy, as in Pillow."""
    _chk_frames(frames, "resample_u8.frames")
    N, H, W, _ = frames.shape
    w, h = int(size[0]), int(size[1])
    out = _chk_out(out, (N, h, w, 3), U8, frames.device, "resample_u8.out")
    if w != W and h != H:
        resample_pass(_horizontal(frames, w, filter, workspace), h, filter, 0, out=out)
    elif w != W:
        resample_pass(frames, w, filter, 1, out=out)
    elif h != H:
        resample_pass(frames, h, filter, 0, out=out)
    else:
        out.copy_(frames)
    return out


def u8_to_chw_norm(frames: torch.Tensor, box: Optional[Tuple[int, int, int, int]] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Crop `box` = (left, upper, right, lower), HWC -> planar, ToTensor + Normalize(0.5, 0.5): (N, 3, h, w) fp32."""
    _chk_frames(frames, "u8_to_chw_norm.frames")
    N, H, W, _ = frames.shape
    x0, y0, x1, y1 = (0, 0, W, H) if box is None else (int(v) for v in box)
    out = _chk_out(out, (N, 3, y1 - y0, x1 - x0), F32, frames.device, "u8_to_chw_norm.out")
    call("vgpt_u8_to_chw_norm", frames.data_ptr(), out.data_ptr(), N, H, W, y0, x0, y1 - y0, x1 - x0, _stream())
    return out


def resample_v_chw_norm(frames: torch.Tensor, out_h: int, filter: int, box: Optional[Tuple[int, int, int, int]] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The vertical pass to `out_h` rows writing the window `box` of its result as normalised planar fp32: bit for bit
    resample_pass(axis 0) + u8_to_chw_norm, without the uint8 image in between."""
    _chk_frames(frames, "resample_v_chw_norm.frames")
    N, H, W, _ = frames.shape
    x0, y0, x1, y1 = (0, 0, W, out_h) if box is None else (int(v) for v in box)
    bounds, coeffs, ksize = resample_table(H, out_h, filter, frames.device)
    out = _chk_out(out, (N, 3, y1 - y0, x1 - x0), F32, frames.device, "resample_v_chw_norm.out")
    call("vgpt_resample_u8_v_chw_norm", frames.data_ptr(), out.data_ptr(), bounds.data_ptr(), coeffs.data_ptr(), ksize, N, H,
         W, out_h, y0, x0, y1 - y0, x1 - x0, _stream())
    return out


def resample_chw_norm(frames: torch.Tensor, size: Tuple[int, int], filter: int,
                      box: Optional[Tuple[int, int, int, int]] = None, out: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resample_u8 + u8_to_chw_norm with the last pass fused: whenever the height changes, the vertical pass writes the
    cropped, normalised tensor itself; a resize with no vertical pass ends in u8_to_chw_norm."""
    _chk_frames(frames, "resample_chw_norm.frames")
    N, H, W, _ = frames.shape
    w, h = int(size[0]), int(size[1])
    box = (0, 0, w, h) if box is None else box
    if w != W:
        frames = _horizontal(frames, w, filter, workspace)
    if h != H:
        return resample_v_chw_norm(frames, h, filter, box, out=out)
    return u8_to_chw_norm(frames, box, out=out)
