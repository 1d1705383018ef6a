"""LoRA adapter files and the merge into the base weights (LVM/pipeline.py:97-101: PeftModel.from_pretrained +
merge_and_unload).

An adapter directory is peft's: adapter_config.json + adapter_model.safetensors with the keys
`base_model.model.llm.layers.{i}.self_attn.{qkv_proj,o_proj}.lora_{A,B}.weight`, lora_A (r, in), lora_B (out, r).  peft is
not a dependency and no peft-written fixture pins this: the layout is written from knowledge of peft's format (parity
unpinned).  The merge is W <- bf16(float(W) + (lora_alpha / r) B A) per adapted projection, one rounding, on
the HIP path (ops_lora.lora_up_add with Y = W, U = B, S = A)."""
from __future__ import annotations

import json
import os
import re
from typing import Dict, Tuple

import torch

from . import ops_lora as LO
from .engine import bump_weight_generation
from .ops import BF16, VgptError

TARGETS = ("qkv_proj", "o_proj")
_KEY = re.compile(r"^base_model\.model\.llm\.layers\.(\d+)\.self_attn\.(\w+)\.lora_([AB])(?:\.default)?\.weight$")


def adapter_config(r: int, lora_alpha: float, target_modules) -> dict:
    """The adapter_config.json of the one configuration built here (train_x1_stage1_noiseinput.py:204-212)."""
    return {"peft_type": "LORA", "task_type": None, "r": int(r), "lora_alpha": lora_alpha, "lora_dropout": 0.0,
            "target_modules": list(target_modules), "init_lora_weights": "gaussian", "bias": "none",
            "fan_in_fan_out": False, "use_rslora": False, "use_dora": False, "rank_pattern": {}, "alpha_pattern": {},
            "modules_to_save": None, "inference_mode": True}


def load_adapter(path: str) -> Tuple[dict, Dict[str, torch.Tensor]]:
    """(config, tensors) of the adapter directory `path`; refuses every configuration the merge and the trainer do not
    implement instead of merging something else."""
    with open(os.path.join(path, "adapter_config.json")) as f:
        cfg = json.load(f)
    if cfg.get("peft_type", "LORA") != "LORA":
        raise VgptError(f"{path}: peft_type {cfg.get('peft_type')!r}: only LORA adapters are built")
    for flag in ("use_dora", "use_rslora", "fan_in_fan_out"):
        if cfg.get(flag):
            raise VgptError(f"{path}: {flag} adapters are not built")
    if cfg.get("bias", "none") != "none":
        raise VgptError(f"{path}: bias={cfg['bias']!r} adapters are not built (bias must be 'none')")
    for field in ("rank_pattern", "alpha_pattern", "modules_to_save"):
        if cfg.get(field):
            raise VgptError(f"{path}: a non-empty {field} is not built")
    targets = cfg.get("target_modules")
    targets = [targets] if isinstance(targets, str) else list(targets or [])
    if not targets or any(t not in TARGETS for t in targets):
        raise VgptError(f"{path}: target_modules {targets!r}: adapters are built for {TARGETS} only")
    r = cfg.get("r")
    if not isinstance(r, int) or not 1 <= r <= 64:
        raise VgptError(f"{path}: rank r={r!r}: 1 <= r <= 64 is built")
    if "lora_alpha" not in cfg:
        raise VgptError(f"{path}: adapter_config.json has no lora_alpha")
    from safetensors.torch import load_file
    raw = load_file(os.path.join(path, "adapter_model.safetensors"))
    tensors = {}
    for k, v in raw.items():
        m = _KEY.match(k)
        if m is None or m.group(2) not in targets:
            raise VgptError(f"{path}: unexpected adapter tensor {k!r}")
        if v.dim() != 2 or (v.shape[0] if m.group(3) == "A" else v.shape[1]) != r:
            raise VgptError(f"{path}: {k} has shape {tuple(v.shape)}, not rank {r}")
        tensors[k.replace(".default.weight", ".weight")] = v
    return cfg, tensors


def merge_adapter(model, adapter) -> None:
    """W <- bf16(float(W) + s B A) in place on every adapted projection of `model`; `adapter`: load_adapter()'s result.
    Waits for a trainer's update in flight first and bumps the weight generation afterwards (cached sampler engines refold)."""
    from .train import lora_key, wait_for_pending_update
    cfg, tensors = adapter
    r = int(cfg["r"])
    rp, s = LO.padded_rank(r), float(cfg["lora_alpha"]) / r
    wait_for_pending_update(model)
    work = []
    for i, layer in enumerate(model.llm.layers):
        for mod in cfg["target_modules"] if not isinstance(cfg["target_modules"], str) else [cfg["target_modules"]]:
            w = getattr(layer.self_attn, mod).weight
            ka, kb = lora_key(i, mod, "A"), lora_key(i, mod, "B")
            if ka not in tensors or kb not in tensors:
                raise VgptError(f"merge_adapter: the adapter has no {ka if ka not in tensors else kb}")
            a, b = tensors[ka], tensors[kb]
            if tuple(a.shape) != (r, w.shape[1]) or tuple(b.shape) != (w.shape[0], r):
                raise VgptError(f"merge_adapter: {ka} / {kb} do not fit a weight of shape {tuple(w.shape)}")
            work.append((w, a, b))
    if len(tensors) != 2 * len(work):
        raise VgptError("merge_adapter: the adapter has tensors for layers this model does not have")
    for w, a, b in work:            # everything validated: now write
        ap = torch.zeros(rp, w.shape[1], dtype=BF16, device=w.device)
        bp = torch.zeros(w.shape[0], rp, dtype=BF16, device=w.device)
        ap[:r].copy_(a)
        bp[:, :r].copy_(b)
        LO.lora_up_add(w.data, bp, ap, s_is_rp_by_n=True, alpha=s)
    bump_weight_generation(model)
