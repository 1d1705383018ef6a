"""Seeded inputs shared by tests/make_golden.py (which runs the REFERENCE's own LVM / LVMTraining / loss on them
through oracle/extract_reference.py), tests/test_oracle_pins.py (oracle restatement == those vectors) and the GPU
parity tests (HIP path == those vectors).  Inputs are regenerated from CPU generators; only outputs are stored."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import restate as R

BF = torch.bfloat16
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCH_KEYS = ("input_ids", "input_image_sizes", "attention_mask", "position_ids", "denoise_image_sizes", "time_emb_inx")


def single_target_case(cfg=R.TINY):
    """LVM.forward inputs (LVM/model.py:330-397): [condition ids | time token | x] with an OmniGen-style mask."""
    g = torch.Generator("cpu").manual_seed(11)
    B, Lc, hw, N = 2, 21, (8, 8), 16
    L = Lc + 1 + N
    ids = torch.randint(3, cfg.vocab_size, (B, Lc), generator=g)
    x = torch.randn(B, 4, *hw, generator=g).to(BF).float()
    t = torch.tensor([0.2, 0.9])
    lat = [torch.randn(1, 4, *hw, generator=g).to(BF).float()]
    sizes = {0: [[2, 2 + N]]}
    mask = torch.tril(torch.ones(L, L)).bool()[None].repeat(B, 1, 1)
    mask[:, -N:, -N:] = True
    pos = torch.arange(L)[None].repeat(B, 1)
    return dict(ids=ids, x=x, t=t, lat=lat, sizes=sizes, mask=mask, pos=pos, Lc=Lc, N=N)


def stage1_case(cfg=R.TINY, seed=3):
    """Stage-1 batch (F = 3 and 2 frames, 8x8 latents) with externally drawn noise / times."""
    p = {k: v.to(BF).float() for k, v in R.make_params(cfg, seed).items()}
    batch = R.collate_stage1([3, 2], 16)
    gen = torch.Generator("cpu").manual_seed(0)
    nd = sum(len(v) for v in batch["denoise_image_sizes"].values())
    nc = sum(len(v) for v in batch["input_image_sizes"].values())
    mk = lambda n: torch.randn(n, 4, 8, 8, generator=gen)
    x1, x0, clean, x0i = mk(nd), mk(nd), mk(nc), mk(nc)
    t = torch.rand(nd, generator=gen)
    ti = 0.9 + 0.1 * torch.rand(nc, generator=gen)
    return p, batch, x1, x0, t, clean, x0i, ti


def frame_block_training_batch(fbs_list=((1, 2, 2), (3, 1)), N=16):
    """Stage-2+ batch from the reference-generated collator fixture (ref_collator_fbtrain_3x2N16.npz) with the index
    dicts of TrainDataCollator_FrameBlock (LVM/train_helper/data.py:503-523)."""
    d = np.load(os.path.join(GOLD, "ref_collator_fbtrain_3x2N16.npz"))
    shape = tuple(int(v) for v in d["mask_shape"])
    mask = torch.from_numpy(np.unpackbits(d["mask_bits"], axis=-1)[:, : shape[1] * shape[2]].reshape(shape)).bool()
    sizes = {}
    for b, s, e in d["image_sizes"]:
        sizes.setdefault(int(b), []).append([int(s), int(e)])
    den, inp, tix = {}, {}, {}
    for b, fbs in enumerate(fbs_list):
        den[b], inp[b], tix[b], idx = [], [], [], 0
        for k, f in enumerate(fbs):
            if k != len(fbs) - 1:
                for _ in range(f):
                    den[b].append(sizes[b][idx]); inp[b].append(sizes[b][idx + f]); tix[b].append(sizes[b][idx][0] - 1)
                    idx += 1
                idx += f
            else:
                for _ in range(f):
                    den[b].append(sizes[b][idx]); tix[b].append(sizes[b][idx][0] - 1); idx += 1
    return dict(input_ids=torch.from_numpy(d["input_ids"]), position_ids=torch.from_numpy(d["position_ids"]),
                attention_mask=mask, input_image_sizes=inp, denoise_image_sizes=den, time_emb_inx=tix,
                frame_blocks={b: list(f) for b, f in enumerate(fbs_list)})


def sampled_grad(gr: torch.Tensor, cap: int = 6000) -> np.ndarray:
    """Every stride-th element of a flattened gradient (whole tensor when it has <= cap elements)."""
    flat = gr.detach().reshape(-1)
    stride = max(1, (flat.numel() + cap - 1) // cap)
    return flat[::stride].float().numpy()


def load(name):
    return np.load(os.path.join(GOLD, name))


def save_values(path, values: dict):
    """Store a dict of tensors, lists of tensors and plain Python values (ints, lists, tuples, dicts, None) as one .npz:
    tensors keep their dtype, plain values are stored as their repr and come back through ast.literal_eval, so a loaded
    value compares with == / torch.equal exactly as the original object did (tuples stay tuples, int keys stay ints)."""
    out = {}
    for k, v in values.items():
        if torch.is_tensor(v):
            out[f"t__{k}"] = v.numpy()
        elif isinstance(v, list) and v and all(torch.is_tensor(x) for x in v):
            out[f"n__{k}"] = np.asarray(len(v))
            for i, x in enumerate(v):
                out[f"l__{k}__{i}"] = x.numpy()
        else:
            out[f"r__{k}"] = np.asarray(repr(v))
    np.savez_compressed(path, **out)


def load_values(name) -> dict:
    """Inverse of save_values for tests/golden/<name>."""
    import ast
    d = np.load(os.path.join(GOLD, name))
    out = {}
    for key in d.files:
        kind, k = key.split("__", 1)
        if kind == "t":
            out[k] = torch.from_numpy(d[key])
        elif kind == "n":
            out[k] = [torch.from_numpy(d[f"l__{k}__{i}"]) for i in range(int(d[key]))]
        elif kind == "r":
            out[k] = ast.literal_eval(str(d[key]))
    return out


def train_collator_features(processor_cls, SpecialTokenizer):
    """Features for TrainDataCollator (stage-1 layout, F = 3) and TrainDataCollator_FrameBlock (frame blocks [1, 2, 1]) as
    the processor lays them out (tests/test_dropin_imports.py; their reference-collated form is
    tests/golden/ref_train_collators.npz)."""
    proc = processor_cls(SpecialTokenizer(10, 11, 12))
    F = 3
    prompt = "".join(f"<|diffusion|><|image_{i + 1}|><img><|image_{i + 1}|></img>" if i < F - 1 else f"<|diffusion|><|image_{i + 1}|>"
                     for i in range(F))
    feat = proc.process_multi_modal_prompt_training(prompt, [torch.full((3, 64, 64), float(i)) for i in range(F)])
    fbs = [1, 2, 1]
    prompt2, i, j, n = "", 0, 0, 0
    for k, fb in enumerate(fbs):
        for _ in range(fb):
            prompt2 += f"<|diffusion|><|image_{i + 1}|>"; i += 1; n += 1
        if k != len(fbs) - 1:
            for _ in range(fb):
                prompt2 += f"<img><|image_{j + 1}|></img>"; j += 1
    feat2 = proc.process_multi_modal_prompt_frame_block_training(prompt2, [torch.full((3, 64, 64), float(q)) for q in range(n)], fbs)
    feat2["frame_blocks"] = fbs
    return feat, F, feat2, fbs, len(feat2["image_sizes"])
