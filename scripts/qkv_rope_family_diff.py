"""four-wave vs eight-wave family on qkv + RoPE with general tables: number of differing output elements (library under VGPT_LIB)"""
import importlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
importlib.import_module("video-gpt_amd")
ops = importlib.import_module("video-gpt_amd.ops")
lib = importlib.import_module("video-gpt_amd._lib").load()
dev = "cuda:0"; BF = torch.bfloat16
for (M, K, nq, nkv) in ((4096, 128, 16, 16), (4096, 192, 16, 16), (4096, 128, 24, 12), (2048, 128, 32, 32), (4096, 3072, 32, 32)):
    N = (nq + 2 * nkv) * 96
    gen = torch.Generator(dev).manual_seed(7)
    x = torch.randn(M, K, device=dev, generator=gen).to(BF)
    w = (torch.randn(N, K, device=dev, generator=gen) * 0.1).to(BF)
    cos, sin = ops.rope_table(torch.randperm(M, device=dev, generator=gen), ops.rope_inv_freq(96, 10000.0, dev), round_bf16=False)
    outs = []
    for fam in (0, 1):
        prev = lib.vgpt_gemm_set_family(fam)
        y = torch.empty(M, N, dtype=BF, device=dev)
        ops.linear_qkv_rope(x, w, cos, sin, nq, nkv, 96, out=y)
        torch.cuda.synchronize()
        lib.vgpt_gemm_set_family(prev)
        outs.append(y)
    d = outs[0].view(torch.int16) != outs[1].view(torch.int16)
    print(os.environ.get("VGPT_LIB", "product")[-20:], f"M={M} N={N} K={K} heads {nq}+{nkv}+{nkv}: {int(d.sum())} of {d.numel()} differ between the families; in v columns: {int(d[:, (nq + nkv) * 96:].sum())}")
