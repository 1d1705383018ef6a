"""Developer probe (GPU): attention forward / backward kernels on the cfg-3 stage-1 mask (B=2, L=3870, 32 heads).

  --head-dim 64,96,128   the widths to run, one after the other in this process (default 96: the two lines it always printed)
  --floor                also time torch's scaled_dot_product_attention autograd backward (bf16, same q, k, v and additive
                         mask) and print, per width, the backward's time, its FLOP/s (10 hd per visible (query, key) pair
                         and head: the five products S, dP, dQ, dK, dV), the floor, and the FLOP/s relative to head dim 96"""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
importlib.import_module("video-gpt_amd")
P = importlib.import_module("video-gpt_amd.processor"); ops = importlib.import_module("video-gpt_amd.ops")
T = importlib.import_module("video-gpt_amd.ops_train")
dev = "cuda:0"; BF = torch.bfloat16
F, hw, bs, nh = 8, (32, 32), 2, 32
def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
head_dims = [int(v) for v in _opt("--head-dim", "96").split(",")]
floor = "--floor" in sys.argv
if "--cfg4" in sys.argv:   # 512^2, 16 frames, bs 1: L = 31 806 (mask from token attributes: the dense form is 1 GB)
    LY = importlib.import_module("video-gpt_amd.layout")
    F, N4 = 16, 1024
    kinds, _ = P.plan_stage1(2 * F - 1)
    B, L = 1, (2 * F - 1) * (N4 + 2)
    pm = LY.TokenLayout.from_plans([(kinds, N4 + 2, 0)], L).packed_mask(dev)
else:
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12))
    rows = []
    for _ in range(bs):
        prompt = "".join(f"<|diffusion|><|image_{i + 1}|><img><|image_{i + 1}|></img>" if i < F - 1 else f"<|diffusion|><|image_{i + 1}|>" for i in range(F))
        rows.append(proc.process_multi_modal_prompt_training(prompt, [torch.zeros(3, 256, 256) for _ in range(F)]))
    batch = proc.collator.collate_stage1(rows, F)
    mask = batch["attention_mask"].to(dev)
    B, L = mask.shape[:2]
    pm = ops.pack_mask(mask)
summ = pm.summary.cpu()
print("B", B, "L", L, "active (128-row block, 64-key tile) pairs per batch item:", int((summ != 0).sum()) // B, "of", summ[0].numel())
def timeit(f, n=10):
    for _ in range(2): f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3
def sdpa_bwd_us(qkv, dout, hd):
    """torch's SDPA autograd backward alone (the forward's graph is kept), on the additive mask the reference builds."""
    add = torch.zeros(B, 1, L, L, dtype=BF, device=dev).masked_fill_(~mask[:, None], float("-inf"))
    q, k, v = (t.reshape(B, L, nh, hd).transpose(1, 2).detach().requires_grad_() for t in qkv.split(nh * hd, -1))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=add)
    do = dout.view(B, L, nh, hd).transpose(1, 2)
    return timeit(lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True), n=5)
rows = {}
for hd in head_dims:
    qkv = torch.randn(B, L, 3 * nh * hd, device=dev).to(BF)
    out = torch.empty(B, L, nh * hd, dtype=BF, device=dev); lse = torch.empty(B, nh, L, dtype=torch.float32, device=dev)
    dout = torch.randn(B, L, nh * hd, device=dev).to(BF); dqkv = torch.empty_like(qkv); delta = torch.empty_like(lse)
    if len(head_dims) > 1 or floor: print("head_dim", hd)
    print("fwd us", timeit(lambda: T.attention_qkv_train(qkv, pm, nh, nh, hd, out, lse)))
    bwd = timeit(lambda: T.attention_qkv_bwd(qkv, out, dout, lse, delta, dqkv, pm, nh, nh, hd))
    print("bwd (delta + dQ + dV + dK) us", bwd)
    if floor:
        flops = 10.0 * hd * nh * float(mask.sum())
        rows[hd] = (bwd, flops / bwd * 1e-6, sdpa_bwd_us(qkv, dout, hd))
if floor:
    base = rows.get(96)
    for hd, (bwd, tf, ref) in rows.items():
        rel = f"{tf / base[1]:.3f}" if base else "n/a"
        print(f"head_dim {hd}: bwd {bwd:.1f} us = {tf:.1f} TFLOP/s ({rel} of head dim 96) | torch SDPA backward (floor) {ref:.1f} us "
              f"| floor / bwd {ref / bwd:.2f} {'ok' if bwd <= ref else 'MISSES THE FLOOR'}")
