"""Developer probe (GPU): qkv_proj + RoPE at the sampler's shape (M = 4096, N = 9216, K = 3072, 32 + 32 + 32 heads of 96), with
and without the folded norm's rstd.  Prints the sha256 of both outputs on seeded inputs (bit identity between two builds) and
the time per call over a rotating set of weight matrices (weights from HBM, as in the sampler step).  VGPT_LIB selects another
build of the library for a same-box A/B run."""
import hashlib, importlib, sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
importlib.import_module("video-gpt_amd")
ops = importlib.import_module("video-gpt_amd.ops")
dev = "cuda:0"; BF = torch.bfloat16
M, N, K, H, HD, NW = 4096, 9216, 3072, 32, 96, 6
gen = torch.Generator(dev).manual_seed(1234)
x = torch.randn(M, K, device=dev, generator=gen).to(BF)
ws = [(torch.randn(N, K, device=dev, generator=gen) * 0.05).to(BF) for _ in range(NW)]
pos = torch.randperm(M, device=dev, generator=gen)
cos, sin = ops.rope_table(pos, ops.rope_inv_freq(HD, 10000.0, dev))
rstd = (torch.rand(M, device=dev, generator=gen) + 0.5).float()
y = torch.empty(M, N, dtype=BF, device=dev)
forms = (("rope", lambda i: ops.linear_qkv_rope(x, ws[i % NW], cos, sin, H, H, HD, out=y)),
         ("rope_prenorm", lambda i: ops.linear_qkv_rope_prenorm(x, ws[i % NW], cos, sin, rstd, H, H, HD, out=y)))
def timeit(f, n=30):
    for i in range(6): f(i)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n): f(i)
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3
out = []
for name, f in forms:
    y.fill_(float("nan")); f(0); torch.cuda.synchronize()
    sha = hashlib.sha256(y.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:16]
    out.append(f"{name} sha256 {sha} {timeit(f):6.1f} us")
print(os.environ.get("VGPT_LIB", "product")[-20:], " | ".join(out))
