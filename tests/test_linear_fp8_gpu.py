"""MX-fp8 projections (video-gpt_amd/csrc/gemm_mx8.hip; the sampler's `linear_precision = "fp8"` option) through the C ABI
and the engine.

Tolerance, stated separately from the bf16 path:
  * the quantisers are checked byte for byte against a numpy model of the format (OCP e4m3, one E8M0 scale per 32 k,
    smallest e with amax 2^-e <= 448, round-to-nearest-even) in the record layout include/vgpt.h documents;
  * the GEMM against fp64 A_deq W_deq^T built from the kernel's own quantised bytes, same epilogue: rel-L2 <= 4e-3 and every
    element within 2^-6 relative (a few bf16 ulps) -- only the bf16 output rounding and the fp32 summation order separate them;
  * the GEMM against the unquantised fp64 product (unit-normal activations, N(0, 0.02) weights): rel-L2 <= 6e-2 (two e4m3
    roundings, ~3-4e-2 expected);
  * the sampler (tiny model, 3 Euler steps with CFG) against the fp32 oracle: rel-L2 <= 6e-2, as the fp8 attention option.
"""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    importlib.import_module("video-gpt_amd")
    return importlib.import_module("video-gpt_amd.ops")


def g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def e4m3_table():
    t = np.zeros(256, dtype=np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        if e == 15 and m == 7:
            v = np.nan
        t[b] = -v if s else v
    return t


TAB = e4m3_table()


def model_quantise(x):
    """numpy model of the format: x (rows, K) float64 (fp32-exact values) -> expected payload bytes (rows, K) and scale
    bytes (rows, K / 32)."""
    rows, K = x.shape
    blk = x.reshape(rows, K // 32, 32)
    amax = np.abs(blk).max(axis=-1)
    f, E = np.frexp(amax)
    e = np.where(f <= 0.875, E - 9, E - 8)
    e = np.clip(np.where(amax > 0, e, 0), -127, 127)
    y = blk * 2.0 ** (-e[..., None].astype(np.float64))
    pos = TAB[:127]                                  # non-negative finite values, ascending with the byte
    a = np.abs(y)
    idx = np.clip(np.searchsorted(pos, a), 1, 126)
    lo, hi = pos[idx - 1], pos[idx]
    pick_hi = (a - lo > hi - a) | ((a - lo == hi - a) & ((idx % 2) == 0))   # ties to the even mantissa
    byte = np.where(pick_hi, idx, idx - 1).astype(np.uint8)
    byte = np.where((y < 0) & (byte != 0), byte | 0x80, byte).astype(np.uint8)
    return byte.reshape(rows, K), (e + 127).astype(np.uint8)


def decode(rec, rows, K):
    """The record layout of include/vgpt.h -> (payload bytes (rows, K), scale bytes (rows, K / 32)); also checks the padding."""
    raw = rec.data.cpu().numpy()
    MG, KB = -(-rows // 32), -(-K // 64)
    npay = MG * KB * 2048
    pay = raw[:npay].reshape(MG, KB, 2, 2, 32, 16)            # g, kb, p, h, r, j -> (32 g + r, 64 kb + 32 p + 16 h + j)
    q = pay.transpose(0, 4, 1, 2, 3, 5).reshape(MG * 32, KB * 64)
    off = (npay + 255) // 256 * 256
    sc = raw[off:off + MG * KB * 64].reshape(MG, KB, 2, 32).transpose(0, 3, 1, 2).reshape(MG * 32, KB * 2)
    assert not q[rows:].any() and not q[:, K:].any()                        # padding: zero payload, scale 127
    assert (sc[rows:] == 127).all() and (sc[:, K // 32:] == 127).all()
    return q[:rows, :K], sc[:rows, :K // 32]


def dequant(q, s):
    return TAB[q] * np.repeat(2.0 ** (s.astype(np.float64) - 127), 32, axis=1)


def check_bytes(q, s, x):
    wq, ws = model_quantise(x)
    assert np.array_equal(s, ws)
    zero = TAB[wq] == 0          # a value that rounds to zero may keep its sign bit
    assert np.array_equal(q[~zero], wq[~zero]) and not (q[zero] & 0x7F).any()


def special_rows(M, K, seed):
    """Random rows with blocks of very different magnitudes, plus the format's corner cases."""
    mag = torch.logspace(-3, 2, K // 32)[torch.randperm(K // 32, generator=g(seed + 1))].repeat_interleave(32)
    x = torch.randn(M, K, generator=g(seed)) * mag
    x[0, :32] = 0                                         # all-zero block
    x[1, 32:64] = torch.randn(32, generator=g(seed + 2)) * 100
    x[1, 40] = 448.0 * 8                                  # amax exactly 448 2^3
    x[2, :32] = torch.randn(32, generator=g(seed + 3)) * 2e-5
    x[2, 5] = 1.0                                         # most of the block lands on e4m3 subnormals
    x[3, 64:96] = 2.0 ** -130                             # bf16 subnormal block (scale clamped to 2^-127)
    return x.to(BF)


def test_row_quantiser_bytes_and_rstd(ops):
    M, K = 70, 224                                        # ragged row group, K tail of 32 past the last 64-tile
    x = special_rows(M, K, 10)
    rec = ops.Mx8Tensor(M, K, DEV)
    rec.data.fill_(0xAB)                                  # every byte of the record is written
    rstd = torch.empty(M, dtype=torch.float32, device=DEV)
    ops.mx8_quantize_rows(x.to(DEV), rec, rstd, eps=1e-5)
    q, s = decode(rec, M, K)
    xf = x.float().numpy().astype(np.float64)
    check_bytes(q, s, xf)
    assert s[1, 1] == 127 + 3 and q[1, 40] == 0x7E        # 448 2^3 -> scale 2^3, payload 448
    assert not q[0, :32].any() and s[0, 0] == 127
    want = 1.0 / np.sqrt((xf ** 2).mean(axis=1) + 1e-5)
    np.testing.assert_allclose(rstd.cpu().numpy(), want, rtol=1e-5)


@pytest.mark.parametrize("with_gain", [False, True])
def test_weight_quantiser_bytes(ops, with_gain):
    N, K = 96, 192
    w = special_rows(N, K, 20)
    gain = (1 + 0.5 * torch.randn(K, generator=g(21))).to(BF) if with_gain else None
    rec = ops.mx8_quantize_weight(w.to(DEV), None if gain is None else gain.to(DEV))
    q, s = decode(rec, N, K)
    x = w.float().numpy()
    if gain is not None:
        x = x * gain.float().numpy()                      # fp32 product, rounded once to e4m3
    check_bytes(q, s, x.astype(np.float32).astype(np.float64))


def ulp_check(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = rel_l2(got, ref)
    scale = np.sqrt((ref ** 2).mean())
    worst = float((np.abs(got - ref) / np.maximum(np.abs(ref), scale)).max())   # in units of the output (or the row scale)
    return e, worst


def rope_ref(y, cos, sin, n_rot):
    """y (M, N) float64 already rounded to bf16: RoPE on the first n_rot heads of 96."""
    out = y.copy()
    for h in range(n_rot):
        a, b = y[:, 96 * h:96 * h + 48], y[:, 96 * h + 48:96 * h + 96]
        out[:, 96 * h:96 * h + 48] = a * cos - b * sin
        out[:, 96 * h + 48:96 * h + 96] = b * cos + a * sin
    return out


def bf(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).float().to(BF).double().numpy()


def run_epilogue(ops, epi, M, N, K, seed, rows=None):
    """Returns (kernel output rows, fp64 reference on the dequantised operands, fp64 reference on the unquantised ones)."""
    a = torch.randn(M, K, generator=g(seed)).to(BF)
    w = (0.02 * torch.randn(N, K, generator=g(seed + 1))).to(BF)
    ad, wd = a.to(DEV), w.to(DEV)
    a8 = ops.Mx8Tensor(M, K, DEV)
    rstd = torch.empty(M, dtype=torch.float32, device=DEV)
    ops.mx8_quantize_rows(ad, a8, rstd, eps=1e-5)
    w8 = ops.mx8_quantize_weight(wd)
    n_out = N // 2 if epi == "gated" else N
    out = torch.empty(M, n_out, dtype=BF, device=DEV)
    kw = {}
    resid = None
    if epi == "resid":
        resid = torch.randn(M, N, generator=g(seed + 2)).to(BF)
        out.copy_(resid.to(DEV))
        kw = dict(residual=out)                                       # in place, as the engine runs it
    elif epi in ("rope", "gated"):
        kw = dict(rstd=rstd)
    cos = sin = None
    if epi == "rope":
        ang = torch.rand(M, 48, generator=g(seed + 3)).double() * 6.3
        cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
        kw.update(cos=cos.to(DEV), sin=sin.to(DEV), n_rot_heads=N // 96 - 1, head_dim=96)
    ops.linear_mx8(a8, w8, out, epi, **kw)
    rows = np.arange(M) if rows is None else np.asarray(rows)
    qa, sa = decode(a8, M, K)
    qw, sw = decode(w8, N, K)
    ad_ = dequant(qa[rows], sa[rows])
    wd_ = dequant(qw, sw)
    af = a.float().numpy().astype(np.float64)[rows]
    wf = w.float().numpy().astype(np.float64)
    rs = rstd.cpu().numpy().astype(np.float64)[rows]

    def epilogue(p):
        if epi == "none":
            return p
        if epi == "resid":
            return p + resid.float().numpy().astype(np.float64)[rows]
        p = p * rs[:, None]
        if epi == "rope":
            return rope_ref(bf(p), cos.numpy().astype(np.float64)[rows], sin.numpy().astype(np.float64)[rows], N // 96 - 1)
        gt, up = bf(p[:, :N // 2]), bf(p[:, N // 2:])
        return gt / (1 + np.exp(-gt)) * up
    got = out.float().cpu().numpy().astype(np.float64)[rows]
    return got, epilogue(ad_ @ wd_.T), epilogue(af @ wf.T)


SHAPES = [(70, 576, 192, "rope"), (70, 192, 192, "resid"), (70, 1024, 192, "gated"), (70, 192, 512, "resid"), (70, 256, 224, "none"),
          (4128, 9216, 3072, "rope"), (4128, 3072, 3072, "resid"), (4128, 16384, 3072, "gated"), (4128, 3072, 8192, "resid")]


@pytest.mark.parametrize("M,N,K,epi", SHAPES)
def test_gemm_against_dequantised_and_exact(ops, M, N, K, epi):
    rows = None if M < 1000 else np.r_[0:96, 2000:2032, 4064:4128]      # fp64 references on a row sample at full width
    got, deq, exact = run_epilogue(ops, epi, M, N, K, seed=M + N + K, rows=rows)
    e_deq, worst = ulp_check(got, deq)
    e_ex = rel_l2(got, exact)
    print(f"mx8 GEMM {epi} M={M} N={N} K={K}: rel-L2 vs dequantised {e_deq:.2e} (worst elem {worst:.2e} rel), vs exact {e_ex:.3e}")
    assert np.isfinite(got).all()
    assert e_deq <= 4e-3 and worst <= 2.0 ** -6
    assert e_ex <= 6e-2


@pytest.mark.parametrize("epi", ["none", "resid", "rope", "gated"])
def test_rows_do_not_depend_on_m_or_tile(ops, epi):
    """Rows [0, 256) and [4096, 4128) of an M = 4128 call equal, bit for bit, the same rows computed by M = 256 and M = 32 calls."""
    M, N, K = 4128, 576 if epi == "rope" else 1024, 3072
    a = torch.randn(M, K, generator=g(5)).to(BF).to(DEV)
    w = (0.02 * torch.randn(N, K, generator=g(6))).to(BF).to(DEV)
    w8 = ops.mx8_quantize_weight(w)
    resid = torch.randn(M, N, generator=g(7)).to(BF).to(DEV)
    ang = torch.rand(M, 48, generator=g(8)) * 6.3
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)

    def call(r0, r1):
        m = r1 - r0
        a8 = ops.Mx8Tensor(m, K, DEV)
        rstd = torch.empty(m, dtype=torch.float32, device=DEV)
        ops.mx8_quantize_rows(a[r0:r1].contiguous(), a8, rstd)
        out = torch.empty(m, N // 2 if epi == "gated" else N, dtype=BF, device=DEV)
        kw = {}
        if epi == "resid":
            out.copy_(resid[r0:r1])
            kw = dict(residual=out)
        elif epi == "gated":
            kw = dict(rstd=rstd)
        elif epi == "rope":
            kw = dict(rstd=rstd, cos=cos[r0:r1].contiguous(), sin=sin[r0:r1].contiguous(), n_rot_heads=4)
        return ops.linear_mx8(a8, w8, out, epi, **kw)
    full = call(0, M)
    assert torch.equal(full[:256], call(0, 256))
    assert torch.equal(full[4096:], call(4096, M))


def _sample(ops, lin, attn, mode, use_graph=True, model=None, cache=False):
    from tests import smoke_case as SC
    from oracle import restate as R
    S = importlib.import_module("video-gpt_amd.scheduler")
    P = importlib.import_module("video-gpt_amd.processor")
    LY = importlib.import_module("video-gpt_amd.layout")
    cfg, steps, C, G, hw = R.TINY, 3, 2, 2, (16, 16)
    bl = (hw[0] // 2) * (hw[1] // 2) + 2
    p, batch, z, cond = SC.build_case(cfg, C=C, G=G, hw=hw, use_cfg=True)
    lay = LY.TokenLayout.from_plans([(P.plan_inference([C, G])[0], bl, 0), (P.plan_inference([0, G])[0], bl, C * bl)], (C + G) * bl)
    if model is None:
        model = SC.build_product_model(cfg, p, DEV)
    sched = S.LVMScheduler(num_steps=steps)
    sched.reuse_condition_prefix = sched.hoist_special_rows = mode == "hoist"
    sched.attention_precision, sched.linear_precision = attn, lin
    sched.use_graph = use_graph
    sched.cache_engines = cache
    kw = SC.model_kwargs(batch, cond, DEV, use_cfg=True)
    kw["attention_mask"] = lay
    out = torch.cat(sched([x.to(DEV, BF) for x in z], model.frame_block_forward_with_cfg, kw, prediction_type="x1"))
    return out, sched, (cfg, p, batch, z, cond, steps, model)


@pytest.mark.parametrize("mode", ["hoist", "none"])
@pytest.mark.parametrize("attn", ["bf16", "fp8"])
def test_sampler_with_fp8_projections(ops, mode, attn):
    """Tiny model, 3 Euler steps with CFG: the fp8-projection sampler against the fp32 oracle and the bf16 engine; graph
    replay equals eager launches bit for bit."""
    from tests import smoke_case as SC
    out8, sched, (cfg, p, batch, z, cond, steps, _) = _sample(ops, "fp8", attn, mode)
    eng = sched.last_engine
    assert eng.lin_fp8 and eng.mx8 is not None and eng.fuse is None and eng.attn_fp8 == (attn == "fp8")
    eager, _, _ = _sample(ops, "fp8", attn, mode, use_graph=False)
    assert torch.equal(out8, eager)
    out16, sched16, _ = _sample(ops, "bf16", attn, mode)
    assert not sched16.last_engine.lin_fp8
    ref = torch.cat(SC.oracle_sample(cfg, p, batch, z, cond, steps, "x1", use_cfg=True))
    e_ref, e_bf = rel_l2(out8, ref), rel_l2(out8, out16)
    print(f"sampler with fp8 projections ({mode}, attention {attn}): rel-L2 vs oracle {e_ref:.3e}, vs bf16-projection engine "
          f"{e_bf:.3e}; bf16 engine vs oracle {rel_l2(out16, ref):.3e}")
    assert torch.isfinite(out8).all() and not torch.equal(out8, out16)
    assert e_ref < 6e-2


@pytest.mark.parametrize("update", ["load_state_dict", "in_place_step"])
def test_cached_engine_requantises_updated_weights(ops, update):
    """Sample, update the model's parameters in place, sample the same layout again with the engine cache on (the engine is
    re-bound, not rebuilt): the result equals a fresh engine on the updated model bit for bit."""
    from oracle import restate as R
    _, sched, (cfg, p, batch, z, cond, steps, model) = _sample(ops, "fp8", "bf16", "hoist", cache=True)
    first = sched.last_engine
    with torch.no_grad():
        if update == "load_state_dict":
            other = {k: v.to(BF).float() for k, v in R.make_params(cfg, 3).items()}
            model.load_state_dict(other)
        else:                              # what an optimizer step does: every parameter (norm gains included) moves in place
            for i, prm in enumerate(model.parameters()):
                prm.add_(0.05 * torch.randn(prm.shape, generator=g(100 + i)).to(prm.device, prm.dtype))
    again, sched2, _ = _sample(ops, "fp8", "bf16", "hoist", model=model, cache=True)
    assert sched2.last_engine_reused and sched2.last_engine is first
    fresh, sched3, _ = _sample(ops, "fp8", "bf16", "hoist", model=model, cache=False)
    assert sched3.last_engine is not first
    assert torch.equal(again, fresh)


def test_scheduler_refuses_fp8_projections_off_the_fast_path(ops):
    S = importlib.import_module("video-gpt_amd.scheduler")
    sched = S.LVMScheduler(num_steps=2)
    sched.linear_precision = "fp8"
    z = torch.zeros(2, 4, 8, 8, device=DEV, dtype=BF)
    with pytest.raises(Exception, match="linear_precision"):
        sched(z, lambda *a, **k: (z, None), {})


def test_fp8_projections_at_full_width():
    """cfg-2 geometry, two full-width decoder layers, 3 Euler steps: the fp8-projection sampler against the bf16 one on the
    same noise: one step's prediction within rel-L2 1e-1, the 3-step latents within 1.5e-1; graph replay equals eager."""
    import bench
    from tests import test_fullsize_gpu as F
    mods = {n: importlib.import_module(f"video-gpt_amd.{n}") for n in ["model", "processor", "engine", "scheduler", "ops"]}
    M, P = mods["model"], mods["processor"]
    cfg = bench.full_config(M, 2)
    model = bench.build_model(M, cfg, torch.device(DEV), seed=0)
    C, G, hw = 4, 8, (32, 32)
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12))
    prompt = "".join(f"<img><|image_{i + 1}|></img>" if i < C else f"<|diffusion|><|image_{i + 1}|>" for i in range(C + G))
    prompt_ = "".join(f"<|diffusion|><|image_{i + 1}|>" for i in range(G))
    batch = proc.prompt_condition_frame_block_inference([prompt, prompt_], [[torch.zeros(3, 256, 256)] * C, []], height=256,
                                                        width=256, use_img_cfg=True, frame_blocks=[C, G])
    gz = torch.Generator("cpu").manual_seed(7)
    z = [torch.randn(1, 4, *hw, generator=gz).to(DEV, BF) for _ in range(G)] * 2
    cond = [torch.randn(1, 4, *hw, generator=gz).to(DEV, BF) for _ in range(C)]
    cfg2 = (cfg, model, batch, z, cond, hw)
    preds = {}
    for prec in ("bf16", "fp8"):     # one step: the model's prediction of every frame (the output of the 2-layer forward)
        e = F._engine(mods, cfg2, reuse_condition_prefix=True, linear_precision=prec)
        _one = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(_one):
            e.run(1, use_graph=False)
        _one.synchronize()
        preds[prec] = e.pred.clone()
        del e
    ref = F._run(F._engine(mods, cfg2, reuse_condition_prefix=True), use_graph=False)
    e8 = F._engine(mods, cfg2, reuse_condition_prefix=True, linear_precision="fp8")
    assert e8.lin_fp8
    out8 = F._run(e8, use_graph=False)
    assert torch.equal(F._run(F._engine(mods, cfg2, reuse_condition_prefix=True, linear_precision="fp8"), use_graph=True), out8)
    e_step, rel = rel_l2(preds["fp8"], preds["bf16"]), rel_l2(out8, ref)
    print(f"fp8 projections vs bf16 at full width (2 layers): one step's prediction rel-L2 {e_step:.3e}; latents after 3 Euler "
          f"steps with CFG 1.6 rel-L2 {rel:.3e}")
    # measured 7.5e-2 / 9.0e-2: above the 6e-2 of a single projection -- the per-projection errors against the exact
    # product (2.8-5.4e-2, test_gemm_against_dequantised_and_exact) compound over four projections x two random-init layers,
    # and the latents carry three steps of it through the CFG combination u + 1.6 (c - u)
    assert torch.isfinite(out8).all() and 0 < e_step < 1e-1
    assert rel < 1.5e-1


def test_pipeline_chained_rounds_with_fp8_projections():
    """LVMPipeline with linear_precision = "fp8": chained rounds on the tiny model; the later rounds present the same
    sequence, so the scheduler re-binds the cached engine (weights re-quantised by its per-clip setup)."""
    from oracle import restate as R
    from oracle import vae_ref as VR
    from tests import smoke_case as SC
    PL = importlib.import_module("video-gpt_amd.pipeline")
    P = importlib.import_module("video-gpt_amd.processor")
    S = importlib.import_module("video-gpt_amd.scheduler")
    V = importlib.import_module("video-gpt_amd.vae")
    cfg, vcfg = R.TINY, VR.TINY_VAE8
    p = {k: v.to(BF).float() for k, v in R.make_params(cfg, 0).items()}
    model = SC.build_product_model(cfg, p, DEV)
    vae = V.AutoencoderKL(block_out_channels=vcfg.block_out_channels, layers_per_block=vcfg.layers_per_block,
                          norm_num_groups=vcfg.norm_num_groups)
    vae.load_state_dict(VR.make_vae_params(vcfg, seed=2))
    pipe = PL.LVMPipeline(vae.to(DEV, torch.float32).eval(), model, P.LVMProcessor(P.SpecialTokenizer(10, 11, 12)), device=DEV)
    px = 128
    gv = torch.Generator("cpu").manual_seed(300)
    frames = [torch.rand(3, px, px, generator=gv) * 2 - 1 for _ in range(2)]
    vnoise = [torch.randn(1, 4, px // 8, px // 8, generator=gv) for _ in range(2 + 4 + 4)]
    rnoise = [torch.randn(1, 4, px // 8, px // 8, generator=gv) for _ in range(4 + 4)]
    rec = []

    class Recording(S.LVMScheduler):
        def __call__(self, z, func, model_kwargs, **kw):
            out = super().__call__(z, func, model_kwargs, **kw)
            rec.append((self.linear_precision, self.last_engine, self.last_engine_reused, torch.cat(out).clone()))
            return out
    orig = PL.LVMScheduler
    PL.LVMScheduler = Recording
    try:
        outs = {}
        for prec in ("bf16", "fp8"):
            pipe.linear_precision = prec
            outs[prec] = pipe.prompt_condition_frame_block_autoregressive_inference(
                input_images=frames, height=px, width=px, gen_nums=[2, 2, 2], num_inference_steps=2, use_img_guidance=True,
                img_guidance_scale=1.6, seed=11, output_type="pt", prediction_type="x1", clean_image_noise_level=0.1,
                max_frame_window=6, generator_device="cpu", vae_noise=vnoise, renoise_noise=rnoise)
    finally:
        PL.LVMScheduler = orig
        pipe.linear_precision = "bf16"
    r16, r8 = rec[:3], rec[3:]
    assert all(r[0] == "fp8" and r[1].lin_fp8 for r in r8) and not any(r[1].lin_fp8 for r in r16)
    assert r8[2][2] and r8[2][1] is r8[1][1]                          # the slid window re-binds the cached engine
    for (_, _, _, a), (_, _, _, b) in zip(r16, r8):
        assert torch.isfinite(b).all()
    e0 = rel_l2(r8[0][3], r16[0][3])
    print(f"pipeline round 0 latents, fp8 projections vs bf16: rel-L2 {e0:.3e}")
    assert 0 < e0 < 6e-2
    assert len(outs["fp8"]) == 2 + 6
