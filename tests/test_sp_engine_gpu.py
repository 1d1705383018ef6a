"""Ulysses sequence parallelism inside the sampler engine (LVMScheduler.sequence_parallel_engine, engine.StaticDenoiser
sharded form).  The pack / unpack kernels against torch index operations, byte for byte; then two spawned ranks over gloo
on the one GPU of the test box (as tests/test_sequence_parallel_gpu.py: RCCL refuses two ranks on one device, the
exchanges go through host memory) whose sharded samples must equal the SP=1 engine's BIT FOR BIT: rows of a GEMM do not
depend on M, every head's attention is computed by one rank over all rows with the same kernel, and the final-layer
outputs are exchanged, not recomputed."""
import importlib
import socket
import traceback

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import smoke_case as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
FULL2 = R.Phi3Cfg(hidden_size=3072, intermediate_size=8192, num_hidden_layers=2, num_attention_heads=32,
                  num_key_value_heads=32, vocab_size=64, pos_embed_max_size=24)


# ---- pack / unpack kernels ------------------------------------------------------------------------------------------

def _ref_pack(x, P, nq, nk, hd):
    rows = x.shape[0]
    q, k, v = x[:, :nq * hd], x[:, nq * hd:(nq + nk) * hd], x[:, (nq + nk) * hd:]
    cut = lambda t, n: t.view(rows, P, n // P * hd).permute(1, 0, 2)
    return torch.cat([cut(q, nq), cut(k, nk), cut(v, nk)], dim=2).contiguous()


@pytest.mark.parametrize("heads", [(32, 32), (2, 2), (32, 8)], ids=["32x96", "tiny-2x96", "gqa-32q8kv"])
@pytest.mark.parametrize("P", [1, 2, 4, 8])
@pytest.mark.parametrize("rows", [1, 37, 255, 1001, 3347])
def test_pack_unpack_match_torch_index_ops(P, heads, rows):
    ops = importlib.import_module("video-gpt_amd.ops")
    nq, nk = heads
    hd = 96
    if nq % P or nk % P:
        with pytest.raises(ops.VgptError, match="multiples of n_ranks"):
            ops.sp_pack_qkv(torch.zeros(rows, (nq + 2 * nk) * hd, dtype=BF, device=DEV), P, nq, nk, hd)
        return
    g = torch.Generator("cpu").manual_seed(rows * 31 + P)
    # arbitrary 16-bit patterns (NaN / Inf bit patterns included): the kernels must move bytes, not values
    bits = torch.randint(-32768, 32767, (rows, (nq + 2 * nk) * hd), generator=g, dtype=torch.int16)
    x = bits.to(DEV).view(BF)
    packed = ops.sp_pack_qkv(x, P, nq, nk, hd)
    torch.cuda.synchronize()
    assert packed.shape == (P, rows, (nq + 2 * nk) // P * hd)
    assert torch.equal(packed.view(torch.int16).cpu(), _ref_pack(bits, P, nq, nk, hd))
    # unpack: (P, rows, Dc) head blocks -> (rows, P Dc) in head order
    Dc = nq // P * hd
    blocks = torch.randint(-32768, 32767, (P, rows, Dc), generator=g, dtype=torch.int16)
    out = ops.sp_unpack_ctx(blocks.to(DEV).view(BF), P)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16).cpu(), blocks.permute(1, 0, 2).reshape(rows, P * Dc))
    # round trip on the q columns: the q part of every chunk, unpacked, is the q block of the input
    q_chunks = packed[:, :, :Dc].contiguous()
    back = ops.sp_unpack_ctx(q_chunks, P)
    torch.cuda.synchronize()
    assert torch.equal(back.view(torch.int16).cpu(), bits[:, :nq * hd])


def test_pack_unpack_round_trip_of_a_full_head_set():
    """unpack(pack(x)) == x when q, k and v carry the same head count (each chunk is then [q_j | k_j | v_j], and the three
    groups unpack back in order)."""
    ops = importlib.import_module("video-gpt_amd.ops")
    nq = nk = 4
    hd, P, rows = 96, 4, 517
    x = torch.randn(rows, 3 * nq * hd, device=DEV).to(BF)
    packed = ops.sp_pack_qkv(x, P, nq, nk, hd)                       # (P, rows, 3 hd)
    # regroup the chunks into three (P, rows, hd) block sets and unpack each
    parts = [ops.sp_unpack_ctx(packed[:, :, i * hd:(i + 1) * hd].contiguous(), P) for i in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(parts, dim=1), x)


def test_pack_unpack_refuse_bad_arguments():
    ops = importlib.import_module("video-gpt_amd.ops")
    x = torch.zeros(8, 3 * 2 * 96, dtype=BF, device=DEV)
    with pytest.raises(ops.VgptError, match="last dim"):
        ops.sp_pack_qkv(x, 2, 2, 4, 96)
    with pytest.raises(ops.VgptError, match="dtype"):
        ops.sp_pack_qkv(x.float(), 2, 2, 2, 96)
    with pytest.raises(ops.VgptError, match="out is"):
        ops.sp_pack_qkv(x, 2, 2, 2, 96, out=torch.empty(7, 3 * 2 * 96, dtype=BF, device=DEV))
    with pytest.raises(ops.VgptError, match="out is"):          # right element count, wrong shape
        ops.sp_pack_qkv(x, 2, 2, 2, 96, out=torch.empty(8, 3 * 2 * 96, dtype=BF, device=DEV))
    with pytest.raises(ops.VgptError, match="are not"):         # (1, 5, 16) must not be read as (2, 2, 16)
        ops.sp_unpack_ctx(torch.zeros(1, 5, 16, dtype=BF, device=DEV), 2)
    with pytest.raises(ops.VgptError, match="are not"):
        ops.sp_unpack_ctx(torch.zeros(2 * 4, 16, dtype=BF, device=DEV), 2)
    with pytest.raises(ops.VgptError, match="multiple of 8"):
        ops.sp_unpack_ctx(torch.zeros(2, 4, 12, dtype=BF, device=DEV), 2)
    with pytest.raises(ops.VgptError, match="out"):
        ops.sp_unpack_ctx(torch.zeros(2, 4, 16, dtype=BF, device=DEV), 2, out=torch.empty(4, 16, dtype=BF, device=DEV))


# ---- two ranks ------------------------------------------------------------------------------------------------------

def _spawn(target, world=2, timeout=900):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    try:
        res = dict(q.get(timeout=timeout) for _ in procs)
    finally:
        for p_ in procs:
            p_.join(timeout=120)
            if p_.is_alive():
                p_.kill()
    for r in range(world):
        assert "error" not in res[r], f"rank {r} failed:\n{res[r]['error']}"
    for p_ in procs:
        assert p_.exitcode == 0
    return [res[r] for r in range(world)]


def _init(rank, world, port):
    import os
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    importlib.import_module("video-gpt_amd")
    return dist


def _sampler(case, model, sp, fuse=None, cache=False, lin="bf16", attn="bf16", **opts):
    S = importlib.import_module("video-gpt_amd.scheduler")
    sched = S.LVMScheduler(num_steps=case.steps, time_shifting_factor=1)
    sched.sequence_parallel_engine, sched.fuse_norms, sched.cache_engines = sp, fuse, cache
    sched.attention_precision, sched.linear_precision = attn, lin
    for k, v in opts.items():       # hoist_special_rows, reuse_condition_prefix
        setattr(sched, k, v)
    kw = SC.model_kwargs(case.batch, case.cond, DEV)
    kw["attention_mask"] = case.lay
    out = torch.cat(sched([t.to(DEV, BF) for t in case.z], model.frame_block_forward_with_cfg, kw, prediction_type="x1"))
    torch.cuda.synchronize()
    return out.float().cpu().numpy(), sched


def _shard_facts(eng, cfg):
    sp = eng.sp
    M = eng.L - eng.S
    cut = sp["cut"]
    bound = -(-(-(-M // 2)) // cut) * cut
    return {"width": int(eng.qkv_full.shape[-1]), "want_width": 3 * (cfg.num_attention_heads // 2) * cfg.head_dim,
            "m": sp["m"], "bound": bound, "M": M, "fused": eng.fuse is not None, "hoist": bool(eng.hoist), "S": eng.S,
            "parts": _norm_parts(sp["m"], cfg)}


def _norm_parts(M, cfg):
    """Partial sums of squares per row the folded-norm GEMMs (o_proj, down_proj: N = H) leave at M rows -- 2 x the number
    of tile columns, i.e. the tile width they pick -- read off the workspace size (csrc/gemm_bf16.hip norm_partials);
    0: no folded form at this M."""
    ops = importlib.import_module("video-gpt_amd.ops")
    H = cfg.hidden_size
    cnt = (-(-M // 256) * 4 + 255) // 256 * 256
    out = []
    for K in (cfg.num_attention_heads * cfg.head_dim, cfg.intermediate_size):
        b = ops.norm_workspace_bytes(M, H, K)
        out.append(0 if b == 0 else (b - cnt) // (4 * M))
    return tuple(out)


def _same_or_within(a, b, same_form, what):
    """Bit for bit when shard and whole run the same norm form at the same tile widths; otherwise within the forward
    tolerance: the folded norm's 1/rms sums one partial per tile column, the tile width follows M, and a share with fewer
    than 128 output tiles does not fold at all (it runs the separate RMSNorm kernel)."""
    if same_form:
        assert np.array_equal(a, b), f"{what}: same norm form and tile widths, yet rel-L2 " \
                                     f"{SC.rel_l2(torch.from_numpy(a), torch.from_numpy(b)):.3e}"
        return 0.0
    err = SC.rel_l2(torch.from_numpy(a), torch.from_numpy(b))
    print(f"{what}: other norm form / tile width than SP=1, rel-L2 {err:.3e}")
    assert err < SC.tol("forward_latents")
    return err


def _tiny_worker(rank, world, port, q):
    res = {}
    try:
        dist = _init(rank, world, port)
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        E = importlib.import_module("video-gpt_amd.engine")
        ops = importlib.import_module("video-gpt_amd.ops")
        WU = importlib.import_module("tests.test_weight_updates_gpu")
        cfg = R.TINY
        case = WU.Case(cfg, C=2, G=2, hw=(16, 16), steps=3)
        model = SC.build_product_model(cfg, case.p, DEV)
        # today's engine, before any sequence-parallel group exists (SP = 1)
        res["base_default"], s = _sampler(case, model, False)
        res["base_fused"] = s.last_engine.fuse is not None     # the folded norms exist at full width only (H = 192: off)
        res["base_nofuse"], _ = _sampler(case, model, False, fuse=False)
        res["base_nohoist"], _ = _sampler(case, model, False, hoist_special_rows=False)
        res["base_noreuse"], _ = _sampler(case, model, False, reuse_condition_prefix=False)
        res["base_pipe"] = _pipeline(sp_engine=False)
        SPM.initialize_sequence_parallel_state(world)
        res["off"], s = _sampler(case, model, False)                 # option off under the group: replicated, unchanged
        res["off_sharded"] = s.last_engine.sp is not None
        res["nofuse"], s = _sampler(case, model, True, fuse=False)
        res["nofuse_facts"] = _shard_facts(s.last_engine, model.llm.config)
        res["default"], s = _sampler(case, model, True)
        res["default_facts"] = _shard_facts(s.last_engine, model.llm.config)
        res["nohoist"], s = _sampler(case, model, True, hoist_special_rows=False)       # sharded prefill()
        res["nohoist_facts"] = _shard_facts(s.last_engine, model.llm.config)
        res["noreuse"], s = _sampler(case, model, True, reuse_condition_prefix=False)   # every row live, S == 0
        res["noreuse_facts"] = _shard_facts(s.last_engine, model.llm.config)
        res["noreuse_layers"] = int(s.last_engine.qkv_full.shape[0])
        # engine cache: the second clip of the same layout reuses the sharded engine
        res["cache1"], s1 = _sampler(case, model, True, cache=True)
        res["cache2"], s2 = _sampler(case, model, True, cache=True)
        res["reused"] = bool(s2.last_engine_reused and s2.last_engine is s1.last_engine)
        # an in-place weight change the autograd counters do not see, announced by bump_weight_generation
        with torch.no_grad():
            for layer in model.llm.layers:
                for p_ in (layer.self_attn.qkv_proj.weight, layer.mlp.gate_up_proj.weight, layer.input_layernorm.weight,
                           layer.post_attention_layernorm.weight):
                    p_.data.copy_(p_.data.roll(1, dims=-1))
        E.bump_weight_generation(model)
        res["cache3"], s3 = _sampler(case, model, True, cache=True)
        res["reused3"] = bool(s3.last_engine_reused)
        fresh = SC.build_product_model(cfg, {k: v.detach().float().cpu() for k, v in model.state_dict().items()}, DEV)
        res["fresh3"], _ = _sampler(case, fresh, False)
        # refusals
        for name, kw in (("attn", dict(attn="fp8")), ("lin", dict(lin="fp8"))):
            try:
                _sampler(case, fresh, True, **kw)
                res[f"refuse_{name}"] = None
            except ops.VgptError as e_:
                res[f"refuse_{name}"] = str(e_)
        res["pipe"] = _pipeline(sp_engine=True)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


def _pipeline(sp_engine):
    """One round of the tiny LVMPipeline (tests/test_pipeline_gpu.py's case) with the SP=2 collator."""
    from oracle import vae_ref as VR
    cfg, vcfg = R.TINY, VR.TINY_VAE8
    p = {k: v.to(BF).float() for k, v in R.make_params(cfg, 0).items()}
    model = SC.build_product_model(cfg, p, DEV)
    V = importlib.import_module("video-gpt_amd.vae")
    vae = V.AutoencoderKL(block_out_channels=vcfg.block_out_channels, layers_per_block=vcfg.layers_per_block,
                          norm_num_groups=vcfg.norm_num_groups)
    vae.load_state_dict(VR.make_vae_params(vcfg, seed=2))
    vae = vae.to(DEV, torch.float32).eval()
    P = importlib.import_module("video-gpt_amd.processor")
    PL = importlib.import_module("video-gpt_amd.pipeline")
    pipe = PL.LVMPipeline(vae, model, P.LVMProcessor(P.SpecialTokenizer(10, 11, 12), sequence_parallel_size=2), device=DEV)
    pipe.sequence_parallel_engine = sp_engine
    frames = [torch.rand(3, 64, 64, generator=torch.Generator("cpu").manual_seed(50 + i)) * 2 - 1 for i in range(2)]
    vnoise = [torch.randn(1, 4, 8, 8, generator=torch.Generator("cpu").manual_seed(70 + i)) for i in range(2)]
    out = pipe.prompt_condition_frame_block_autoregressive_inference(
        input_images=frames, height=64, width=64, gen_nums=[2], num_inference_steps=2, use_img_guidance=True,
        img_guidance_scale=1.6, seed=42, output_type="pt", prediction_type="x1", generator_device="cpu", vae_noise=vnoise)
    torch.cuda.synchronize()
    return {"samples": torch.cat(pipe.last_samples[0]).float().cpu().numpy(),
            "images": np.stack([o.cpu().numpy() for o in out])}


@pytest.fixture(scope="module")
def tiny():
    return _spawn(_tiny_worker)


@pytest.mark.parametrize("mode", ["nofuse", "default"])
def test_tiny_sharded_sampler_equals_sp1_engine_bit_for_bit(tiny, mode):
    base = "base_nofuse" if mode == "nofuse" else "base_default"
    for r in range(2):
        assert np.array_equal(tiny[r][mode], tiny[r][base]), \
            f"rank {r}: rel-L2 {SC.rel_l2(torch.from_numpy(tiny[r][mode]), torch.from_numpy(tiny[r][base])):.3e}"
    assert np.array_equal(tiny[0][mode], tiny[1][mode])


@pytest.mark.parametrize("mode", ["nofuse", "default"])
def test_tiny_engine_really_shards(tiny, mode):
    for r in range(2):
        f = tiny[r][f"{mode}_facts"]
        assert f["width"] == f["want_width"]                 # qkv_full holds this rank's heads only
        assert f["m"] <= f["bound"] and f["hoist"]
        assert f["fused"] == (tiny[r]["base_fused"] if mode == "default" else False)
    assert tiny[0][f"{mode}_facts"]["m"] + tiny[1][f"{mode}_facts"]["m"] == tiny[0][f"{mode}_facts"]["M"]


@pytest.mark.parametrize("mode", ["nohoist", "noreuse"])
def test_tiny_sharded_prefill_and_uncached_layouts(tiny, mode):
    """nohoist: a static condition prefix computed once by the sharded prefill(), no special rows hoisted; noreuse: no
    cached prefix, every row computed at every step (one fused buffer for all layers)."""
    for r in range(2):
        f = tiny[r][f"{mode}_facts"]
        assert not f["hoist"] and f["width"] == f["want_width"] and f["m"] <= f["bound"]
        assert (f["S"] > 0) == (mode == "nohoist")
        assert np.array_equal(tiny[r][mode], tiny[r][f"base_{mode}"])
    assert tiny[0]["noreuse_layers"] == 1
    assert np.array_equal(tiny[0][mode], tiny[1][mode])


def test_option_off_keeps_the_replicated_engine(tiny):
    for r in range(2):
        assert not tiny[r]["off_sharded"]
        assert np.array_equal(tiny[r]["off"], tiny[r]["base_default"])


def test_engine_cache_and_weight_updates(tiny):
    for r in range(2):
        t = tiny[r]
        assert t["reused"] and t["reused3"]
        assert np.array_equal(t["cache1"], t["base_default"]) and np.array_equal(t["cache2"], t["base_default"])
        assert not np.array_equal(t["cache3"], t["base_default"])
        assert np.array_equal(t["cache3"], t["fresh3"])
    assert np.array_equal(tiny[0]["cache3"], tiny[1]["cache3"])


def test_fp8_options_are_refused_under_sp(tiny):
    for r in range(2):
        assert tiny[r]["refuse_attn"] is not None and "attention_precision" in tiny[r]["refuse_attn"]
        assert tiny[r]["refuse_lin"] is not None and "linear_precision" in tiny[r]["refuse_lin"]


def test_pipeline_with_sharded_engine_equals_sp1(tiny):
    for r in range(2):
        a, b = tiny[r]["pipe"], tiny[r]["base_pipe"]
        assert np.array_equal(a["samples"], b["samples"])
        assert np.array_equal(a["images"], b["images"])


# ---- full width -----------------------------------------------------------------------------------------------------

def _roll_folded_weights(model):
    """An in-place change of every parameter the folded copies derive from, invisible to autograd's version counters."""
    E = importlib.import_module("video-gpt_amd.engine")
    with torch.no_grad():
        for layer in model.llm.layers:
            for p_ in (layer.self_attn.qkv_proj.weight, layer.mlp.gate_up_proj.weight, layer.input_layernorm.weight,
                       layer.post_attention_layernorm.weight):
                p_.data.copy_(p_.data.roll(1, dims=-1))
    E.bump_weight_generation(model)


def _full_worker(rank, world, port, q):
    res = {}
    try:
        dist = _init(rank, world, port)
        torch.set_num_threads(8)
        SPM = importlib.import_module("video-gpt_amd.sequence_parallel")
        WU = importlib.import_module("tests.test_weight_updates_gpu")
        cfg8 = WU.Case(FULL2, C=4, G=8, hw=(32, 32), steps=2)       # cfg-2: 4096 live rows, 2048-row shares
        cfg12 = WU.Case(FULL2, C=4, G=12, hw=(32, 32), steps=2)     # 6144 live rows: 3072-row shares take the folded norms
        model = SC.build_product_model(FULL2, cfg8.p, DEV)
        lc = model.llm.config
        res["base_nofuse"], _ = _sampler(cfg8, model, False, fuse=False)
        res["base_default"], s = _sampler(cfg8, model, False)
        res["base_fused"], res["base_parts"] = s.last_engine.fuse is not None, _norm_parts(s.last_engine.Ma, lc)
        res["base12"], s = _sampler(cfg12, model, False)
        res["base12_fused"], res["base12_parts"] = s.last_engine.fuse is not None, _norm_parts(s.last_engine.Ma, lc)
        SPM.initialize_sequence_parallel_state(world)
        res["nofuse"], s = _sampler(cfg8, model, True, fuse=False)
        res["nofuse_facts"] = _shard_facts(s.last_engine, lc)
        res["default"], s = _sampler(cfg8, model, True)
        res["default_facts"] = _shard_facts(s.last_engine, lc)
        res["f12"], s1 = _sampler(cfg12, model, True, cache=True)
        res["f12_facts"] = _shard_facts(s1.last_engine, lc)
        # folded copies refilled on a cached sharded engine after a weight change autograd does not see
        _roll_folded_weights(model)
        res["f12u"], s2 = _sampler(cfg12, model, True, cache=True)
        res["f12u_reused"] = bool(s2.last_engine_reused and s2.last_engine is s1.last_engine)
        res["f12u_fused"] = s2.last_engine.fuse is not None
        res["f12_fresh"], s3 = _sampler(cfg12, model, True)                 # a new sharded engine on the new weights
        res["f12_fresh_new"] = s3.last_engine is not s1.last_engine
        res["base12u"], _ = _sampler(cfg12, model, False)                   # SP = 1 on the new weights
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        res = {"error": traceback.format_exc()}
    q.put((rank, res))


@pytest.fixture(scope="module")
def full():
    return _spawn(_full_worker, timeout=1500)


def test_full_width_sharded_sampler(full):
    for r in range(2):
        f = full[r]
        assert f["nofuse_facts"]["width"] == 3 * 16 * 96 and f["nofuse_facts"]["m"] <= f["nofuse_facts"]["bound"]
        # separate RMSNorm kernels: every GEMM row is independent of M, every head's attention is one rank's -> exact
        assert np.array_equal(f["nofuse"], f["base_nofuse"])
        # default options at cfg-2: the whole 4096 rows fold the norms, a 2048-row share (8 x 12 = 96 < 128 output
        # tiles) does not
        d = f["default_facts"]
        assert f["base_fused"] and not d["fused"]
        _same_or_within(f["default"], f["base_default"], d["parts"] == f["base_parts"], f"rank {r} cfg-2 defaults")
    for k in ("nofuse", "default"):
        assert np.array_equal(full[0][k], full[1][k])


def test_full_width_sharded_folded_norms(full):
    """6144 live rows: every rank's 3072-row share (12 x 12 = 144 output tiles) runs the folded RMSNorms --
    rms_rstd / linear_qkv_rope_prenorm / linear_resid_rstd / gated_mlp_act_prenorm on the share."""
    for r in range(2):
        f = full[r]
        d = f["f12_facts"]
        assert d["fused"] and f["base12_fused"] and d["m"] == 3072 and all(d["parts"])
        _same_or_within(f["f12"], f["base12"], d["parts"] == f["base12_parts"], f"rank {r} folded")
    assert np.array_equal(full[0]["f12"], full[1]["f12"])


def test_full_width_sharded_folded_norms_follow_weight_updates(full):
    """After an in-place change of the folded weights' sources + bump_weight_generation, the CACHED sharded engine refolds:
    it equals a freshly built sharded engine on the new weights bit for bit, and SP = 1 on them as the folded test does."""
    for r in range(2):
        f = full[r]
        assert f["f12u_reused"] and f["f12u_fused"] and f["f12_fresh_new"]
        assert not np.array_equal(f["f12u"], f["f12"])
        assert np.array_equal(f["f12u"], f["f12_fresh"])
        _same_or_within(f["f12u"], f["base12u"], f["f12_facts"]["parts"] == f["base12_parts"], f"rank {r} updated")
    assert np.array_equal(full[0]["f12u"], full[1]["f12u"])
