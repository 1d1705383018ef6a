"""AutoencoderKL.attention_impl (video-gpt_amd/vae.py): the fused mid-block attention (ops.vae_attention, no score matrix)
against the materialised path (conv2d -> col_softmax -> conv2d) and against the CPU oracle, the `auto` rule on both sides
of HW = 4096, the memory the fused path allocates, and graph capture.

Tiny model: oracle.vae_ref.TINY_VAE = block_out_channels (32, 64), one layer per block, 8 groups: a mid-block of C = 64 at
half the image resolution.  Tolerances are those of tests/test_vae_gpu.py: rel-L2 2e-5 for one stage, 5e-4 against the
oracle through the whole encoder / decoder, uint8 images at most one level apart."""
import importlib

import pytest
import torch

from oracle import vae_ref as VR
from tests.test_train_kernels_gpu import _within
from tests.test_vae_attn_kernels_gpu import attn_ref_and_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = VR.TINY_VAE


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _vae(precision="fp32", impl="auto", cfg=CFG, params=None):
    V = importlib.import_module("video-gpt_amd.vae")
    vae = V.AutoencoderKL(block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
                          norm_num_groups=cfg.norm_num_groups, scaling_factor=cfg.scaling_factor,
                          shift_factor=cfg.shift_factor)
    vae.load_state_dict(VR.make_vae_params(cfg, seed=1) if params is None else params, strict=True)
    vae = vae.to(DEV, torch.float32).eval()
    vae.conv_precision, vae.attention_impl = precision, impl
    return vae


def _with(vae, impl, fn):
    vae.attention_impl = impl
    return fn()


# ---- 1. fused against materialised ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("h,w", [(4, 4), (5, 5), (22, 40)])
def test_fused_matches_materialised(precision, h, w):
    """Latent h x w = the mid-block's HW (16, 25: one ragged key tile and an odd ld; 880: the 176 x 320 frame).  Measured
    (MEASURE lines, profiles/vae_attn_tests.log): rel-L2 at most 4.5e-7 / 8.9e-7 (encode / decode) in fp32 and 2.5e-6 /
    6.9e-6 in bf16x3; uint8 pixels one level apart: 2.8e-4 of them at 22 x 40 in bf16x3, none in the other five cases."""
    vae = _vae(precision)
    x = torch.randn(2, 3, 2 * h, 2 * w, generator=g(30)).clamp(-1, 1).to(DEV)
    z = torch.randn(2, 4, h, w, generator=g(31)).to(DEV)
    mom = {i: _with(vae, i, lambda: vae.encode(x).latent_dist.parameters) for i in ("materialised", "fused")}
    img = {i: _with(vae, i, lambda: vae.decode(z).sample) for i in ("materialised", "fused")}
    u8 = {i: _with(vae, i, lambda: vae.decode_to_uint8(z * CFG.scaling_factor)) for i in ("materialised", "fused")}
    e_enc, e_dec = rel_l2(mom["fused"], mom["materialised"]), rel_l2(img["fused"], img["materialised"])
    diff = (u8["fused"].int() - u8["materialised"].int()).abs()
    share = float((diff > 0).float().mean())
    print(f"MEASURE fused vs materialised {precision} {h}x{w}: rel-L2 encode {e_enc:.3g} decode {e_dec:.3g}, "
          f"uint8 pixels one level apart: {share:.3g}")
    assert e_enc <= 2e-5 and e_dec <= 2e-5
    assert int(diff.max()) <= 1 and share < 5e-3


# ---- 2. fused against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_fused_matches_oracle(precision):
    p = VR.make_vae_params(CFG, seed=1)
    vae = _vae(precision, "fused", params=p)
    x = torch.randn(2, 3, 16, 24, generator=g(20)).clamp(-1, 1)
    noise = torch.randn(2, 4, 8, 12, generator=g(21))
    mean, logvar = VR.encode_moments(p, CFG, x)
    assert rel_l2(vae.encode(x.to(DEV)).latent_dist.parameters, torch.cat([mean, logvar], 1)) < 5e-4
    z_ref = VR.vae_encode(p, CFG, x, noise)
    img_ref = VR.decode(p, CFG, z_ref / CFG.scaling_factor)
    img = vae.decode(z_ref.to(DEV) / CFG.scaling_factor).sample
    assert img.shape == img_ref.shape and rel_l2(img, img_ref) < 5e-4
    diff = (vae.decode_to_uint8(z_ref.to(DEV)).cpu().int() - VR.decode_to_uint8(p, CFG, z_ref).int()).abs()
    assert int(diff.max()) <= 1 and float((diff > 0).float().mean()) < 5e-3


# ---- 3. the default -------------------------------------------------------------------------------------------------
def test_auto_keeps_the_materialised_bits_up_to_4096_positions():
    vae = _vae("bf16x3")
    assert vae.attention_impl == "auto" and importlib.import_module("video-gpt_amd.vae").AutoencoderKL().attention_impl == "auto"
    z = torch.randn(1, 4, 64, 64, generator=g(40)).to(DEV)                       # HW = 4096, C = 64
    auto = vae.decode(z).sample
    assert torch.equal(auto, _with(vae, "materialised", lambda: vae.decode(z).sample))
    assert not torch.equal(auto, _with(vae, "fused", lambda: vae.decode(z).sample))


def test_auto_is_fused_above_4096_positions():
    vae = _vae("bf16x3")
    z = torch.randn(1, 4, 17, 241, generator=g(41)).to(DEV)                      # HW = 4097
    auto = vae.decode(z).sample
    assert torch.equal(auto, _with(vae, "fused", lambda: vae.decode(z).sample))
    assert not torch.equal(auto, _with(vae, "materialised", lambda: vae.decode(z).sample))


def test_fused_refuses_unsupported_channels_and_auto_does_not():
    VgptError = importlib.import_module("video-gpt_amd._lib").VgptError
    cfg = VR.VaeCfg(block_out_channels=(32, 96), layers_per_block=1, norm_num_groups=8)
    vae = _vae("fp32", "fused", cfg=cfg, params=VR.make_vae_params(cfg, seed=2))
    z = torch.randn(1, 4, 5, 5, generator=g(42)).to(DEV)
    with pytest.raises(VgptError, match="96"):
        vae.decode(z)
    with pytest.raises(VgptError, match="attention_impl"):
        _with(vae, "flash", lambda: vae.decode(z))
    assert torch.isfinite(_with(vae, "auto", lambda: vae.decode(z).sample)).all()


# ---- 4. memory ------------------------------------------------------------------------------------------------------
def test_fused_attention_allocates_no_score_matrix(ops):
    """C = 64, 96 x 96 positions, one image: the score matrix would be 9216^2 * 4 = 340 MB, an activation is 2.4 MB.  The
    fused run may allocate q, k, v, o, the statistics and the result, far under 64 MB (measured: 11.3 MiB).  64 sampled queries are held to the
    float64 bound of tests/test_vae_attn_kernels_gpu.py."""
    V = importlib.import_module("video-gpt_amd.vae")
    C, H, W, groups = 64, 96, 96, 8
    torch.manual_seed(50)
    att = V._Attention(C).to(DEV, torch.float32).eval()
    x = torch.randn(1, C, H, W, generator=g(51)).to(DEV)
    with torch.no_grad():
        att.run(x, groups, 1e-6, "fp32", "fused")                                 # warm-up: nothing lazy is left to allocate
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        y = att.run(x, groups, 1e-6, "fp32", "fused")
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - start
        print(f"MEASURE fused _Attention.run 64 x 96 x 96: peak allocation above the start {peak / 2 ** 20:.1f} MiB")
        assert peak < 64 * 2 ** 20
        gn = (ops.groupnorm_stats(x, groups, 1e-6), att.group_norm.weight, att.group_norm.bias, groups, 0)
        q, k, v = (ops.conv2d(x, m.weight, m.bias, ksize=1, gn=gn) for m in (att.to_q, att.to_k, att.to_v))
        o = ops.vae_attention(q, k, v, 1 / C ** 0.5)
        assert torch.equal(y, ops.conv2d(o, att.to_out[0].weight, att.to_out[0].bias, ksize=1, resid=x))
    pick = torch.randperm(H * W, generator=g(52))[:64].sort().values.to(DEV)
    ref, bound, eta = attn_ref_and_bound(q.view(1, C, -1), k.view(1, C, -1), v.view(1, C, -1), 1 / C ** 0.5, queries=pick)
    assert eta < 0.01
    _within(o.view(1, C, -1)[:, :, pick], ref, bound, "fused 64 x 9216, 64 sampled queries")


# ---- 5. graph capture -----------------------------------------------------------------------------------------------
def test_fused_attention_replays_from_a_graph():
    V = importlib.import_module("video-gpt_amd.vae")
    C, groups = 64, 8
    torch.manual_seed(60)
    att = V._Attention(C).to(DEV, torch.float32).eval()
    x = torch.randn(2, C, 5, 5, generator=g(61)).to(DEV)
    with torch.no_grad():
        eager = att.run(x, groups, 1e-6, "fp32", "fused").clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            att.run(x, groups, 1e-6, "fp32", "fused")
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                             # one stream: a single branch
            out = att.run(x, groups, 1e-6, "fp32", "fused")
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
