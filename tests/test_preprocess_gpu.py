"""Decoded uint8 frames through the device path vs the host Pillow path, bit for bit: LVMProcessor.process_frames against
stacked process_image(PIL frame) at one size per branch of crop_arr, center_crop_frames against a Pillow restatement of
center_crop_arr, LVMPipeline.encode_frames against the existing encode path on the Pillow-processed tensors, and one sampled
round fed with preprocess_frames against the same round fed with PIL images."""
import importlib

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import restate as R
from oracle import vae_ref as VR
from tests import smoke_case as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def P():
    return importlib.import_module("video-gpt_amd.processor")


def frames_u8(N, H, W, seed):
    """Smooth content plus noise plus saturated rows: real-frame statistics and the resampler's clamp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (127 + 120 * np.sin(xx / 7.0 + seed) * np.cos(yy / 5.0))[None, :, :, None]
    x = np.clip(base + rng.normal(0, 40, (N, H, W, 3)), 0, 255).astype(np.uint8)
    x[:, ::5] = rng.integers(0, 2, (N, H, W, 3), dtype=np.uint8)[:, ::5] * 255
    return x


# (W, H, max_image_size, output (w, h)): one case per branch of crop_arr
BRANCHES = [(70, 52, 1024, (64, 48)),      # crop only
            (64, 64, 1024, (64, 64)),      # nothing to do
            (300, 260, 64, (64, 48)),      # two BOX halvings -> 75x65, BICUBIC -> 64x55, crop
            (40, 9, 1024, (64, 16)),       # enlarge to 71x16, crop
            (129, 70, 64, (64, 32)),       # BICUBIC shrink -> 64x35, crop
            (129, 140, 64, (48, 64))]      # an odd side halved (129 // 2) -> 64x70, BICUBIC -> 59x64, crop


@pytest.mark.parametrize("W,H,max_size,out", BRANCHES, ids=[f"{c[0]}x{c[1]}-max{c[2]}" for c in BRANCHES])
def test_process_frames_equals_process_image(P, W, H, max_size, out):
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12), max_image_size=max_size)
    x = frames_u8(3, H, W, W + H)
    want = torch.stack([proc.process_image(Image.fromarray(f)) for f in x])
    assert tuple(want.shape) == (3, 3, out[1], out[0])
    xd = torch.from_numpy(x).to(DEV)
    got = proc.process_frames(xd)
    assert got.dtype == torch.float32 and got.is_cuda and torch.equal(got.cpu(), want)
    assert torch.equal(proc.process_frames([xd[i] for i in range(3)]), got)          # a list of (H, W, 3) frames
    assert torch.equal(proc.process_frames(xd[1:2]), got[1:2])                        # one frame, an odd base address


def test_process_frames_refuses_other_inputs(P):
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12))
    ops = importlib.import_module("video-gpt_amd.ops")
    with pytest.raises(ValueError):
        proc.process_frames(torch.zeros(2, 32, 32, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        proc.process_frames(torch.zeros(2, 32, 32, 3, device=DEV))
    with pytest.raises(ValueError):
        proc.process_frames([torch.zeros(32, 32, 3, dtype=torch.uint8, device=DEV), torch.zeros(32, 48, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(ops.VgptError, match="GPU tensor"):
        proc.process_frames(torch.zeros(2, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ops.VgptError, match="contiguous"):
        proc.process_frames(torch.zeros(2, 32, 3, 32, dtype=torch.uint8, device=DEV).permute(0, 1, 3, 2))


def _pil_center_crop(img, image_size):
    """LVM/utils.py:47-66 restated."""
    while min(*img.size) >= 2 * image_size:
        img = img.resize(tuple(x // 2 for x in img.size), resample=Image.BOX)
    scale = image_size / min(*img.size)
    img = img.resize(tuple(round(x * scale) for x in img.size), resample=Image.BICUBIC)
    arr = np.array(img)
    cy, cx = (arr.shape[0] - image_size) // 2, (arr.shape[1] - image_size) // 2
    return arr[cy: cy + image_size, cx: cx + image_size]


@pytest.mark.parametrize("W,H,size", [(150, 90, 32), (31, 90, 16), (64, 64, 64), (20, 30, 48), (257, 129, 64)])
def test_center_crop_frames_equals_pillow(P, W, H, size):
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12))
    x = frames_u8(2, H, W, 3 * W + H)
    arr = np.stack([_pil_center_crop(Image.fromarray(f), size) for f in x])
    want = (torch.from_numpy(arr).permute(0, 3, 1, 2).float().div(255.0) - 0.5) / 0.5
    got = proc.center_crop_frames(torch.from_numpy(x).to(DEV), size)
    assert tuple(got.shape) == (2, 3, size, size) and torch.equal(got.cpu(), want)


@pytest.fixture(scope="module")
def pipe():
    cfg, vcfg = R.TINY, VR.TINY_VAE8
    p = {k: v.to(BF).float() for k, v in R.make_params(cfg, 0).items()}
    model = SC.build_product_model(cfg, p, DEV)
    V = importlib.import_module("video-gpt_amd.vae")
    vae = V.AutoencoderKL(block_out_channels=vcfg.block_out_channels, layers_per_block=vcfg.layers_per_block,
                          norm_num_groups=vcfg.norm_num_groups)
    vae.load_state_dict(VR.make_vae_params(vcfg, seed=2))
    vae = vae.to(DEV, torch.float32).eval()
    Pm = importlib.import_module("video-gpt_amd.processor")
    PL = importlib.import_module("video-gpt_amd.pipeline")
    return PL.LVMPipeline(vae, model, Pm.LVMProcessor(Pm.SpecialTokenizer(10, 11, 12)), device=DEV)


def test_encode_frames_equals_the_existing_path_on_pillow_tensors(pipe):
    x = frames_u8(3, 70, 70, 5)
    noise = [torch.randn(1, 4, 8, 8, generator=torch.Generator("cpu").manual_seed(20 + i)) for i in range(3)]
    got = pipe.encode_frames(torch.from_numpy(x).to(DEV), BF, noise=noise)
    host = [pipe.processor.process_image(Image.fromarray(f)).unsqueeze(0).to(DEV) for f in x]
    dists = pipe.vae_posteriors(host)
    want = [pipe.vae_encode(None, BF, noise[i].to(DEV), dist=d) for i, d in enumerate(dists)]
    assert len(got) == 3 and got[0].shape == (1, 4, 8, 8) and got[0].dtype == BF
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # without `noise` the samples are drawn per frame in the entry points' order: the same generator state gives the same latents
    torch.manual_seed(3)
    a = pipe.encode_frames(torch.from_numpy(x).to(DEV), BF)
    torch.manual_seed(3)
    b = [pipe.vae_encode(None, BF, None, dist=d) for d in pipe.vae_posteriors(host)]
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_sampled_round_from_device_frames_equals_the_round_from_pil_images(pipe):
    x = frames_u8(2, 70, 70, 9)
    vnoise = [torch.randn(1, 4, 8, 8, generator=torch.Generator("cpu").manual_seed(70 + i)) for i in range(2)]
    kw = dict(height=64, width=64, gen_nums=[2], num_inference_steps=1, use_img_guidance=True, img_guidance_scale=1.6, seed=4,
              output_type="pt", prediction_type="x1", generator_device="cpu", vae_noise=vnoise)
    frames = pipe.preprocess_frames(torch.from_numpy(x).to(DEV))
    assert len(frames) == 2 and frames[0].shape == (3, 64, 64) and frames[0].is_cuda
    out_dev = pipe.prompt_condition_frame_block_autoregressive_inference(input_images=frames, **kw)
    lat_dev, smp_dev = [t.clone() for t in pipe.last_latents], torch.cat(pipe.last_samples[0]).clone()
    out_pil = pipe.prompt_condition_frame_block_autoregressive_inference(input_images=[Image.fromarray(f) for f in x], **kw)
    assert len(out_dev) == len(out_pil) == 4
    for a, b in zip(lat_dev, pipe.last_latents):
        assert torch.equal(a, b)
    assert torch.equal(smp_dev, torch.cat(pipe.last_samples[0]))
    for a, b in zip(out_dev, out_pil):
        assert torch.equal(a, b)
