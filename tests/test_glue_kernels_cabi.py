"""The entry points of csrc/glue.hip, csrc/norm_rope.hip and csrc/mask.hip without a GPU.

First the host-side refusals, read from the VGPT_REQUIRE lines: every call below either fails a check, with the documented
return code, the function's name and (where the message carries it) the offending value in vgpt_last_error(), or returns
VGPT_OK from the zero-size early return that follows validation.  The pointers are fake: a launch would fault.
vgpt_mask_count_empty_rows has no such early return to test, it clears its counter on the device first.

Then a CPU model of each kernel's rounding points (fp32 accumulation in the kernel's order: a chain per lane, the xor
butterfly across the 64 lanes; bf16 roundings where the kernel rounds), run on the seeded inputs of the GPU modules and held
against their element-wise bounds: an honest implementation stays inside every bound, and the worst |error| / bound over a
kernel's cases is at least 1/2, so no bound is slack enough to hide a wrong kernel.  The trigonometric outputs are held
against the accuracy the math library documents, not against a model, and the bit-exact ones (fold_norm_gain, the cast, the
copies) need none."""
import importlib
import math
import os

import pytest
import torch

from tests import test_glue_kernels_gpu as GG
from tests import test_norm_rope_kernels_gpu as NG
from tests.kernel_guards import BF

FAKE = 1 << 20   # a non-null, 256-byte aligned address that is never dereferenced
OK, INVALID, UNSUPPORTED = 0, -1, -2
F32 = torch.float32


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib.load()


def _refused(lib, rc, code, *texts):
    msg = lib.vgpt_last_error()
    assert rc == code, (rc, msg)
    for t in texts:
        assert t in msg, (t, msg)


def _table(lib, name, defaults, order, rows, ok):
    """Call `name` with `defaults` overridden by each row's keywords; rows are (overrides, code, texts...)."""
    fn = getattr(lib, name)
    call = lambda kw: fn(*[{**defaults, **kw}[a] for a in order], None)   # noqa: E731
    for kw, code, *texts in rows:
        assert set(kw) <= set(order), kw
        _refused(lib, call(kw), code, name.encode() + b":", *texts)
    for kw in ok:
        assert call(kw) == OK, (name, kw, lib.vgpt_last_error())


def _nulls(*names):
    return [({n: None}, INVALID, b"null pointer") for n in names]


# ---- norm_rope.hip -------------------------------------------------------------------------------------------------------

def test_rmsnorm_refusals(lib):
    _table(lib, "vgpt_rmsnorm_fwd", dict(x=FAKE, w=FAKE, y=FAKE, rows=4, H=64, eps=1e-5), ["x", "w", "y", "rows", "H", "eps"],
           _nulls("x", "w", "y") + [({"rows": -1}, INVALID, b"bad shape"), ({"H": 0}, INVALID, b"bad shape"),
                                    ({"H": -8}, INVALID, b"bad shape"), ({"H": 12}, UNSUPPORTED, b"H=12 not a multiple of 8"),
                                    ({"H": 4100}, UNSUPPORTED, b"H=4100"), ({"H": 1 << 31}, UNSUPPORTED, b"too large")],
           [{"rows": 0}])


def test_rope_table_and_rope_qk_refusals(lib):
    _table(lib, "vgpt_rope_table", dict(pos=FAKE, inv=FAKE, cos=FAKE, sin=FAKE, tokens=3, half=48, rnd=1, scale=1.0),
           ["pos", "inv", "cos", "sin", "tokens", "half", "rnd", "scale"],
           _nulls("pos", "inv", "cos", "sin") + [({"tokens": -1}, INVALID, b"bad shape"), ({"half": 0}, INVALID, b"bad shape"),
                                                 ({"half": -4}, INVALID, b"bad shape")], [{"tokens": 0}])
    _table(lib, "vgpt_rope_qk_inplace", dict(qkv=FAKE, cos=FAKE, sin=FAKE, tokens=3, nq=2, nkv=1, hd=96),
           ["qkv", "cos", "sin", "tokens", "nq", "nkv", "hd"],
           _nulls("qkv", "cos", "sin") + [({"tokens": -1}, INVALID, b"bad shape"), ({"nq": 0}, INVALID, b"bad shape"),
                                          ({"nkv": 0}, INVALID, b"bad shape"), ({"hd": 0}, INVALID, b"bad shape"),
                                          ({"hd": 24}, UNSUPPORTED, b"head_dim=24"), ({"hd": 8}, UNSUPPORTED, b"head_dim=8"),
                                          ({"hd": 100}, UNSUPPORTED, b"head_dim=100")], [{"tokens": 0}])


def test_rms_rstd_and_fold_norm_gain_refusals(lib):
    shape = b"H and ldx must be multiples of 8, ldx >= H"
    _table(lib, "vgpt_rms_rstd", dict(x=FAKE, out=FAKE, rows=4, H=64, ldx=72, eps=1e-5), ["x", "out", "rows", "H", "ldx", "eps"],
           _nulls("x", "out") + [({"rows": -1}, INVALID, shape), ({"H": 0}, INVALID, shape), ({"H": 60, "ldx": 64}, INVALID, shape),
                                 ({"ldx": 56}, INVALID, shape), ({"ldx": 68}, INVALID, shape), ({"eps": -1e-5}, INVALID, shape),
                                 ({"x": FAKE + 8}, UNSUPPORTED, b"16-byte aligned"), ({"x": FAKE + 2}, UNSUPPORTED, b"16-byte aligned"),
                                 ({"H": 1 << 31, "ldx": 1 << 31}, UNSUPPORTED, b"too large")],
           [{"rows": 0}, {"rows": 0, "x": None, "out": None}, {"rows": 0, "ldx": 64}])
    kmsg = b"K must be a multiple of 8"
    _table(lib, "vgpt_fold_norm_gain", dict(W=FAKE, g=FAKE, out=FAKE, N=3, K=24), ["W", "g", "out", "N", "K"],
           _nulls("W", "g", "out") + [({"N": -1}, INVALID, kmsg), ({"K": 0}, INVALID, kmsg), ({"K": 12}, INVALID, kmsg),
                                      ({"W": FAKE + 8}, UNSUPPORTED, b"16-byte aligned"), ({"g": FAKE + 4}, UNSUPPORTED, b"16-byte aligned"),
                                      ({"out": FAKE + 2}, UNSUPPORTED, b"16-byte aligned"), ({"K": 1 << 31}, UNSUPPORTED, b"too large")],
           [{"N": 0}, {"N": 0, "W": None, "g": None, "out": None}])


# ---- glue.hip ------------------------------------------------------------------------------------------------------------

def test_embed_gather_and_timestep_refusals(lib):
    _table(lib, "vgpt_embed_gather", dict(ids=FAKE, table=FAKE, out=FAKE, rows=5, H=64, vocab=11),
           ["ids", "table", "out", "rows", "H", "vocab"],
           _nulls("ids", "table", "out") + [({"rows": -1}, INVALID, b"bad shape"), ({"H": 0}, INVALID, b"bad shape"),
                                            ({"vocab": 0}, INVALID, b"bad shape"), ({"H": 12}, UNSUPPORTED, b"H must be a multiple of 8"),
                                            ({"H": 1 << 31}, UNSUPPORTED, b"too large")], [{"rows": 0}])
    _table(lib, "vgpt_timestep_sinusoid", dict(t=FAKE, freqs=FAKE, out=FAKE, n=3, half=128), ["t", "freqs", "out", "n", "half"],
           _nulls("t", "freqs", "out") + [({"n": -1}, INVALID, b"bad shape"), ({"half": 0}, INVALID, b"bad shape")], [{"n": 0}])


def test_patch_embed_and_final_layer_refusals(lib):
    needs = b"needs in_channels=4, patch 2, even latent size"
    _table(lib, "vgpt_patch_embed_fwd", dict(x=FAKE, W=FAKE, b=FAKE, pos=FAKE, dst=FAKE, seq=FAKE, nf=2, C=4, h=8, w=6, H=64, pm=16),
           ["x", "W", "b", "pos", "dst", "seq", "nf", "C", "h", "w", "H", "pm"],
           _nulls("x", "W", "b", "pos", "dst", "seq") + [
               ({"nf": -1}, INVALID, b"bad shape"), ({"C": 0}, INVALID, b"bad shape"), ({"h": 0}, INVALID, b"bad shape"),
               ({"w": -2}, INVALID, b"bad shape"), ({"H": 0}, INVALID, b"bad shape"), ({"C": 3}, UNSUPPORTED, needs),
               ({"C": 8}, UNSUPPORTED, needs), ({"h": 7}, UNSUPPORTED, needs), ({"w": 5}, UNSUPPORTED, needs),
               ({"H": 6}, UNSUPPORTED, b"H must be a multiple of 4"), ({"pm": 3}, INVALID, b"latent larger than pos_embed_max_size"),
               ({"pm": 2, "h": 4}, INVALID, b"latent larger than pos_embed_max_size"), ({"H": 1 << 31}, UNSUPPORTED, b"too large")],
           [{"nf": 0}])
    needs = b"needs out_channels=4, patch 2, even latent size"
    width = b"H must be a multiple of 8 and <= 4096"
    _table(lib, "vgpt_final_layer_fwd", dict(hid=FAKE, src=FAKE, mod=FAKE, W=FAKE, b=FAKE, out=FAKE, nf=2, C=4, h=8, w=6, H=64, eps=1e-6),
           ["hid", "src", "mod", "W", "b", "out", "nf", "C", "h", "w", "H", "eps"],
           _nulls("hid", "src", "mod", "W", "b", "out") + [
               ({"nf": -1}, INVALID, b"bad shape"), ({"C": 0}, INVALID, b"bad shape"), ({"h": 0}, INVALID, b"bad shape"),
               ({"w": 0}, INVALID, b"bad shape"), ({"H": 0}, INVALID, b"bad shape"), ({"C": 3}, UNSUPPORTED, needs),
               ({"h": 7}, UNSUPPORTED, needs), ({"w": 5}, UNSUPPORTED, needs), ({"H": 12}, UNSUPPORTED, width),
               ({"H": 4104}, UNSUPPORTED, width), ({"H": 8192}, UNSUPPORTED, width), ({"H": 1 << 32}, UNSUPPORTED, width)],
           [{"nf": 0}])


def test_linear_small_refusals(lib):
    align = b"K and ldx must be multiples of 8"
    _table(lib, "vgpt_linear_small", dict(x=FAKE, W=FAKE, b=FAKE, out=FAKE, rows=None, M=4, N=5, K=24, ldx=32, ldo=8, pre=3, post=3),
           ["x", "W", "b", "out", "rows", "M", "N", "K", "ldx", "ldo", "pre", "post"],
           _nulls("x", "W", "out") + [
               ({"M": -1}, INVALID, b"bad shape"), ({"N": 0}, INVALID, b"bad shape"), ({"K": 0}, INVALID, b"bad shape"),
               ({"M": 33}, UNSUPPORTED, b"M=33 > 32"), ({"M": 64}, UNSUPPORTED, b"M=64 > 32"), ({"K": 12}, UNSUPPORTED, align),
               ({"ldx": 36}, UNSUPPORTED, align), ({"N": 1 << 31, "ldo": 1 << 31}, UNSUPPORTED, b"dimension too large"),
               ({"K": 1 << 31, "ldx": 1 << 31}, UNSUPPORTED, b"dimension too large"),
               ({"ldx": 16}, INVALID, b"ldx=16 < K=24"), ({"ldo": 4}, INVALID, b"ldo=4 < N=5"), ({"ldo": 0}, INVALID, b"ldo=0 < N=5"),
               ({"ldo": -8}, INVALID, b"ldo=-8 < N=5")],
           [{"M": 0}, {"M": 0, "b": None, "ldo": 5, "ldx": 24}])


def test_sampler_refusals(lib):
    _table(lib, "vgpt_sampler_set_timesteps", dict(sigma=FAKE, step=FAKE, n_steps=5, ts=FAKE, n=4), ["sigma", "step", "n_steps", "ts", "n"],
           _nulls("sigma", "step", "ts") + [({"n": -1}, INVALID, b"bad shape"), ({"n_steps": 0}, INVALID, b"bad shape"),
                                            ({"n_steps": -3}, INVALID, b"bad shape")], [{"n": 0}])
    _table(lib, "vgpt_euler_cfg_update", dict(z=FAKE, zm=FAKE, pred=FAKE, sigma=FAKE, step=FAKE, n_steps=5, nf=4, elems=256, pt=1, cfg=1, scale=1.6),
           ["z", "zm", "pred", "sigma", "step", "n_steps", "nf", "elems", "pt", "cfg", "scale"],
           _nulls("z", "zm", "pred", "sigma", "step") + [
               ({"nf": -1}, INVALID, b"bad shape"), ({"elems": -1}, INVALID, b"bad shape"), ({"n_steps": 0}, INVALID, b"bad shape"),
               ({"pt": 2}, INVALID, b"unknown prediction type 2"), ({"pt": -1}, INVALID, b"unknown prediction type -1"),
               ({"nf": 3}, INVALID, b"CFG needs an even number of frames"), ({"nf": 1}, INVALID, b"CFG needs an even number of frames")],
           [{"nf": 0}, {"elems": 0}, {"nf": 0, "cfg": 0}, {"elems": 0, "nf": 3, "cfg": 0}])
    align = b"sizes, strides and pointers must be multiples of 16 bytes"
    _table(lib, "vgpt_sampler_copy_step_rows", dict(src=FAKE, dst=FAKE, step=FAKE, n_steps=4, layers=3, slab=64, ss=512, sl=128, dl=96),
           ["src", "dst", "step", "n_steps", "layers", "slab", "ss", "sl", "dl"],
           _nulls("src", "dst", "step") + [
               ({"n_steps": 0}, INVALID, b"bad shape"), ({"layers": -1}, INVALID, b"bad shape"), ({"slab": -16}, INVALID, b"bad shape"),
               ({"slab": 24}, UNSUPPORTED, align), ({"ss": 520}, UNSUPPORTED, align), ({"sl": 132}, UNSUPPORTED, align),
               ({"dl": 100}, UNSUPPORTED, align), ({"src": FAKE + 8}, UNSUPPORTED, align), ({"dst": FAKE + 4}, UNSUPPORTED, align)],
           [{"layers": 0}, {"slab": 0}])
    _table(lib, "vgpt_sampler_advance", dict(step=FAKE), ["step"], _nulls("step"), [])
    _table(lib, "vgpt_cast_f32_to_bf16", dict(src=FAKE, dst=FAKE, n=8), ["src", "dst", "n"],
           _nulls("src", "dst") + [({"n": -1}, INVALID, b"bad shape")], [{"n": 0}])


# ---- mask.hip ------------------------------------------------------------------------------------------------------------

def test_mask_refusals(lib):
    big = [({"L": 1 << 24}, INVALID, b"bad shape"), ({"L": 1 << 30}, INVALID, b"bad shape")]
    neg = [({"B": -1}, INVALID, b"bad shape"), ({"L": -1}, INVALID, b"bad shape")]
    wide = [({"B": 65536}, INVALID, b"bad shape"), ({"B": 1 << 20}, INVALID, b"bad shape")]
    _table(lib, "vgpt_mask_pack_bool", dict(mask=FAKE, bits=FAKE, B=1, L=100), ["mask", "bits", "B", "L"],
           _nulls("mask", "bits") + neg + big, [{"B": 0}, {"L": 0}])
    _table(lib, "vgpt_mask_pack_additive", dict(mask=FAKE, f32=1, bits=FAKE, B=1, L=100), ["mask", "f32", "bits", "B", "L"],
           _nulls("mask", "bits") + neg + big, [{"B": 0}, {"L": 0}, {"L": 0, "f32": 0}])
    _table(lib, "vgpt_mask_build_tokens", dict(attr=FAKE, bits=FAKE, B=1, L=100), ["attr", "bits", "B", "L"],
           _nulls("attr", "bits") + neg + big + wide + [({"attr": FAKE + 4}, UNSUPPORTED, b"attr must be 8-byte aligned"),
                                                        ({"bits": FAKE + 8}, UNSUPPORTED, b"bits must be 16-byte aligned")],
           [{"B": 0}, {"L": 0}])
    _table(lib, "vgpt_mask_tile_summary", dict(bits=FAKE, summary=FAKE, B=1, L=100), ["bits", "summary", "B", "L"],
           _nulls("bits", "summary") + neg + big + wide + [({"L": 65536 * 128 - 127}, UNSUPPORTED, b"L too large"),
                                                           ({"L": (1 << 24) - 1}, UNSUPPORTED, b"L too large")],
           [{"B": 0}, {"L": 0}])
    _table(lib, "vgpt_mask_count_empty_rows", dict(bits=FAKE, count=FAKE, B=1, L=100), ["bits", "count", "B", "L"],
           _nulls("bits", "count") + neg + big, [])
    _table(lib, "vgpt_attn_qblock_order", dict(summary=FAKE, B=2, L=1000, q0=256, order=FAKE), ["summary", "B", "L", "q0", "order"],
           _nulls("summary", "order") + neg + big + [({"q0": 100}, INVALID, b"bad shape"), ({"q0": 64}, INVALID, b"bad shape"),
                                                     ({"q0": -128}, INVALID, b"bad shape"), ({"q0": 1024}, INVALID, b"bad shape"),
                                                     ({"q0": 1152}, INVALID, b"bad shape")],
           [{"B": 0}, {"L": 1024, "q0": 1024}, {"L": 0, "q0": 0}, {"B": 0, "q0": 0}])


# ============================================================================================================
# CPU models of the kernels' rounding points against the element-wise bounds of the GPU modules
# ============================================================================================================
_XOR = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def wave_sum(v):
    """common.h wave_sum on (..., 64) fp32: six xor-butterfly steps, every lane ends with the same bits."""
    for idx in _XOR:
        v = v + v[..., idx]
    return v[..., 0]


def lane_chain(terms):
    """(..., n) fp32 terms of a row, element k owned by lane (k / 8) % 64 in slab k / 512: each lane adds its terms in order
    of k, starting from 0 (what the `off = (c * 64 + lane) * 8` loops of the kernels do).  Returns (..., 64)."""
    n = terms.shape[-1]
    slabs = (n + 511) // 512
    padded = torch.zeros(*terms.shape[:-1], slabs * 512, dtype=F32)
    padded[..., :n] = terms
    t = padded.view(*terms.shape[:-1], slabs, 64, 8)
    acc = torch.zeros(*terms.shape[:-1], 64, dtype=F32)
    for c in range(slabs):
        for j in range(8):
            acc = acc + t[..., c, :, j]
    return acc


def row_sum(terms):
    return wave_sum(lane_chain(terms))


def model_rstd(x, eps):
    xf = x.float()
    return torch.rsqrt(row_sum(xf * xf) / float(x.shape[-1]) + torch.tensor(eps, dtype=F32))


def model_rmsnorm(x, w, eps):
    n = (x.float() * model_rstd(x, eps)[:, None]).to(BF)
    return (w.float() * n.float()).to(BF)


def model_rope_qk(qkv, cos, sin, hd, nq, nkv):
    tokens, half, n_rot = qkv.shape[0], hd // 2, nq + nkv
    x = qkv.float()[:, :n_rot * hd].view(tokens, n_rot, 2, half)
    a, b, c, s = x[:, :, 0], x[:, :, 1], cos[:, None], sin[:, None]
    o = torch.stack([(a * c - b * s).to(BF), (b * c + a * s).to(BF)], 2).reshape(tokens, n_rot * hd)
    return torch.cat([o, qkv[:, n_rot * hd:]], 1)


def model_patch_embed(x, W, bias, pos, pos_max):
    _, _, h, w = x.shape
    p, Wf = GG.patches_of(x).float(), W.float()
    acc = torch.zeros(p.shape[0], p.shape[1], W.shape[0], dtype=F32)
    for e in range(16):
        acc = acc + Wf[None, None, :, e] * p[:, :, None, e]
    return (acc + bias.float() + GG.cropped_pos(pos, pos_max, h, w).float()[None]).to(BF)


def act32(x, act):
    if act == GG.ACT_SILU:
        return x * (1.0 / (1.0 + torch.exp(-x)))
    if act == GG.ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))
    if act == GG.ACT_GELU_TANH:
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    return x


def model_linear_small(x, W, b, pre, post):
    a = x.float()
    if pre != GG.ACT_NONE:
        a = act32(a, pre).to(BF).float()
    v = row_sum(a[:, None, :] * W.float()[None])             # bf16 x bf16 is exact in fp32: only the additions round
    if b is not None:
        v = v + b.float()
    return act32(v, post).to(BF)


def model_final_layer(hidden, mod, Wf, b, h, w, eps=GG.FINAL_EPS):
    ntok, H = (h // 2) * (w // 2), hidden.shape[1]
    rows, _ = GG.final_rows(ntok)
    x = torch.stack([hidden[r:r + ntok] for r in rows]).float()
    mean = row_sum(x) / float(H)
    d = x - mean[..., None]
    rstd = torch.rsqrt(row_sum(d * d) / float(H) + torch.tensor(eps, dtype=F32))
    v = d * rstd[..., None] * (1.0 + mod.float()[:, None, H:]) + mod.float()[:, None, :H]
    y = row_sum(v[:, :, None, :] * Wf.float()[None, None]) + b.float()
    return GG.unpatchify(y.to(BF), h, w)


def model_euler(z0, pred, sigma, step, pred_type, use_cfg, scale):
    sg, sg_next = sigma[step], sigma[step + 1]
    dt, inv = sg_next - sg, 1.0 / (1.0 - sg)
    z, p, scale = z0.clone(), pred.float(), torch.tensor(scale, dtype=F32)
    v = (p - z) * inv if pred_type == GG.PRED_X1 else p
    if use_cfg:
        half = z.shape[0] // 2
        guided = v[half:] + scale * (v[:half] - v[half:])
        v = torch.cat([guided, guided])
    return z + dt * v


def _worst(err, bound):
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    return float((err / bound.clamp_min(1e-300)).max())


def _ratios_rmsnorm():
    out = {}
    for rows, H in NG.RMS_CASES:
        x, w = NG.rms_inputs(rows, H)
        y64 = NG.rmsnorm_reference(x, w)
        out[(rows, H)] = _worst((model_rmsnorm(x, w, NG.EPS).double() - y64).abs(), NG.rmsnorm_bound(y64, H))
    return out


def _ratios_rstd():
    out = {}
    for rows, H, _ in NG.RSTD_CASES:
        x, _w = NG.rms_inputs(rows, H)
        r64 = NG.rstd_reference(x)
        out[(rows, H)] = _worst((model_rstd(x, NG.EPS).double() - r64).abs(), NG.rstd_bound(x))
    return out


def _ratios_rope_qk():
    out = {}
    for hd, nq, nkv, tokens in NG.ROPE_CASES:
        qkv, cos, sin = NG.rope_qk_inputs(hd, nq, nkv, tokens)
        o64, mag = NG.rope_qk_reference(qkv, cos, sin, hd, nq, nkv)
        out[(hd, nq, nkv, tokens)] = _worst((model_rope_qk(qkv, cos, sin, hd, nq, nkv).double() - o64).abs(), NG.rope_qk_bound(o64, mag))
    return out


def _ratios_patch_embed():
    out = {}
    for h, w, H in GG.PATCH_CASES:
        x, W, bias, pos = GG.patch_inputs(h, w, H)
        pm = GG.PATCH_GRIDS[(h, w)]
        o64, terms = GG.patch_reference(x, W, bias, pos, pm)
        out[(h, w, H)] = _worst((model_patch_embed(x, W, bias, pos, pm).double() - o64).abs(), GG.patch_bound(o64, terms))
    return out


def _ratios_linear_small():
    out = {}
    for case, cid in zip(GG.LINEAR_CASES, GG.LINEAR_IDS):
        M, N, K, pre, post, bias, _ = case
        x, W, b = GG.linear_inputs(M, N, K, bias)
        o64, mag = GG.linear_reference(x, W, b, pre, post)
        out[cid] = _worst((model_linear_small(x, W, b, pre, post).double() - o64).abs(), GG.linear_bound(o64, mag, K, pre, post))
    return out


def _ratios_final_layer():
    out = {}
    for h, w, H in GG.FINAL_CASES:
        hidden, mod, Wf, b = GG.final_inputs(h, w, H)
        o64, mag = GG.final_reference(hidden, mod, Wf, b, h, w)
        out[(h, w, H)] = _worst((model_final_layer(hidden, mod, Wf, b, h, w).double() - o64).abs(), GG.final_bound(o64, mag, H))
    return out


def _ratios_euler():
    out, sigma, step = {}, GG.sampler_sigma(), 2
    for pred_type, use_cfg, scale in GG.EULER_CASES:
        z0, pred = GG.euler_inputs(4, 250)
        z64, bound = GG.euler_reference(z0, pred, sigma, step, pred_type, use_cfg, float(torch.tensor(scale, dtype=F32)))
        out[(pred_type, use_cfg, scale)] = _worst((model_euler(z0, pred, sigma, step, pred_type, use_cfg, scale).double() - z64).abs(), bound)
    return out


MODELS = {"rmsnorm": _ratios_rmsnorm, "rms_rstd": _ratios_rstd, "rope_qk": _ratios_rope_qk, "patch_embed": _ratios_patch_embed,
          "linear_small": _ratios_linear_small, "final_layer": _ratios_final_layer, "euler_cfg": _ratios_euler}


@pytest.mark.parametrize("kernel", list(MODELS))
def test_cpu_model_stays_inside_its_bound_and_fills_half_of_it(kernel):
    ratios = MODELS[kernel]()                  # asserts err <= bound on every element of every case
    worst = max(ratios.values())
    print(f"MEASURE cpu model {kernel}: worst |err|/bound over {len(ratios)} cases = {worst:.3g}, "
          f"smallest per-case worst = {min(ratios.values()):.3g}")
    assert worst >= 0.5


def test_cpu_trigonometry_meets_the_documented_accuracy():
    """The rule the device tables are held to, applied to the host's fp32 cosf / sinf on the same angles: an honest fp32
    implementation passes, both unrounded and rounded to bf16."""
    for half, tokens, scale, rnd in NG.TABLE_CASES:
        pos, inv = NG.rope_table_inputs(half, tokens)
        ang = pos.float()[:, None] * inv[None, :]
        s32 = torch.tensor(scale, dtype=F32)
        c64, s64 = NG.rope_table_reference(pos, inv)
        for fn, ref in ((torch.cos, c64), (torch.sin, s64)):
            out = fn(ang) * s32
            out = out.to(BF).float() if rnd else out
            assert NG.trig_table_ok(out, ref, float(s32), rnd)[0], (half, tokens, scale, rnd)


def test_bf16_helpers():
    from tests.kernel_guards import bf16_ulp, bf16_ulps_apart, to_bf16
    one = torch.tensor([1.0], dtype=BF)
    nxt = torch.tensor([1.0 + 2.0 ** -7], dtype=BF)
    assert int(bf16_ulps_apart(one, nxt)) == 1 and int(bf16_ulps_apart(-one, one)) == 2 * 0x3F80
    assert int(bf16_ulps_apart(torch.tensor([0.0], dtype=BF), torch.tensor([-0.0], dtype=BF))) == 0
    assert float(bf16_ulp(torch.tensor([1.0]))) == 2.0 ** -7 and float(bf16_ulp(torch.tensor([1.99]))) == 2.0 ** -7
    assert float(bf16_ulp(torch.tensor([-0.75]))) == 2.0 ** -8
    assert torch.equal(to_bf16(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=torch.float64)),
                       torch.tensor([1.0, 1 + 2.0 ** -6], dtype=BF))
    assert math.isclose(NG.LONGROPE_SCALE, 1.1902380714238083)
