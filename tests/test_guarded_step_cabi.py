"""The guarded optimizer step's entry points (include/vgpt.h, "guarded optimizer step") without a GPU: they are declared,
exported and bound under ABI version 8; every host-side refusal happens before any launch and names the offending value;
the trainer's own refusals of skip_bad_steps / skip_grad_norm_above raise before a model or the device is touched."""
import importlib
import os
import re

import pytest

FAKE = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
INVALID, UNSUPPORTED = -1, -2
NEW = ("vgpt_clip_coef_guarded", "vgpt_adamw_step_guarded", "vgpt_adamw_ema_step_guarded", "vgpt_sumsq_keep",
       "vgpt_count_nonfinite")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("video-gpt_amd")


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib.load()


def _refused(lib, rc, code, *texts):
    msg = lib.vgpt_last_error()
    assert rc == code, (rc, msg)
    for t in texts:
        assert t in msg, msg


def test_entry_points_are_declared_exported_and_bound_under_abi_8(pkg, lib):
    with open(os.path.join(ROOT, "include", "vgpt.h")) as f:
        header = f.read()
    assert re.search(r"#define VGPT_ABI_VERSION 8\b", header)
    assert pkg._lib.ABI_VERSION == 8 and lib.vgpt_abi_version() == 8
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        res, args = pkg._lib.SIGNATURES[name]
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, header, re.S).group(1)
        assert len(args) == proto.count(",") + 1, (name, len(args), proto)
    # the unguarded entry points keep their signatures
    assert len(pkg._lib.SIGNATURES["vgpt_clip_coef"][1]) == 7 and len(pkg._lib.SIGNATURES["vgpt_adamw_step"][1]) == 15
    assert len(pkg._lib.SIGNATURES["vgpt_adamw_ema_step"][1]) == 17 and len(pkg._lib.SIGNATURES["vgpt_sumsq"][1]) == 6


def _clip(lib, sumsq=FAKE, n=1, coef=FAKE, norm=FAKE, max_norm=1.0, extra=1.0, skip_norm=0.0, verdict=FAKE):
    return lib.vgpt_clip_coef_guarded(sumsq, n, coef, norm, max_norm, extra, skip_norm, verdict, None)


def test_clip_coef_guarded_refusals_name_the_value(lib):
    for name in ("sumsq", "coef", "verdict"):
        _refused(lib, _clip(lib, **{name: None}), INVALID, b"vgpt_clip_coef_guarded: null pointer", b"(nil)")
    for n in (0, -3):
        _refused(lib, _clip(lib, n=n), INVALID, b"vgpt_clip_coef_guarded: n = %d" % n)
    _refused(lib, _clip(lib, max_norm=-1.5), INVALID, b"vgpt_clip_coef_guarded: max_norm = -1.5")
    _refused(lib, _clip(lib, skip_norm=-2.5), INVALID, b"vgpt_clip_coef_guarded: skip_norm = -2.5")
    _refused(lib, _clip(lib, max_norm=float("nan")), INVALID, b"vgpt_clip_coef_guarded: max_norm = ", b"nan")
    _refused(lib, _clip(lib, skip_norm=float("nan")), INVALID, b"vgpt_clip_coef_guarded: skip_norm = ", b"nan")


def _adamw(lib, ema_variant, master=FAKE, param=FAKE, grad=FAKE, grad_f32=0, m=FAKE, v=FAKE, n=1000, step=1, ema=FAKE,
           decay=0.9999, verdict=FAKE):
    if ema_variant:
        return lib.vgpt_adamw_ema_step_guarded(master, param, grad, grad_f32, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.1, step, None,
                                               ema, decay, verdict, None)
    return lib.vgpt_adamw_step_guarded(master, param, grad, grad_f32, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.1, step, None, verdict,
                                       None)


@pytest.mark.parametrize("ema_variant", [False, True], ids=["plain", "ema"])
def test_adamw_guarded_refusals_name_the_value(lib, ema_variant):
    who = b"vgpt_adamw_ema_step_guarded" if ema_variant else b"vgpt_adamw_step_guarded"
    for name in ("master", "param", "grad", "m", "v"):
        _refused(lib, _adamw(lib, ema_variant, **{name: None}), INVALID, who + b": null pointer", b"(nil)")
    _refused(lib, _adamw(lib, ema_variant, verdict=None), INVALID, who + b": null verdict")
    _refused(lib, _adamw(lib, ema_variant, verdict=FAKE + 2), UNSUPPORTED, who + b": verdict = 0x100002")
    for bad in (2, -1):
        _refused(lib, _adamw(lib, ema_variant, grad_f32=bad), INVALID, who + b": grad_f32 = %d" % bad)
    _refused(lib, _adamw(lib, ema_variant, n=-5), INVALID, who + b": negative length n = -5")
    _refused(lib, _adamw(lib, ema_variant, step=0), INVALID, who + b": step = 0")
    for kw in (dict(master=FAKE + 4), dict(m=FAKE + 8), dict(v=FAKE + 12), dict(param=FAKE + 2), dict(grad=FAKE + 6),
               dict(grad=FAKE + 8, grad_f32=1)):
        _refused(lib, _adamw(lib, ema_variant, **kw), UNSUPPORTED, who + b": buffers must be 16-byte (fp32) / 8-byte (bf16) aligned")
    if ema_variant:
        _refused(lib, _adamw(lib, True, ema=None), INVALID, who + b": null ema")
        _refused(lib, _adamw(lib, True, decay=1.5), INVALID, who + b": ema_decay = 1.5")
        _refused(lib, _adamw(lib, True, ema=FAKE + 4), UNSUPPORTED, who + b": buffers must be")
    assert _adamw(lib, ema_variant, master=FAKE + 4, n=0) == 0      # n == 0: nothing to do, nothing read


def _keep(lib, g=FAKE, g_f32=0, total=FAKE, part=FAKE, n=1000, ws=FAKE):
    return lib.vgpt_sumsq_keep(g, g_f32, total, part, n, ws, None)


def test_sumsq_keep_refusals_name_the_value(lib):
    for name in ("g", "total", "part", "ws"):
        _refused(lib, _keep(lib, **{name: None}), INVALID, b"vgpt_sumsq_keep: null pointer", b"(nil)")
    _refused(lib, _keep(lib, n=-7), INVALID, b"vgpt_sumsq_keep: negative length n = -7")
    _refused(lib, _keep(lib, g_f32=3), INVALID, b"vgpt_sumsq_keep: g_f32 = 3")


def _count(lib, x=FAKE, x_f32=0, n=1000, off=FAKE, T=3, counts=FAKE):
    return lib.vgpt_count_nonfinite(x, x_f32, n, off, T, counts, None)


def test_count_nonfinite_refusals_name_the_value(lib):
    for name in ("x", "counts"):
        _refused(lib, _count(lib, **{name: None}), INVALID, b"vgpt_count_nonfinite: null pointer", b"(nil)")
    _refused(lib, _count(lib, off=None), INVALID, b"vgpt_count_nonfinite: null offsets table")
    _refused(lib, _count(lib, T=-1), INVALID, b"vgpt_count_nonfinite: T = -1")
    _refused(lib, _count(lib, T=65536), INVALID, b"vgpt_count_nonfinite: T = 65536")
    _refused(lib, _count(lib, x_f32=2), INVALID, b"vgpt_count_nonfinite: x_f32 = 2")
    _refused(lib, _count(lib, n=-9), INVALID, b"vgpt_count_nonfinite: negative length n = -9")
    _refused(lib, _count(lib, x=FAKE + 2), UNSUPPORTED, b"vgpt_count_nonfinite: x = 0x100002")
    assert _count(lib, T=0) == 0                                   # no segments: nothing to do, nothing read


def test_trainer_refuses_bad_guard_arguments_before_it_touches_anything():
    TR = importlib.import_module("video-gpt_amd.train")
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError

    class Untouchable:            # any attribute access would raise AttributeError, not VgptError
        __slots__ = ()
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True, "3"):
        with pytest.raises(VgptError, match="skip_grad_norm_above .*positive finite"):
            TR.Stage1Trainer(Untouchable(), skip_bad_steps=True, skip_grad_norm_above=bad)
    with pytest.raises(VgptError, match="skip_grad_norm_above 2.5 without skip_bad_steps=True"):
        TR.Stage1Trainer(Untouchable(), skip_grad_norm_above=2.5)
    with pytest.raises(VgptError, match="skip_bad_steps with forward_only"):
        TR.Stage1Trainer(Untouchable(), skip_bad_steps=True, forward_only=True)
    with pytest.raises(VgptError, match="skip_bad_steps with forward_only"):
        TR.Stage1Trainer.for_evaluation(Untouchable(), skip_bad_steps=True)
    with pytest.raises(VgptError, match="without skip_bad_steps=True"):
        TR.Stage1Trainer.for_evaluation(Untouchable(), skip_grad_norm_above=1.0)
    assert TR.check_guard_arguments(True, 3, False) == 3.0 and TR.check_guard_arguments(False, None, True) is None
    assert TR.SKIP_REASONS == {0: None, 1: "nonfinite", 2: "grad_norm"}
