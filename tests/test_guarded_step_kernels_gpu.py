"""The guarded optimizer step's kernels (video-gpt_amd/ops_train.py -> csrc/train.hip: vgpt_clip_coef_guarded,
vgpt_adamw_step_guarded, vgpt_adamw_ema_step_guarded, vgpt_sumsq_keep, vgpt_count_nonfinite) on the GPU.

Every comparison is torch.equal on the raw bits, against the unguarded entry point on cloned inputs (clip, AdamW, sumsq) or
against torch.isnan / torch.isinf on a CPU copy (the counts): the guarded kernels promise the unguarded kernels' arithmetic
in the same order, and counting is integer work, so there is nothing to tolerate.  Outputs sit between NaN or sentinel guard
bands that must survive (the Guarded helper of tests/test_accum_ema_kernels_gpu.py)."""
import importlib

import numpy as np
import pytest
import torch

from tests.test_accum_ema_kernels_gpu import PAD, Guarded, _adamw_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
I32 = torch.int32
SENTINEL = -77
ADAMW_SIZES = [1, 3, 4, 1023, 4097, (1 << 20) + 2]


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("video-gpt_amd.ops_train")


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF else I32)


class Verdict:
    """Two int32 words between sentinel bands."""
    def __init__(self, first=SENTINEL, second=SENTINEL):
        self.buf = torch.full((2 + 2 * PAD,), SENTINEL, dtype=I32, device=DEV)
        self.t = self.buf[PAD:PAD + 2]
        self.t.copy_(torch.tensor([first, second], dtype=I32))

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all() and (self.buf[-PAD:] == SENTINEL).all())


def _guarded_clip(T, partials, max_norm, extra, skip_norm):
    coef, norm, verdict = Guarded(torch.full((1,), 123.0, device=DEV)), Guarded(torch.full((1,), 456.0, device=DEV)), Verdict()
    before = partials.clone()
    T.clip_coef_guarded(partials, coef.t, norm.t, max_norm, extra, skip_norm, verdict.t)
    torch.cuda.synchronize()
    assert coef.intact() and norm.intact() and verdict.intact(), "guard band overwritten"
    assert torch.equal(_bits(partials), _bits(before)), "the partial sums were written"
    return coef.t.clone(), norm.t.clone(), verdict.t.tolist()


def _plain_clip(T, partials, max_norm, extra):
    coef, norm = torch.full((1,), 123.0, device=DEV), torch.full((1,), 456.0, device=DEV)
    T.clip_coef(partials, coef, norm, max_norm, extra)
    torch.cuda.synchronize()
    return coef, norm


# ---- clip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 8, 65, 130])
def test_clip_guarded_on_finite_sums_is_clip_coef(T, n):
    gen = torch.Generator("cpu").manual_seed(900 + n)
    for scale in (50.0, 1e-4):                     # a norm above and a norm below the positive max_norm values
        partials = (torch.rand(n, generator=gen) * scale).to(DEV)
        for max_norm in (0.0, 1.0, 1e4):           # no clipping; active on the large sums; idle
            for extra in (1.0, 0.125):
                want_c, want_n = _plain_clip(T, partials, max_norm, extra)
                for skip_norm in (0.0, 1e30):      # no threshold, and one that is never reached
                    c, nrm, verdict = _guarded_clip(T, partials, max_norm, extra, skip_norm)
                    what = f"n={n} scale={scale} max_norm={max_norm} extra={extra} skip_norm={skip_norm}"
                    assert verdict == [0, 0], what
                    assert torch.equal(_bits(c), _bits(want_c)) and torch.equal(_bits(nrm), _bits(want_n)), what
        assert float(want_n) > 0


@pytest.mark.parametrize("kind,n", [(k, n) for k in ("nan", "inf", "overflow") for n in (1, 2, 8, 65, 130)
                                    if not (k == "overflow" and n == 1)])        # an overflowing sum takes two partials
def test_clip_guarded_skips_a_non_finite_sum(T, n, kind):
    gen = torch.Generator("cpu").manual_seed(950 + n)
    partials = torch.rand(n, generator=gen) * 50.0
    at = int(torch.randint(n, (1,), generator=gen))
    if kind == "nan":
        partials[at] = float("nan")
    elif kind == "inf":
        partials[at] = float("inf")
    else:
        partials[at] = 3e38
        partials[(at + 1) % n] = 3e38
    assert kind != "overflow" or bool(torch.isfinite(partials).all())       # every partial finite, only their sum is not
    for max_norm in (0.0, 1.0):
        for skip_norm in (0.0, 5.0):
            c, nrm, verdict = _guarded_clip(T, partials.to(DEV), max_norm, 0.5, skip_norm)
            assert verdict == [1, 1], (kind, n, verdict)
            assert int(_bits(c)) == 0, "coef must be +0.0 exactly"
            if kind == "nan":
                assert bool(torch.isnan(nrm))
            else:
                assert float(nrm) == float("inf")


def test_clip_guarded_threshold_is_strict(T):
    gen = torch.Generator("cpu").manual_seed(990)
    for n in (1, 8, 130):
        partials = (torch.rand(n, generator=gen) * 50.0).to(DEV)
        want_c, want_n = _plain_clip(T, partials, 1.0, 0.25)
        nrm32 = np.float32(float(want_n))
        below = float(np.nextafter(nrm32, np.float32(0)))           # the norm is the next float above this threshold
        # a norm equal to the threshold is applied
        c, nrm, verdict = _guarded_clip(T, partials, 1.0, 0.25, float(nrm32))
        assert verdict == [0, 0] and torch.equal(_bits(c), _bits(want_c)) and torch.equal(_bits(nrm), _bits(want_n))
        # the next float above it is skipped, reason 2, and the norm is still reported
        c, nrm, verdict = _guarded_clip(T, partials, 1.0, 0.25, below)
        assert verdict == [1, 2] and int(_bits(c)) == 0 and torch.equal(_bits(nrm), _bits(want_n))
    # 4.0 has the exact root 2.0: the boundary without reading the norm off a first run
    four = torch.tensor([4.0], device=DEV)
    assert _guarded_clip(T, four, 0.0, 1.0, 2.0)[2] == [0, 0]
    assert _guarded_clip(T, four, 0.0, 1.0, float(np.nextafter(np.float32(2.0), np.float32(0))))[2] == [1, 2]
    # a threshold of 0 never skips, however large the finite norm
    huge = torch.tensor([3e38], device=DEV)
    c, nrm, verdict = _guarded_clip(T, huge, 1.0, 1.0, 0.0)
    want_c, want_n = _plain_clip(T, huge, 1.0, 1.0)
    assert verdict == [0, 0] and torch.equal(_bits(c), _bits(want_c)) and torch.equal(_bits(nrm), _bits(want_n))


# ---- AdamW -------------------------------------------------------------------------------------------------------------
def _launch(T, bufs, lr, step, gs_t, ema_d, verdict):
    """The guarded (verdict given) or unguarded launch on (master, param, grad, m, v, ema | None)."""
    master, param, grad, m, v, ema = bufs
    b1, b2, eps, wd = 0.9, 0.999, 1e-8, 0.01
    if verdict is None:
        if ema is None:
            T.adamw_step(master, param, grad, m, v, lr, b1, b2, eps, wd, step, gs_t)
        else:
            T.adamw_ema_step(master, param, grad, m, v, lr, b1, b2, eps, wd, step, gs_t, ema, ema_d)
    elif ema is None:
        T.adamw_step_guarded(master, param, grad, m, v, lr, b1, b2, eps, wd, step, gs_t, verdict)
    else:
        T.adamw_ema_step_guarded(master, param, grad, m, v, lr, b1, b2, eps, wd, step, gs_t, ema, ema_d, verdict)


NAMES = ("master", "param", "grad", "m", "v", "ema")


def _inputs(n, gdt, use_ema, seed, nan_grad=False):
    gen = torch.Generator(DEV).manual_seed(seed)
    p0, grad, m0, v0, ema0 = _adamw_case(n, gdt, 2, gen)
    if nan_grad:
        grad[::3] = float("nan")
        grad[n // 2] = float("inf")
    return [p0, p0.to(BF), grad, m0, v0, ema0 if use_ema else None]


@pytest.mark.parametrize("n", ADAMW_SIZES)
@pytest.mark.parametrize("use_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("gdt", [BF, F32], ids=["bf16", "fp32"])
def test_adamw_guarded_verdict_0_is_the_unguarded_step(T, gdt, use_ema, n):
    for gs in (None, 0.25):
        gs_t = None if gs is None else torch.tensor([gs], dtype=F32, device=DEV)
        src = _inputs(n, gdt, use_ema, 1200 + n % 977)
        ref = [None if t is None else t.clone() for t in src]
        _launch(T, ref, 3e-3, 2, gs_t, 0.5, None)
        got = [None if t is None else Guarded(t) for t in src]
        verdict = Verdict(0, 0)
        _launch(T, [None if g is None else g.t for g in got], 3e-3, 2, gs_t, 0.5, verdict.t)
        torch.cuda.synchronize()
        for name, g, r, s in zip(NAMES, got, ref, src):
            if g is None:
                continue
            assert torch.equal(_bits(g.t), _bits(r)), f"{name} differs from the unguarded entry point (n={n}, gs={gs})"
            assert g.intact(), f"guard band of {name} overwritten"
            if name not in ("grad",):
                assert n < 4 or not torch.equal(_bits(g.t), _bits(s)), f"{name} did not move"
        assert verdict.t.tolist() == [0, 0] and verdict.intact()


@pytest.mark.parametrize("n", ADAMW_SIZES)
@pytest.mark.parametrize("use_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("gdt", [BF, F32], ids=["bf16", "fp32"])
def test_adamw_guarded_verdict_1_writes_nothing(T, gdt, use_ema, n):
    for nan_grad in (False, True):
        for reason in (1, 2):
            src = _inputs(n, gdt, use_ema, 1300 + n % 977, nan_grad)
            got = [None if t is None else Guarded(t) for t in src]
            before = [None if g is None else _bits(g.buf).clone() for g in got]
            gs_t = torch.tensor([0.0], dtype=F32, device=DEV)        # what a skipping clip kernel leaves in coef
            verdict = Verdict(1, reason)
            _launch(T, [None if g is None else g.t for g in got], 3e-3, 2, gs_t, 0.5, verdict.t)
            torch.cuda.synchronize()
            for name, g, b in zip(NAMES, got, before):
                if g is not None:
                    assert torch.equal(_bits(g.buf), b), f"{name} was written by a skipped launch (n={n}, nan_grad={nan_grad})"
            assert verdict.t.tolist() == [1, reason] and verdict.intact() and float(gs_t) == 0.0


@pytest.mark.parametrize("use_ema", [False, True], ids=["plain", "ema"])
def test_adamw_guarded_beside_a_busy_stream(T, use_ema):
    n = (1 << 20) + 2
    src = _inputs(n, BF, use_ema, 1400)
    ref = [None if t is None else t.clone() for t in src]
    _launch(T, ref, 3e-3, 2, None, 0.5, None)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    a = torch.randn(2048, 2048, device=DEV, dtype=BF)
    for v in (0, 1):
        got = [None if t is None else t.clone() for t in src]
        verdict = Verdict(v, v)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(8):
                a @ a
        _launch(T, got, 3e-3, 2, None, 0.5, verdict.t)
        torch.cuda.synchronize()
        for name, g, r, s in zip(NAMES, got, ref, src):
            if g is not None:
                assert torch.equal(_bits(g), _bits(r if v == 0 else s)), (name, v)


# ---- sumsq_keep --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1023, (1 << 20) + 3])
@pytest.mark.parametrize("gdt", [BF, F32], ids=["bf16", "fp32"])
def test_sumsq_keep_adds_what_sumsq_adds_and_keeps_it(T, gdt, n):
    gen = torch.Generator(DEV).manual_seed(1500 + n % 977)
    g = Guarded(torch.randn(n, generator=gen, device=DEV).to(gdt))
    g_before = _bits(g.buf).clone()
    alone = torch.zeros(1, dtype=F32, device=DEV)
    T.sumsq(g.t, alone)                              # from zero: the increment itself
    for start in (0.0, 3.25, 1e9):
        want = torch.full((1,), start, dtype=F32, device=DEV)
        T.sumsq(g.t, want)
        total, part = Guarded(torch.full((1,), start, device=DEV)), Guarded(torch.full((1,), -5.0, device=DEV))
        T.sumsq_keep(g.t, total.t, part.t)
        torch.cuda.synchronize()
        assert torch.equal(_bits(total.t), _bits(want)), f"total differs from vgpt_sumsq's (n={n}, start={start})"
        assert torch.equal(_bits(part.t), _bits(alone)), f"part is not the increment (n={n}, start={start})"
        assert total.intact() and part.intact()
    assert torch.equal(_bits(g.buf), g_before) and float(alone) > 0


# ---- count_nonfinite ---------------------------------------------------------------------------------------------------
SPECIAL = {   # both NaN signs, quiet payloads, a signalling pattern, +-Inf, subnormals, the largest finite values
    BF: [0x7FC0, 0xFFC0, 0x7FC1, 0xFFFF, 0x7FFF, 0x7F81, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x007F, 0x7F7F, 0xFF7F, 0x8000],
    F32: [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFFFFFFF, 0x7FFFFFFF, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001,
          0x80000001, 0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x80000000],
}


@pytest.mark.parametrize("lead", [0, 3], ids=["from-0", "from-3"])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_count_nonfinite_against_torch_on_the_cpu(T, dt, lead):
    lengths = [1, 0, 5, 4096, 0, 100003, 1, 5]                # every length of {0, 1, 5, 4096, 100003}; starts at odd elements
    edges = np.concatenate([[lead], lead + np.cumsum(lengths)]).astype(np.int64)
    total = int(edges[-1]) + 11                                # elements behind the last segment belong to nobody
    rng = np.random.default_rng(1600 + lead)
    ut = np.uint16 if dt == BF else np.uint32
    host = torch.randn(total, generator=torch.Generator("cpu").manual_seed(1601)).to(dt)
    raw = host.view(torch.int16 if dt == BF else I32).numpy().view(ut)
    raw[:lead] = SPECIAL[dt][0]                                # NaN in front of the first segment and behind the last
    raw[int(edges[-1]):] = SPECIAL[dt][1]
    for a, b in zip(edges[:-1], edges[1:]):                    # specials at random places, and at both ends of every segment
        if b > a:
            k = min(int(b - a), 40)
            at = np.unique(np.concatenate([[a, b - 1], rng.integers(a, b, k)]))
            raw[at] = rng.choice(np.array(SPECIAL[dt], dtype=ut), at.size)
    x = Guarded(host)
    x_before = _bits(x.buf).clone()
    counts = T.count_nonfinite(x.t, torch.from_numpy(edges).to(DEV))
    torch.cuda.synchronize()
    assert counts.dtype == I32 and counts.shape == (len(lengths), 2)
    want = [[int(torch.isnan(host[a:b]).sum()), int(torch.isinf(host[a:b]).sum())] for a, b in zip(edges[:-1], edges[1:])]
    assert counts.tolist() == want
    assert sum(w[0] for w in want) > 20 and sum(w[1] for w in want) > 5 and want[1] == [0, 0]
    assert torch.equal(_bits(x.buf), x_before), "the buffer was written"
    assert torch.equal(T.count_nonfinite(x.t, torch.from_numpy(edges).to(DEV)), counts)       # and again: the same counts
