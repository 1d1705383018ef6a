"""vgpt_adamw_ema_step and vgpt_grad_accumulate (video-gpt_amd/ops_train.py -> csrc/train.hip) on the GPU, in the manner of
tests/test_train_kernels_gpu.py::test_adamw_against_fp64_torch_semantics: every size at which the kernels take another path
(below one vector, the n % 4 tails, one block of 256 vectors = 1024 elements and its neighbours, several blocks plus a tail,
2^20 + 7), both gradient types, and NaN guard bands before and after every buffer that must be intact afterwards.

What is bit for bit and why:
  * adamw_ema_step's master / param / m / v against adamw_step on clones: the same expressions in the same order;
  * grad_accumulate against torch on the CPU: one fp32 addition and one round-to-nearest-even conversion are correctly
    rounded operations, so there is nothing to tolerate.  A NaN is compared as "NaN at the same place": IEEE 754 does not
    pin the sign / payload of a generated NaN (inf - inf is 0x7FC00000 on this GPU and 0xFFC00000 on x86).
The EMA is compared with a float64 restatement under a bound derived from its two fp32 roundings (see _ema_bound)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
U32 = 2.0 ** -24   # fp32 unit roundoff
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 3 * 1024 + 2, (1 << 20) + 7]
PAD = 64           # guard elements on either side: 128 (bf16) / 256 (fp32) bytes, so the payload keeps its alignment


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("video-gpt_amd.ops_train")


class Guarded:
    """A payload of n elements between two bands of NaN; intact() says whether the bands still hold their bits."""
    def __init__(self, values: torch.Tensor):
        n = values.numel()
        self.buf = torch.full((n + 2 * PAD,), float("nan"), dtype=values.dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n]
        self.t.copy_(values)
        self.it = torch.int16 if values.dtype == BF else torch.int32
        self.before = self.buf.view(self.it).clone()
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        now = self.buf.view(self.it)
        return bool(torch.equal(now[:PAD], self.before[:PAD]) and torch.equal(now[-PAD:], self.before[-PAD:]))


def _same_bits(a, b):
    """Bit for bit, a NaN matching any NaN at the same place."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = torch.int16 if a.dtype == BF else torch.int32
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a.view(it)[~na], b.view(it)[~nb]))


def _f32(x):
    return float(np.float32(x))


def _ema_bound(d, p_new, ema_old):
    """The documented form is ema' = fmaf(d, ema, q) with q = fl((1 - d) * p_new), d and 1 - d fp32 values (1 - d formed in
    fp32 on the host).  With X = d ema + (1 - d) p_new exact (float64 here; its own error, 2^-53 relative, is nothing beside
    2^-24) and u = 2^-24:
        |q - (1 - d) p_new| <= u |(1 - d) p_new|                          (the product's rounding)
        |ema' - (d ema + q)| <= u |d ema + q| <= u (|X| + u |(1 - d) p_new|)   (the fused multiply-add's ONE rounding)
    so |ema' - X| <= u (|(1 - d) p_new| + |X|) + u^2 |(1 - d) p_new|.  The u^2 term is covered by the factor (1 + 2^-20); the
    floor 2^-149 is the spacing of fp32 subnormals, where the relative model of a rounding stops.  Returns (X, bound)."""
    D = _f32(d)
    omd = float(np.float32(1.0) - np.float32(d))
    X = D * ema_old.double() + omd * p_new.double()
    return X, U32 * ((omd * p_new.double()).abs() + X.abs()) * (1 + 2.0 ** -20) + 2.0 ** -149


def _adamw_case(n, gdt, step, gen):
    p0 = torch.randn(n, generator=gen, device=DEV)
    grad = torch.randn(n, generator=gen, device=DEV).to(gdt)
    if step == 1:
        m0, v0 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    else:
        m0 = 0.1 * torch.randn(n, generator=gen, device=DEV)
        v0 = 0.01 * torch.rand(n, generator=gen, device=DEV)
    ema0 = p0 + 0.05 * torch.randn(n, generator=gen, device=DEV)
    return p0, grad, m0, v0, ema0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gdt", [BF, F32], ids=["bf16", "fp32"])
def test_adamw_ema_step_is_adamw_step_plus_the_ema(T, gdt, n):
    lr, b1, b2, eps = 3e-3, 0.9, 0.999, 1e-8
    for step in (1, 2):
        for wd in (0.0, 0.01):
            for gs in (None, 0.25):
                gen = torch.Generator(DEV).manual_seed(700 + n % 977 + 10 * step + int(wd * 100) + (0 if gs is None else 3))
                p0, grad, m0, v0, ema0 = _adamw_case(n, gdt, step, gen)
                gs_t = None if gs is None else torch.tensor([gs], dtype=F32, device=DEV)
                what = f"adamw_ema {gdt} n={n} step={step} wd={wd} gs={gs}"
                # the yardstick: adamw_step on clones
                rm, rm_, rv = p0.clone(), m0.clone(), v0.clone()
                rparam = torch.empty(n, dtype=BF, device=DEV)
                T.adamw_step(rm, rparam, grad, rm_, rv, lr, b1, b2, eps, wd, step, gs_t)
                for d in (0.9999, 0.5, 0.0, 1.0):
                    master, m, v, ema = Guarded(p0), Guarded(m0), Guarded(v0), Guarded(ema0)
                    param = Guarded(torch.zeros(n, dtype=BF, device=DEV))
                    gr = Guarded(grad)
                    T.adamw_ema_step(master.t, param.t, gr.t, m.t, v.t, lr, b1, b2, eps, wd, step, gs_t, ema.t, d)
                    torch.cuda.synchronize()
                    for name, got, want in (("master", master.t, rm), ("param", param.t, rparam), ("m", m.t, rm_), ("v", v.t, rv)):
                        assert torch.equal(got, want), f"{what} d={d}: {name} differs from adamw_step's"
                    assert torch.equal(gr.t, grad), f"{what}: the gradient was written"
                    for name, gd in (("master", master), ("param", param), ("m", m), ("v", v), ("ema", ema), ("grad", gr)):
                        assert gd.intact(), f"{what} d={d}: guard band of {name} overwritten"
                    X, bound = _ema_bound(d, master.t, ema0)
                    assert torch.isfinite(ema.t).all()
                    ratio = float(((ema.t.double() - X).abs() / bound).max())
                    assert ratio <= 1.0, f"{what} d={d}: ema worst |err|/bound = {ratio:.3g}"
                    if d == 0.0:
                        assert torch.equal(ema.t, master.t), f"{what}: decay 0 must give ema == master_new bit for bit"
                    if d == 1.0:
                        assert torch.equal(ema.t.view(torch.int32), ema0.view(torch.int32)), f"{what}: decay 1 must leave ema as it was"
                    if d == 0.5 and n >= 1023:
                        assert not torch.equal(ema.t, ema0) and not torch.equal(ema.t, master.t)


def _special(n, gdt, seed):
    """(acc, grad) of n elements on the CPU: the edge values first (as many as fit), random data behind them."""
    gen = torch.Generator("cpu").manual_seed(seed)
    acc = torch.randn(n, generator=gen)
    grad = torch.randn(n, generator=gen).to(gdt)
    inf, nan = float("inf"), float("nan")
    edge = [  # (acc, grad)
        (3.0, 5.0), (-7.0, 7.0), (16777216.0, 1.0),           # integers; 2^24 + 1 is an fp32 tie (to even: 2^24)
        (2.0 ** -8, 1.0),                                     # 1 + 2^-8: a bf16 tie, to even = down to 1.0
        (3 * 2.0 ** -8, 1.0),                                 # 1 + 3 * 2^-8: a bf16 tie, to even = up to 1 + 2^-6
        (2.0 ** -8 + 2.0 ** -20, 1.0), (2.0 ** -8 - 2.0 ** -20, 1.0),   # just above / below the tie
        (-2.0 ** -8, -1.0), (-3 * 2.0 ** -8, -1.0),
        (inf, 1.0), (-inf, 1.0), (1.0, inf), (inf, -inf), (inf, inf),
        (nan, 1.0), (1.0, nan), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (1.0, -1.0),
        (3.0e38, 3.0e38),                                     # overflows to +inf in fp32
        (3.3e38, 1.0e37),                                     # finite in fp32, rounds to +inf in bf16
    ]
    for perm in (0, 1):                      # twice, the second time shifted by one: every edge meets both lanes of a tail
        for i, (a, g_) in enumerate(edge):
            j = perm * (len(edge) + 1) + i
            if j < n:
                acc[j] = a
                grad[j] = g_
    return acc, grad


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gdt", [BF, F32], ids=["bf16", "fp32"])
def test_grad_accumulate_every_mode_against_cpu_arithmetic(T, gdt, n):
    acc0, g0 = _special(n, gdt, 900 + n % 977)
    want = {0: (g0.float(), g0), 1: (acc0 + g0.float(), g0), 2: (acc0, (acc0 + g0.float()).to(gdt))}
    for mode in (0, 1, 2):
        acc, grad = Guarded(acc0.to(DEV)), Guarded(g0.to(DEV))
        T.grad_accumulate(acc.t, grad.t, mode)
        torch.cuda.synchronize()
        what = f"grad_accumulate {gdt} n={n} mode={mode}"
        assert _same_bits(acc.t, want[mode][0]), what + ": acc"
        assert _same_bits(grad.t, want[mode][1]), what + ": grad"
        assert acc.intact() and grad.intact(), what + ": guard band overwritten"
        if mode == 2:      # acc untouched: its very bits, NaN payloads included
            assert torch.equal(acc.t.view(torch.int32).cpu(), acc0.view(torch.int32)), what
        else:              # grad untouched
            it = torch.int16 if gdt == BF else torch.int32
            assert torch.equal(grad.t.view(it).cpu(), g0.view(it)), what


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gdt", [BF, F32], ids=["bf16", "fp32"])
def test_grad_accumulate_sequence_is_the_ordered_fp32_sum(T, gdt, n):
    """Modes 0, 1, 1, 2 over four micro-gradients: the bucket ends as T(((g0 + g1) + g2) + g3), one rounding to T."""
    gen = torch.Generator("cpu").manual_seed(950 + n % 977)
    gs = [(torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-3, 3, (1,), generator=gen))).to(gdt) for _ in range(4)]
    acc = Guarded(torch.full((n,), float("nan"), device=DEV))       # mode 0 must not read it: NaN would stick
    last = None
    for g_, mode in zip(gs, (0, 1, 1, 2)):
        last = Guarded(g_.to(DEV))
        T.grad_accumulate(acc.t, last.t, mode)
    torch.cuda.synchronize()
    s = ((gs[0].float() + gs[1].float()) + gs[2].float())
    assert torch.equal(acc.t.cpu(), s)
    assert torch.equal(last.t.cpu(), (s + gs[3].float()).to(gdt))
    assert acc.intact() and last.intact()
    if gdt == BF and n >= 1023:      # one rounding, not four: summing in bf16 gives something else
        naive = ((gs[0] + gs[1]) + gs[2]) + gs[3]
        assert not torch.equal(last.t.cpu(), naive)


def test_wrappers_refuse_mismatched_tensors(T):
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    acc = torch.zeros(8, device=DEV)
    with pytest.raises(VgptError, match="length"):
        T.grad_accumulate(acc, torch.zeros(9, device=DEV), 0)
    with pytest.raises(VgptError, match="dtype"):
        T.grad_accumulate(acc.to(BF), torch.zeros(8, device=DEV), 0)
    with pytest.raises(VgptError, match="bf16 or fp32"):
        T.grad_accumulate(acc, torch.zeros(8, device=DEV, dtype=torch.float16), 0)
    with pytest.raises(VgptError, match="bad argument"):
        T.grad_accumulate(acc, torch.zeros(8, device=DEV), 3)
    with pytest.raises(VgptError, match="aligned"):
        T.grad_accumulate(torch.zeros(9, device=DEV)[1:], torch.zeros(8, device=DEV), 0)
