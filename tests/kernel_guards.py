"""Guard-banded device allocations and bf16 ulp helpers shared by the element-wise kernel tests (a plain module: import it,
it registers nothing with pytest).

Guarded(rows, cols, dtype, ld=...) is a (rows, cols) tensor in the middle of a sentinel-filled allocation: BAND elements of
sentinel in front, BAND behind, and, where the row stride ld is larger than cols, sentinel in every padding column.  A kernel
that reads a band or a padding column poisons its result (NaN for float / bf16); one that writes there is caught by
bands_intact().  The sentinels are NaN (float32, bfloat16), 0xDEADBEEF (int32; uint32 data travels as int32),
0xDEADBEEFDEADBEEF (int64) and 0xA5 (uint8).  BAND * itemsize is a multiple of 16 for every dtype, so the inner view starts
16-byte aligned; rows stay aligned when ld * itemsize is a multiple of 16."""
import torch

DEV = "cuda:0"
BF = torch.bfloat16
BAND = 64

_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64,
         torch.uint8: torch.uint8}
_INT_SENTINEL = {torch.int32: 0xDEADBEEF - (1 << 32), torch.int64: 0xDEADBEEFDEADBEEF - (1 << 64), torch.uint8: 0xA5}


def sentinel(dtype):
    return float("nan") if dtype.is_floating_point else _INT_SENTINEL[dtype]


class Guarded:
    """A (rows, cols) tensor `t` with row stride `ld` in the middle of a sentinel-filled allocation `full`."""

    def __init__(self, rows, cols, dtype, ld=None, device=DEV):
        ld = cols if ld is None else ld
        assert ld >= cols and dtype in _BITS
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        n = rows * ld
        self.full = torch.full((n + 2 * BAND,), sentinel(dtype), dtype=dtype, device=device)
        self.padded = self.full[BAND:BAND + n].view(rows, ld)
        self.t = self.padded[:, :cols]
        assert self.t.data_ptr() % 16 == 0
        live = torch.zeros(n + 2 * BAND, dtype=torch.bool, device=device)
        live[BAND:BAND + n].view(rows, ld)[:, :cols] = True
        self._dead = ~live
        self._sentinel_bits = self.full.view(_BITS[dtype])[0].clone()

    @classmethod
    def of(cls, value, ld=None, device=DEV):
        """A guarded copy of a CPU tensor (1-D values become one row)."""
        v = value.reshape(1, -1) if value.dim() < 2 else value.reshape(-1, value.shape[-1])
        g = cls(v.shape[0], v.shape[1], value.dtype, ld, device)
        g.t.copy_(v)
        return g

    def bands_intact(self):
        """Both bands and every padding column still hold the sentinel, bit for bit."""
        return bool((self.full.view(_BITS[self.dtype])[self._dead] == self._sentinel_bits).all())

    def bits(self):
        """A copy of the whole allocation as integers: equal before and after a launch <=> the launch wrote nothing."""
        return self.full.view(_BITS[self.dtype]).clone()

    def flat(self):
        """The inner elements as one contiguous 1-D view (only without row padding)."""
        assert self.ld == self.cols
        return self.full[BAND:BAND + self.rows * self.cols]


def all_intact(*bufs):
    return all(b.bands_intact() for b in bufs)


# ---- bf16 ------------------------------------------------------------------------------------------------------------------

# One rounding to bf16 (8 significant bits) moves a value by at most half an ulp: 2^-9 of the value at the top of a binade,
# 2^-8 at the bottom.  Bounds on a single final rounding use half_ulp(reference), the exact figure; U is the relative worst
# case, for roundings whose binade the reference does not fix (a rounded intermediate that is multiplied on).
U = 2.0 ** -8
E = 2.0 ** -24    # the same for fp32 (24 significant bits), relative worst case


def to_bf16(x64):
    """float64 -> bf16 through float32 (the two roundings differ from one only within 2^-29 of a bf16 tie)."""
    return x64.to(torch.float32).to(BF)


def bf16_ordinal(x):
    """bf16 values as integers that count representable values: adjacent bf16 numbers differ by 1, -0 and +0 by 0."""
    b = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def bf16_ulps_apart(a, b):
    return (bf16_ordinal(a) - bf16_ordinal(b)).abs()


def bf16_ulp(x):
    """The spacing of bf16 numbers at |x| (fp64 in, fp64 out; normal range)."""
    x = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 7)


def half_ulp(x64):
    """The largest error of rounding x to bf16: between 2^-9 |x| and 2^-8 |x|."""
    return 0.5 * bf16_ulp(x64)


def half_ulp32(x64):
    """The largest error of rounding x to fp32 (normal range; 0 for x = 0): between 2^-25 |x| and 2^-24 |x|."""
    x = x64.double().abs()
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp_min(2.0 ** -126))) - 24), torch.zeros_like(x))


_BUTTERFLY = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def running_row_sum(terms64):
    """sum_k terms[..., k] in fp64 in the order the one-wave-per-row kernels add in fp32 (element k belongs to lane (k / 8) % 64
    of slab k / 512; every lane adds its terms in order of k, then the six xor-butterfly steps of common.h wave_sum), with
    the running error bound of that fp32 summation: half an fp32 ulp of every partial sum that an addition can round (one
    whose two operands are both non-zero).  Returns (sum, bound), first order in 2^-24."""
    n = terms64.shape[-1]
    slabs = (n + 511) // 512
    padded = torch.zeros(*terms64.shape[:-1], slabs * 512, dtype=torch.float64)
    padded[..., :n] = terms64
    t = padded.view(*terms64.shape[:-1], slabs, 64, 8)
    acc = torch.zeros(*terms64.shape[:-1], 64, dtype=torch.float64)
    err = torch.zeros_like(acc)
    for c in range(slabs):
        for j in range(8):
            a = t[..., c, :, j]
            rounds = (a != 0) & (acc != 0)
            acc = acc + a
            err = err + torch.where(rounds, half_ulp32(acc), torch.zeros_like(acc))
    for idx in _BUTTERFLY:
        b, eb = acc[..., idx], err[..., idx]
        rounds = (b != 0) & (acc != 0)
        acc = acc + b
        err = err + eb + torch.where(rounds, half_ulp32(acc), torch.zeros_like(acc))
    return acc[..., 0], err[..., 0]
