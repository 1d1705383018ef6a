"""The deterministic twins of the three atomic reductions of the training step (include/vgpt.h: vgpt_rmsnorm_bwd_det,
vgpt_ln_mod_bwd_det, vgpt_embed_bwd_det) on the GPU, called through the C ABI with buffers this file owns:

  * what the twin computes without a reduction (dx / rstd, dhidden) comes back bit for bit;
  * the reduced outputs (dw, dmod, dtable) meet the float64 restatement under the bound the atomic entry point is held to
    in tests/test_train_kernels_gpu.py (same additions, another order), and accumulate into a pre-filled buffer;
  * ten launches on fresh, identically filled buffers give the same bits, and so does a launch that runs beside a 256 MB
    copy on another stream (the scheduling change that reorders atomics: a smoke -- the proof is one writer per element);
  * every output and the workspace sit between NaN guard bands that must come back untouched.
"""
import importlib

import pytest
import torch

from tests.test_ops_gpu import bf, g
from tests.test_train_kernels_gpu import U32, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
PAD = 64          # guard elements on each side of a guarded buffer (a multiple of 16 bytes for every dtype used)
REPEATS = 10


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("video-gpt_amd.ops_train")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("video-gpt_amd._lib")


@pytest.fixture(scope="module")
def busy(L):
    """busy(): starts a 256 MB vgpt_calib_copy on a side stream; the caller's next launch runs beside it."""
    n = 256 << 20
    src = torch.zeros(n, dtype=torch.uint8, device=DEV)
    dst = torch.empty(n, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)

    def start():
        side.wait_stream(torch.cuda.current_stream())
        L.call("vgpt_calib_copy", src.data_ptr(), dst.data_ptr(), n, side.cuda_stream)
    yield start
    torch.cuda.synchronize()


class Guarded:
    """A flat buffer of `n` elements between two NaN bands of PAD elements; .t is the payload, .check() the bands."""

    def __init__(self, n, dtype, like=None):
        self.buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n]
        if like is not None:
            self.t.copy_(like.reshape(-1))
        self.n = n

    def check(self, what):
        idt = torch.int16 if self.buf.element_size() == 2 else torch.int32
        nan = torch.full((PAD,), float("nan"), dtype=self.buf.dtype, device=DEV).view(idt)
        assert torch.equal(self.buf[:PAD].view(idt), nan), f"{what}: bytes before the buffer changed"
        assert torch.equal(self.buf[PAD + self.n:].view(idt), nan), f"{what}: bytes past the buffer changed"


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: bits differ"


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ============================================================================================================
# RMSNorm backward
# ============================================================================================================
def _rms_det(L, x, w, dy, dres, dw0, eps):
    """One vgpt_rmsnorm_bwd_det launch on fresh guarded buffers -> (dx, rstd, dw) clones."""
    rows, H = x.shape
    need = L.load().vgpt_rmsnorm_bwd_det_workspace_bytes(rows, H)
    assert need >= 0 and need % 4 == 0
    dx, rstd, dw = Guarded(rows * H, BF), Guarded(rows, F32), Guarded(H, F32, like=dw0)
    ws = Guarded(need // 4, F32)          # exactly what the query answers, NaN-filled: nothing is read before written
    L.call("vgpt_rmsnorm_bwd_det", x.data_ptr(), w.data_ptr(), dy.data_ptr(), None if dres is None else dres.data_ptr(),
           dx.t.data_ptr(), dw.t.data_ptr(), rstd.t.data_ptr(), rows, H, eps, ws.t.data_ptr(), ws.n, _stream())
    torch.cuda.synchronize()
    for name, b in (("dx", dx), ("rstd", rstd), ("dw", dw), ("workspace", ws)):
        b.check(f"rmsnorm_bwd_det {name}")
    return dx.t.clone(), rstd.t.clone(), dw.t.clone()


def _rms_twin(L, x, w, dy, dres, dw0, eps):
    rows, H = x.shape
    dx = torch.empty(rows * H, dtype=BF, device=DEV)
    rstd = torch.empty(rows, dtype=F32, device=DEV)
    dw = dw0.clone()
    L.call("vgpt_rmsnorm_bwd", x.data_ptr(), w.data_ptr(), dy.data_ptr(), None if dres is None else dres.data_ptr(),
           dx.data_ptr(), dw.data_ptr(), rstd.data_ptr(), rows, H, eps, _stream())
    return dx, rstd, dw


@pytest.mark.parametrize("H", [192, 520, 3072, 4096])
@pytest.mark.parametrize("rows", [1, 9, 67, 515, 1030])     # 1 strip, 3 strips, 17, 103 (of 5 rows), 115 (of 9)
def test_rmsnorm_backward(L, busy, H, rows):
    gen = g(700 + rows + H)
    x = bf(torch.randn(rows, H, generator=gen) * 2).to(DEV, BF)
    w = bf(1 + 0.3 * torch.randn(H, generator=gen)).to(DEV, BF)
    dy = bf(torch.randn(rows, H, generator=gen)).to(DEV, BF)
    dres = bf(torch.randn(rows, H, generator=gen)).to(DEV, BF)
    dw0 = torch.randn(H, generator=gen).to(DEV)              # a pre-filled dw: the call accumulates
    zero = torch.zeros(H, device=DEV)
    eps = 1e-5
    rstd64 = torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + eps)
    terms = dy.double() * x.double() * rstd64
    n_add = rows / 512 + 133     # section B of test_train_kernels_gpu.py: lane chain + 3 LDS + <= 128 strips + initial value
    for res in (None, dres):
        what = f"rmsnorm_bwd_det H={H} rows={rows} dres={res is not None}"
        dx_t, rstd_t, _ = _rms_twin(L, x, w, dy, res, dw0, eps)
        dx, rstd, dw = _rms_det(L, x, w, dy, res, dw0, eps)
        _same_bits(dx, dx_t, what + " dx")
        _same_bits(rstd, rstd_t, what + " rstd")
        _within(dw, dw0.double() + terms.sum(0), n_add * U32 * (terms.abs().sum(0) + dw0.double().abs()) + 1e-30, what + " dw")
        _, _, dwz = _rms_det(L, x, w, dy, res, zero, eps)
        _within(dwz, terms.sum(0), n_add * U32 * terms.abs().sum(0) + 1e-30, what + " dw from zero")
        # pre-fill + gradient: the total is formed first and added to the caller's value in one fp32 addition
        assert torch.equal(dw, dw0 + dwz), what + ": dw is not pre-fill + gradient"
    for i in range(REPEATS):
        _same_bits(_rms_det(L, x, w, dy, dres, dw0, eps)[2], dw, f"{what} launch {i}")
    busy()
    _same_bits(_rms_det(L, x, w, dy, dres, dw0, eps)[2], dw, what + " beside a busy stream")


# ============================================================================================================
# final-layer adaLN backward
# ============================================================================================================
def _ln_det(L, dv, xhat, rstd, mod, dst, n_rows, dmod0, nf, ntok, H):
    need = L.load().vgpt_ln_mod_bwd_det_workspace_bytes(nf, ntok, H)
    assert need >= 0 and need % 4 == 0
    dhid = Guarded(n_rows * H, BF)
    dhid.t.fill_(7.0)
    dmod = Guarded(nf * 2 * H, F32, like=dmod0)
    ws = Guarded(need // 4, F32)
    L.call("vgpt_ln_mod_bwd_det", dv.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), mod.data_ptr(), dst.data_ptr(),
           dhid.t.data_ptr(), dmod.t.data_ptr(), nf, ntok, H, ws.t.data_ptr(), ws.n, _stream())
    torch.cuda.synchronize()
    for name, b in (("dhidden", dhid), ("dmod", dmod), ("workspace", ws)):
        b.check(f"ln_mod_bwd_det {name}")
    return dhid.t.clone().view(n_rows, H), dmod.t.clone().view(nf, 2 * H)


# the (nf, ntok) grid of test_ln_mod_forward_and_backward (ntok = 1 included) + token counts that are no multiple of the
# tokens a wave walks (ceil(ntok / 64): 130 -> 3, the last wave gets one token; 1000 -> 16, the last wave gets 8)
@pytest.mark.parametrize("H", [192, 3072])
@pytest.mark.parametrize("nf,ntok", [(1, 1), (3, 5), (16, 256), (3, 1024), (16, 1024), (1, 256), (16, 1), (2, 130), (3, 1000)])
def test_ln_mod_backward(T, L, busy, H, nf, ntok):
    gen = g(800 + H + nf + ntok)
    gap0, gap = 3, 2
    n_rows = gap0 + nf * (ntok + gap)
    src = torch.tensor([gap0 + f * (ntok + gap) for f in range(nf)], dtype=torch.int32)
    dst = src.flip(0).contiguous().to(DEV)
    hidden = bf(torch.randn(n_rows, H, generator=gen) * 1.5 + 0.3).to(DEV, BF)
    mod = bf(0.5 * torch.randn(nf, 2 * H, generator=gen)).to(DEV, BF)
    eps = 1e-6
    v = torch.empty(nf * ntok, H, dtype=BF, device=DEV)
    xhat = torch.empty(nf * ntok, H, dtype=F32, device=DEV)
    rstd = torch.empty(nf * ntok, dtype=F32, device=DEV)
    T.ln_mod_fwd(hidden, src.to(DEV), mod, v, xhat, rstd, ntok, eps)
    dv = bf(torch.randn(nf * ntok, H, generator=gen)).to(DEV, BF)
    dmod0 = torch.randn(nf, 2 * H, generator=gen).to(DEV)
    zero = torch.zeros(nf, 2 * H, device=DEV)
    what = f"ln_mod_bwd_det H={H} nf={nf} ntok={ntok}"

    dhid_t = torch.full((n_rows, H), 7.0, dtype=BF, device=DEV)
    T.ln_mod_bwd(dv, xhat, rstd, mod, dst, dhid_t, dmod0.clone(), ntok)
    dhid, dmod = _ln_det(L, dv, xhat, rstd, mod, dst, n_rows, dmod0, nf, ntok, H)
    _same_bits(dhid, dhid_t, what + " dhidden")        # rows outside the frames keep the sentinel in both

    # float64 restatement and bound of test_ln_mod_forward_and_backward (section D): xhat restated from the hidden rows
    rows_of = (src[:, None].long() + torch.arange(ntok)).reshape(-1).to(DEV)
    x64 = hidden.double()[rows_of]
    mean = x64.mean(-1, keepdim=True)
    xh = (x64 - mean) * torch.rsqrt((x64 - mean).pow(2).mean(-1, keepdim=True) + eps)
    t_sh = dv.double().view(nf, ntok, H)
    t_sc = (dv.double() * xh).view(nf, ntok, H)
    grad = torch.cat([t_sh.sum(1), t_sc.sum(1)], 1)
    mag = torch.cat([t_sh.abs().sum(1), t_sc.abs().sum(1)], 1)
    _within(dmod, dmod0.double() + grad, 4e-6 * (mag + dmod0.double().abs()) + 1e-30, what + " dmod")
    _, dmodz = _ln_det(L, dv, xhat, rstd, mod, dst, n_rows, zero, nf, ntok, H)
    # from zero there is no pre-fill to lend the bound slack for the fp32 xhat the kernel is handed (2e-6 (1 + |xhat|) off
    # the float64 one, section D): restated on that input, as the kernel reads it
    k_sc = (dv.double() * xhat.double()).view(nf, ntok, H)
    _within(dmodz, torch.cat([t_sh.sum(1), k_sc.sum(1)], 1), 4e-6 * torch.cat([t_sh.abs().sum(1), k_sc.abs().sum(1)], 1) + 1e-30,
            what + " dmod from zero")
    assert torch.equal(dmod, dmod0 + dmodz), what + ": dmod is not pre-fill + gradient"
    for i in range(REPEATS):
        _same_bits(_ln_det(L, dv, xhat, rstd, mod, dst, n_rows, dmod0, nf, ntok, H)[1], dmod, f"{what} launch {i}")
    busy()
    _same_bits(_ln_det(L, dv, xhat, rstd, mod, dst, n_rows, dmod0, nf, ntok, H)[1], dmod, what + " beside a busy stream")


# ============================================================================================================
# embedding backward
# ============================================================================================================
def _emb_det(L, ids, keep, dseq, table0):
    rows, H = dseq.shape
    vocab = table0.shape[0]
    need = L.load().vgpt_embed_bwd_det_workspace_bytes(rows)
    assert need >= 0 and need % 4 == 0
    dt = Guarded(vocab * H, F32, like=table0)
    ws = Guarded(need // 4, F32)
    L.call("vgpt_embed_bwd_det", ids.data_ptr(), keep.data_ptr(), dseq.data_ptr(), dt.t.data_ptr(), rows, H, vocab,
           ws.t.data_ptr(), ws.n, _stream())
    torch.cuda.synchronize()
    dt.check("embed_bwd_det dtable")
    ws.check("embed_bwd_det workspace")
    return dt.t.clone().view(vocab, H)


def _id_patterns(rows, vocab, gen):
    """name -> (ids, keep).  Ids are int64, keep uint8."""
    ones = torch.ones(rows, dtype=torch.uint8)
    pats = {"one_id": (torch.full((rows,), vocab // 3, dtype=torch.int64), ones)}
    # all distinct where the vocabulary allows it, else every id rows / vocab times, in a shuffled order
    pats["distinct"] = ((torch.randperm(max(rows, vocab), generator=gen)[:rows] % vocab).long(), ones)
    pad = torch.randint(0, vocab, (rows,), generator=gen)
    pad[torch.rand(rows, generator=gen) < 0.9] = vocab - 1                 # the stage-1 shape: one id on 90 % of the rows
    pats["pad90"] = (pad, ones)
    oor = torch.randint(0, vocab, (rows,), generator=gen)
    bad = torch.tensor([-1, -(1 << 40), vocab, vocab + 10, 1 << 40, (1 << 32) + 5])   # (1 << 32) + 5: in range as 32 bits
    where = torch.randperm(rows, generator=gen)[: max(1, rows // 4)]
    oor[where] = bad[torch.arange(where.numel()) % bad.numel()]
    pats["out_of_range"] = (oor, ones)
    keep = (torch.rand(rows, generator=gen) > 0.4).to(torch.uint8)
    keep[0] = 0
    pats["keep0"] = (torch.randint(0, min(vocab, 8), (rows,), generator=gen), keep)
    return pats


def _added(ids, keep, vocab):
    return keep.bool() & (ids >= 0) & (ids < vocab)


@pytest.mark.parametrize("vocab", [64, 1000])
@pytest.mark.parametrize("H", [192, 520, 3072])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_embed_backward_exact_integers(L, rows, H, vocab):
    """dseq holds integers in [-8, 8] and the table small integers: every fp32 sum is exact in any order, so the result
    equals an integer scatter-add bit for bit; table rows whose id never occurs keep their bits, a NaN pre-fill included."""
    gen = g(900 + rows + H + vocab)
    dseq = torch.randint(-8, 9, (rows, H), generator=gen)
    table = torch.randint(-100, 101, (vocab, H), generator=gen)
    for name, (ids, keep) in _id_patterns(rows, vocab, gen).items():
        sel = _added(ids, keep, vocab)
        ref = table.clone().index_add(0, ids[sel], dseq[sel]).float()
        touched = torch.zeros(vocab, dtype=torch.bool)
        touched[ids[sel]] = True
        t0 = table.float()
        t0[~touched] = float("nan")
        ref[~touched] = float("nan")
        out = _emb_det(L, ids.to(DEV), keep.to(DEV), dseq.to(DEV, BF), t0.to(DEV))
        _same_bits(out, ref.to(DEV), f"embed_bwd_det {name} rows={rows} H={H} vocab={vocab}")


@pytest.mark.parametrize("vocab", [64, 1000])
@pytest.mark.parametrize("H", [192, 520, 3072])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_embed_backward_random_values(T, L, busy, rows, H, vocab):
    gen = g(950 + rows + H + vocab)
    dseq = bf(torch.randn(rows, H, generator=gen)).to(DEV, BF)
    table = torch.randn(vocab, H, generator=gen).to(DEV)
    pats = _id_patterns(rows, vocab, gen)
    for name in ("pad90", "keep0", "out_of_range"):
        ids, keep = pats[name]
        what = f"embed_bwd_det {name} rows={rows} H={H} vocab={vocab}"
        sel = _added(ids, keep, vocab).to(DEV)
        ids_d, keep_d = ids.to(DEV), keep.to(DEV)
        ref = table.double().index_add(0, ids_d[sel], dseq.double()[sel])
        mag = table.double().abs().index_add(0, ids_d[sel], dseq.double().abs()[sel])
        n_id = torch.zeros(vocab, dtype=torch.float64, device=DEV).index_add(0, ids_d[sel], torch.ones(int(sel.sum()), dtype=torch.float64, device=DEV))
        bound = n_id[:, None] * U32 * mag          # n_id additions (n_id - 1 among the rows, one onto the table); 0 where no row
        out = _emb_det(L, ids_d, keep_d, dseq, table)
        assert torch.equal(out[n_id == 0], table[n_id == 0]), what + ": a row whose id never occurs changed"
        live = n_id > 0
        twin = table.clone()
        T.embed_bwd(ids_d, keep_d, dseq, twin)
        if bool(live.any()):       # rows = 1 with its one row not kept: nothing is added, and the line above said it all
            _within(out[live], ref[live], bound[live] + 1e-30, what + " vs float64")
            _within(out[live], twin[live], bound[live] + 1e-30, what + " vs the atomic twin")
        for i in range(REPEATS):
            _same_bits(_emb_det(L, ids_d, keep_d, dseq, table), out, f"{what} launch {i}")
        busy()
        _same_bits(_emb_det(L, ids_d, keep_d, dseq, table), out, what + " beside a busy stream")


def test_wrappers_take_the_flag(T):
    """ops_train's deterministic=True reaches the same entry points with a workspace the module owns and grows."""
    gen = g(990)
    rows, H, vocab = 130, 520, 50
    x = bf(torch.randn(rows, H, generator=gen)).to(DEV, BF)
    w = bf(1 + 0.3 * torch.randn(H, generator=gen)).to(DEV, BF)
    dy = bf(torch.randn(rows, H, generator=gen)).to(DEV, BF)
    outs = []
    for _ in range(2):
        dx = torch.empty(rows, H, dtype=BF, device=DEV)
        dw = torch.zeros(H, device=DEV)
        T.rmsnorm_bwd(x, w, dy, dx, dw, 1e-5, deterministic=True)
        ids = torch.randint(0, vocab, (rows,), generator=g(991)).to(DEV)
        keep = torch.ones(rows, dtype=torch.uint8, device=DEV)
        dt = torch.zeros(vocab, H, device=DEV)
        T.embed_bwd(ids, keep, dy, dt, deterministic=True)
        outs.append((dx, dw, dt))
    dx_t = torch.empty(rows, H, dtype=BF, device=DEV)
    dw_t = torch.zeros(H, device=DEV)
    T.rmsnorm_bwd(x, w, dy, dx_t, dw_t, 1e-5)
    _same_bits(outs[0][0], dx_t, "wrapper dx")
    assert torch.allclose(outs[0][1], dw_t, rtol=1e-4, atol=1e-4)
    for a, b in zip(*outs):
        _same_bits(a, b, "wrapper repeat")
    ref = torch.zeros(vocab, H, dtype=torch.float64, device=DEV).index_add(0, ids, dy.double())
    assert torch.allclose(outs[0][2].double(), ref, rtol=1e-5, atol=1e-5)
