"""The frame-preprocessing kernels (include/vgpt.h, "frame preprocessing") against Pillow, bit for bit: each pass of
vgpt_resample_u8, the two-pass resize, the crop + normalise kernel and the fused last pass.  Every destination and workspace
is a slice of a buffer with 64 sentinel bytes on either side, which must come back untouched.  The oracle is the Pillow
installed here; tests/test_preprocess_cabi.py shows a disagreeing Pillow version without a GPU."""
import importlib

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX, BICUBIC = 0, 1
PIL_FILTER = {BOX: Image.BOX, BICUBIC: Image.BICUBIC}
GUARD, MARK = 64, 0xA5
# (H, W) -> (h, w): the no-GPU table test's shapes
SHAPES = [((7, 9), (3, 4)), ((33, 47), (16, 23)), ((100, 64), (37, 64)), ((17, 5), (54, 16)), ((129, 257), (64, 128)),
          ((31, 31), (31, 16)), ((64, 64), (5, 5))]
# tile tails of the horizontal pass (64 output pixels per tile), rows shorter than a dword, heights 1 and 3
EDGES = ([((5, 300), (5, w)) for w in (63, 64, 65, 257)]
         + [((5, 30), (5, 1))]                                           # out width 1 from a width inside the ksize cap
         + [((6, 1), (4, 3)), ((6, 2), (3, 5)), ((9, 5), (4, 2)), ((9, 5), (9, 11))]
         + [((1, 40), (1, 17)), ((3, 40), (1, 40)), ((1, 9), (3, 9)), ((3, 21), (7, 10)), ((40, 700), (90, 700))])
# ksize at the cap of 129, one filter each (the other filter's ksize is over it); ratios at which the launch shrinks its
# tile to keep the staged span inside LDS (vertical: 16 -> 2 output rows at ratio 30)
CASES = ([(s, f) for s in SHAPES + EDGES for f in (BOX, BICUBIC)]
         + [(((3, 128), (2, 1)), BOX), (((2, 32), (2, 1)), BICUBIC), (((32, 3), (1, 3)), BICUBIC),
            (((600, 3), (20, 3)), BICUBIC), (((3, 600), (3, 20)), BICUBIC), (((2, 4000), (2, 125)), BOX)])


@pytest.fixture(scope="module")
def oi():
    return importlib.import_module("video-gpt_amd.ops_image")


def frames_u8(N, H, W, seed):
    """Random bytes, a third of the rows 0 / 255 only (those drive the bicubic lobes into the clamp)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    sat = rng.integers(0, 2, (N, H, W, 3), dtype=np.uint8) * 255
    x[:, ::3] = sat[:, ::3]
    return x


def pil_resize(x, w, h, filt):
    return np.stack([np.array(Image.fromarray(f).resize((w, h), resample=PIL_FILTER[filt])) for f in x])


class Guarded:
    """A tensor of `shape` inside a buffer with GUARD sentinel bytes before and after it."""

    def __init__(self, shape, dtype=torch.uint8, skew=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + skew + n + GUARD,), MARK, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = GUARD + skew, GUARD + skew + n
        self.t = self.buf[self.lo:self.hi].view(dtype).view(shape)

    def check(self):
        assert bool((self.buf[:self.lo] == MARK).all()) and bool((self.buf[self.hi:] == MARK).all()), "sentinel overwritten"
        return self.t


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0][0]}x{c[0][0][1]}to{c[0][1][0]}x{c[0][1][1]}-{'bicubic' if c[1] else 'box'}")
def test_passes_and_resize_equal_pillow(oi, case, N):
    ((H, W), (h, w)), filt = case
    x = frames_u8(N, H, W, 1000 * H + W)
    xd = torch.from_numpy(x).to(DEV)
    # each pass alone, against Pillow resizing that axis only; skew 1 and 2 put the destinations on odd addresses
    if w != W:
        g = Guarded((N, H, w, 3), skew=1)
        oi.resample_pass(xd, w, filt, 1, out=g.t)
        assert torch.equal(g.check().cpu(), torch.from_numpy(pil_resize(x, w, H, filt)))
    if h != H:
        g = Guarded((N, h, W, 3), skew=2)
        oi.resample_pass(xd, h, filt, 0, out=g.t)
        assert torch.equal(g.check().cpu(), torch.from_numpy(pil_resize(x, W, h, filt)))
    # the resize: horizontal pass into the workspace, vertical pass on its uint8 result
    want = torch.from_numpy(pil_resize(x, w, h, filt))
    out, ws = Guarded((N, h, w, 3)), Guarded((N * H * w * 3,), skew=3)
    oi.resample_u8(xd, (w, h), filt, out=out.t, workspace=ws.t)
    ws.check()
    assert torch.equal(out.check().cpu(), want)
    # the cached workspace gives the same image, and so does a second launch
    again = oi.resample_u8(xd, (w, h), filt)
    assert torch.equal(again, out.t) and torch.equal(oi.resample_u8(xd, (w, h), filt), again)
    # the frames of a batch equal single-frame launches
    if N > 1:
        for i in range(N):
            assert torch.equal(oi.resample_u8(xd[i:i + 1], (w, h), filt), out.t[i:i + 1])


@pytest.mark.parametrize("filt,w", [(BOX, 1), (BICUBIC, 1), (BICUBIC, 9)])
def test_ksize_over_the_cap_is_refused(oi, filt, w):
    """Width 300 -> 1 needs ksize 301 (BOX) / 1201 (BICUBIC), 300 -> 9 BICUBIC 135: over VGPT_RESAMPLE_MAX_KSIZE = 129,
    refused before any launch with the value in the message."""
    xd = torch.zeros(1, 4, 300, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(oi.VgptError, match=r"ksize = \d+ .*exceeds 129"):
        oi.resample_u8(xd, (w, 4), filt)


def test_wrappers_refuse_what_the_kernels_do_not_take(oi):
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(oi.VgptError, match="GPU tensor"):
        oi.resample_u8(x.cpu(), (4, 4), BOX)
    with pytest.raises(oi.VgptError, match=r"\(N, H, W, 3\)"):
        oi.resample_u8(torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=DEV), (4, 4), BOX)
    with pytest.raises(oi.VgptError, match="contiguous"):
        oi.resample_u8(torch.zeros(1, 8, 3, 8, dtype=torch.uint8, device=DEV).permute(0, 1, 3, 2), (4, 4), BOX)
    with pytest.raises(oi.VgptError, match="dtype"):
        oi.u8_to_chw_norm(x.float())
    with pytest.raises(oi.VgptError, match=r"x0 = 4.*w = 8.*W = 8"):
        oi.u8_to_chw_norm(x, (4, 0, 12, 8))
    with pytest.raises(oi.VgptError, match="filter = 5"):
        oi.resample_u8(x, (4, 4), 5)


def _norm_cpu(x_u8, box):
    """ToTensor + Normalize(0.5, 0.5) on the CPU, on the crop `box` = (left, upper, right, lower) of (N, H, W, 3) uint8."""
    x0, y0, x1, y1 = box
    t = x_u8[:, y0:y1, x0:x1].permute(0, 3, 1, 2)
    return (t.float().div(255.0) - 0.5) / 0.5


def test_u8_to_chw_norm_on_all_byte_values(oi):
    """Every byte value in every channel, on a row longer than one 256-pixel piece, whole image and an odd-offset crop."""
    v = torch.arange(256, dtype=torch.uint8)
    x = torch.stack([v.roll(7 * c + 3 * y) for y in range(5) for c in range(3)]).view(5, 3, 256).permute(0, 2, 1)   # (5, 256, 3)
    x = torch.cat([x, x.flip(1), x[:, :9]], dim=1)[None].repeat(2, 1, 1, 1).contiguous()                           # (2, 5, 521, 3)
    x[1] = x[1].flip(0)
    xd = x.to(DEV)
    for box in ((0, 0, 521, 5), (1, 1, 520, 4), (3, 1, 260, 2), (257, 0, 258, 5), (5, 2, 21, 5)):
        g = Guarded((2, 3, box[3] - box[1], box[2] - box[0]), dtype=torch.float32)
        oi.u8_to_chw_norm(xd, box, out=g.t)
        want = _norm_cpu(x, box)
        assert torch.equal(g.check().cpu(), want), box
        assert torch.equal(oi.u8_to_chw_norm(xd[1:2], box), g.t[1:2])
    got = oi.u8_to_chw_norm(xd)
    assert float(got.min()) == -1.0 and float(got.max()) == 1.0 and set(got.unique().tolist()) == set(_norm_cpu(x, (0, 0, 521, 5)).unique().tolist())


@pytest.mark.parametrize("filt", [BOX, BICUBIC], ids=["box", "bicubic"])
@pytest.mark.parametrize("case", [((33, 23), 16, (1, 3, 16, 16)),      # the vertical pass of 33x47 -> 16x23, crop box (1, 3, 16, 16)
                                  ((33, 47), 16, (3, 1, 19, 16)),      # a 16-wide window at odd offsets
                                  ((17, 5), 54, (0, 3, 5, 51)),        # enlarging, a window 5 wide
                                  ((17, 70), 54, (1, 0, 70, 54)),      # more than one 64-pixel strip, unaligned float rows
                                  ((40, 200), 20, (4, 2, 196, 18)),
                                  ((9, 16), 3, None)],
                         ids=["33x23to16", "33x47to16", "17x5to54", "17x70to54", "40x200to20", "9x16to3-whole"])
def test_fused_vertical_pass_equals_the_unfused_pair(oi, case, filt):
    (H, W), out_h, box = case
    N = 2
    x = frames_u8(N, H, W, 7 * H + W)
    xd = torch.from_numpy(x).to(DEV)
    mid = oi.resample_pass(xd, out_h, filt, 0)
    assert torch.equal(mid.cpu(), torch.from_numpy(pil_resize(x, W, out_h, filt)))
    pair = oi.u8_to_chw_norm(mid, box)
    b = (0, 0, W, out_h) if box is None else box
    g = Guarded((N, 3, b[3] - b[1], b[2] - b[0]), dtype=torch.float32)
    oi.resample_v_chw_norm(xd, out_h, filt, box, out=g.t)
    assert torch.equal(g.check(), pair)
    assert torch.equal(pair.cpu(), _norm_cpu(mid.cpu(), b))
    assert torch.equal(oi.resample_v_chw_norm(xd[1:2], out_h, filt, box), pair[1:2])


@pytest.mark.parametrize("shape", [((33, 47), (16, 23)), ((100, 64), (37, 64)), ((31, 31), (31, 16)), ((17, 5), (54, 16)),
                                   ((20, 20), (20, 20))], ids=["two-pass", "vertical-only", "horizontal-only", "enlarging", "copy"])
def test_resample_chw_norm_equals_resize_then_normalise(oi, shape):
    (H, W), (h, w) = shape
    x = frames_u8(2, H, W, 31 * H + W)
    xd = torch.from_numpy(x).to(DEV)
    box = (w % 16 // 2, h % 16 // 2, w - (w % 16 - w % 16 // 2), h - (h % 16 - h % 16 // 2))
    ws = Guarded((2 * H * w * 3,), skew=1)
    got = oi.resample_chw_norm(xd, (w, h), BICUBIC, box, workspace=ws.t)
    ws.check()
    want = _norm_cpu(torch.from_numpy(pil_resize(x, w, h, BICUBIC)), box)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(oi.u8_to_chw_norm(oi.resample_u8(xd, (w, h), BICUBIC), box), got)
