"""Frame preprocessing (include/vgpt.h, "frame preprocessing") without a GPU: the five symbols are exported, declared and
bound with the ABI version unchanged; every host-side refusal comes back before any launch with the documented code and the
offending value in vgpt_last_error(); the coefficient table equals a Python restatement of the header's arithmetic entry for
entry, and a numpy pass driven by the C table equals PIL.Image.resize byte for byte; crop_arr_plan / center_crop_plan give
the sizes and the crop of the Pillow code they restate."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # non-null addresses that are never dereferenced: every device call below returns before a launch
SRC, DST, BND, COF = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE
OK, INVALID, UNSUPPORTED = 0, -1, -2
BOX, BICUBIC = 0, 1
PIL_FILTER = {BOX: Image.BOX, BICUBIC: Image.BICUBIC}
NAMES = ("vgpt_resample_ksize", "vgpt_resample_coeffs", "vgpt_resample_u8", "vgpt_u8_to_chw_norm",
         "vgpt_resample_u8_v_chw_norm")
# (H, W) -> (h, w): both passes shrinking, odd sizes, one pass only, enlarging, a long table, one axis unchanged, ksize 53
SHAPES = [((7, 9), (3, 4)), ((33, 47), (16, 23)), ((100, 64), (37, 64)), ((17, 5), (54, 16)), ((129, 257), (64, 128)),
          ((31, 31), (31, 16)), ((64, 64), (5, 5))]


@pytest.fixture(scope="module")
def binding():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib


@pytest.fixture(scope="module")
def lib(binding):
    return binding.load()


@pytest.fixture(scope="module")
def processor_mod():
    return importlib.import_module("video-gpt_amd.processor")


def _refused(lib, rc, code, *texts):
    msg = lib.vgpt_last_error()
    assert rc == code, (rc, msg)
    for t in texts:
        assert t in msg, msg


# ---- symbols --------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_bound(binding, lib):
    hdr = open(os.path.join(ROOT, "include", "vgpt.h")).read()
    nargs = dict(zip(NAMES, (3, 5, 11, 10, 14)))
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in binding.SIGNATURES and len(binding.SIGNATURES[name][1]) == nargs[name], name
        assert re.search(rf"\bint {name}\(", hdr), name
    assert re.search(r"#define VGPT_FILTER_BOX 0\b", hdr) and re.search(r"#define VGPT_FILTER_BICUBIC 1\b", hdr)
    assert re.search(r"#define VGPT_RESAMPLE_MAX_KSIZE 129\b", hdr)
    assert (binding.FILTER_BOX, binding.FILTER_BICUBIC) == (0, 1)
    assert binding.missing_exports() == []


def test_abi_version_is_still_8(binding, lib):
    assert lib.vgpt_abi_version() == 8 == binding.ABI_VERSION


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_ksize_values_and_refusals(lib):
    assert lib.vgpt_resample_ksize(1280, 640, BOX) == 3
    assert lib.vgpt_resample_ksize(640, 320, BICUBIC) == 9
    assert lib.vgpt_resample_ksize(5, 16, BICUBIC) == 5      # enlarging: the support is the filter's own
    assert lib.vgpt_resample_ksize(64, 5, BICUBIC) == 53
    assert lib.vgpt_resample_ksize(128, 1, BOX) == 129
    assert lib.vgpt_resample_ksize(32, 1, BICUBIC) == 129
    _refused(lib, lib.vgpt_resample_ksize(0, 4, BOX), INVALID, b"vgpt_resample_ksize", b"in = 0")
    _refused(lib, lib.vgpt_resample_ksize(4, -2, BICUBIC), INVALID, b"out = -2")
    _refused(lib, lib.vgpt_resample_ksize(4, 4, 2), INVALID, b"filter = 2")
    _refused(lib, lib.vgpt_resample_ksize(4, 4, -1), INVALID, b"filter = -1")
    _refused(lib, lib.vgpt_resample_ksize(4096, 1, BOX), UNSUPPORTED, b"ksize = 4097", b"in = 4096", b"129")
    _refused(lib, lib.vgpt_resample_ksize(33, 1, BICUBIC), UNSUPPORTED, b"ksize = 133")
    _refused(lib, lib.vgpt_resample_ksize(2 ** 31 - 1, 1, BICUBIC), UNSUPPORTED, b"ksize = ")


def test_coeffs_refusals(lib):
    b, c = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 64)()
    _refused(lib, lib.vgpt_resample_coeffs(8, 4, BOX, None, c), INVALID, b"vgpt_resample_coeffs", b"null pointer")
    _refused(lib, lib.vgpt_resample_coeffs(8, 4, BOX, b, None), INVALID, b"null pointer")
    _refused(lib, lib.vgpt_resample_coeffs(0, 4, BOX, b, c), INVALID, b"in = 0")
    _refused(lib, lib.vgpt_resample_coeffs(8, 0, BOX, b, c), INVALID, b"out = 0")
    _refused(lib, lib.vgpt_resample_coeffs(8, 4, 7, b, c), INVALID, b"filter = 7")
    _refused(lib, lib.vgpt_resample_coeffs(4096, 1, BOX, b, c), UNSUPPORTED, b"ksize = 4097")
    assert lib.vgpt_resample_coeffs(8, 4, BOX, b, c) == OK


def _pass(lib, src=SRC, dst=DST, bounds=BND, coeffs=COF, ksize=9, n=1, in_h=8, in_w=8, out_len=4, axis=1):
    return lib.vgpt_resample_u8(src, dst, bounds, coeffs, ksize, n, in_h, in_w, out_len, axis, None)


@pytest.mark.parametrize("which", ["src", "dst", "bounds", "coeffs"])
def test_resample_null_pointer(lib, which):
    _refused(lib, _pass(lib, **{which: None}), INVALID, b"vgpt_resample_u8", b"null pointer")


def test_resample_refusals_name_the_value(lib):
    _refused(lib, _pass(lib, axis=2), INVALID, b"axis = 2")
    _refused(lib, _pass(lib, axis=-1), INVALID, b"axis = -1")
    _refused(lib, _pass(lib, n=-3), INVALID, b"n_frames = -3")
    _refused(lib, _pass(lib, in_h=0), INVALID, b"H = 0")
    _refused(lib, _pass(lib, in_w=-5), INVALID, b"W = -5")
    _refused(lib, _pass(lib, out_len=0), INVALID, b"out_len = 0")
    _refused(lib, _pass(lib, ksize=0), INVALID, b"ksize = 0")
    _refused(lib, _pass(lib, ksize=130), UNSUPPORTED, b"ksize = 130", b"129")
    _refused(lib, _pass(lib, ksize=4097, in_w=4096, out_len=1), UNSUPPORTED, b"ksize = 4097")
    _refused(lib, _pass(lib, in_w=(1 << 24) + 1), UNSUPPORTED, b"W = 16777217")
    _refused(lib, _pass(lib, dst=SRC), INVALID, b"overlaps")
    # n_frames = 0 returns VGPT_OK without a launch once every check has passed
    assert _pass(lib, n=0) == OK and _pass(lib, n=0, axis=0, ksize=129) == OK


def _norm(lib, src=SRC, dst=DST, n=1, H=20, W=30, y0=1, x0=3, h=16, w=16):
    return lib.vgpt_u8_to_chw_norm(src, dst, n, H, W, y0, x0, h, w, None)


def _fused(lib, src=SRC, dst=DST, bounds=BND, coeffs=COF, ksize=9, n=1, in_h=40, in_w=30, out_h=20, y0=1, x0=3, h=16, w=16):
    return lib.vgpt_resample_u8_v_chw_norm(src, dst, bounds, coeffs, ksize, n, in_h, in_w, out_h, y0, x0, h, w, None)


@pytest.mark.parametrize("call,name", [(_norm, b"vgpt_u8_to_chw_norm"), (_fused, b"vgpt_resample_u8_v_chw_norm")])
def test_crop_window_refusals_name_the_value(lib, call, name):
    _refused(lib, call(lib, src=None), INVALID, name, b"null pointer")
    _refused(lib, call(lib, dst=None), INVALID, name, b"null pointer")
    _refused(lib, call(lib, n=-1), INVALID, b"n_frames = -1")
    _refused(lib, call(lib, y0=-1), INVALID, name, b"y0 = -1")
    _refused(lib, call(lib, x0=-2), INVALID, b"x0 = -2")
    _refused(lib, call(lib, h=0), INVALID, b"h = 0")
    _refused(lib, call(lib, w=-4), INVALID, b"w = -4")
    _refused(lib, call(lib, y0=5), INVALID, b"y0 = 5", b"h = 16", b"H = 20")       # rows 5..20 of 20
    _refused(lib, call(lib, x0=15), INVALID, b"x0 = 15", b"w = 16", b"W = 30")
    _refused(lib, call(lib, y0=2 ** 31 - 1), INVALID, b"y0 = 2147483647")
    assert call(lib, n=0) == OK
    assert call(lib, n=0, y0=4, x0=14) == OK                                       # the window may touch the far edges


def test_fused_pass_refusals(lib):
    for which in ("bounds", "coeffs"):
        _refused(lib, _fused(lib, **{which: None}), INVALID, b"null pointer")
    _refused(lib, _fused(lib, in_h=0), INVALID, b"H = 0")
    _refused(lib, _fused(lib, out_h=0), INVALID, b"out_h = 0")
    _refused(lib, _fused(lib, ksize=0), INVALID, b"ksize = 0")
    _refused(lib, _fused(lib, ksize=200), UNSUPPORTED, b"ksize = 200")


# ---- the coefficient table ------------------------------------------------------------------------------------------

def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def restated_table(n_in, n_out, filt):
    """The header's arithmetic, literally (Python floats are the C doubles; int() truncates toward zero)."""
    f, S = (_box, 0.5) if filt == BOX else (_bicubic, 2.0)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = S * fs
    ksize = 2 * int(math.ceil(sup)) + 1
    ss = 1.0 / fs
    bounds, coeffs = [], []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)
        xmax = min(int(center + sup + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * (1 << 22) + 0.5) if v >= 0 else int(v * (1 << 22) - 0.5) for v in w]
        bounds.append((xmin, xmax))
        coeffs.append(k + [0] * (ksize - xmax))
    return ksize, bounds, coeffs


def c_table(lib, n_in, n_out, filt):
    ksize = lib.vgpt_resample_ksize(n_in, n_out, filt)
    assert ksize > 0, lib.vgpt_last_error()
    b = np.full(2 * n_out + 2, -77, np.int32)        # one guard pair / row behind each table
    c = np.full((n_out + 1) * ksize, -77, np.int32)
    rc = lib.vgpt_resample_coeffs(n_in, n_out, filt, b.ctypes.data, c.ctypes.data)
    assert rc == OK, lib.vgpt_last_error()
    assert (b[-2:] == -77).all() and (c[-ksize:] == -77).all(), "vgpt_resample_coeffs wrote past its tables"
    return ksize, b[:-2].reshape(n_out, 2), c[:-ksize].reshape(n_out, ksize)


LENGTHS = sorted({(a[i], b[i]) for a, b in SHAPES for i in (0, 1)} | {(1280, 640), (640, 320), (720, 360), (360, 180),
                                                                     (30, 1), (300, 63), (300, 257), (1, 4), (2, 7), (75, 64)})


@pytest.mark.parametrize("filt", [BOX, BICUBIC])
@pytest.mark.parametrize("n_in,n_out", LENGTHS)
def test_table_equals_the_restatement(lib, n_in, n_out, filt):
    ksize, bounds, coeffs = c_table(lib, n_in, n_out, filt)
    rk, rb, rc = restated_table(n_in, n_out, filt)
    assert ksize == rk
    assert bounds.tolist() == [list(p) for p in rb]
    assert coeffs.tolist() == rc
    assert (np.abs(coeffs.astype(np.int64)).sum(axis=1) * 255 < 2 ** 31).all()   # the 32-bit sum cannot overflow


def numpy_pass(img, bounds, coeffs, axis):
    """One pass of the resampler on (H, W, 3) uint8, driven by a table: int32 sum, arithmetic shift, clamp."""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << 21, np.int32)
        for x in range(xmax):
            acc = acc + src[xmin + x] * np.int32(coeffs[xx, x])
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def make_image(H, W, seed):
    """Random bytes with a third of the rows 0 / 255 only: those drive the bicubic lobes into the clamp."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    sat = rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255
    img[::3] = sat[::3]
    return img


@pytest.mark.parametrize("filt", [BOX, BICUBIC])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_numpy_pass_on_the_c_table_equals_pillow(lib, shape, filt):
    (H, W), (h, w) = shape
    img = make_image(H, W, 100 * H + W)
    x = img
    if w != W:       # the horizontal pass first, the vertical one on its uint8 result; an unchanged axis is skipped
        _, b, c = c_table(lib, W, w, filt)
        x = numpy_pass(x, b, c, 1)
    if h != H:
        _, b, c = c_table(lib, H, h, filt)
        x = numpy_pass(x, b, c, 0)
    want = np.array(Image.fromarray(img).resize((w, h), resample=PIL_FILTER[filt]))
    assert x.shape == want.shape and np.array_equal(x, want), f"Pillow {Image.__version__}"


# ---- the plans ------------------------------------------------------------------------------------------------------

def _plan_size(steps, width, height):
    return steps[-1][1] if steps else (width, height)


PLAN_SWEEP = (
    [(w, h, m) for m in (16, 64) for w in (2 * m - 1, 2 * m, 2 * m + 1, 4 * m) for h in (2 * m - 1, 2 * m, 3 * m, 4 * m + 3)]
    + [(7, 9, 2), (7, 7, 2), (15, 31, 3), (129, 140, 64),            # odd sides under halving (7 -> 3), both sides < 16 afterwards
       (5, 9, 1024), (15, 15, 1024), (3, 200, 1024),   # both sides < 16; one side < 16
       (100, 9, 64), (200, 20, 64), (130, 17, 64),     # one side < 16 after the shrink
       (100, 50, 80), (100, 25, 90), (100, 15, 70), (20, 36, 24), (10, 13, 1024),   # x * scale ends in .5 (half to even)
       (1280, 720, 320), (70, 52, 1024), (64, 64, 1024), (300, 260, 64), (40, 9, 1024), (129, 70, 64), (70, 70, 1024)])


@pytest.mark.parametrize("width,height,max_size", PLAN_SWEEP)
def test_crop_arr_plan_gives_the_shape_of_crop_arr(processor_mod, width, height, max_size):
    steps, box = processor_mod.crop_arr_plan(width, height, max_size)
    arr = processor_mod.LVMProcessor(max_image_size=max_size).crop_arr(Image.new("RGB", (width, height)))
    x1, y1, x2, y2 = box
    assert (y2 - y1, x2 - x1) == arr.shape[:2]
    # the crop is the centred one of crop_arr on the last step's size
    w, h = _plan_size(steps, width, height)
    assert (x1, y1) == ((w % 16) // 2, (h % 16) // 2) and (x2, y2) == (w - (w % 16 - x1), h - (h % 16 - y1))
    for filt, (sw, sh) in steps:
        assert filt in (BOX, BICUBIC) and sw >= 1 and sh >= 1


def test_crop_arr_plan_steps(processor_mod):
    plan = processor_mod.crop_arr_plan
    assert plan(1280, 720, 320) == ([(BOX, (640, 360)), (BICUBIC, (320, 180))], (0, 2, 320, 178))
    assert plan(300, 260, 64) == ([(BOX, (150, 130)), (BOX, (75, 65)), (BICUBIC, (64, 55))], (0, 3, 64, 51))
    assert plan(129, 70, 64) == ([(BICUBIC, (64, 35))], (0, 1, 64, 33))
    assert plan(129, 140, 64) == ([(BOX, (64, 70)), (BICUBIC, (59, 64))], (5, 0, 53, 64))   # 129 // 2: an odd side halved
    assert plan(40, 9, 1024) == ([(BICUBIC, (71, 16))], (3, 0, 67, 16))
    assert plan(64, 64, 1024) == ([], (0, 0, 64, 64))
    assert plan(70, 52, 1024) == ([], (3, 2, 67, 50))
    assert plan(100, 50, 80)[0] == [(BICUBIC, (80, 40))]
    assert plan(100, 25, 90)[0] == [(BICUBIC, (90, 22))]       # 22.5 rounds to the even 22, not to 23
    with pytest.raises(ValueError):
        plan(0, 5, 64)
    with pytest.raises(ValueError):
        plan(4000, 1, 64)                                      # the shrink rounds the short side to 0: Pillow refuses it too


def _pil_center_crop(img, image_size):
    """LVM/utils.py:47-66 restated."""
    while min(*img.size) >= 2 * image_size:
        img = img.resize(tuple(x // 2 for x in img.size), resample=Image.BOX)
    scale = image_size / min(*img.size)
    img = img.resize(tuple(round(x * scale) for x in img.size), resample=Image.BICUBIC)
    arr = np.array(img)
    cy, cx = (arr.shape[0] - image_size) // 2, (arr.shape[1] - image_size) // 2
    return arr[cy: cy + image_size, cx: cx + image_size], img.size, (cx, cy)


@pytest.mark.parametrize("width,height,size", [(1280, 720, 256), (100, 70, 32), (31, 90, 16), (64, 64, 64), (20, 30, 48),
                                               (513, 257, 64), (100, 25, 90)])
def test_center_crop_plan_gives_the_shape_of_center_crop_arr(processor_mod, width, height, size):
    steps, box = processor_mod.center_crop_plan(width, height, size)
    arr, resized, (cx, cy) = _pil_center_crop(Image.new("RGB", (width, height)), size)
    assert _plan_size(steps, width, height) == resized
    assert box == (cx, cy, cx + size, cy + size) and arr.shape[:2] == (size, size)
