"""The MX-fp8 projection entry points (include/vgpt.h, vgpt_mx8_* / vgpt_gemm_mx8) without a GPU: the header declares them,
the library exports them, host-side argument checks refuse bad calls before any launch, and the engine refuses an unknown
linear_precision."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vgpt_mx8_bytes", "vgpt_mx8_quant_rows", "vgpt_mx8_quant_weight", "vgpt_gemm_mx8")


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("video-gpt_amd")
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg._lib


def test_header_and_binding_carry_the_mx8_surface(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vgpt.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(vgpt_[a-z0-9_]+)\s*\(", text))
    cdll = lib.load()
    for name in NEW:
        assert name in syms and name in lib.SIGNATURES and hasattr(cdll, name)
    for i, epi in enumerate(("NONE", "RESID", "ROPE", "GATED")):
        assert re.search(rf"#define VGPT_MX8_EPI_{epi} {i}\b", text)
        assert getattr(lib, f"MX8_EPI_{epi}") == i


def test_record_size(lib):
    cdll = lib.load()
    # 70 rows -> 3 row groups, K 224 -> 4 k tiles of 64: payload 12 x 2048 (256-aligned), scales 12 x 64
    assert cdll.vgpt_mx8_bytes(70, 224) == 12 * 2048 + 12 * 64
    assert cdll.vgpt_mx8_bytes(9216, 3072) == 288 * 48 * 2048 + 288 * 48 * 64
    assert cdll.vgpt_mx8_bytes(64, 100) == -1 and cdll.vgpt_mx8_bytes(0, 64) == -1


def test_gemm_and_quantisers_check_arguments_before_launching(lib):
    cdll = lib.load()
    fake = 1 << 20          # never dereferenced: every call below fails its host-side checks first
    rc = cdll.vgpt_gemm_mx8(fake, fake, fake, None, None, None, None, 64, 64, 96 + 8, 64, 64, 0, 0, 96, 0, None)
    assert rc == -1 and b"multiple of 32" in cdll.vgpt_last_error()
    rc = cdll.vgpt_gemm_mx8(None, fake, fake, None, None, None, None, 64, 64, 64, 64, 64, 0, 0, 96, 0, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    rc = cdll.vgpt_gemm_mx8(fake, fake, fake, None, None, None, None, 64, 64, 64, 64, 64, 1, 0, 96, 0, None)   # resid missing
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()
    rc = cdll.vgpt_gemm_mx8(fake, fake, fake, None, fake, fake, fake, 64, 192, 64, 192, 192, 2, 2, 128, 0, None)  # head_dim
    assert rc == -2 and b"head_dim 96" in cdll.vgpt_last_error()
    rc = cdll.vgpt_gemm_mx8(fake, fake, fake, None, None, None, None, 64, 64, 64, 64, 64, 7, 0, 96, 0, None)
    assert rc == -1 and b"epilogue" in cdll.vgpt_last_error()
    rc = cdll.vgpt_mx8_quant_rows(fake, 48, fake, None, 4, 48, 1e-5, None)
    assert rc == -1 and b"multiple of 32" in cdll.vgpt_last_error()
    rc = cdll.vgpt_mx8_quant_weight(None, None, fake, 4, 64, None)
    assert rc == -1 and b"null pointer" in cdll.vgpt_last_error()


def test_engine_rejects_unknown_linear_precision():
    E = importlib.import_module("video-gpt_amd.engine")

    class NotReady:
        def _check_ready(self):
            return None
    with pytest.raises(Exception, match="linear_precision"):
        E.StaticDenoiser(NotReady(), None, None, None, None, None, None, None, 1, (2, 2), False, 1.0, linear_precision="fp4")
