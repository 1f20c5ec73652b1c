"""include/streamchat_hip_w8_batched.h (changelog entry w8-2): the header declares sc_gemm_w8_f16, the cross-compiled library exports it, and
the base ABI version is unchanged - the extension is additive."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_header_declares_the_symbol_and_extends_w8():
    h = _read("include", "streamchat_hip_w8_batched.h")
    assert re.search(r"\bint\s+sc_gemm_w8_f16\s*\(", h) and "w8-2" in h and '#include "streamchat_hip_w8.h"' in h
    assert "sc_gemm_w8_f16" not in _read("include", "streamchat_hip_w8.h") and "sc_gemm_w8_f16" not in _read("include", "streamchat_hip.h")
    assert re.search(r"#define\s+SC_ABI_VERSION\s+9\b", _read("include", "streamchat_hip.h"))


def test_library_exports_it_and_the_abi_is_still_9():
    from streamchat_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sc_gemm_w8_f16")
    lib.sc_abi_version.restype = ctypes.c_int
    assert lib.sc_abi_version() == 9 == _lib.ABI_VERSION
    assert list(_lib.W8_BATCHED_SIGNATURES) == ["sc_gemm_w8_f16"] and "sc_gemm_w8_f16" not in _lib.EXT_SIGNATURES
    assert len(_lib.W8_BATCHED_SIGNATURES["sc_gemm_w8_f16"][1]) == 15
