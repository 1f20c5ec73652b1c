"""CPU: the FP8 weight-only extension header (include/streamchat_hip_w8.h) - every symbol it declares is exported and bound from
_lib.EXT_SIGNATURES and vice versa, the base header / SIGNATURES / ABI number are untouched by it, argument errors come back before any device
work, the entry point's flag parses, and every function of the header with a writable pointer has a test in tests/test_gpu_w8_write_bounds.py
(what tests/test_abi.py and tests/test_guard_helper.py do for the base header)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "streamchat_hip_w8.h")


def _text():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def declared_symbols():
    return sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", _text())))


def test_extension_symbols_exported_and_bound(hip_lib):
    from streamchat_amd import _lib
    names = declared_symbols()
    assert names == ["sc_decode_qkv_tab_w8", "sc_gemv_w8_f16", "sc_quantize_rows_e4m3"]
    raw = ctypes.CDLL(os.path.join(ROOT, "streamchat_amd", "libstreamchat_hip.so"))
    assert not [n for n in names if not hasattr(raw, n)]
    assert sorted(_lib.EXT_SIGNATURES) == names
    for n in names:                                                  # bound by load(): restype / argtypes are set
        assert getattr(hip_lib, n).argtypes == _lib.EXT_SIGNATURES[n][1]


def test_base_header_and_abi_number_are_unchanged(hip_lib):
    from streamchat_amd import _lib
    from tests.test_abi import declared_symbols as base_symbols
    assert not set(declared_symbols()) & set(base_symbols()) and not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert sorted(_lib.SIGNATURES) == base_symbols()
    assert hip_lib.sc_abi_version() == _lib.ABI_VERSION == 9
    src = open(HEADER).read()
    assert "additive; base ABI 9" in src and "SC_ABI_VERSION" in src and "#define SC_ABI_VERSION" not in src


def test_argument_errors_come_back_before_any_device_work(hip_lib):
    from ctypes import c_float, c_void_p
    p, odd = c_void_p(4096), c_void_p(4096 + 8)
    eps = c_float(1e-6)
    g = hip_lib.sc_gemv_w8_f16
    assert g(None, p, p, None, None, p, 8, 64, 0, 0, None, 0, None, eps, None) == -1 and b"null pointer" in hip_lib.sc_last_error()
    assert g(p, None, p, None, None, p, 8, 64, 0, 0, None, 0, None, eps, None) == -1 and b"null pointer" in hip_lib.sc_last_error()
    assert g(p, p, p, None, None, p, 8, 24, 0, 0, None, 0, None, eps, None) == -1 and b"multiple of 16" in hip_lib.sc_last_error()      # K = 24
    assert g(odd, p, p, None, None, p, 8, 64, 0, 0, None, 0, None, eps, None) == -1 and b"16-byte aligned" in hip_lib.sc_last_error()   # misaligned W
    assert g(p, p, p, p, None, p, 8, 64, 3, 0, None, 0, None, eps, None) == -1 and b"SwiGLU" in hip_lib.sc_last_error()                 # SwiGLU + bias
    assert g(p, p, p, None, None, p, 8, 64, 0, 1, p, 64, None, eps, None) == -1 and b"dynamic output row" in hip_lib.sc_last_error()     # y_row + fp32
    d = hip_lib.sc_decode_qkv_tab_w8
    assert d(p, p, p, None, None, None, p, p, eps, p, p, 512, p, 4, 2, 64, 256, p, p, 64, None) == -1 and b"null pointer" in hip_lib.sc_last_error()
    assert d(p, p, p, p, None, None, p, p, eps, p, p, 512, p, 4, 2, 64, 24, p, p, 64, None) == -1 and b"bad sizes" in hip_lib.sc_last_error()
    assert d(p, p, p, p, None, None, p, p, eps, p, p, 100, p, 4, 2, 64, 256, p, p, 64, None) == -1 and b"row stride" in hip_lib.sc_last_error()
    assert d(p, p, odd, p, None, None, p, p, eps, p, p, 512, p, 4, 2, 64, 256, p, p, 64, None) == -1 and b"16-byte aligned" in hip_lib.sc_last_error()
    qz = hip_lib.sc_quantize_rows_e4m3
    assert qz(None, 64, 4, 64, p, p, None) == -1 and b"null pointer" in hip_lib.sc_last_error()
    assert qz(p, 64, 4, 60, p, p, None) == -1 and b"multiples of 8" in hip_lib.sc_last_error()
    assert qz(p, 32, 4, 64, p, p, None) == -1                                                                          # ldw < K


def test_wrappers_refuse_cpu_tensors():
    import torch
    from streamchat_amd import ops
    from streamchat_amd._lib import StreamChatHipError
    q, s, x = torch.zeros(4, 16, dtype=torch.uint8), torch.ones(4), torch.zeros(16, dtype=torch.float16)
    with pytest.raises(StreamChatHipError):
        ops.quantize_rows_e4m3(torch.zeros(4, 16, dtype=torch.float16))
    with pytest.raises(StreamChatHipError):
        ops.gemv_w8(q, s, x)
    with pytest.raises(StreamChatHipError):
        ops.decode_qkv_tab_w8(q, s, q, s, None, None, x, None, 1e-6, x, x.view(1, -1), torch.zeros(1, dtype=torch.int32), 1, 1, 2, torch.zeros(4, 2), torch.zeros(4, 2))


def test_decode_weights_flag_and_setting():
    import inference_streaming_longva_v2 as E
    from streamchat_amd import llm as LM
    base = ["--video_dir", "v", "--model_name", "m", "--memory_basic_dir", "d", "--save_file", "s", "--annotations", "a", "--language", "en"]
    assert E.parse_args(base).decode_weights == "fp16"
    assert E.parse_args(base + ["--decode_weights", "fp8"]).decode_weights == "fp8"
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--decode_weights", "int4"])
    assert LM.DECODE_WEIGHTS == ("fp16", "fp8") and LM.check_decode_weights("fp8") == "fp8"
    with pytest.raises(ValueError):
        LM.check_decode_weights("int4")
    from streamchat_amd.persistence import FINGERPRINT_FIELDS
    assert "decode_weights" not in FINGERPRINT_FIELDS                  # a decoding setting like --temperature: a session resumes across it


def _writable_pointer_functions():
    """the regex walk of tests/test_guard_helper.py over the extension header"""
    out = []
    for ret, name, args in re.findall(r"\b(int|size_t|const char\*)\s+(sc_\w+)\s*\(([^;{}]*?)\)\s*;", _text(), flags=re.S):
        params = [p.strip() for p in args.split(",")]
        if any("*" in p and not p.startswith("const ") for p in params):
            out.append(name)
    return out


def test_every_extension_function_with_a_writable_pointer_is_in_the_write_bound_module():
    from tests import test_gpu_w8_write_bounds as W
    names = _writable_pointer_functions()
    assert sorted(names) == ["sc_decode_qkv_tab_w8", "sc_gemv_w8_f16", "sc_quantize_rows_e4m3"], names
    assert sorted(W.COVERED) == sorted(names)
    src = open(W.__file__).read()
    for name, tests in W.COVERED.items():
        assert tests, name
        for t in tests:
            assert callable(getattr(W, t, None)), f"COVERED names {t} for {name}, which the module does not define"
        assert re.search(rf"\b{name}\b", src.split("COVERED", 1)[1].split("}", 1)[1]), f"{name} is listed but never named by a test"
