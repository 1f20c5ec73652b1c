"""CPU: the FP8 KV-cache extension (include/streamchat_hip_kv8.h) - the torch specification of the format behaves as the header says, every
symbol the header declares is exported and bound from _lib.KV8_SIGNATURES, argument errors come back before any device work, unknown modes are
refused by name, and the comparison the GPU attention tests use (tests/_kv8.same_bits against the fp16 result on the dequantised cache) rejects
the wrong readings a broken kernel could take."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import _kv8, _w8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "streamchat_hip_kv8.h")
NAMES = ["sc_attention_kv8", "sc_kv8_dequantize_rows", "sc_kv8_quantize_rows"]


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", src)))


# ---- the reference itself
def test_dequantised_values_are_fp16_exact_and_scales_cover_amax():
    for kv_heads, seed in ((1, 0), (2, 1), (4, 2)):
        x = torch.cat([_kv8.random_rows(64, kv_heads, seed), _kv8.edge_rows(kv_heads)])
        codes, scale = _kv8.quantize_ref(x, kv_heads)
        assert not bool(((codes & 0x7F) == 0x7F).any())                                   # no NaN code
        d = _kv8.dequantize_ref(codes, scale)
        assert torch.equal(d.half().double(), d)                                          # code * 2^e is a fp16 value
        e = torch.log2(scale)
        assert torch.equal(e, e.round()) and e.min() >= -14 and e.max() <= 7
        amax = x.float().view(x.shape[0], 2 * kv_heads, 128).abs().amax(dim=2)
        free = (e > -14) & (e < 7) & (amax > 0)
        assert bool((448 * scale >= amax)[e < 7].all())                                   # covers amax wherever e is not clamped from above
        assert bool((448 * scale / 2 < amax)[free].all())                    # and it is the SMALLEST such power of two
        dv, xv = d.view(-1, 2 * kv_heads, 128)[free], x.double().view(-1, 2 * kv_heads, 128)[free]
        rel = ((dv - xv).norm(dim=1) / xv.norm(dim=1)).max().item()                       # e4m3 keeps 3 mantissa bits: at most 2^-4 per element
        assert rel < 2.0 ** -4, rel


def test_edge_rows():
    kv_heads = 2
    x = _kv8.edge_rows(kv_heads)
    codes, scale = _kv8.quantize_ref(x, kv_heads)
    d = _kv8.dequantize_ref(codes, scale).view(5, 2 * kv_heads, 128)
    assert bool((scale[0] == 1).all()) and bool((codes[0] == 0).all())                   # all zero: e = 0
    assert bool((scale[1] == 128).all()) and bool((d[1, :, 5] == 57344).all())            # 65504 saturates at 448 * 2^7
    assert bool((scale[2] == 2.0 ** -14).all())                                           # amax below 448 * 2^-14: clamped
    assert bool((scale[3] == 2.0 ** -3).all()) and bool((d[3, :, 9] == -56).all())        # amax = 448 * 2^-3 exactly: e = -3, not -2
    c4 = codes.view(5, 2 * kv_heads, 128)[4, :, 3]
    assert bool((c4 == 0x80).all())                                                       # -0.0 kept
    # the frexp formulation at exact powers of two times 448, over the whole unclamped range
    for k in range(-13, 7):
        row = torch.zeros(1, 256, dtype=torch.float16)
        row[0, 0] = 448 * 2.0 ** k
        row[0, 128] = 448 * 2.0 ** k * (1 + 2.0 ** -10)
        _, s = _kv8.quantize_ref(row, 1)
        assert s[0, 0] == 2.0 ** k and s[0, 1] == 2.0 ** (k + 1), k


# ---- the library surface
def test_extension_symbols_exported_and_bound(hip_lib):
    from streamchat_amd import _lib
    assert declared_symbols() == NAMES
    raw = ctypes.CDLL(os.path.join(ROOT, "streamchat_amd", "libstreamchat_hip.so"))
    assert not [n for n in NAMES if not hasattr(raw, n)]
    assert sorted(_lib.KV8_SIGNATURES) == NAMES
    for n in NAMES:
        assert getattr(hip_lib, n).argtypes == _lib.KV8_SIGNATURES[n][1]
    assert not set(NAMES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    src = open(HEADER).read()
    assert hip_lib.sc_abi_version() == _lib.ABI_VERSION == 9 and "additive; base ABI 9" in src and "#define SC_ABI_VERSION" not in src


def test_argument_errors_come_back_before_any_device_work(hip_lib):
    from ctypes import c_float, c_void_p
    p, odd = c_void_p(4096), c_void_p(4096 + 8)
    err = hip_lib.sc_last_error
    qz = hip_lib.sc_kv8_quantize_rows
    assert qz(None, 512, 1, 2, 128, p, 512, p, 8, 0, None, 0, None) == -1 and b"null pointer" in err()
    assert qz(p, 512, 1, 2, 64, p, 512, p, 8, 0, None, 0, None) == -4 and b"head dim 64 unsupported" in err()
    assert qz(p, 256, 1, 2, 128, p, 512, p, 8, 0, None, 0, None) == -1 and b"row strides" in err()
    assert qz(odd, 512, 1, 2, 128, p, 512, p, 8, 0, None, 0, None) == -1 and b"16-byte aligned" in err()
    assert qz(p, 512, 4, 2, 128, p, 512, p, 8, 6, None, 0, None) == -1 and b"exceed the cache" in err()
    dq = hip_lib.sc_kv8_dequantize_rows
    assert dq(p, 512, None, 8, 0, 1, 2, 128, p, 512, None) == -1 and b"null pointer" in err()
    assert dq(p, 512, p, 8, 0, 1, 2, 32, p, 512, None) == -4 and b"unsupported" in err()
    assert dq(p, 512, p, 8, 7, 2, 2, 128, p, 512, None) == -1 and b"exceed the cache" in err()
    assert dq(p, 512, p, 8, 0, 1, 2, 128, odd, 512, None) == -1 and b"16-byte aligned" in err()
    at = hip_lib.sc_attention_kv8
    one = c_float(1.0)
    assert at(p, 128, None, 512, p, p, 128, 7, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, None) == -1 and b"null pointer" in err()
    assert at(p, 128, p, 256, p, p, 64, 7, 64, 2, 64, one, 2, None, 2, p, 1 << 20, 0, 0, None) == -4 and b"head dim 64 unsupported" in err()
    assert at(p, 128, p, 512, p, p, 128, 7, 64, 2, 128, one, 1, None, 2, p, 1 << 20, 0, 0, None) == -1 and b"non-causal" in err()
    assert at(p, 128, p, 512, p, p, 128, 17, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, None) == -1 and b"bad sizes" in err()
    assert at(p, 128, p, 520, p, p, 128, 7, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, None) == -1 and b"row stride" in err()
    assert at(p, 128, p, 512, p, p, 128, 7, 64, 2, 128, one, 2, None, 0, p, 1 << 20, 0, 0, None) == -1 and b"nsplit" in err()
    assert at(p, 128, p, 512, p, p, 128, 7, 64, 2, 128, one, 2, None, 2, p, 64, 0, 0, None) == -2 and b"workspace" in err()
    assert at(p, 128, p, 512, p, p, 128, 7, 64, 2, 128, one, 2, None, 2, None, 0, 0, 0, None) == -2


def test_wrappers_refuse_cpu_tensors():
    from streamchat_amd import ops
    from streamchat_amd._lib import StreamChatHipError
    x, c, s = torch.zeros(1, 256, dtype=torch.float16), torch.zeros(4, 256, dtype=torch.uint8), torch.ones(4, 2)
    with pytest.raises(StreamChatHipError):
        ops.kv8_quantize_rows(x, c, s, 0, 1, 128)
    with pytest.raises(StreamChatHipError):
        ops.kv8_dequantize_rows(c, s, 0, 1, 1, 128, x)
    with pytest.raises(StreamChatHipError):
        ops.attention_kv8(x.view(1, 1, 256), c, s, 1, 128, 1.0, nsplit=2)


def test_unknown_modes_are_refused_by_name():
    import inference_streaming_longva_v2 as E
    from streamchat_amd import llm as LM
    base = ["--video_dir", "v", "--model_name", "m", "--memory_basic_dir", "d", "--save_file", "s", "--annotations", "a", "--language", "en"]
    assert E.parse_args(base).kv_cache == "fp16" and E.parse_args(base + ["--kv_cache", "fp8"]).kv_cache == "fp8"
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--kv_cache", "x"])
    assert LM.KV_CACHE == ("fp16", "fp8") and LM.DEFAULT_KV_CACHE in LM.KV_CACHE
    with pytest.raises(ValueError, match="int4"):
        LM.check_kv_cache("int4")
    cfg = LM.Qwen2ConfigLite(hidden=128, layers=1, heads=1, kv_heads=1, intermediate=128, vocab=128)
    with pytest.raises(ValueError, match="int4"):
        LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, device="cpu"), cfg, device="cpu", kv_cache="int4")
    with pytest.raises(ValueError, match="head_dim 128"):
        LM.Qwen2Model({}, LM.Qwen2ConfigLite(hidden=128, layers=1, heads=2, kv_heads=1, intermediate=128, vocab=128), device="cpu", kv_cache="fp8")
    from streamchat_amd.persistence import FINGERPRINT_FIELDS
    assert "kv_cache" not in FINGERPRINT_FIELDS
    # the process default is read once at import and checked there
    r = subprocess.run([sys.executable, "-c", "import streamchat_amd.llm"], cwd=ROOT, env=dict(os.environ, SC_KV_CACHE="bf16"), capture_output=True, text=True)
    assert r.returncode != 0 and "kv_cache must be one of" in r.stderr and "bf16" in r.stderr
    r = subprocess.run([sys.executable, "-c", "import streamchat_amd.llm as L; print(L.DEFAULT_KV_CACHE)"], cwd=ROOT, env=dict(os.environ, SC_KV_CACHE="fp8"),
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "fp8", r.stderr


# ---- power: the GPU comparison (bit identity with the fp16 result on the dequantised cache) rejects wrong kernels
def _fnuz_values(codes):
    v = codes.view(torch.float8_e4m3fnuz).double()
    return torch.where(torch.isnan(v), torch.zeros_like(v), v)


def _attention_row_by_row(q, cache16, Hkv, kv_len):
    """an attention written independently of tests/_kv8.attention_fp64: one pass over the rows of the DEQUANTISED fp16 cache (what the fp16 decode
    kernel is handed), a running maximum and running sums in fp64, the exponentials in base 2 as the kernels take them"""
    G = q.shape[0]
    out = torch.zeros(G, Hkv * 128, dtype=torch.float64)
    for h in range(Hkv):
        qh = q[:, h * 128:(h + 1) * 128].double()
        m = torch.full((G,), -float("inf"), dtype=torch.float64)
        den, acc = torch.zeros(G, dtype=torch.float64), torch.zeros(G, 128, dtype=torch.float64)
        for r in range(kv_len):
            k, v = cache16[r, h * 128:(h + 1) * 128].double(), cache16[r, (Hkv + h) * 128:(Hkv + h + 1) * 128].double()
            s = qh @ k
            m2 = torch.maximum(m, s)
            a, p = torch.exp2(m - m2), torch.exp2(s - m2)
            den, acc, m = den * a + p, acc * a[:, None] + p[:, None] * v, m2
        out[:, h * 128:(h + 1) * 128] = acc / den[:, None]
    return out


@pytest.mark.parametrize("S,G", [(33, 7), (769, 16)])
def test_comparison_rejects_wrong_kernels(S, G):
    """The GPU tests compare fp16 bits (tests/_kv8.same_bits) with a correct fp16 attention over the dequantised cache.  Here the correct one is
    an independently written row-by-row attention over `dequantize_ref(...).half()`: rounded to fp16 it has the bits of the fp64 reference, and
    every wrong reading is not only different in its bits but off by far more than the fp16 decode kernel's own error could hide (> 1 % of max |ref|)."""
    Hkv = 2
    codes, scale, q = _kv8.attention_case(S + 40, G, Hkv, seed=S)
    ref = _kv8.attention_fp64(q, codes, scale, Hkv, kv_len=S)
    cache16 = _kv8.dequantize_ref(codes, scale).half()
    assert torch.equal(cache16.double(), _kv8.dequantize_ref(codes, scale))                       # (the dequantised cache is exact in fp16)
    assert _kv8.same_bits(_attention_row_by_row(q, cache16, Hkv, S).half(), ref.half())
    sk, sv = scale[:, :Hkv], scale[:, Hkv:]
    mutants = {
        "bytes decoded as e4m3fnuz": dict(values=_fnuz_values),
        "the scale of the neighbouring row": dict(scale_k=torch.roll(sk, -1, 0), scale_v=torch.roll(sv, -1, 0)),
        "the scale of the neighbouring head": dict(scale_k=torch.roll(sk, 1, 1), scale_v=torch.roll(sv, 1, 1)),
        "K's scale applied to V": dict(scale_v=sk),
        # (the GPU test poisons the rows behind kv_len with NaN bytes and NaN scales: a kernel that reads them returns NaN)
        "the masked tail not masked": dict(kv_len=S + 40, values=lambda c: _w8.e4m3_values(torch.cat([c[:S], torch.full_like(c[S:], 0x7F)]))),
    }
    for name, kw in mutants.items():
        out = _kv8.attention_fp64(q, codes, scale, Hkv, **{"kv_len": S, **kw})
        assert not _kv8.same_bits(out.half(), ref.half()), name
        assert not ((out - ref).abs().max() / ref.abs().max()).item() <= 1e-2, name


def test_attention_inputs_cover_every_code_and_the_scale_range():
    codes, scale = _kv8.random_cache(769, 2, seed=5)
    assert len(torch.unique(codes)) == 254
    e = torch.log2(scale)
    assert e.min() == -14 and e.max() == 7 and len(torch.unique(e)) == 22
