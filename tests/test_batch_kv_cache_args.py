"""CPU: the surface of the batched decode's FP8 KV cache (changelog entry kv8-2: include/streamchat_hip_kv8_batched.h, llm.BatchDecoder(kv_cache=...),
--batch_kv_cache, SC_BATCH_KV_CACHE) - the flag parses and defaults to fp16, unknown modes are refused by name, the process default is checked at
import, the two new symbols are declared, exported and bound from a table of their own, and their argument errors come back before any device work."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "streamchat_hip_kv8_batched.h")
KV8_HEADER = os.path.join(ROOT, "include", "streamchat_hip_kv8.h")
NAMES = ["sc_attention_kv8_batched", "sc_kv8_rope_qkv_rows"]
BASE = ["--video_dir", "v", "--model_name", "m", "--memory_basic_dir", "d", "--save_file", "s", "--annotations", "a", "--language", "en"]


def declared_symbols(path):
    src = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", src)))


def test_flag_parses_and_defaults_to_fp16():
    import inference_streaming_longva_v2 as E
    a = E.parse_args(BASE)
    assert a.batch_kv_cache == "fp16" and a.kv_cache == "fp16"
    a = E.parse_args(BASE + ["--batch_kv_cache", "fp8"])
    assert a.batch_kv_cache == "fp8" and a.kv_cache == "fp16"                # independent of --kv_cache, in both directions
    assert E.parse_args(BASE + ["--kv_cache", "fp8"]).batch_kv_cache == "fp16"
    with pytest.raises(SystemExit):
        E.parse_args(BASE + ["--batch_kv_cache", "int4"])
    from streamchat_amd.persistence import FINGERPRINT_FIELDS
    assert "batch_kv_cache" not in FINGERPRINT_FIELDS


def test_unknown_modes_are_refused_by_name_and_views_inherit():
    from streamchat_amd import llm as LM
    assert LM.DEFAULT_BATCH_KV_CACHE in LM.KV_CACHE
    with pytest.raises(ValueError, match="batch_kv_cache must be one of.*int4"):
        LM.check_batch_kv_cache("int4")
    cfg = LM.Qwen2ConfigLite(hidden=128, layers=1, heads=1, kv_heads=1, intermediate=128, vocab=128)
    sd = LM.random_qwen2_state_dict(cfg, device="cpu")
    with pytest.raises(ValueError, match="int4"):
        LM.Qwen2Model(sd, cfg, device="cpu", batch_kv_cache="int4")
    with pytest.raises(ValueError, match="batch_kv_cache='fp8' needs head_dim 128"):
        LM.Qwen2Model({}, LM.Qwen2ConfigLite(hidden=128, layers=1, heads=2, kv_heads=1, intermediate=128, vocab=128), device="cpu", batch_kv_cache="fp8")
    m = LM.Qwen2Model(sd, cfg, device="cpu", kv_cache="fp16", batch_kv_cache="fp8")
    assert m.batch_kv_cache == "fp8" and m.kv_cache == "fp16" and m.shared_view().batch_kv_cache == "fp8"
    assert m.set_batch_kv_cache("fp16") is m and m.batch_kv_cache == "fp16"
    m8 = LM.Qwen2Model(sd, cfg, device="cpu", kv_cache="fp8", batch_kv_cache="fp16")      # the batch-1 mode does not decide the batched one
    assert m8.kv_cache == "fp8" and m8.batch_kv_cache == "fp16"
    with pytest.raises(ValueError, match="batch_kv_cache must be one of"):
        LM.BatchDecoder(m, [], 1, kv_cache="bf16")


def test_process_default_is_read_once_and_checked_at_import():
    env = {k: v for k, v in os.environ.items() if k != "SC_BATCH_KV_CACHE"}
    r = subprocess.run([sys.executable, "-c", "import streamchat_amd.llm"], cwd=ROOT, env=dict(env, SC_BATCH_KV_CACHE="bogus"), capture_output=True, text=True)
    assert r.returncode != 0 and "batch_kv_cache must be one of" in r.stderr and "bogus" in r.stderr
    code = "import streamchat_amd.llm as L; print(L.DEFAULT_BATCH_KV_CACHE, L.DEFAULT_KV_CACHE)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SC_BATCH_KV_CACHE="fp8", SC_KV_CACHE="fp16"), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["fp8", "fp16"], r.stderr
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SC_KV_CACHE="fp8"), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["fp16", "fp8"], r.stderr


def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from streamchat_amd import _lib
    assert declared_symbols(HEADER) == NAMES
    src, kv8 = open(HEADER).read(), open(KV8_HEADER).read()
    assert '#include "streamchat_hip_kv8.h"' in src and "#define SC_ABI_VERSION" not in src
    assert "kv8-2" in kv8 and all(n in kv8 for n in NAMES) and "streamchat_hip_kv8_batched.h" in kv8          # the changelog entry names them
    raw = ctypes.CDLL(os.path.join(ROOT, "streamchat_amd", "libstreamchat_hip.so"))
    assert not [n for n in NAMES if not hasattr(raw, n)]
    assert sorted(_lib.KV8_BATCHED_SIGNATURES) == NAMES
    for n in NAMES:
        assert getattr(hip_lib, n).argtypes == _lib.KV8_BATCHED_SIGNATURES[n][1]
    assert not set(NAMES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.KV8_SIGNATURES) | set(_lib.TEXT_SIGNATURES))
    assert hip_lib.sc_abi_version() == _lib.ABI_VERSION == 9                 # purely additive


def test_argument_errors_come_back_before_any_device_work(hip_lib):
    from ctypes import c_float, c_void_p
    p, odd = c_void_p(4096), c_void_p(4096 + 8)
    err, one = hip_lib.sc_last_error, c_float(1.0)
    at = hip_lib.sc_attention_kv8_batched
    #  q  ldq cache ld   bs       scales out ldo  B  Sq Skv Hkv Dh  scale flags kv_len nsplit ws  bytes  qhs ohs qbs obs stream
    assert at(p, 128, None, 512, 512 * 64, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"null pointer" in err()
    assert at(p, 128, p, 256, 256 * 64, p, p, 64, 3, 7, 64, 2, 64, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -4 and b"head dim 64 unsupported" in err()
    assert at(p, 128, p, 512, 512 * 64, p, p, 128, 3, 7, 64, 2, 128, one, 1, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"non-causal" in err()
    assert at(p, 128, p, 512, 512 * 64, p, p, 128, 3, 17, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"bad sizes" in err()
    assert at(p, 128, p, 512, 512 * 64, p, p, 128, 0, 7, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"bad sizes" in err()
    assert at(p, 128, p, 520, 520 * 64, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"row stride" in err()
    assert at(p, 128, p, 512, 512 * 64 + 8, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"batch stride" in err()
    assert at(p, 128, p, 512, 512 * 63, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"batch stride" in err()
    # one sequence's slice at or past 2 GiB is refused, a whole allocation past it is not (the next error, the workspace, is reached)
    assert at(p, 128, p, 512, 1 << 32, p, p, 128, 3, 7, 1 << 22, 2, 128, one, 2, None, 2, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"below 2 GiB" in err()
    assert at(p, 128, p, 512, 1 << 31, p, p, 128, 3, 7, (1 << 22) - 1, 2, 128, one, 2, None, 2, p, 64, 0, 0, 0, 0, None) == -2 and b"workspace" in err()
    assert at(p, 128, p, 512, 512 * 64, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 0, p, 1 << 20, 0, 0, 0, 0, None) == -1 and b"nsplit" in err()
    need = 3 * 2 * 7 * 2 * 130 * 4                                           # B * kv_heads * Sq * nsplit * (Dh + 2) floats
    assert at(p, 128, p, 512, 512 * 64, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 2, p, need - 4, 0, 0, 0, 0, None) == -2 and b"workspace" in err()
    assert at(p, 128, p, 512, 512 * 64, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 2, None, 0, 0, 0, 0, 0, None) == -2
    assert at(p, 128, p, 512, 512 * 64, p, p, 128, 3, 7, 64, 2, 128, one, 2, None, 2, p, need, 0, 0, 4, 0, None) == -1 and b"strides" in err()
    rq = hip_lib.sc_kv8_rope_qkv_rows
    #  x  ldx  tab_q tab_k rows pos B  Hq Hkv Dh  q_out ldq cache bs        ld  scales cache_rows stream
    assert rq(p, 1024, p, p, 64, p, 2, 4, 2, 128, p, 512, None, 512 * 64, 512, p, 64, None) == -1 and b"null pointer" in err()
    assert rq(p, 1024, p, p, 64, p, 2, 4, 2, 128, p, 512, p, 512 * 64, 512, None, 64, None) == -1 and b"null pointer" in err()
    assert rq(p, 512, p, p, 64, p, 2, 4, 2, 64, p, 256, p, 256 * 64, 256, p, 64, None) == -4 and b"head dim 64 unsupported" in err()
    assert rq(p, 1024, p, p, 64, p, 0, 4, 2, 128, p, 512, p, 512 * 64, 512, p, 64, None) == -1 and b"bad sizes" in err()
    assert rq(p, 1000, p, p, 64, p, 2, 4, 2, 128, p, 512, p, 512 * 64, 512, p, 64, None) == -1 and b"leading dimensions" in err()
    assert rq(p, 1024, p, p, 64, p, 2, 4, 2, 128, p, 512, p, 512 * 64, 508, p, 64, None) == -1 and b"leading dimensions" in err()
    assert rq(p, 1024, p, p, 64, p, 2, 4, 2, 128, p, 512, p, 512 * 63, 512, p, 64, None) == -1 and b"leading dimensions" in err()
    assert rq(odd, 1024, p, p, 64, p, 2, 4, 2, 128, p, 512, p, 512 * 64, 512, p, 64, None) == -1 and b"aligned" in err()


def test_wrappers_refuse_cpu_tensors_and_wrong_layouts():
    from streamchat_amd import ops
    from streamchat_amd._lib import StreamChatHipError
    c, s = torch.zeros(2, 4, 256, dtype=torch.uint8), torch.ones(2, 4, 2)
    x, t, pos, q = torch.zeros(2, 384), torch.zeros(8, 128), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 128, dtype=torch.float16)
    with pytest.raises(StreamChatHipError):
        ops.attention_kv8_batched(q.view(2, 1, 128), c, s, 1, 128, 1.0, nsplit=2)
    with pytest.raises(StreamChatHipError):
        ops.kv8_rope_qkv_rows(x, t, t, pos, 1, 1, 128, q, c, s)
