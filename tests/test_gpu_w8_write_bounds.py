"""GPU: the three functions of include/streamchat_hip_w8.h write their outputs and nothing else (tests/_guard.py; the walk over the header that
requires this module to cover each of them is tests/test_w8_abi.py).  Tail bands are sized from the largest tile a launch can have: a workgroup
of eight waves covers 64 rows (8 per wave), the quantiser writes 8 bytes per thread."""
import pytest
import torch

from ctypes import c_void_p

from streamchat_amd import _lib, ops
from tests import _w8
from tests._guard import Arena, frozen
from tests._tol import assert_close_fp16

pytestmark = pytest.mark.gpu

COVERED = {
    "sc_quantize_rows_e4m3": ["test_quantize_rows_write_bounds"],
    "sc_gemv_w8_f16": ["test_gemv_w8_write_bounds"],
    "sc_decode_qkv_tab_w8": ["test_decode_qkv_tab_w8_write_bounds"],
}


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _cuda(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


@pytest.mark.parametrize("N,K", [(5, 16), (37, 1040)])
def test_quantize_rows_write_bounds(N, K):
    """sc_quantize_rows_e4m3: q is an arena view of exactly [N, K] bytes with a tail band of 64 more rows, the scales an arena vector of exactly
    N floats; W is a row-strided view whose other columns are NaN (a read of them shows in amax) and stays frozen."""
    full = torch.full((N, K + 24), float("nan"), dtype=torch.float16, device="cuda")
    full[:, :K] = (torch.randn(N, K, generator=_w8.gen(1)) * 0.02).half().cuda()
    w = full[:, :K]
    ar = Arena("cuda")
    q, s = ar.out(N, K, torch.uint8, tail_rows=64), ar.flat(N, torch.float32)
    lib = _lib.load()
    with frozen(full):
        rc = lib.sc_quantize_rows_e4m3(c_void_p(w.data_ptr()), w.stride(0), N, K, c_void_p(q.data_ptr()), c_void_p(s.data_ptr()), ops.stream_ptr("cuda:0"))
        assert rc == 0, lib.sc_last_error()
    qr, sr = _w8.quantize_ref(w)
    assert torch.equal(q.cpu(), qr) and torch.equal(_bits(s).cpu(), _bits(sr))
    ar.check("sc_quantize_rows_e4m3")


@pytest.mark.parametrize("N,K", [(37, 1040), (50, 3584), (50, 18944)])
def test_gemv_w8_write_bounds(N, K):
    """sc_gemv_w8_f16: K = 1040 the loop kernels, K = 3584 / 18944 the straight-line ones - fp16 out (bias + residual), fp32 out with the fused
    norm, SwiGLU (N' / 2 outputs) into arena vectors of exactly the output size; `out_row`: y is a KV-cache view [12, N] with ld = N + 64
    (KV_ROW_PAD), only row 5 may change.  The weight bytes and scales are arena inputs with a tail band themselves (a read past the last row
    would meet the NaN pattern 0x7E... = 448 * 2^-1: visible in the sums); all inputs frozen."""
    c = _cuda(_w8.gemv_case(N, K, seed=3, bias=True, res=True))
    cn = _cuda(_w8.gemv_case(N, K, seed=4, norm=True, bias=True))
    cs = _cuda(_w8.gemv_case(N // 4 * 4, K, seed=5, swiglu=True))
    ar = Arena("cuda")
    qa = ar.out(N, K, torch.uint8, tail_rows=64)
    qa.copy_(c["q"])
    assert qa.is_contiguous()
    y16, y32, ysw = ar.flat(N, torch.float16), ar.flat(N, torch.float32), ar.flat(N // 4 * 2, torch.float16)
    cache = ar.out(12, N, torch.float16, ld=N + 64, tail_rows=16)
    cache.fill_(7.0)
    row = torch.tensor([5], dtype=torch.int32, device="cuda")
    ins = [c["scale"], c["x"], c["bias"], c["res"], cn["q"], cn["scale"], cn["x"], cn["gamma"], cn["bias"], cs["q"], cs["scale"], cs["x"], row]
    with frozen(qa, *ins):
        ops.gemv_w8(qa, c["scale"], c["x"], c["bias"], c["res"], out=y16)
        ops.gemv_w8(cn["q"], cn["scale"], cn["x"], cn["bias"], out=y32, rms_gamma=cn["gamma"], rms_eps=1e-6)
        ops.gemv_w8(cs["q"], cs["scale"], cs["x"], epilogue="swiglu", out=ysw)
        ops.gemv_w8(qa, c["scale"], c["x"], c["bias"], out=cache, out_row=row)
    assert_close_fp16(y16, c["ref"], what="fp16 out")
    assert_close_fp16(y32, cn["ref"], what="fp32 out, fused norm")
    assert_close_fp16(ysw, cs["ref"], what="swiglu")
    assert_close_fp16(cache[5], c["ref"] - c["res"].double(), what="dynamic row")
    keep = torch.arange(12, device="cuda") != 5
    assert bool((cache[keep] == 7.0).all()), "sc_gemv_w8_f16 with y_row changed another cache row"
    ar.check("sc_gemv_w8_f16")


@pytest.mark.parametrize("Hq,Hkv,Dh,K", [(4, 2, 64, 256), (28, 4, 128, 3584)])
def test_decode_qkv_tab_w8_write_bounds(Hq, Hkv, Dh, K):
    """sc_decode_qkv_tab_w8: q_out is an arena vector of exactly Hq Dh elements, the KV cache an arena view [40, 2 Hkv Dh] with cache_ld 64
    elements wider (KV_ROW_PAD): only row pos[0] = 23 may change.  Bitwise gemv_w8(out_f32) + rope_f32in."""
    pos, cap, dq, dkv = 23, 40, Hq * Dh, Hkv * Dh
    c = _cuda(_w8.gemv_case(dq + 2 * dkv, K, seed=7, norm=True, bias=True))
    wq, sq, wkv, skv, bq, bkv = c["q"][:dq], c["scale"][:dq], c["q"][dq:], c["scale"][dq:], c["bias"][:dq].contiguous(), c["bias"][dq:].contiguous()
    tq, tk = ops.rope_table(64, Dh, 1e6, Dh ** -0.5 * ops.LOG2E, "cuda:0"), ops.rope_table(64, Dh, 1e6, 1.0, "cuda:0")
    row = torch.tensor([pos], device="cuda", dtype=torch.int32)
    ar = Arena("cuda")
    q_out = ar.flat(dq, torch.float16)
    cache = ar.out(cap, 2 * dkv, torch.float16, ld=2 * dkv + 64, tail_rows=16)
    cache.fill_(7.0)
    with frozen(c["q"], c["scale"], c["bias"], c["x"], c["gamma"], row, tq, tk):
        ops.decode_qkv_tab_w8(wq, sq, wkv, skv, bq, bkv, c["x"], c["gamma"], 1e-6, q_out, cache, row, Hq, Hkv, Dh, tq, tk)
    q32 = ops.gemv_w8(wq, sq, c["x"], bq, out_f32=True, rms_gamma=c["gamma"], rms_eps=1e-6).view(1, -1)
    kv32 = ops.gemv_w8(wkv, skv, c["x"], bkv, out_f32=True, rms_gamma=c["gamma"], rms_eps=1e-6).view(1, -1)
    q_b = ops.rope_f32in(q32, tq, Hq, Dh, torch.empty((1, dq), dtype=torch.float16, device="cuda"), 0, pos)
    want = torch.full((cap, 2 * dkv), 7.0, dtype=torch.float16, device="cuda")
    ops.rope_f32in(kv32, tk, Hkv, Dh, want[pos:pos + 1], dkv, pos)
    assert torch.equal(_bits(q_out), _bits(q_b.view(-1))) and torch.equal(_bits(cache), _bits(want))
    ar.check("sc_decode_qkv_tab_w8")
