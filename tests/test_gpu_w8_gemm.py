"""sc_gemm_w8_f16 (gemm_w8.hip, include/streamchat_hip_w8_batched.h): the M <= 32 GEMM over e4m3 weight rows of the batched decode step.
Inputs and references: tests/_w8_gemm.py; that the two contracts used here reject wrong kernels: tests/test_w8_gemm_power.py."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _exact, _w8_gemm as G
from tests._tol import assert_close_fp16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(family, N, K, bias, res, swiglu):
    c = (G.contract_case if family == "contract" else G.exact_case)(N, K, seed=1, bias=bias, res=res, swiglu=swiglu)
    return c, {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _strided(t, pad):
    """the same values in rows `pad` elements longer than the row"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _run(d, M, f32=False, strided=False, stream=None):
    with G.on_stream(stream):
        return _launch(d, M, f32, strided)


def _launch(d, M, f32, strided):
    from streamchat_amd import ops
    a, res = d["a"][:M], None if d["res"] is None else d["res"][:M]
    out = None
    if strided:
        a, res = _strided(a, 8), None if res is None else _strided(res, 4)
        n_out = d["q"].shape[0] // 2 if d["swiglu"] else d["q"].shape[0]
        out = torch.zeros((M, n_out + 4), dtype=torch.float32 if f32 else torch.float16, device="cuda")[:, :n_out]
    return ops.gemm_w8(a, d["q"], d["scale"], d["bias"], res, epilogue="swiglu" if d["swiglu"] else "none", out=out, out_f32=f32)


VARIANTS = (("f16", False, False, False, False), ("f32 + bias", True, False, False, True), ("f16 + bias + residual", True, True, False, False),
            ("swiglu", False, False, True, False))


@pytest.mark.parametrize("N,K", G.SHAPES)
def test_contract_family_against_fp64(N, K):
    """every finite code, spread scales: the fp16 GEMM / GEMV contract against fp64, for every M, epilogue and output type; rows longer than the
    row (lda / ldc / ldr) for the odd M"""
    for stream in G.streams_for(N, K):
        for what, bias, res, swiglu, f32 in VARIANTS:
            c, d = _case("contract", N, K, bias, res, swiglu)
            for M in G.MS:
                y = _run(d, M, f32=f32, strided=M % 2 == 1, stream=stream)
                assert y.dtype == (torch.float32 if f32 else torch.float16)
                assert_close_fp16(y, c["ref"][:M], what=f"gemm_w8 {what} M={M} N={N} K={K}{'' if stream is None else ' masked stream'}")


@pytest.mark.parametrize("N,K", G.SHAPES)
def test_exact_family_bitwise(N, K):
    """exact-arithmetic operands: the fp32 output IS the fp64 value, the fp16 output is it rounded once, SwiGLU within half an ulp + tau"""
    for stream, M in ((s, m) for s in G.streams_for(N, K) for m in G.MS):
        c, d = _case("exact", N, K, True, True, False)
        ref = c["ref"][:M]
        y32 = _run(d, M, f32=True, strided=M % 2 == 1, stream=stream).cpu()
        bad = _exact.differing(y32.double(), ref)
        assert not bool(bad.any()), f"fp32 M={M} N={N} K={K}: {int(bad.sum())} of {bad.numel()} differ from the exact value"
        y16 = _run(d, M, strided=M % 2 == 1, stream=stream).cpu()
        bad = _exact.differing(y16, _exact.rne16(ref))
        assert not bool(bad.any()), f"fp16 M={M} N={N} K={K}: {int(bad.sum())} of {bad.numel()} differ from the exact value rounded once"
        c, d = _case("exact", N, K, False, False, True)
        ys = _run(d, M, stream=stream).cpu()
        z, y = c["z"][:M], c["ref"][:M]
        bad = _exact.half_ulp_excess(ys, y, _exact.tau_swiglu(y, z))
        assert not bool(bad.any()), f"swiglu M={M} N={N} K={K}: {int(bad.sum())} of {bad.numel()} beyond half an ulp + tau"
    assert _exact.unrounded_share(_case("exact", N, K, True, True, False)[0]["ref"]) > 0          # the rounding IS exercised


@pytest.mark.parametrize("N,K", [(48, 256), (48, 2048), (4112, 3584), (48, 18944)])
def test_row_bits_do_not_depend_on_the_other_rows(N, K):
    for bias, res, swiglu, f32 in ((True, True, False, False), (True, False, False, True), (False, False, True, False)):
        c, d = _case("contract", N, K, bias, res, swiglu)
        y26 = _run(d, 26, f32=f32)
        for stream in G.streams_for(N, K):          # (the masked stream's launches against the whole chip's: the grid does not change the bits either)
            y17 = _run(d, 17, f32=f32, stream=stream)
            assert torch.equal(y26[:17], y17), "rows of the M = 26 launch differ from the same rows of an M = 17 launch"
            assert stream is None or torch.equal(_run(d, 26, f32=f32, stream=stream), y26), "the CU-masked launch differs from the whole chip's"
            for r in (0, 15, 16, 25):
                one = dict(d, a=d["a"][r:r + 1], res=None if d["res"] is None else d["res"][r:r + 1])
                assert torch.equal(_run(one, 1, f32=f32, stream=stream)[0], y26[r]), f"row {r} of the M = 26 launch differs from its own M = 1 launch"


def test_more_than_32_rows_are_row_blocks():
    from streamchat_amd import ops
    c, d = _case("contract", 48, 2048, True, True, False)
    a, r = torch.cat([d["a"], d["a"].flip(0), d["a"][:6]]), torch.cat([d["res"], d["res"].flip(0), d["res"][:6]])
    y = ops.gemm_w8(a, d["q"], d["scale"], d["bias"], r)
    y32 = _run(d, 32)
    assert torch.equal(y[:32], y32) and torch.equal(y[32:64], y32.flip(0)) and torch.equal(y[64:], y32[:6])


def _probe(tmp, generic):
    out = os.path.join(tmp, f"w8_gemm_{'generic' if generic else 'default'}.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("SC_SKINNY_W8_GENERIC", None)
    if generic:
        env["SC_SKINNY_W8_GENERIC"] = "1"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_w8_gemm_probe.py"), out], check=True, env=env, cwd=ROOT, timeout=600)
    return np.load(out)


def test_default_dispatch_equals_generic_bitwise(tmp_path):
    a, b = _probe(str(tmp_path), True), _probe(str(tmp_path), False)
    assert sorted(a.files) == sorted(b.files) and len(a.files) == (len(G.SHAPES) + 1) * 5 * 3          # (+ 1: MASKED_SHAPE on the masked stream)
    for k in a.files:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{k}: the default dispatch differs from the generic kernel in {int((a[k] != b[k]).sum())} of {a[k].size} outputs"


def test_argument_errors_return_before_device_work():
    from streamchat_amd import _lib
    lib = _lib.load()
    c, d = _case("contract", 48, 256, True, True, False)
    out = torch.full((32, 48), 7.0, dtype=torch.float16, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    a40 = torch.zeros((40, 256), dtype=torch.float16, device="cuda")

    def call(a=d["a"], lda=256, w=d["q"], woff=0, M=32, K=256, epi=0):
        return lib.sc_gemm_w8_f16(P(a), lda, ctypes.c_void_p(w.data_ptr() + woff), P(d["scale"]), P(d["bias"]), None, 0, P(out), 48, M, 48, K, epi, 0, None)
    for kw, rc, word in ((dict(a=a40, M=33), -1, "M"), (dict(K=192, lda=192), -1, "K"), (dict(woff=8), -1, "aligned"), (dict(epi=1), -4, "epilogue"),
                         (dict(epi=2), -4, "epilogue"), (dict(M=0), -1, "M")):
        assert call(**kw) == rc, kw
        assert word in lib.sc_last_error().decode(), (kw, lib.sc_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
