"""GPU: k_gemm_mid (gemm.hip), the GEMM kernel for 32 < rows < 1024 with K >= 512.

(a) exact-arithmetic operands (tests/_exact.py): `none` with and without bias + residual bit-exact against fp64 rounded once, QuickGELU and
    erf-GELU within half an fp16 ulp + tau.  M = 33, 63 (one partial row tile), 64, 65 (an exact tile and one row past it), 129, 577, 1023;
    N = 128, 384; K = 512 (the shortest the ring takes), 576 (no multiple of the ring depth), 1024.
(b) random fp16 operands: bit-identical to the dispatch without the kernel (a child process with SC_GEMM_MID=0: k_gemm128), at the shapes of (a)
    with K = 1024 and at the BERT-large layer shapes with M = 160 and their real epilogues.
(c) writes go nowhere but rows < M, columns < N of a padded output (tests/_guard.py).
Every case first asserts the dispatcher's precondition for the kernel, restated here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from streamchat_amd import ops
from tests import _exact as X
from tests import _gemm_mid_probe as P
from tests._guard import Arena, frozen
from tests.test_gpu_gemm_exact import _check, _dev_a, _dev_bias, _dev_padded, _fam, _out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MS, NS, KS = (33, 63, 64, 65, 129, 577, 1023), (128, 384), (512, 576, 1024)
# (epilogue, bias, residual)
VARIANTS = {"none-plain": ("none", None, False), "none-bias-res": ("none", "aligned", True), "quick_gelu-bias": ("quick_gelu", "aligned", False),
            "gelu-bias-res": ("gelu", "aligned", True)}


def _takes_mid(M, N, K, epi, a, w, out_f32=False, a_rows=None):
    """launch_gemm's condition for k_gemm_mid (gemm.hip)"""
    return (os.environ.get("SC_GEMM_MID", "")[:1] != "0" and 32 < M < 1024 and not out_f32 and a_rows is None and epi in ("none", "quick_gelu", "gelu")
            and N % 128 == 0 and K % 64 == 0 and K >= 512 and a.stride(0) % 8 == 0 and a.stride(0) * 128 < 2 ** 31 and K * 128 < 2 ** 31
            and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_gemm_mid_exact(M, N, K):
    for kind in X.KINDS:
        a64, w64, b64, r64, acc64 = _fam(M, N, K, kind)
        a, w = _dev_a(a64, None), w64.half().cuda()
        for variant, (epi, bias, res) in VARIANTS.items():
            if epi == "none" and kind == "act":                      # `act` only scales the operands into the activations' bend
                continue
            b, r = _dev_bias(b64, bias), (_dev_padded(r64, 8) if res else None)
            out = _out(M, N, torch.float16)
            assert _takes_mid(M, N, K, epi, a, w)
            ops.gemm(a, w, b, r, epi, out=out, M=M)
            torch.cuda.synchronize()
            _check(f"k_gemm_mid M{M} N{N} K{K} {variant} {kind}", out, acc64 if bias is None else acc64 + b64, r64 if res else None, epi, False)


def _run(tmp, mid):
    out = os.path.join(tmp, f"gemm_{'mid' if mid else 'gemm128'}.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("SC_GEMM_MID", None)
    if not mid:
        env["SC_GEMM_MID"] = "0"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_gemm_mid_probe.py"), out], check=True, env=env, cwd=ROOT, timeout=600)
    return np.load(out)


def test_gemm_mid_equals_gemm128_bitwise(tmp_path):
    a, b = _run(str(tmp_path), False), _run(str(tmp_path), True)
    assert sorted(a.files) == sorted(b.files) and len(a.files) == len(P.MS) * len(P.NS) + 4
    probe = torch.empty((8, 1024), dtype=torch.float16, device="cuda")
    for M, N, K, epi, _, _ in P.cases():
        assert _takes_mid(M, N, K, epi, probe, probe)                # torch allocations: 16-byte aligned, dense rows
    for k in a.files:
        assert not np.isnan(a[k].view(np.float16)).any()
        assert np.array_equal(a[k], b[k]), f"{k}: k_gemm_mid differs from k_gemm128 in {int((a[k] != b[k]).sum())} of {a[k].size} outputs"


@pytest.mark.parametrize("M,N,K,epi,res", [(33, 128, 512, "none", True), (65, 384, 576, "gelu", False), (577, 128, 512, "quick_gelu", True),
                                           (1023, 384, 512, "none", False)])
def test_gemm_mid_writes_only_its_output(M, N, K, epi, res):
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    rn = lambda *s, std=1.0: (torch.randn(*s, device="cuda", generator=g) * std).half()
    a, w, b = rn(M, K), rn(N, K, std=0.03), rn(N, std=0.1)
    r = rn(M, N + 8)[:, :N] if res else None
    arena = Arena("cuda")
    out = arena.out(M, N, torch.float16, ld=N + 8, tail_rows=128)
    assert _takes_mid(M, N, K, epi, a, w)
    with frozen(a, w, b, r):
        ops.gemm(a, w, b, r, epi, out=out)
        torch.cuda.synchronize()
    arena.check(f"k_gemm_mid M{M} N{N} K{K}")
    ref = ops.gemm(a, w, b, r, epi)
    assert not torch.isnan(out.float()).any() and torch.equal(out, ref)
