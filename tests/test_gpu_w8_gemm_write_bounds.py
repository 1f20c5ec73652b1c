"""sc_gemm_w8_f16 writes its output and nothing else: C lives in a tests/_guard.Arena (lead band, the ldc - N gap of every row, a tail band of
further rows), every input is `frozen`.  Shapes, row counts and the CU-masked stream of the persistent kernel: tests/_w8_gemm.py."""
import pytest
import torch

from tests import _guard, _w8_gemm as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,K", G.SHAPES)
def test_gemm_w8_writes_only_its_output(N, K):
    from streamchat_amd import ops
    for bias, res, swiglu, f32 in ((True, True, False, False), (True, False, False, True), (False, False, True, False)):
        c = G.contract_case(N, K, seed=2, bias=bias, res=res, swiglu=swiglu)
        d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        n_out = N // 2 if swiglu else N
        for stream, M in ((s, m) for s in G.streams_for(N, K) for m in G.MS):
            arena = _guard.Arena("cuda")
            # (tail band: 32 rows - the two row groups of 16 a launch may walk - whatever M is)
            out = arena.out(M, n_out, torch.float32 if f32 else torch.float16, ld=n_out + 4 * (M % 2), tail_rows=32)
            a, r = d["a"][:M], None if d["res"] is None else d["res"][:M]
            with _guard.frozen(a, d["q"], d["scale"], d["bias"], r), G.on_stream(stream):
                ops.gemm_w8(a, d["q"], d["scale"], d["bias"], r, epilogue="swiglu" if swiglu else "none", out=out)
                torch.cuda.synchronize()
            arena.check(f"gemm_w8 M={M} N={N} K={K} swiglu={swiglu} f32={f32}")
            assert bool(torch.isfinite(out.float()).all()), "an output element was not written (or a guard byte was read)"
