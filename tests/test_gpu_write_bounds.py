"""GPU: every C ABI entry point that stores through a leading dimension, a stride or a workspace writes ONLY its outputs.

Outputs are views of a guarded arena (tests/_guard.py: lead band, the ld - cols gap of every row, a tail band of at least one tile of the
largest kernel that can take the call), inputs are `frozen`, the result inside the view is still compared with the reference the
existing parity tests use (their tolerances, none new), then every guard byte must still hold the pattern.  Each docstring says which
kernel the shape takes, read off the launchers (gemm.hip launch_gemm / launch_fat, attention.hip sc_attention_f16, kmeans.hip fit_impl).
tests/test_guard_helper.py (host) proves the arena detects and locates stray writes and that COVERED below is complete."""
from ctypes import c_float, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import oracle
from streamchat_amd import _lib, ops
from tests._guard import Arena, frozen
from tests.test_gpu_dense import _attn_ref
from tests.test_gpu_misc import ref_preprocess

pytestmark = pytest.mark.gpu

# C ABI function with a writable device pointer -> the tests below that run it against the arena (checked by tests/test_guard_helper.py)
COVERED = {
    "sc_gemm_f16": ["test_gemm_write_bounds", "test_gemm_on_a_cu_masked_stream"],
    "sc_gemm_headed_f16": ["test_gemm_headed_write_bounds"],
    "sc_gemv_f16": ["test_gemv_write_bounds"],
    "sc_decode_qkv_tab_f16": ["test_decode_qkv_tab_write_bounds"],
    "sc_rope_table_f32": ["test_rope_table_write_bounds"],
    "sc_rope_f32in_f16": ["test_rope_f32in_write_bounds"],
    "sc_rope_qkv_rows_f16": ["test_rope_qkv_rows_write_bounds"],
    "sc_layernorm_f16": ["test_norm_write_bounds"],
    "sc_rmsnorm_f16": ["test_norm_write_bounds"],
    "sc_attention_f16": ["test_attention_write_bounds", "test_attention_head_packed_decode_write_bounds"],
    "sc_pick_token_f32": ["test_pick_and_sample_token_write_bounds"],
    "sc_sample_token_f32": ["test_pick_and_sample_token_write_bounds"],
    "sc_kmeans_fit": ["test_kmeans_write_bounds"],
    "sc_kmeans_assign": ["test_kmeans_write_bounds"],
    "sc_kmeans_update": ["test_kmeans_write_bounds"],
    "sc_sim_topk": ["test_sim_topk_write_bounds"],
    "sc_decode_advance": ["test_decode_advance_write_bounds"],
    "sc_counter_uniform_f32": ["test_counter_uniform_write_bounds"],
    "sc_preprocess_u8": ["test_preprocess_write_bounds"],
    "sc_preprocess_patchify_u8": ["test_preprocess_write_bounds"],
    "sc_patchify_f16": ["test_preprocess_write_bounds"],
    "sc_pool_f16": ["test_pool_and_avgpool_write_bounds"],
    "sc_avgpool_tokens_f16": ["test_pool_and_avgpool_write_bounds"],
    "sc_gather_rows_f16": ["test_gather_rows_write_bounds"],
    "sc_vit_embed_ln_f16": ["test_embed_ln_write_bounds"],
    "sc_bert_embed_ln_f16": ["test_embed_ln_write_bounds"],
}
# not run against the arena, and why
EXEMPT = {
    "sc_kmeans_fit_cols": "multi-GPU path (needs a caller-supplied exchange; tests/test_gpu_kmeans_cols.py, test_gpu_sharded.py), out of this module's scope",
    "sc_stream_create_masked": "its only pointer is a HOST out-parameter (the stream handle)",
    "sc_device_info": "host out-parameters only",
}


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, device="cuda", generator=_gen(seed)) * scale).half()


def _strided(rows, cols, ld, seed, scale=1.0, dtype=torch.float16):
    """an INPUT [rows, cols] with row stride ld > cols (a column slice of a wider tensor whose other columns are NaN: a read of them shows)"""
    full = torch.full((rows, ld), float("nan"), dtype=dtype, device="cuda")
    full[:, :cols] = (torch.randn((rows, cols), device="cuda", generator=_gen(seed)) * scale).to(dtype)
    return full[:, :cols]


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _P(t):
    return None if t is None else c_void_p(t.data_ptr())


def _epi_ref(z, epi):
    if epi == "quick_gelu":
        return z * torch.sigmoid(1.702 * z)
    if epi == "gelu":
        return torch.nn.functional.gelu(z)
    if epi == "swiglu":
        q = z.view(z.shape[0], z.shape[1] // 4, 2, 2)                  # interleaved (g0, g1, u0, u1) quads
        return (torch.nn.functional.silu(q[:, :, 0]) * q[:, :, 1]).reshape(z.shape[0], z.shape[1] // 2)
    return z


def _run_gemm(M, N, K, epi="none", f32=False, bias="aligned", res=False, ldc_pad=8, c_misalign=0, a_rows=None):
    """one sc_gemm_f16 call with a guarded C (ldc = output width + ldc_pad; for swiglu ldc = N: the right half of every row is guard),
    a strided A, a residual with ldr > N; returns (out, arena, reference)"""
    a_store = M if a_rows is None else (M // a_rows[0]) * a_rows[1] + a_rows[2] + 1
    a = _strided(a_store, K, K + 8, 1)
    w = _rand((N, K), 2, K ** -0.5)
    b = None if bias is None else (_rand((N,), 3) if bias == "aligned" else _rand((N + 4,), 3)[4:])     # "odd": 8-byte aligned only
    r = _strided(M, N, N + 8, 4) if res else None
    ncol = N // 2 if epi == "swiglu" else N
    ar = Arena("cuda")
    out = ar.out(M, ncol, torch.float32 if f32 else torch.float16, ld=N if epi == "swiglu" else ncol + ldc_pad, tail_rows=256,
                 align=16 if c_misalign else 256, misalign=c_misalign)
    with frozen(a, w, b, r):
        ops.gemm(a, w, b, r, epi, out=out, a_rows=a_rows, M=M)
    if a_rows is None:
        al = a
    else:
        m = torch.arange(M, device="cuda")
        al = a[(m // a_rows[0]) * a_rows[1] + a_rows[2] + m % a_rows[0]]
    z = al.float() @ w.float().t()
    ref = _epi_ref(z if b is None else z + b.float(), epi)
    if r is not None:
        ref = ref + r.float()
    return out, ar, ref


GEMM_CASES = {
    # k_gemm128: M < 1024, or N % 256 != 0, or a C that is only 8-byte aligned (wide_ok false)
    "gemm128_tail130": dict(M=130, N=384, K=192, epi="quick_gelu", res=True),
    "gemm128_M33": dict(M=33, N=256, K=128, epi="gelu"),
    "gemm128_f32_N384": dict(M=1100, N=384, K=256, f32=True),
    "gemm128_swiglu": dict(M=130, N=512, K=128, epi="swiglu"),
    "gemm128_c_8byte_aligned": dict(M=1154, N=256, K=128, c_misalign=8, ldc_pad=4),
    # k_gemm256: M >= 1024, N % 256 == 0, and fp32 out / a row map / K % 128 != 0 / an 8-byte aligned bias
    "gemm256_f32": dict(M=1154, N=512, K=256, f32=True, ldc_pad=4),
    "gemm256_a_rows": dict(M=1152, N=256, K=128, a_rows=(576, 577, 1)),
    "gemm256_K192": dict(M=1154, N=256, K=192, epi="gelu", res=True),
    "gemm256_bias_8byte_aligned": dict(M=1300, N=512, K=128, bias="odd"),
    # k_gemm_fat: M >= 1024, fp16 out, K % 128 == 0, 16-byte aligned everything
    "fat_single_tiles_1154": dict(M=1154, N=512, K=256),
    "fat_persistent_4099_residual": dict(M=4099, N=4096, K=128, epi="quick_gelu", res=True),
    "fat_swiglu_1154": dict(M=1154, N=512, K=128, epi="swiglu"),
    # k_gemm_skinny: M <= 32 with an epilogue other than none / swiglu, a misaligned operand, or a K the LDS-ring kernels do not take
    "skinny_M1_quick_gelu": dict(M=1, N=128, K=128, epi="quick_gelu"),
    "skinny_M17_gelu_residual": dict(M=17, N=256, K=256, epi="gelu", res=True),
    "skinny_M16_bias_8byte_aligned": dict(M=16, N=256, K=2048, bias="odd"),
    "skinny_M32_K384": dict(M=32, N=384, K=384, ldc_pad=4),
    # k_gemm_skinny_l: M <= 32, none / swiglu, K % 512 == 0, K >= 2048, N / 16 < 2 x CUs
    "skinny_l_M16_residual": dict(M=16, N=512, K=2048, res=True),
    "skinny_l_M17_f32": dict(M=17, N=1024, K=2048, f32=True),
    "skinny_l_M32_swiglu": dict(M=32, N=1024, K=4096, epi="swiglu", bias=None),
    "skinny_l_M1_K3584": dict(M=1, N=3584, K=3584),
    # k_gemm_skinny_lx: M <= 32, K = 3584, N / 16 >= 2 x CUs
    "skinny_lx_M16": dict(M=16, N=8320, K=3584),
    "skinny_lx_M32_swiglu": dict(M=32, N=9216, K=3584, epi="swiglu", bias=None),
}


@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm_write_bounds(case):
    """sc_gemm_f16, one case per dispatch branch of launch_gemm (gemm.hip), named by the kernel it selects:
    k_gemm128 (128 x 128 tiles): M < 1024 (130 = one whole tile + 2 rows; 33 = just past the skinny limit), N % 256 != 0 (384) also with fp32
      out at M >= 1024, swiglu, and M >= 1024 with a C that is only 8-byte aligned (the 16-byte epilogue stores of the 256-tiles need more);
    k_gemm256: M >= 1024 and N % 256 == 0 with what k_gemm_fat does not take - fp32 out, the A row map (576, 577, 1), K = 192, a bias at an
      8-byte offset;  k_gemm_fat: fp16, aligned, K % 128 == 0 - 1154 x 512 (10 tiles, one per workgroup), 4099 x 4096 (272 tiles > 256 CUs:
      the persistent walk) with residual, swiglu;
    k_gemm_skinny (M <= 32): quick_gelu / gelu epilogues (M = 1, 17), a bias at an 8-byte offset (M = 16), K = 384;
    k_gemm_skinny_l: K % 512 == 0, K >= 2048, N / 16 < 512 strips - M = 16 (MG 1), 17 and 32 (MG 2), fp32 out, swiglu, M = 1 at K = 3584;
    k_gemm_skinny_lx: K = 3584 with N / 16 = 520 / 576 strips - M = 16 and 32, swiglu.
    C has ldc > N (swiglu: ldc = N, its right half is guard), the residual ldr > N, A lda > K; tail band: 256 rows (one k_gemm_fat tile)."""
    kw = GEMM_CASES[case]
    out, ar, ref = _run_gemm(**kw)
    tol = 1e-3 if kw.get("f32") else 2e-3
    torch.testing.assert_close(out.float(), ref, rtol=tol, atol=tol)
    ar.check(f"sc_gemm_f16 {case}")


def test_gemm_on_a_cu_masked_stream():
    """sc_gemm_f16 on ops.masked_stream(0, 64) (torch.cuda.ExternalStream over sc_stream_create_masked, as session.py runs its jobs):
    k_gemm_fat (4099 x 4096: 272 tiles walked by 64 workgroups instead of 256), k_gemm_skinny_l (N = 1152: 72 strips over 64 workgroups, 1 each
    + 8 left over, against 72 workgroups on the default stream) and k_gemm_skinny_lx (N = 8320: 520 strips = 8 x 64 + 8 against 2 x 256 + 8)
    size their grids from the stream's CU count.  Bitwise equal to the default stream's result, guards intact.  The stream stays owned by
    ops._masked_streams."""
    s = ops.masked_stream(0, 64)
    assert ops.masked_stream(0, 64) is s
    for kw in (dict(M=4099, N=4096, K=128, epi="quick_gelu", res=True), dict(M=16, N=1152, K=2048), dict(M=32, N=8320, K=3584)):
        base, ar0, ref = _run_gemm(**kw)
        ar0.check(f"default stream {kw}")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            out, ar, _ = _run_gemm(**kw)
            s.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(base)), kw
        torch.testing.assert_close(out.float(), ref, rtol=2e-3, atol=2e-3)
        ar.check(f"masked stream {kw}")
    assert ops._masked_streams and s in ops._masked_streams.values()


@pytest.mark.parametrize("mode,M,N,K,lead", [("rope", 1154, 512, 256, 256), ("rope", 4099, 4096, 128, 3584), ("colscale", 1154, 768, 128, 256)])
def test_gemm_headed_write_bounds(mode, M, N, K, lead):
    """sc_gemm_headed_f16 -> launch_fat<SC_EPI_ROPE / SC_EPI_COLSCALE> (k_gemm_fat only) with lead_cols < N and a ragged last row tile
    (1154 = 4 x 256 + 130; 4099 x 4096 is the persistent walk).  ROPE: bitwise the fp32 projection + sc_rope_f32in_f16, as
    tests/test_gpu_rope_fused.py pins it; COLSCALE: plain columns bitwise the ordinary GEMM, scaled ones against fp64 with that file's bound."""
    a, w, b = _strided(M, K, K + 8, 1), _rand((N, K), 2, K ** -0.5), _rand((N,), 3)
    ar = Arena("cuda")
    out = ar.out(M, N, torch.float16, ld=N + 8, tail_rows=256)
    assert ops.gemm_headed_ok(N, K, a, w, b, out)
    if mode == "rope":
        tab = ops.rope_table(5 + M, 128, 1e6, 1.0, "cuda:0")
        with frozen(a, w, b, tab):
            ops.gemm_headed(a, w, b, out, "rope", lead, tab, 5)
        acc = ops.gemm(a, w, b, out_f32=True)
        two = ops.rope_f32in(acc, tab, lead // 128, 128, torch.empty((M, N), dtype=torch.float16, device="cuda"), N - lead, 5)
        assert torch.equal(_bits(out), _bits(two))
    else:
        c = 0.125 * ops.LOG2E
        with frozen(a, w, b):
            ops.gemm_headed(a, w, b, out, "colscale", lead, col_scale=c)
        assert torch.equal(_bits(out[:, lead:]), _bits(ops.gemm(a, w, b)[:, lead:]))
        z = (a.double() @ w[:lead].double().t() + b[:lead].double()) * c
        assert (out[:, :lead].double() - z).abs().max().item() <= 1.1 * 2 ** -11 * z.abs().max().item() + 1e-4
    ar.check(f"sc_gemm_headed_f16 {mode}")


@pytest.mark.parametrize("N,K", [(512, 256), (1024, 3584)])
def test_gemv_write_bounds(N, K):
    """sc_gemv_f16: K = 256 takes the generic k_gemv kernels, K = 3584 the straight-line k_gemv_u ones (no y_row) - plain fp16, fp32 out with
    fused RMSNorm + bias + residual, swiglu (N/2 outputs), into arena vectors of exactly the output size; and `out_row`: y is a KV-cache
    view [12, N] with ld = N + 64, the row index lives on the device - only row 5 may change (k_gemv with y_row, both K)."""
    w, x, b, r = _rand((N, K), 1, K ** -0.5), _rand((K,), 2), _rand((N,), 3), _rand((N,), 4)
    g = (1 + _rand((K,), 5, 0.1).float()).half()
    ar = Arena("cuda")
    y16, y32, ysw = ar.flat(N, torch.float16), ar.flat(N, torch.float32), ar.flat(N // 2, torch.float16)
    cache = ar.out(12, N, torch.float16, ld=N + 64, tail_rows=16)
    cache.fill_(7.0)
    row = torch.tensor([5], dtype=torch.int32, device="cuda")
    with frozen(w, x, b, r, g, row):
        ops.gemv(w, x, b, r, out=y16)
        ops.gemv(w, x, b, r, out=y32, rms_gamma=g, rms_eps=1e-6)
        ops.gemv(w, x, epilogue="swiglu", out=ysw)
        ops.gemv(w, x, b, out=cache, out_row=row)
    z = w.float() @ x.float() + b.float()
    torch.testing.assert_close(y16.float(), z + r.float(), rtol=2e-3, atol=2e-3)
    xn = (g.double() * (x.double() * torch.rsqrt((x.double() ** 2).mean() + 1e-6)).half().double()).half().double()
    torch.testing.assert_close(y32.double(), w.double() @ xn + b.double() + r.double(), rtol=1e-3, atol=1e-3)
    q = (w.float() @ x.float()).view(N // 4, 2, 2)
    torch.testing.assert_close(ysw.float(), (torch.nn.functional.silu(q[:, 0]) * q[:, 1]).reshape(-1), rtol=3e-3, atol=3e-3)
    torch.testing.assert_close(cache[5].float(), z, rtol=2e-3, atol=2e-3)
    keep = torch.arange(12, device="cuda") != 5
    assert bool((cache[keep] == 7.0).all()), "sc_gemv_f16 with y_row changed another cache row"
    ar.check("sc_gemv_f16")


@pytest.mark.parametrize("Hq,Hkv,K", [(4, 2, 512), (28, 4, 3584)])
def test_decode_qkv_tab_write_bounds(Hq, Hkv, K):
    """sc_decode_qkv_tab_f16: K = 512 is the generic k_decode_qkv, K = 3584 with RMSNorm the straight-line k_decode_qkv_u<7>.  q_out is an arena
    vector of exactly Hq Dh elements, the KV cache an arena view [40, 2 Hkv Dh] with cache_ld 64 elements wider: only row pos[0] = 23 may
    change.  Bitwise gemv(out_f32) + rope_f32in, as tests/test_gpu_rope_fused.py pins it."""
    Dh, pos, cap = 128, 23, 40
    wq, wkv = _rand((Hq * Dh, K), 1, K ** -0.5), _rand((2 * Hkv * Dh, K), 2, K ** -0.5)
    bq, bkv, x, g = _rand((Hq * Dh,), 3), _rand((2 * Hkv * Dh,), 4), _rand((K,), 5), (1 + _rand((K,), 6, 0.1).float()).half()
    tq, tk = ops.rope_table(64, Dh, 1e6, Dh ** -0.5 * ops.LOG2E, "cuda:0"), ops.rope_table(64, Dh, 1e6, 1.0, "cuda:0")
    row = torch.tensor([pos], device="cuda", dtype=torch.int32)
    ar = Arena("cuda")
    q_out = ar.flat(Hq * Dh, torch.float16)
    cache = ar.out(cap, 2 * Hkv * Dh, torch.float16, ld=2 * Hkv * Dh + 64, tail_rows=16)
    cache.fill_(7.0)
    with frozen(wq, wkv, bq, bkv, x, g, row, tq, tk):
        ops.decode_qkv_tab(wq, wkv, bq, bkv, x, g, 1e-6, q_out, cache, row, Hq, Hkv, Dh, tq, tk)
    q32 = ops.gemv(wq, x, bq, out_f32=True, rms_gamma=g, rms_eps=1e-6).view(1, -1)
    kv32 = ops.gemv(wkv, x, bkv, out_f32=True, rms_gamma=g, rms_eps=1e-6).view(1, -1)
    q_b = ops.rope_f32in(q32, tq, Hq, Dh, torch.empty((1, Hq * Dh), dtype=torch.float16, device="cuda"), 0, pos)
    want = torch.full((cap, 2 * Hkv * Dh), 7.0, dtype=torch.float16, device="cuda")
    ops.rope_f32in(kv32, tk, Hkv, Dh, want[pos:pos + 1], Hkv * Dh, pos)
    assert torch.equal(_bits(q_out), _bits(q_b.view(-1))) and torch.equal(_bits(cache), _bits(want))
    ar.check("sc_decode_qkv_tab_f16")


def test_rope_table_write_bounds():
    """sc_rope_table_f32 / k_rope_table: a table of exactly max_pos x Dh floats (max_pos x Dh / 2 = 999 x 64 threads: a partial last block)"""
    ar = Arena("cuda")
    tab = ar.flat(999 * 128, torch.float32)
    _lib.check(_lib.load().sc_rope_table_f32(_P(tab), 999, 128, c_float(1e6), c_float(0.5), _lib.stream_ptr("cuda:0")), "sc_rope_table_f32")
    assert torch.equal(_bits(tab.view(999, 2, 64)), _bits(ops.rope_table(999, 128, 1e6, 0.5, "cuda:0")[:999]))
    ar.check("sc_rope_table_f32")


def test_rope_f32in_write_bounds():
    """sc_rope_f32in_f16 / k_rope_f32in: ldo > width (8 guard columns per row), plain_cols > 0, explicit positions (one past the table: clamped),
    a strided fp32 input; bitwise the same call into a dense output."""
    rows, heads, Dh, plain = 37, 4, 128, 512
    wd = heads * Dh + plain
    x = _strided(rows, wd, wd + 4, 7, dtype=torch.float32)
    pos = torch.randint(0, 5000, (rows,), device="cuda", generator=_gen(8), dtype=torch.int32)
    pos[3] = 10 ** 6
    tab = ops.rope_table(5000, Dh, 1e6, 1.0, "cuda:0")
    ar = Arena("cuda")
    out = ar.out(rows, wd, torch.float16, ld=wd + 8, tail_rows=16)
    with frozen(x, pos, tab):
        ops.rope_f32in(x, tab, heads, Dh, out, plain, 0, pos)
    dense = ops.rope_f32in(x.contiguous(), tab, heads, Dh, torch.empty((rows, wd), dtype=torch.float16, device="cuda"), plain, 0, pos.clamp(max=tab.shape[0] - 1))
    assert torch.equal(_bits(out), _bits(dense)) and torch.equal(_bits(out[:, heads * Dh:]), _bits(x[:, heads * Dh:].half()))
    ar.check("sc_rope_f32in_f16")


def test_rope_qkv_rows_write_bounds():
    """sc_rope_qkv_rows_f16 / k_rope_qkv_rows: B = 5, distinct positions incl. -3 and 1000 (clamped to cache rows 0 and cap - 1), q_out with
    ldq > Hq Dh, the cache an arena view [B, cap, 2 Hkv Dh] with cache_ld 64 elements wider: per sequence only the (clamped) row changes.
    Reference: sc_rope_f32in_f16 twice + a row scatter (tests/test_gpu_rope_fused.py)."""
    B, Hq, Hkv, Dh, cap = 5, 28, 4, 128, 40
    dq, dkv = Hq * Dh, Hkv * Dh
    x = _strided(B, dq + 2 * dkv, dq + 2 * dkv + 4, 3, 3.0, torch.float32)
    tq, tk = ops.rope_table(64, Dh, 1e6, Dh ** -0.5 * ops.LOG2E, "cuda:0"), ops.rope_table(64, Dh, 1e6, 1.0, "cuda:0")
    rows = min(tq.shape[0], tk.shape[0])                              # (the cached tables grow independently; the ABI takes one row count)
    tq, tk = tq[:rows], tk[:rows]
    pos = torch.tensor([0, 7, 1000, 12, -3], dtype=torch.int32, device="cuda")
    ar = Arena("cuda")
    q = ar.out(B, dq, torch.float16, ld=dq + 8, tail_rows=16)
    cache = ar.out(B * cap, 2 * dkv, torch.float16, ld=2 * dkv + 64, tail_rows=cap).unflatten(0, (B, cap))
    cache.fill_(7.0)
    with frozen(x, pos, tq, tk):
        ops.rope_qkv_rows(x, tq, tk, pos, Hq, Hkv, Dh, q, cache)
    tpos, rpos = pos.clamp(0, tq.shape[0] - 1), pos.clamp(0, cap - 1).long()
    xc = x.contiguous()
    q_ref = ops.rope_f32in(xc[:, :dq], tq, Hq, Dh, torch.empty((B, dq), dtype=torch.float16, device="cuda"), 0, 0, tpos)
    kv_ref = ops.rope_f32in(xc[:, dq:], tk, Hkv, Dh, torch.empty((B, 2 * dkv), dtype=torch.float16, device="cuda"), dkv, 0, tpos)
    want = torch.full((B, cap, 2 * dkv), 7.0, dtype=torch.float16, device="cuda")
    want[torch.arange(B, device="cuda"), rpos] = kv_ref
    assert torch.equal(_bits(q), _bits(q_ref)) and torch.equal(_bits(cache), _bits(want))
    ar.check("sc_rope_qkv_rows_f16")


@pytest.mark.parametrize("rows,cols", [(5, 64), (7, 384), (33, 1024), (6, 3584), (1001, 4096), (3, 1280)])
def test_norm_write_bounds(rows, cols):
    """sc_layernorm_f16 / sc_rmsnorm_f16 -> k_norm<NV, RMS>: cols 64 and 384 are NV = 1 (384: a partial vector group), 1024 NV = 2, 1280 and 3584
    NV = 4 / 8 with a partial last group, 4096 NV = 8 full; rows never a multiple of the 4 rows of a workgroup; ldx != ldy, both > cols."""
    x, g, b = _strided(rows, cols, cols + 16, 1, 3.0), _rand((cols,), 2), _rand((cols,), 3)
    ar = Arena("cuda")
    y, z = ar.out(rows, cols, torch.float16, ld=cols + 8, tail_rows=8), ar.out(rows, cols, torch.float16, ld=cols + 24, tail_rows=8)
    with frozen(x, g, b):
        ops.layernorm(x, g, b, 1e-5, out=y)
        ops.rmsnorm(x, g, 1e-6, out=z)
    xf = x.float()
    torch.testing.assert_close(y.float(), torch.nn.functional.layer_norm(xf, (cols,), g.float(), b.float(), 1e-5), rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(z.float(), g.float() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)).half().float(), rtol=2e-3, atol=2e-3)
    ar.check("sc_layernorm_f16 / sc_rmsnorm_f16")


@pytest.mark.parametrize("B,Sq,Skv,Hq,Hkv,Dh,causal,ns,variant", [
    (2, 577, 577, 4, 4, 64, False, 1, 0), (3, 7, 130, 4, 2, 64, False, 1, 0), (1, 1, 130, 4, 4, 128, False, 1, 0), (2, 7, 300, 4, 4, 64, False, 4, 0),
    (1, 2050, 2050, 2, 1, 128, True, 1, 1), (2, 7, 3000, 4, 2, 128, False, 16, 3)])
def test_attention_write_bounds(B, Sq, Skv, Hq, Hkv, Dh, causal, ns, variant):
    """sc_attention_f16 with out_ld = Hq Dh + 8 (8 guard columns behind the last head of every row), tail band 256 rows (> the 128 / 192 query rows
    of a k_attn workgroup).  variant 0 = k_attn<Dh, 2> (Sq 577 = 4 x 128 + 65, 7, 1; Dh 64 and 128; nsplit 4 with its combine kernel), variant 1 =
    k_attn<128, 3, 32> (Sq 2050 >= 2048 = 10 x 192 + 130, causal, GQA), variant 3 = k_attn_decode + combine (Dh 128, Sq 7 <= 16, nsplit 16).  With
    nsplit > 1 the workspace is an arena view of EXACTLY ops.attention_workspace_bytes() bytes.  Where B > 1 the last batch row is fully padded
    (kv_len = 0): whatever it holds, it is written inside its own rows only; the other rows against the fp32 reference."""
    assert ops.attention_variant(Dh, Sq, ns) == variant
    q, k, v = _rand((B, Sq, Hq * Dh), 1), _rand((B, Skv, Hkv * Dh), 2), _rand((B, Skv, Hkv * Dh), 3)
    kv_len = None
    if B > 1:
        kv_len = torch.tensor([Skv - 3, Skv, 0][-B:] if B == 3 else [Skv - 3, 0], dtype=torch.int32, device="cuda")
        k[0, Skv - 3:], v[0, Skv - 3:] = float("nan"), float("nan")
    ar = Arena("cuda")
    out = ar.out(B * Sq, Hq * Dh, torch.float16, ld=Hq * Dh + 8, tail_rows=256).unflatten(0, (B, Sq))
    ws = ar.flat(ops.attention_workspace_bytes(B, Hq, Sq, ns, Dh), torch.uint8) if ns > 1 else None
    with frozen(q, k, v, kv_len):
        ops.attention(q, k, v, Hq, Hkv, Dh, Dh ** -0.5, causal, kv_len=kv_len, out=out, nsplit=ns, ws=ws)
    live = B if kv_len is None else B - 1
    kk, vv = torch.nan_to_num(k[:live]), torch.nan_to_num(v[:live])
    ref = _attn_ref(q[:live], kk, vv, Hq, Hkv, Dh, Dh ** -0.5, causal, None if kv_len is None else kv_len[:live])
    torch.testing.assert_close(out[:live].float(), ref, rtol=2e-3, atol=2e-3)
    ar.check(f"sc_attention_f16 variant {variant}")


@pytest.mark.parametrize("Dh,ns,variant", [(128, 8, 3), (64, 4, 0)])
def test_attention_head_packed_decode_write_bounds(Dh, ns, variant):
    """The batched decode step's addressing (llm.BatchDecoder): q is [B, Hq Dh]; with ldq = Dh, q_head_stride = G Dh and q_batch_stride = Hq Dh the G
    query heads of a GQA group are G query ROWS of one KV head, and out is written the same way (out_ld = Dh, o_head_stride = G Dh, o_batch_stride
    = the row stride of out).  out is an arena view [B, Hq Dh] with 64 guard elements behind the last head of every packed row, the workspace
    exactly the reported bytes, one sequence fully padded.  Dh 128 -> k_attn_decode (variant 3), Dh 64 -> k_attn + combine (variant 0)."""
    B, Hq, Hkv, Skv = 3, 8, 2, 700
    G, dq = Hq // Hkv, Hq * Dh
    assert ops.attention_variant(Dh, G, ns) == variant
    q, k, v = _rand((B, dq), 1), _rand((B, Skv, Hkv * Dh), 2), _rand((B, Skv, Hkv * Dh), 3)
    kv_len = torch.tensor([Skv, 333, 0], dtype=torch.int32, device="cuda")
    k[1, 333:], v[1, 333:] = float("nan"), float("nan")
    ar = Arena("cuda")
    out2 = ar.out(B, dq, torch.float16, ld=dq + 64, tail_rows=64)
    out = out2.as_strided((B, G, Hkv * Dh), (dq + 64, Hkv * Dh, 1))
    ws = ar.flat(ops.attention_workspace_bytes(B, Hkv, G, ns, Dh), torch.uint8)
    with frozen(q, k, v, kv_len):
        ops.attention(q.as_strided((B, G, Dh), (dq, Dh, 1)), k, v, Hkv, Hkv, Dh, Dh ** -0.5, causal=False, kv_len=kv_len, out=out, nsplit=ns,
                      q_head_stride=G * Dh, o_head_stride=G * Dh, out_ld=Dh, ws=ws)
    ref = _attn_ref(q[:2].view(2, 1, dq), torch.nan_to_num(k[:2]), torch.nan_to_num(v[:2]), Hq, Hkv, Dh, Dh ** -0.5, False, kv_len[:2])
    torch.testing.assert_close(out2[:2].float(), ref.view(2, dq), rtol=2e-3, atol=2e-3)
    ar.check(f"sc_attention_f16 head-packed, variant {variant}")


def test_pick_and_sample_token_write_bounds():
    """sc_pick_token_f32 (k_pick_partial + k_pick_final) and sc_sample_token_f32 - the candidate path (top_k 20 <= 64: k_topk_partial / k_topk_final)
    and the radix-select path (top_k 100, and a nucleus without top-k: k_full_filter) - on logits rows with ld = V + 24, `ws` an arena view
    of EXACTLY the reported bytes, `out` an arena vector.  The logits are unchanged whenever repetition_penalty == 1 and changed exactly at
    the distinct previous ids (x < 0 ? x r : x / r) when it is not - the documented contract, both ways."""
    lib = _lib.load()
    B, V = 3, 5000
    lg = _strided(B, V, V + 24, 1, 3.0, torch.float32)
    lg[0, 17] = 50.0
    u = torch.tensor([0.1, 0.5, 0.9], device="cuda")
    ar = Arena("cuda")
    out = ar.flat(B, torch.int64)
    ws_p = ar.flat(lib.sc_pick_token_workspace_bytes(B), torch.uint8)
    ws_s = ar.flat(ops.sample_token_workspace_bytes(B), torch.uint8)
    with frozen(lg, u):
        assert ops.pick_token(lg, out=out, ws=ws_p).tolist() == torch.argmax(lg, -1).tolist()
        got = ops.pick_token(lg, 0.7, u, out=out, ws=ws_p).tolist()
        assert got[0] == 17 and all(0 <= t < V for t in got)
        for top_k, top_p in ((20, 1.0), (20, 0.8), (100, 1.0), (0, 0.9), (0, 1.0)):
            got = ops.sample_token(lg, 0.7, u, top_k=top_k, top_p=top_p, out=out, ws=ws_s).tolist()
            keep = V if top_k == 0 else top_k
            for bi, t in enumerate(got):                               # the drawn token is one of the top-k logits of its row
                assert 0 <= t < V and float(lg[bi, t]) >= float(lg[bi].topk(keep).values[-1]), (top_k, top_p, bi, t)
        assert ops.sample_token(lg, 0.0, None, top_k=20, repetition_penalty=1.0, out=out, ws=ws_s).tolist() == torch.argmax(lg, -1).tolist()
    prev = torch.tensor([[17, 17, 3], [5, 6, 5], [0, 1, 2]], device="cuda")
    before = lg.clone()
    with frozen(prev, u):
        got = ops.sample_token(lg, 0.0, None, repetition_penalty=1.5, prev_ids=prev, out=out, ws=ws_s).tolist()
    exp = before.cpu()                                                # (on the host: a true fp32 division, as HF's processor does it)
    for bi in range(B):
        ids = prev[bi].unique().cpu()
        exp[bi, ids] = torch.where(exp[bi, ids] < 0, exp[bi, ids] * 1.5, exp[bi, ids] / 1.5)
    assert torch.equal(_bits(lg.cpu()), _bits(exp)) and not torch.equal(_bits(lg), _bits(before)) and got == torch.argmax(exp, -1).tolist()
    ar.check("sc_pick_token_f32 / sc_sample_token_f32")


def _km_call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args), name)


@pytest.mark.parametrize("T,D,K,dtype,path", [(60, 4096, 4, torch.float16, "two-pass"), (150, 4096, 5, torch.float16, "km2_pass RGW 4"),
                                              (300, 2048, 5, torch.float16, "km2_pass RGW 7"), (70, 100, 3, torch.float32, "two-pass, D 100")])
def test_kmeans_write_bounds(T, D, K, dtype, path):
    """sc_kmeans_fit / sc_kmeans_assign / sc_kmeans_update with C, labels, wsum, info, dist2, C_new, shift2 as arena views of exactly their sizes
    and X, weights, init_idx, reseed_idx, labels-in, C-in frozen (the fit's internal workspace stays ops._workspace's).  fit_impl (kmeans.hip):
    T = 60 < 120 -> km_assign / km_update (two passes); T = 150, K = 5 -> T + 7 K = 185 <= 256: km2_pass<5, 4>; T = 300 -> 335 <= 448:
    km2_pass<5, 7>; D = 100 fp32 -> D % 64 != 0 and D % 8 != 0: the two-pass scalar kernels.  Labels, centroids, weights bit-identical to the
    oracle, dist2 to oracle.kmeans_dist2 (tests/test_gpu_kmeans.py)."""
    lib = _lib.load()
    rng = np.random.default_rng(T)
    Xn = (rng.standard_normal((T, D)) + 3.0 * rng.integers(0, K, (T, 1))).astype(np.float16 if dtype == torch.float16 else np.float32)
    X = torch.from_numpy(Xn).cuda()
    init = torch.from_numpy(rng.choice(T, K, replace=False).astype(np.int32)).cuda()
    reseed = torch.from_numpy(rng.integers(0, T, 30).astype(np.int32)).cuda()
    w = torch.from_numpy((rng.random(T) + 0.5).astype(np.float32)).cuda()
    ar = Arena("cuda")
    C, Cn = ar.out(K, D, torch.float32, tail_rows=16), ar.out(K, D, torch.float32, tail_rows=16)
    labels, labels2 = ar.flat(T, torch.int64), ar.flat(T, torch.int64)
    wsum, wsum2, info = ar.flat(K, torch.float32), ar.flat(K, torch.float32), ar.flat(4, torch.int32)
    d2, shift2 = ar.out(T, K, torch.float64, tail_rows=16), ar.flat(K, torch.float64)
    ws = ops._workspace(lib.sc_kmeans_workspace_bytes(T, D, K), X.device)
    code, st = ops._code(X), _lib.stream_ptr(X.device)
    with frozen(X, w, init, reseed):
        _km_call("sc_kmeans_fit", _P(X), code, T, c_int64(D), K, _P(w), _P(init), _P(reseed), 30, 6, c_float(1e-4), _P(C), _P(labels), _P(wsum), _P(info),
                 _P(ws), c_size_t(ws.numel()), st)
        Cfit, Cold = C.clone(), (C + 0.25).contiguous()
        with frozen(Cfit, Cold):
            _km_call("sc_kmeans_assign", _P(X), code, T, c_int64(D), K, _P(Cfit), _P(labels2), _P(d2), _P(ws), c_size_t(ws.numel()), st)
            lab_in = labels2.clone()
            with frozen(lab_in):
                _km_call("sc_kmeans_update", _P(X), code, T, c_int64(D), K, _P(w), _P(lab_in), _P(Cold), 1, None, 0, _P(Cn), _P(wsum2), _P(shift2),
                         _P(ws), c_size_t(ws.numel()), st)
    ref = oracle.kmeans_fit(Xn, K, init.cpu().numpy(), reseed.cpu().numpy(), weights=w.cpu().numpy(), max_iter=6)
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]) and np.array_equal(C.cpu().numpy(), ref["centroids"]), path
    assert np.array_equal(wsum.cpu().numpy(), ref["wsum"]) and int(info[0]) == ref["iters"]
    dref = oracle.kmeans_dist2(Xn, ref["centroids"])
    assert np.array_equal(d2.cpu().numpy(), dref) and np.array_equal(labels2.cpu().numpy(), dref.argmin(1))
    # the update from those labels against fp64.  Sequential fp32 sums of at most T terms and one division: |err| <= (T + 2) 2^-24 sum|w x| / W
    # (first-order summation bound), the summed weights within T 2^-24 relative; the shift is measured against the centroids handed in
    onehot = torch.nn.functional.one_hot(labels2, K).double() * w.double()[:, None]
    W = onehot.sum(0)
    live = W > 0
    mean = (onehot.t() @ X.double()) / W.clamp(min=1e-30)[:, None]
    bound = (T + 2) * 2.0 ** -24 * (onehot.t() @ X.double().abs()) / W.clamp(min=1e-30)[:, None]
    assert bool(((Cn.double() - mean).abs() <= bound)[live].all()) and bool(live.any())
    np.testing.assert_allclose(wsum2.cpu().numpy(), W.cpu().numpy(), rtol=T * 2.0 ** -24)
    np.testing.assert_allclose(shift2.cpu().numpy(), ((Cold - Cn).double() ** 2).sum(1).cpu().numpy(), rtol=1e-6)
    ar.check(f"sc_kmeans_fit / _assign / _update ({path})")


@pytest.mark.parametrize("metric", ["cos", "l2"])
@pytest.mark.parametrize("M,d,k", [(205, 1024, 8), (300, 130, 64), (1, 16, 1)])
def test_sim_topk_write_bounds(metric, M, d, k):
    """sc_sim_topk: idx [k] int32 and score [k] fp32 as arena vectors of exactly k entries (k = 64 is the limit); indices as the oracle's"""
    rng = np.random.default_rng(M * 7 + d)
    docs, q = rng.standard_normal((M, d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    k = min(k, M)
    qd, dd = torch.from_numpy(q).cuda(), torch.from_numpy(docs).cuda()
    ar = Arena("cuda")
    idx, sc = ar.flat(k, torch.int32), ar.flat(k, torch.float32)
    with frozen(qd, dd):
        _lib.check(_lib.load().sc_sim_topk(_P(qd), _P(dd), M, d, k, 0 if metric == "cos" else 1, _P(idx), _P(sc), _lib.stream_ptr("cuda:0")), "sc_sim_topk")
    ridx, rsc = oracle.topk(q, docs, k, metric)
    assert np.array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_allclose(sc.cpu().numpy(), rsc, rtol=1e-5, atol=1e-6)
    ar.check("sc_sim_topk")


def test_decode_advance_write_bounds():
    """sc_decode_advance: all seven pointers are arena views of exactly their sizes; ring[ring_index] alone changes in the ring"""
    ar = Arena("cuda")
    ring, cnt = ar.flat(8, torch.int64), ar.flat(1, torch.int64)
    tok, pos, ln, npv = (ar.flat(1, torch.int32) for _ in range(4))
    nxt = torch.tensor([4242], dtype=torch.int64, device="cuda")
    ring.zero_()
    cnt.fill_(3)
    for t, v in ((tok, 7), (pos, 100), (ln, 101), (npv, 4)):
        t.fill_(v)
    with frozen(nxt):
        ops.decode_advance(nxt, ring, cnt, tok, pos, ln, npv)
    assert ring.tolist() == [0, 0, 0, 4242, 0, 0, 0, 0] and int(cnt) == 4 and (int(tok), int(pos), int(ln), int(npv)) == (4242, 101, 102, 5)
    ar.check("sc_decode_advance")


def test_counter_uniform_write_bounds():
    """sc_counter_uniform_f32: B = 70 (two blocks of 64 threads, the second partial), u an arena vector of exactly B floats"""
    B = 70
    seeds = torch.arange(B, device="cuda", dtype=torch.int64) * 7919 - 5
    counter = torch.tensor([11], dtype=torch.int64, device="cuda")
    ar = Arena("cuda")
    u = ar.flat(B, torch.float32)
    with frozen(seeds, counter):
        ops.counter_uniform(seeds, counter, 3, out=u)
    assert u.tolist() == [np.float32(ops.counter_uniform_host(int(s), 14)) for s in seeds.tolist()]
    ar.check("sc_counter_uniform_f32")


def test_preprocess_write_bounds():
    """sc_preprocess_u8 (k_pre_chw; h w = 28 x 42 + an odd 15 x 15 image whose plane is not a multiple of the 8-pixel groups), sc_preprocess_patchify_u8
    (k_pre_patch) and sc_patchify_f16 (k_patchify_f16) with ld = 640 > 3 p^2 = 588: the pad columns are OUTPUT, defined as zeros - asserted; the
    guard is around the [rows, ld] block."""
    lib, st = _lib.load(), _lib.stream_ptr("cuda:0")
    mean, std = ops._f3(ops.CLIP_MEAN), ops._f3(ops.CLIP_STD)
    ar = Arena("cuda")
    for n, h, w in ((3, 28, 42), (2, 15, 15)):
        u8 = np.random.default_rng(h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        src = torch.from_numpy(u8).cuda()
        out = ar.flat(n * 3 * h * w, torch.float16)
        with frozen(src):
            _lib.check(lib.sc_preprocess_u8(_P(src), n, h, w, mean, std, _P(out), st), "sc_preprocess_u8")
        assert np.array_equal(out.cpu().numpy().view(np.uint16).reshape(n, 3, h, w), ref_preprocess(u8).view(np.uint16))
    n, h, w, P, ld = 3, 28, 42, 14, 640
    rows = n * (h // P) * (w // P)
    u8 = np.random.default_rng(7).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src = torch.from_numpy(u8).cuda()
    chw = torch.from_numpy(ref_preprocess(u8)).cuda().contiguous()       # (ref_preprocess returns a transposed NHWC array)
    ref = torch.nn.functional.unfold(chw.float(), kernel_size=P, stride=P).transpose(1, 2).reshape(rows, 3 * P * P).half()
    o1, o2 = ar.out(rows, ld, torch.float16, tail_rows=16), ar.out(rows, ld, torch.float16, tail_rows=16)
    with frozen(src, chw):
        _lib.check(lib.sc_preprocess_patchify_u8(_P(src), n, h, w, P, mean, std, _P(o1), ld, st), "sc_preprocess_patchify_u8")
        _lib.check(lib.sc_patchify_f16(_P(chw), n, h, w, P, _P(o2), ld, st), "sc_patchify_f16")
    for o in (o1, o2):
        assert torch.equal(_bits(o[:, :588]), _bits(ref)) and int(torch.count_nonzero(_bits(o[:, 588:]))) == 0
    ar.check("sc_preprocess_u8 / sc_preprocess_patchify_u8 / sc_patchify_f16")


def test_pool_and_avgpool_write_bounds():
    """sc_pool_f16 (k_pool: one workgroup per batch row; lengths 0, 1, L, L + 5; mean + normalisation) and sc_avgpool_tokens_f16 (k_avgpool_tokens: r = 5
    on a 24 x 24 grid drops rows / columns 20..23) into arena views of exactly [B, H] fp32 / [B, g g, D] fp16."""
    lib, st = _lib.load(), _lib.stream_ptr("cuda:0")
    B, L, H = 5, 64, 384
    hidden = _rand((B, L, H), 1)
    ln = torch.tensor([0, 1, L, L + 5, 17], dtype=torch.int32, device="cuda")
    ar = Arena("cuda")
    out = ar.out(B, H, torch.float32, tail_rows=8)
    with frozen(hidden, ln):
        _lib.check(lib.sc_pool_f16(_P(hidden), _P(ln), _P(out), B, L, H, 1, 1, st), "sc_pool_f16")
    assert torch.equal(_bits(out), _bits(ops.pool(hidden, ln, "mean", True)))
    n = ln.clamp(max=L)
    keep = (torch.arange(L, device="cuda")[None] < n[:, None]).double()[..., None]
    m = (hidden.double() * keep).sum(1) / n.clamp(min=1).double()[:, None]
    torch.testing.assert_close(out.double(), m / m.norm(dim=1, keepdim=True).clamp(min=1e-12), rtol=1e-5, atol=1e-6)
    Bp, Pg, D, r = 2, 24, 64, 5
    g = Pg // r
    x = _rand((Bp, Pg * Pg, D), 2)
    o = ar.out(Bp * g * g, D, torch.float16, tail_rows=64)
    with frozen(x):
        _lib.check(lib.sc_avgpool_tokens_f16(_P(x), _P(o), Bp, Pg, D, r, st), "sc_avgpool_tokens_f16")
    ref = torch.nn.functional.avg_pool2d(x.float().reshape(Bp, Pg, Pg, D).permute(0, 3, 1, 2), (r, r)).permute(0, 2, 3, 1).reshape(Bp * g * g, D)
    torch.testing.assert_close(o.float(), ref, rtol=1e-3, atol=1e-3)
    ar.check("sc_pool_f16 / sc_avgpool_tokens_f16")


def test_gather_rows_write_bounds():
    """sc_gather_rows_f16 / k_gather_rows with ldo = H + 8 and ids at both ends and outside the vocabulary (zero rows, still written inside the row)"""
    vocab, H = 1000, 256
    table = _rand((vocab, H), 1)
    ids = torch.tensor([0, -200, vocab - 1, vocab, 5, 2 ** 31 - 1, -1], dtype=torch.int32, device="cuda")
    ar = Arena("cuda")
    out = ar.out(ids.numel(), H, torch.float16, ld=H + 8, tail_rows=8)
    with frozen(ids, table):
        ops.gather_rows(ids, table, out=out)
    ok = (ids >= 0) & (ids < vocab)
    ref = torch.where(ok[:, None], table[ids.long().clamp(0, vocab - 1)], torch.zeros((), dtype=torch.float16, device="cuda"))
    assert torch.equal(_bits(out), _bits(ref))
    ar.check("sc_gather_rows_f16")


def test_embed_ln_write_bounds():
    """sc_vit_embed_ln_f16 (k_vit_embed_ln<4>: D = 1280, 3 x 17 = 51 rows) and sc_bert_embed_ln_f16 (k_bert_embed_ln<1>: H = 384, 9 x 11 = 99 rows):
    the last workgroup holds 3 of its 4 rows and the last vector group is partial; outputs of exactly [rows, D]."""
    N, P, D = 3, 16, 1280
    patch, cls, pos, g, b = _rand((N * P, D), 1), _rand((D,), 2), _rand((P + 1, D), 3, 0.5), _rand((D,), 4), _rand((D,), 5)
    ar = Arena("cuda")
    out = ar.out(N * (P + 1), D, torch.float16, tail_rows=8)
    with frozen(patch, cls, pos, g, b):
        ops.vit_embed_ln(patch, cls, pos, g, b, 1e-5, N, P, out=out)
    v = (torch.cat([cls.expand(N, 1, D), patch.view(N, P, D)], 1) + pos[None]).float().view(-1, D)
    torch.testing.assert_close(out.float(), torch.nn.functional.layer_norm(v, (D,), g.float(), b.float(), 1e-5), rtol=2e-3, atol=2e-3)
    B, L, H, vocab = 9, 11, 384, 500
    word, pe, t0, g, b = _rand((vocab, H), 6), _rand((L, H), 7, 0.5), _rand((H,), 8, 0.5), _rand((H,), 9), _rand((H,), 10)
    ids = torch.randint(0, vocab, (B, L), device="cuda", generator=_gen(11), dtype=torch.int32)
    ids[0, 0], ids[8, 10] = -7, vocab + 3
    out2 = ar.out(B * L, H, torch.float16, tail_rows=8)
    with frozen(ids, word, pe, t0, g, b):
        ops.bert_embed_ln(ids, word, pe, t0, g, b, 1e-12, out=out2)
    v = word[ids.long().clamp(0, vocab - 1).view(-1)].float() + t0.float() + pe.float().repeat(B, 1)
    torch.testing.assert_close(out2.float(), torch.nn.functional.layer_norm(v, (H,), g.float(), b.float(), 1e-12), rtol=2e-3, atol=2e-3)
    ar.check("sc_vit_embed_ln_f16 / sc_bert_embed_ln_f16")
