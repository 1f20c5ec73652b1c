"""GPU: the GEMM / GEMV entry points against fp64 on EXACT inputs (tests/_exact.py): no measured tolerance.

Operands sit on a power-of-two grid on which every product, every partial sum in any order, the bias add and the residual add are exact in
fp32.  SC_EPI_NONE and the headed epilogues must therefore give the fp64 result rounded ONCE to fp16 - whatever the MFMA order, K split, tile
walk or wave merge - and the activation epilogues must stay within half an fp16 ulp plus the derived fp32 term `tau` of the fp64 value.
tests/test_exact_power.py shows on the CPU which wrong kernels this rejects that the 2e-3 comparisons accept (tests/GEMM_EXACT_POWER.md).

Cases are named by the kernel launch_gemm (gemm.hip) / sc_gemv_f16 (gemv.hip) selects; every test first asserts the selecting precondition
through a restatement of the dispatcher (`_gemm_kernel`, `_gemv_kernel`), so a dispatcher change cannot silently move a case.  A is the first
M rows of a larger NaN buffer (the row-map cases put NaN into the skipped rows); A, the residual and C are padded views (lda = K + 8,
ldr = N + 8, ldc = N + 8) unless the case needs otherwise.  The sign of a zero is not pinned (+0 == -0)."""
import functools
import os

import pytest
import torch

from streamchat_amd import ops
from tests import _exact as X

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def _case(kernel, M, N, K, epi="none", bias="aligned", res=False, f32=False, a_rows=None, dr=None, stream64=False, ldr_pad=8):
    tag = [kernel, f"M{M}", f"N{N}", f"K{K}", epi]
    tag += [t for t, on in (("nobias", bias is None), ("bias8", bias == "odd"), ("res", res), ("f32", f32), ("rows%d" % (a_rows or (0,))[0], a_rows),
                            ("ldr+4", ldr_pad == 4), ("cu64", stream64)) if on]
    return "-".join(tag), dict(kernel=kernel, M=M, N=N, K=K, epi=epi, bias=bias, res=res, f32=f32, a_rows=a_rows, dr=dr, stream64=stream64, ldr_pad=ldr_pad)


def _gemm_cases():
    c = []
    # k_gemm_skinny: M <= 32 with gelu / quick_gelu, or a bias at an 8-byte offset
    for M in (1, 16, 17, 32):
        for N, K in ((128, 128), (256, 384)):
            c.append(_case("skinny", M, N, K, "gelu", res=True))
            c.append(_case("skinny", M, N, K, "quick_gelu", bias=None if M == 16 else "aligned"))
        c.append(_case("skinny", M, 256, 2048, bias="odd", f32=M in (16, 32), res=M in (17, 32)))
    c.append(_case("skinny", 17, 128, 128, "quick_gelu", f32=True))
    # k_gemm_skinny_l: none / swiglu, K % 512 == 0, K >= 2048, fewer than 2 x CUs strips; M = 16: MG 1, PD 4; M = 17, 32: MG 2, PD 3
    for M in (16, 17, 32):
        for K in (2048, 2560, 3584):
            c.append(_case("skinny_l", M, 128, K, res=True))
            c.append(_case("skinny_l", M, 128, K, "swiglu", bias=None if K == 2560 else "aligned"))
            c.append(_case("skinny_l", M, 128, K, f32=True))
    c.append(_case("skinny_l", 16, 4224, 2048, res=True))                  # 264 strips > 256 CUs: one strip per workgroup + a remainder
    c.append(_case("skinny_l", 32, 4224, 3584, "swiglu"))
    c.append(_case("skinny_l", 17, 4224, 2560, f32=True))
    # k_gemm_skinny_lx: K = 3584, 520 strips
    for M in (16, 32):
        c.append(_case("skinny_lx", M, 8320, 3584, res=M == 32))
        c.append(_case("skinny_lx", M, 8320, 3584, "swiglu", bias=None))
    # k_gemm128
    for M in (33, 127, 128, 129):
        for N, K in ((128, 64), (384, 192)):
            c.append(_case("gemm128", M, N, K, res=True))
            c.append(_case("gemm128", M, N, K, bias=None))
            c.append(_case("gemm128", M, N, K, "quick_gelu"))
            c.append(_case("gemm128", M, N, K, "gelu", res=True))
            c.append(_case("gemm128", M, N, K, "swiglu"))
            c.append(_case("gemm128", M, N, K, f32=True, res=True))
            c.append(_case("gemm128", M, N, K, "quick_gelu", f32=True))
            c.append(_case("gemm128", M, N, K, a_rows=(3, 5, 1)))
    # k_gemm256 (dispatch_rows = 1024): each reason the dispatcher sends a call here; K = 64, 192, 320 are K % 128 != 0 by themselves,
    # K = 256 makes the other four reasons the only one
    for M in (33, 256, 257):
        for K in (64, 192, 320):
            c.append(_case("gemm256", M, 256, K, dr=1024, res=True))
            c.append(_case("gemm256", M, 256, K, dr=1024, f32=True))
            c.append(_case("gemm256", M, 256, K, dr=1024, a_rows=(576, 577, 1)))
            c.append(_case("gemm256", M, 256, K, dr=1024, bias="odd"))
            c.append(_case("gemm256", M, 256, K, "gelu", dr=1024, res=True, ldr_pad=4))
    c.append(_case("gemm256", 257, 256, 256, dr=1024, f32=True, res=True))
    c.append(_case("gemm256", 257, 256, 256, dr=1024, a_rows=(576, 577, 1)))
    c.append(_case("gemm256", 257, 256, 256, dr=1024, bias="odd"))
    c.append(_case("gemm256", 257, 256, 256, "quick_gelu", dr=1024, res=True, ldr_pad=4))
    c.append(_case("gemm256", 1154, 256, 64, a_rows=(576, 577, 1)))         # two row groups: the group stride is used
    # k_gemm_fat, one tile per workgroup (dispatch_rows = 1024); with and without a residual: both epilogue bodies
    for M in (1, 255, 256, 257):
        for K in (128, 256, 384, 1024):
            for epi in ("none", "quick_gelu", "gelu"):
                c.append(_case("fat", M, 512, K, epi, dr=1024))
                c.append(_case("fat", M, 512, K, epi, dr=1024, res=True))
            c.append(_case("fat", M, 512, K, "swiglu", dr=1024))
    # k_gemm_fat, persistent: 70 tiles on the 64-CU stream, 272 tiles on the default stream
    c.append(_case("fat_persistent", 2305, 1792, 128, res=True, stream64=True))
    c.append(_case("fat_persistent", 4099, 4096, 128, res=True))
    return dict(c)


GEMM_CASES = _gemm_cases()


def _kinds(epi):
    return X.KINDS if epi != "none" else ("wide", "small")


GEMM_PARAMS = [(name, kind) for name, kw in GEMM_CASES.items() for kind in _kinds(kw["epi"])]

HEADED_CASES = {}
for _mode, _lead in (("rope", None), ("rope", "half"), ("colscale", 256)):
    for _M, _K, _pos0 in ((257, 128, 0), (1154, 128, 777), (257, 256, 777), (1154, 256, 0)):
        _N = 512
        _l = _N if _lead is None else (_N // 2 if _lead == "half" else _lead)
        HEADED_CASES[f"fat-{_mode}-lead{_l}-M{_M}-K{_K}-pos{_pos0}"] = dict(mode=_mode, M=_M, N=_N, K=_K, pos0=_pos0, lead=_l)
    _l = 1792 if _lead is None else (896 if _lead == "half" else _lead)
    HEADED_CASES[f"fat_persistent-{_mode}-lead{_l}-M2305-K128-pos5"] = dict(mode=_mode, M=2305, N=1792, K=128, pos0=5, lead=_l)

GEMV_CASES = {}
for _N, _K, _kern in ((130, 264, "gemv"), (37, 1040, "gemv"), (50, 3584, "gemv_u"), (3584, 3584, "gemv_u"), (50, 18944, "gemv_u")):
    GEMV_CASES[f"{_kern}-N{_N}-K{_K}-plain"] = dict(N=_N, K=_K, kernel=_kern)
    GEMV_CASES[f"{_kern}-N{_N}-K{_K}-bias-res"] = dict(N=_N, K=_K, kernel=_kern, bias=True, res=True)
    # fp32 output at K = 18944 and every y_row call take the generic kernel (gemv.hip)
    GEMV_CASES[f"{'gemv' if _K == 18944 else _kern}-N{_N}-K{_K}-bias-res-f32"] = dict(N=_N, K=_K, kernel="gemv" if _K == 18944 else _kern, bias=True, res=True, f32=True)
    GEMV_CASES[f"gemv-N{_N}-K{_K}-bias-y_row"] = dict(N=_N, K=_K, kernel="gemv", bias=True, y_row=True)
GEMV_CASES["gemv-N132-K264-swiglu"] = dict(N=132, K=264, kernel="gemv", epi="swiglu")
GEMV_CASES["gemv_u-N3584-K3584-swiglu"] = dict(N=3584, K=3584, kernel="gemv_u", epi="swiglu")
GEMV_PARAMS = [(name, kind) for name, kw in GEMV_CASES.items() for kind in _kinds(kw.get("epi", "none"))]


def seed_of(M, N, K):
    return (M * 1000003 + N * 101 + K) % (2 ** 31)


def act_inputs():
    """(M, N, K, epilogue, residual?) of every `act` input of this file (tests/test_exact_power.py measures the CPU fp32 share of tau on them)"""
    seen = {(kw["M"], kw["N"], kw["K"], kw["epi"], kw["res"]) for kw in GEMM_CASES.values() if kw["epi"] != "none"}
    seen |= {(1, kw["N"], kw["K"], "swiglu", False) for kw in GEMV_CASES.values() if kw.get("epi") == "swiglu"}
    return sorted(seen)


def exact_ks():
    """{(K, kind)} over every case of this file (headed and decode cases: K = 128, 256, wide and small)"""
    ks = {(kw["K"], kind) for name, kind in GEMM_PARAMS for kw in (GEMM_CASES[name],)}
    ks |= {(GEMV_CASES[name]["K"], kind) for name, kind in GEMV_PARAMS}
    ks |= {(K, kind) for K in (128, 256) for kind in ("wide", "small")}
    return sorted(ks)


# ------------------------------------------------------------------------------------------------
# the dispatchers, restated (gemm.hip launch_gemm / launch_fat, gemv.hip sc_gemv_f16)
# ------------------------------------------------------------------------------------------------
def _gemm_kernel(M, Md, N, K, epi, f32, a_rows, lda, ldc, ldr, pa, pw, pb, pr, pc, cus, dev_cus):
    al = lambda p, n: p is None or p % n == 0
    if Md <= 32 and K % 128 == 0 and a_rows is None and ldc % 4 == 0 and (pr is None or ldr % 4 == 0):
        if epi in ("none", "swiglu") and os.environ.get("SC_SKINNY_GENERIC", "")[:1] != "1" and all(al(p, 16) for p in (pa, pw, pr, pb)) \
                and lda % 8 == 0 and (pr is None or ldr % 8 == 0):
            if N // 16 < 2 * dev_cus and K % 512 == 0 and K >= 2048:
                return "skinny_l"
            if K == 3584:
                return "skinny_lx"
        return "skinny"
    wide_ok = f32 or (ldc % 8 == 0 and pc % 16 == 0)
    if Md >= 1024 and wide_ok and N % 256 == 0 and K % 32 == 0:
        if not f32 and a_rows is None and K % 128 == 0 and lda * 512 < 2 ** 31 and lda % 8 == 0 and al(pa, 16) and al(pw, 16) and al(pb, 16) \
                and (pr is None or (ldr % 8 == 0 and pr % 16 == 0)):
            return "fat_persistent" if -(-M // 256) * (N // 256) > cus else "fat"
        return "gemm256"
    return "gemm128"


def _gemv_kernel(N, K, epi, f32, y_row, rms):
    few = N < 16384 and epi != "swiglu"
    knobs = ("SC_GEMV_WPB_0", "SC_GEMV_WPB_1", "SC_GEMV_WPB_2", "SC_GEMV_WPB_3", "SC_GEMV_RPW_FEW")
    special = os.environ.get("SC_GEMV_GENERIC", "")[:1] != "1" and not any(k in os.environ for k in knobs)
    return "gemv_u" if not y_row and special and (K == 3584 or (K == 18944 and few and not f32 and not rms)) else "gemv"


# ------------------------------------------------------------------------------------------------
# operands and references (fp64 on the CPU, computed once per shape and kind)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _fam(M, N, K, kind, bits=23):
    a, w, b, r = X.family(M, N, K, kind, seed_of(M, N, K), bits)
    return a, w, b, r, a @ w.t()


def _dev_a(a, a_rows, pad=8):
    """A as the kernel gets it: rows of a NaN buffer with lda = K + pad, three further NaN rows behind; under a row map the skipped rows are NaN"""
    M, K = a.shape
    idx = X.a_row_index(M, a_rows)
    buf = torch.full((X.a_store_rows(M, a_rows) + 3, K + pad), NAN, dtype=torch.float16)
    buf[idx, :K] = a.half()
    return buf.cuda()[:, :K]


def _dev_padded(t, pad, dtype=torch.float16):
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=dtype)
    buf[:, :t.shape[1]] = t.to(dtype)
    return buf.cuda()[:, :t.shape[1]]


def _dev_bias(b, how):
    if how is None:
        return None
    if how == "odd":                                               # 8-byte aligned only
        buf = torch.full((b.numel() + 4,), NAN, dtype=torch.float16)
        buf[4:] = b.half()
        return buf.cuda()[4:]
    return b.half().cuda()


def _out(M, cols, dtype, pad=8):
    return torch.full((M + 3, cols + pad), NAN, dtype=dtype, device="cuda")[:M, :cols]


def _report(what, bad, out, ref):
    n = int(bad.sum())
    if n:
        i = bad.nonzero()[0].tolist()
        pytest.fail(f"{what}: {n} of {bad.numel()} elements differ; first at {i}: got {out[tuple(i)].item()!r}, want {ref[tuple(i)].item()!r}")


def _check(what, out, z64, res64, epi, f32):
    """out against the oracle: bit-exact for `none`, half an ulp + tau for the activations (fp32 output: tau + the output's own fp32 rounding)"""
    out = out.cpu()
    act = X.ACT[epi](z64)
    y = act if res64 is None else act + res64
    if epi == "none":
        ref = y.float() if f32 else X.rne16(y)
        assert torch.equal(y.float().double(), y)
        return _report(what, X.differing(out, ref), out, ref)
    tau = X.tau_swiglu(y, z64) if epi == "swiglu" else X.tau_act(act, z64, None if res64 is None else y)
    if f32:
        bad = ~((out.double() - y).abs() <= tau + 2.0 ** -24 * y.abs())
    else:
        bad = X.half_ulp_excess(out, y, tau)
    _report(what, bad, out, y)


# ------------------------------------------------------------------------------------------------
# sc_gemm_f16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", GEMM_PARAMS)
def test_gemm_exact(case, kind):
    """sc_gemm_f16: `none` (with and without bias / residual, fp16 and fp32 output, the A row map) bit-exact against fp64 rounded once;
    QuickGELU, erf-GELU and SwiGLU within half an fp16 ulp + tau of the fp64 value.  One case per dispatch branch and tile edge:
    k_gemm_skinny M = 1, 16, 17, 32; k_gemm_skinny_l M = 16 (MG 1, PD 4), 17 and 32 (MG 2, PD 3), K = 2048, 2560, 3584, 8 and 264 strips (more than
    the CU count); k_gemm_skinny_lx 520 strips; k_gemm128 M = 33 .. 129; k_gemm256 and one-tile-per-workgroup k_gemm_fat at small M through
    dispatch_rows = 1024; the persistent k_gemm_fat walk (70 tiles on the 64-CU stream, 272 on the default stream)."""
    kw = GEMM_CASES[case]
    M, N, K, epi, f32, a_rows = kw["M"], kw["N"], kw["K"], kw["epi"], kw["f32"], kw["a_rows"]
    a64, w64, b64, r64, acc64 = _fam(M, N, K, kind)
    a, w, b = _dev_a(a64, a_rows), w64.half().cuda(), _dev_bias(b64, kw["bias"])
    r = _dev_padded(r64, kw["ldr_pad"]) if kw["res"] else None
    ncol = N // 2 if epi == "swiglu" else N
    out = _out(M, ncol, torch.float32 if f32 else torch.float16)
    stream = ops.masked_stream(0, 64) if kw["stream64"] else None
    dev_cus = ops.device_info()["cu_count"]
    ptr = lambda t: None if t is None else t.data_ptr()
    picked = _gemm_kernel(M, kw["dr"] or M, N, K, epi, f32, a_rows, a.stride(0), out.stride(0), r.stride(0) if kw["res"] else 0, ptr(a), ptr(w), ptr(b), ptr(r),
                          ptr(out), 64 if kw["stream64"] else dev_cus, dev_cus)
    assert picked == kw["kernel"] == case.split("-")[0], (case, picked)
    if kw["kernel"] == "skinny_l" and N == 4224:
        assert N // 16 > dev_cus                                      # one strip per workgroup plus a remainder
    torch.cuda.synchronize()
    if stream is None:
        ops.gemm(a, w, b, r, epi, out=out, a_rows=a_rows, M=M, dispatch_rows=kw["dr"])
    else:
        with torch.cuda.stream(stream):
            ops.gemm(a, w, b, r, epi, out=out, a_rows=a_rows, M=M, dispatch_rows=kw["dr"])
            stream.synchronize()
    torch.cuda.synchronize()
    z64 = acc64 if kw["bias"] is None else acc64 + b64
    _check(f"sc_gemm_f16 {case} {kind}", out, z64, r64 if kw["res"] else None, epi, f32)


# ------------------------------------------------------------------------------------------------
# sc_gemm_headed_f16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("wide", "small"))
@pytest.mark.parametrize("case", list(HEADED_CASES))
def test_gemm_headed_exact(case, kind):
    """sc_gemm_headed_f16 (k_gemm_fat only) on the 64-CU stream, bit-exact: rotary with lead_cols = N (the SC_EPI_ROPE_ALL instantiation), with
    lead_cols = N / 2 (the V columns stay plain), column scale 0.375 below column 256.  The table is the test's own: dyadic "cos" / "sin"
    (multiples of 2^-3 within +-1; the kernel only reads it), so with a 2^20 operand budget the rotated sums stay exact in fp32 and the oracle
    is independent of every rotary kernel of the library.  M = 257, 1154 (ragged last row tile), pos0 = 0, 777; 2305 x 1792 is the persistent
    walk (70 tiles on 64 workgroups)."""
    kw = HEADED_CASES[case]
    M, N, K, mode, lead, pos0 = kw["M"], kw["N"], kw["K"], kw["mode"], kw["lead"], kw["pos0"]
    a64, w64, b64, _, acc64 = _fam(M, N, K, kind, 20)
    a, w, b = _dev_a(a64, None)[:M], w64.half().cuda(), b64.half().cuda()      # (gemm_headed takes M from the view: the NaN rows stay behind it)
    out = _out(M, N, torch.float16)
    assert ops.gemm_headed_ok(N, K, a, w, b, out)
    assert case.split("-")[0] == ("fat_persistent" if -(-M // 256) * (N // 256) > 64 else "fat")
    z64 = acc64 + b64
    s = ops.masked_stream(0, 64)
    torch.cuda.synchronize()
    if mode == "rope":
        tab = X.dyadic_table(pos0 + M + 2, 64, seed_of(M, N, K) + pos0)
        tab_d = tab.cuda()
        with torch.cuda.stream(s):
            ops.gemm_headed(a, w, b, out, "rope", lead, tab_d, pos0)
            s.synchronize()
        y = X.rope(z64, tab, pos0, lead)
    else:
        with torch.cuda.stream(s):
            ops.gemm_headed(a, w, b, out, "colscale", lead, col_scale=0.375)
            s.synchronize()
        y = X.colscale(z64, 0.375, lead)
    torch.cuda.synchronize()
    out, ref = out.cpu(), X.rne16(y)
    _report(f"sc_gemm_headed_f16 {case} {kind}", X.differing(out, ref), out, ref)


# ------------------------------------------------------------------------------------------------
# sc_gemv_f16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", GEMV_PARAMS)
def test_gemv_exact(case, kind):
    """sc_gemv_f16: `none` bit-exact (plain, bias + residual, fp32 output, the y_row device-row append into a [12, N + 64] cache of which only
    row 5 may change), SwiGLU within half an ulp + tau.  Generic k_gemv: (N, K) = (130, 264), (37, 1040) - N no multiple of the rows per
    workgroup, K no multiple of the 512-element slices; straight-line k_gemv_u: K = 3584 (N = 50 and 3584) and K = 18944 (N = 50).  The rms_gamma
    path is not exact and stays with tests/test_gpu_gemv_spec.py."""
    kw = GEMV_CASES[case]
    N, K, epi, f32 = kw["N"], kw["K"], kw.get("epi", "none"), kw.get("f32", False)
    assert _gemv_kernel(N, K, epi, f32, kw.get("y_row", False), False) == kw["kernel"] == case.split("-")[0]
    x64, w64, b64, r64, acc64 = _fam(1, N, K, kind)
    w, x = w64.half().cuda(), x64.half().cuda().view(-1)
    b = b64.half().cuda() if kw.get("bias") else None
    r = r64.half().cuda().view(-1) if kw.get("res") else None
    z64 = acc64 + b64 if kw.get("bias") else acc64
    what = f"sc_gemv_f16 {case} {kind}"
    if kw.get("y_row"):
        cache = torch.full((12, N + 64), 7.0, dtype=torch.float16, device="cuda")
        row = torch.tensor([5], dtype=torch.int32, device="cuda")
        ops.gemv(w, x, b, r, out=cache, out_row=row)
        torch.cuda.synchronize()
        want = torch.full((12, N + 64), 7.0, dtype=torch.float16)
        want[5, :N] = X.rne16(z64)[0]
        got = cache.cpu()
        return _report(what, X.differing(got, want), got, want)
    out = torch.full((N // 2 if epi == "swiglu" else N,), NAN, dtype=torch.float32 if f32 else torch.float16, device="cuda")
    ops.gemv(w, x, b, r, epi, out=out)
    torch.cuda.synchronize()
    _check(what, out.view(1, -1), z64, r64 if kw.get("res") else None, epi, f32)


# ------------------------------------------------------------------------------------------------
# sc_decode_qkv_tab_f16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("wide", "small"))
@pytest.mark.parametrize("Dh", (64, 128))
def test_decode_qkv_tab_exact(Dh, kind):
    """sc_decode_qkv_tab_f16, the generic k_decode_qkv without a norm (K = 256 != 3584, rms_gamma NULL), Hq = 4, Hkv = 2: q = rope(Wq x + bq) with
    the query table, K | V = rope(Wk x + bk) | Wv x + bv with the key table into row pos[0] = 23 of a [40, 2 Hkv Dh + 64] cache whose other
    rows must keep their contents.  Two different dyadic tables, 2^20 operand budget: bit-exact against fp64."""
    Hq, Hkv, K, pos, cap = 4, 2, 256, 23, 40
    dq, dkv = Hq * Dh, Hkv * Dh
    assert K != 3584                                                  # the generic kernel
    x64, w64, b64, _, acc64 = _fam(1, dq + 2 * dkv, K, kind, 20)
    z64 = acc64 + b64
    tq, tk = X.dyadic_table(64, Dh // 2, 11 + Dh), X.dyadic_table(64, Dh // 2, 12 + Dh)
    w, bias, x = w64.half().cuda(), b64.half().cuda(), x64.half().cuda().view(-1)
    q_out = torch.full((dq,), NAN, dtype=torch.float16, device="cuda")
    cache = torch.full((cap, 2 * dkv + 64), 7.0, dtype=torch.float16, device="cuda")
    row = torch.tensor([pos], dtype=torch.int32, device="cuda")
    ops.decode_qkv_tab(w[:dq].contiguous(), w[dq:].contiguous(), bias[:dq].contiguous(), bias[dq:].contiguous(), x, None, 1e-6, q_out, cache, row,
                       Hq, Hkv, Dh, tq.cuda(), tk.cuda())
    torch.cuda.synchronize()
    q_ref = X.rne16(X.rope(z64[:, :dq], tq, pos, dq, Dh))[0]
    want = torch.full((cap, 2 * dkv + 64), 7.0, dtype=torch.float16)
    want[pos, :2 * dkv] = X.rne16(X.rope(z64[:, dq:], tk, pos, dkv, Dh))[0]
    got_q, got_c = q_out.cpu(), cache.cpu()
    _report(f"sc_decode_qkv_tab_f16 q Dh {Dh} {kind}", X.differing(got_q, q_ref), got_q, q_ref)
    _report(f"sc_decode_qkv_tab_f16 k|v Dh {Dh} {kind}", X.differing(got_c, want), got_c, want)
