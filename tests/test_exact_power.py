"""Host: what the exact-input GEMM / GEMV tests (tests/test_gpu_gemm_exact.py) can tell apart, shown on the CPU in fp64.

(a) the construction of tests/_exact.py holds on every (K, kind) the GPU file uses: fp32 sums in forward, reversed, 64- and 512-chunked order
    plus the bias and residual adds equal fp64 (and an int64 matmul of the integer generators) exactly; the fp16 rounding is a real one on at
    least 30 % of the `wide` / `act` outputs; `small` has 0.5 - 20 % nonzero fp16-subnormal outputs; `act` has at least half of z inside |z| < 4
    and some beyond |z| > 6.  (`small` itself cannot reach 30 % roundings: its outputs are multiples of 2^-20 that straddle 2^-14, and a
    multiple of 2^-20 below 2^-9 is an fp16 number - at K = 64 no sum of 64 products of at most 2^-12 gets there often.  Its share is
    reported in the document, the bound is asserted on `wide` and `act`.)
(b) wrong kernels restated in fp64: each is rejected (at least 16 differing / flagged elements) by the new criterion on every case on which it
    can differ (its unrounded value differs from the true one on at least 32 elements - for truncation: 32 outputs need a rounding; for a
    wrong activation: 32 outputs more than an ulp off).
(c) the CPU fp32 evaluation of the activations uses at most half of `tau` on every `act` input of the GPU file.
`python -m tests.test_exact_power` rewrites tests/GEMM_EXACT_POWER.md."""
import functools
import math
import os

import pytest
import torch

from tests import _exact as X
from tests.test_gpu_gemm_exact import act_inputs, exact_ks, seed_of

M, N, LEAD, POS0, A_ROWS, CSCALE = 32, 256, 128, 7, (3, 5, 1), 0.375
CAN, REJECT = 32, 16
KS = exact_ks()


def _to16(x64):
    return x64.float().half()


def _trunc16(x64):
    """fp64 -> fp16 toward zero"""
    h = _to16(x64)
    bits = h.view(torch.int16).to(torch.int32)
    over = h.double().abs() > x64.abs()
    return torch.where(over, ((bits & 0x8000) | ((bits & 0x7FFF) - 1)), bits).to(torch.int16).view(torch.float16)


def _ulp(y64):
    _, e = torch.frexp(y64)
    return torch.pow(2.0, (torch.where(y64 == 0, torch.full_like(e, -14), e - 1).clamp(min=-14) - 10).double())


@functools.lru_cache(maxsize=None)
def setup(K, kind):
    rows = X.a_store_rows(M, A_ROWS)
    s = seed_of(rows, N, K)
    a, w, b, r = X.family(rows, N, K, kind, s)
    ah, wh, bh, _ = X.family(M, N, K, kind, s + 1, 20)                # the headed budget
    return dict(K=K, kind=kind, a_store=a, a=a[:M], w=w, b=b, r=r[:M], ah=ah, wh=wh, bh=bh, tab=X.dyadic_table(POS0 + M + 2, 64, s),
                ints=X.family_ints(rows, N, K, kind, s))


def _truth(S, group):
    a, w, b, r = S["a"], S["w"], S["b"], S["r"]
    z = a @ w.t() + b
    if group == "none":
        return z + r, None
    if group == "rows":
        return S["a_store"][X.a_row_index(M, A_ROWS)] @ w.t() + b + r, None
    zh = S["ah"] @ S["wh"].t() + S["bh"]
    if group == "rope":
        return X.rope(zh, S["tab"], POS0, LEAD), None
    if group == "colscale":
        return X.colscale(zh, CSCALE, LEAD), None
    y = X.ACT[group](z)
    return y, (X.tau_swiglu(y, z) if group == "swiglu" else X.tau_act(y, z))


def _chunked(c):
    def f(S):
        a, w, K = S["a"], S["w"], S["K"]
        step = K // 4 if c == "K/4" else c
        acc = sum(_to16(a[:, k:k + step] @ w[:, k:k + step].t()).double() for k in range(0, K, step))
        return acc + S["b"] + S["r"]
    return f


def _res_ldr(S):
    pad = torch.zeros((M, N + 8), dtype=torch.float64)
    pad[:, :N] = S["r"]
    return S["a"] @ S["w"].t() + S["b"] + pad.reshape(-1)[:M * N].reshape(M, N)


def _tanh_gelu(S):
    z = S["a"] @ S["w"].t() + S["b"]
    return 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))


def _quick_17(S):
    z = S["a"] @ S["w"].t() + S["b"]
    return z / (1 + torch.exp(-1.7 * z))


def _swiglu_gugu(S):
    q = (S["a"] @ S["w"].t() + S["b"]).reshape(M, N // 4, 4)
    return torch.stack([X.silu(q[..., 0]) * q[..., 1], X.silu(q[..., 2]) * q[..., 3]], -1).reshape(M, N // 2)


def _rope_sign(S):
    zh = S["ah"] @ S["wh"].t() + S["bh"]
    t = S["tab"][POS0:POS0 + M].double()
    cos, sin = t[:, None, 0], t[:, None, 1]
    x = zh[:, :LEAD].reshape(M, LEAD // 128, 128)
    x1, x2 = x[..., :64], x[..., 64:]
    return torch.cat([torch.cat([x1 * cos - x2 * sin, x2 * cos - x1 * sin], -1).reshape(M, LEAD), zh[:, LEAD:]], 1)


def _headed(f):
    return lambda S: f(S["ah"] @ S["wh"].t() + S["bh"], S)


# name -> (group: which oracle is the truth, unrounded fp64 value of the wrong kernel, its fp16 conversion)
MUTANTS = {
    "fp16 partials per 64": ("none", _chunked(64), _to16),
    "fp16 partials per 512": ("none", _chunked(512), _to16),
    "fp16 partials per K/4": ("none", _chunked("K/4"), _to16),
    "rounded before the residual": ("none", lambda S: _to16(S["a"] @ S["w"].t() + S["b"]).double() + S["r"], _to16),
    "truncation": ("none", lambda S: S["a"] @ S["w"].t() + S["b"] + S["r"], _trunc16),
    "flush below 2^-14": ("none", lambda S: (lambda y: torch.where(y.abs() < 2.0 ** -14, torch.zeros_like(y), y))(S["a"] @ S["w"].t() + S["b"] + S["r"]), _to16),
    "last 64 of K dropped": ("none", lambda S: S["a"][:, :S["K"] - 64] @ S["w"][:, :S["K"] - 64].t() + S["b"] + S["r"], _to16),
    "bias of column n + 1": ("none", lambda S: S["a"] @ S["w"].t() + S["b"].roll(-1) + S["r"], _to16),
    "residual with ldr = N": ("none", _res_ldr, _to16),
    "tanh-GELU": ("gelu", _tanh_gelu, _to16),
    "QuickGELU 1.7": ("quick_gelu", _quick_17, _to16),
    "SwiGLU quads (g0, u0, g1, u1)": ("swiglu", _swiglu_gugu, _to16),
    "rotary sign of the second half": ("rope", _rope_sign, _to16),
    "table row pos0 + m + 1": ("rope", _headed(lambda z, S: X.rope(z, S["tab"], POS0 + 1, LEAD)), _to16),
    "column scale on the plain columns": ("colscale", _headed(lambda z, S: z * CSCALE), _to16),
    "a_rows offset ignored": ("rows", lambda S: S["a_store"][X.a_row_index(M, (A_ROWS[0], A_ROWS[1], 0))] @ S["w"].t() + S["b"] + S["r"], _to16),
}


GROSS = ("rotary sign of the second half", "table row pos0 + m + 1", "a_rows offset ignored")


@functools.lru_cache(maxsize=None)
def judge(name, K, kind):
    """(can: elements on which the wrong kernel's value can differ, rejected: elements the new criterion flags, old: True if
    assert_close(rtol = atol = 2e-3) against the fp32 reference would have passed it)"""
    group, wrong, conv = MUTANTS[name]
    S = setup(K, kind)
    y, tau = _truth(S, group)
    m64 = wrong(S)
    out = conv(m64)
    if tau is None:
        can = int((X.rne16(y).double() != y).sum()) if conv is _trunc16 else int((m64 != y).sum())
        rejected = int(X.differing(out, X.rne16(y)).sum())
    else:
        can = int(((m64 - y).abs() > _ulp(y)).sum())
        rejected = int(X.half_ulp_excess(out, y, tau).sum())
    ref = y.float()
    old = bool(((out.float() - ref).abs() <= 2e-3 + 2e-3 * ref.abs()).all())
    return can, rejected, old, y.numel()


# ------------------------------------------------------------------------------------------------
# (a) the construction
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def construction(K, kind):
    S = setup(K, kind)
    a, w, b, r = S["a"], S["w"], S["b"], S["r"]
    z = a @ w.t() + b
    y = z + r
    a32, w32, b32, r32 = a.float(), w.float(), b.float(), r.float()
    orders = {}
    for name, ks in (("forward", range(K)), ("reversed", range(K - 1, -1, -1))):
        acc = torch.zeros((8, N), dtype=torch.float32)               # (8 rows: a loop over single k)
        for k in ks:
            acc = acc + a32[:8, k, None] * w32[None, :, k]
        orders[name] = bool(torch.equal(((acc + b32) + r32[:8]).double(), y[:8]))
    for c in (64, 512):
        acc = torch.zeros((M, N), dtype=torch.float32)
        for k in range(0, K, c):
            acc = acc + a32[:, k:k + c] @ w32[:, k:k + c].t()
        orders[f"{c}-chunked"] = bool(torch.equal(((acc + b32) + r32).double(), y))
    f = S["ints"]
    yi = f["ia"][:M] @ f["iw"].t() + f["ib"] + f["ir"][:M]
    orders["int64"] = bool(torch.equal(yi.double() * (f["sa"] * f["sw"]), y)) and int(yi.abs().max()) < 2 ** 23
    zn = a @ w.t()                                                   # the bias-free sum is what SwiGLU / the plain cases see
    return dict(orders=orders, rounded=X.unrounded_share(y), rounded_plain=X.unrounded_share(zn),
                subnormal=float(((y.abs() < 2.0 ** -14) & (y != 0)).double().mean()), subnormal_plain=float(((zn.abs() < 2.0 ** -14) & (zn != 0)).double().mean()),
                below4=float((z.abs() < 4).double().mean()), beyond6=float((z.abs() > 6).double().mean()))


@pytest.mark.parametrize("K,kind", KS)
def test_construction_is_exact(K, kind):
    c = construction(K, kind)
    assert all(c["orders"].values()), c["orders"]
    if kind == "small":
        assert 0.005 <= c["subnormal"] <= 0.20 and 0.005 <= c["subnormal_plain"] <= 0.20, c
    else:
        assert c["rounded"] >= 0.30 and c["rounded_plain"] >= 0.30, c
    if kind == "act":
        assert c["below4"] >= 0.5 and c["beyond6"] > 0, c


def test_oracle_helpers():
    """rne16 refuses a value that would be rounded twice; the half-ulp criterion counts every element, NaN and inf included; truncation"""
    with pytest.raises(AssertionError):
        X.rne16(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    y = torch.tensor([1.0 + 2.0 ** -11, 3e-8, 0.0, 100.0], dtype=torch.float64)
    assert X.within_half_ulp(y.float().half(), y, torch.zeros(4, dtype=torch.float64))
    bad = X.half_ulp_excess(torch.tensor([1.0 + 2.0 ** -9, 2.0 ** -24, float("nan"), float("inf")]).half(), y, torch.zeros(4, dtype=torch.float64))
    assert bad.tolist() == [True, False, True, True]
    assert X.half_ulp_excess(torch.zeros(1).half(), y[1:2], torch.zeros(1, dtype=torch.float64)).tolist() == [True]      # 3e-8 is more than half of 2^-24
    t = _trunc16(torch.tensor([1.0 + 2.0 ** -10 - 2.0 ** -20, -(1.0 + 2.0 ** -10 - 2.0 ** -20), 0.5], dtype=torch.float64))
    assert t.tolist() == [1.0, -1.0, 0.5]
    assert bool(X.differing(torch.tensor([float("nan"), 0.0]), torch.tensor([float("nan"), -0.0])).tolist() == [True, False])


def test_gpu_file_check_rejects_a_wrong_output():
    """the comparison the GPU tests run (`_check` of tests/test_gpu_gemm_exact.py) passes the right outputs and fails a truncated one, a wrong
    activation and an output with one NaN"""
    from tests.test_gpu_gemm_exact import _check
    S = setup(256, "wide")
    z, r = S["a"] @ S["w"].t() + S["b"], S["r"]
    _check("none", X.rne16(z + r), z, r, "none", False)
    _check("none f32", (z + r).float(), z, r, "none", True)
    _check("gelu", _to16(X.gelu_erf(z) + r), z, r, "gelu", False)
    _check("swiglu", _to16(X.swiglu(z)), z, None, "swiglu", False)
    nan = X.rne16(z + r)
    nan[3, 5] = float("nan")
    for out, epi in ((_trunc16(z + r), "none"), (nan, "none"), (_to16(_tanh_gelu(setup(256, "act"))), "gelu")):
        S2 = setup(256, "act") if epi == "gelu" else S
        z2 = S2["a"] @ S2["w"].t() + S2["b"]
        with pytest.raises(pytest.fail.Exception):
            _check("wrong", out, z2, None if epi == "gelu" else r, epi, False)


# ------------------------------------------------------------------------------------------------
# (b) wrong kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MUTANTS))
def test_wrong_kernels_are_rejected(name):
    applies, blind = 0, 0
    for K, kind in KS:
        can, rejected, old, _ = judge(name, K, kind)
        if can >= CAN:
            applies += 1
            blind += old
            assert rejected >= REJECT, (name, K, kind, can, rejected)
    assert applies > 0, name
    # the old criterion is blind to it somewhere - except for the three gross errors that move whole rows by O(|z|): against an INDEPENDENT
    # reference 2e-3 sees those on every input.  (The rotary epilogues had no independent reference: they were compared with other kernels of
    # the library, which share a wrong sign or table row.)
    assert blind > 0 or name in GROSS, f"{name}: applies on {applies} cases, of which the 2e-3 comparison passes {blind}"


# ------------------------------------------------------------------------------------------------
# (c) tau
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tau_share(Mi, Ni, K, epi, res):
    """worst share of tau that torch's fp32 evaluation of the activation (+ residual), rounded to fp16, uses beyond half an ulp"""
    a, w, b, r = X.family(Mi, Ni, K, "act", seed_of(Mi, Ni, K))
    z = a @ w.t() + b
    act = X.ACT[epi](z)
    y = act + r if res else act
    tau = X.tau_swiglu(y, z) if epi == "swiglu" else X.tau_act(act, z, y if res else None)
    f = X.fp32_act(z, epi)
    out = ((f + r.float()) if res else f).half()
    excess = ((out.double() - y).abs() - 0.5 * _ulp(y)).clamp(min=0)
    assert bool((excess[tau == 0] == 0).all())
    return float((excess / tau.clamp(min=1e-300)).max())


def test_cpu_fp32_uses_at_most_half_of_tau():
    for case in act_inputs():
        assert tau_share(*case) <= 0.5, case


# ------------------------------------------------------------------------------------------------
# the document
# ------------------------------------------------------------------------------------------------
def _cell(name, K, kind):
    if (K, kind) not in KS:
        return "-"
    can, rejected, old, n = judge(name, K, kind)
    if can < CAN:
        return "-"
    return f"{100.0 * rejected / n:.3g} % {'rejected' if rejected >= REJECT else 'MISSED'}, 2e-3 {'passed' if old else 'failed'}"


WHY_DASH = """`-`: the wrong kernel cannot differ there (its unrounded value differs from the true one on fewer than 32 of the elements; for truncation:
fewer than 32 outputs need a rounding; for a wrong activation: fewer than 32 outputs are more than an ulp off), or the GPU file has no case of
that kind at that K.  The reasons, by row: fp16 partials - on a coarse grid (large K) a short chunk's partial sum is an fp16 number already,
and `small` partials stay below 2^-9 where every multiple of 2^-20 is one; rounding before the residual and truncation - `small` at K = 64
has almost no output that needs a rounding; flush - only `small` has subnormal outputs; wrong activations - in `small` |z| < 2^-6, where
both GELUs are z / 2 and silu(g) u is g u / 2 to well below half an ulp."""


def document():
    ks = sorted({K for K, _ in KS})
    out = ["# What the exact-input GEMM / GEMV tests can tell apart", "",
           "Written by `python -m tests.test_exact_power`; do not edit.  Inputs: tests/_exact.py, M = %d, N = %d on the CPU in fp64, the K and kinds of" % (M, N),
           "tests/test_gpu_gemm_exact.py.  New criterion: `none` and the headed epilogues bit-exact against fp64 rounded once, activations within half an",
           "fp16 ulp + tau.  A wrong kernel is *rejected* when at least %d elements differ / are flagged; the figure is the share of elements.  Beside" % REJECT,
           "it: whether `torch.testing.assert_close(rtol=2e-3, atol=2e-3)` against the fp32 reference *passed* the same wrong output.", "", WHY_DASH, ""]
    for kind in X.KINDS:
        out += [f"## `{kind}`", "", "| wrong kernel | " + " | ".join(f"K = {K}" for K in ks) + " |", "|---|" + "---|" * len(ks)]
        for name in MUTANTS:
            out.append(f"| {name} | " + " | ".join(_cell(name, K, kind) for K in ks) + " |")
        out.append("")
    out += ["## The construction", "",
            "Exact: fp32 sums in forward, reversed, 64- and 512-chunked order + bias + residual, and the int64 matmul of the generators, all equal fp64.",
            "*rounded*: outputs that their fp16 rounding changes (with bias and residual / the bare sum); *subnormal*: nonzero outputs below 2^-14.", "",
            "| K | kind | unit | exact | rounded | subnormal | abs z < 4 | abs z > 6 |", "|---|---|---|---|---|---|---|---|"]
    for K, kind in KS:
        c = construction(K, kind)
        unit = "2^-10" if kind == "small" else f"2^-{X.unit_exponent(K)}"
        out.append(f"| {K} | {kind} | {unit} | {'yes' if all(c['orders'].values()) else 'NO'} | {100 * c['rounded']:.3g} % / {100 * c['rounded_plain']:.3g} % | "
                   f"{100 * c['subnormal']:.3g} % / {100 * c['subnormal_plain']:.3g} % | {100 * c['below4']:.3g} % | {100 * c['beyond6']:.3g} % |")
    out += ["", "## tau", "",
            "`tau = 2^-18 |act(z)| + 2^-20 |z|` (SwiGLU: `2^-18 |y| + 2^-20 |g u|`; with a residual `+ 2^-23 |y|` for the fp32 add), derived in tests/_exact.py.",
            "Worst share of tau that torch's fp32 evaluation on the CPU, rounded to fp16, uses beyond half an ulp, over every `act` input of the GPU file",
            "(at most 0.5 allowed):", "", "| epilogue | inputs | worst share of tau |", "|---|---|---|"]
    for epi in ("quick_gelu", "gelu", "swiglu"):
        shares = [tau_share(*c) for c in act_inputs() if c[3] == epi]
        out.append(f"| {epi} | {len(shares)} | {max(shares):.3g} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "GEMM_EXACT_POWER.md"), "w") as fh:
        fh.write(document())
