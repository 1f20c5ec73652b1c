"""Exact-arithmetic operands and bit-exact oracles for the dense kernels (host only; tests/test_exact_power.py and tests/test_gpu_gemm_exact.py).

fp16 operands on a power-of-two grid chosen so that every product, every partial sum in ANY order, the bias add and the residual add are
exactly representable in fp32.  Whatever the MFMA order, K split, tile walk or wave merge of a kernel, its fp32 accumulator then holds the
exact sum, and for the epilogues without a transcendental the fp16 output must equal the fp64 result rounded once.  For the activation
epilogues the activation's input z is exact; what is left is half an fp16 ulp plus the small fp32 term `tau` derived below.

The oracles are fp64 restatements of the epilogues as include/streamchat_hip.h describes them, not of the kernels."""
import math

import torch

B_MAX, R_MAX = 2.0, 4.0            # |bias|, |residual| bounds of `wide`
KINDS = ("wide", "small", "act")


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def unit_exponent(K, bits=23):
    """e of the operand unit u = 2^-e of `wide`: the largest of 7 .. 1 with (2 amax wmax K + |bias|max + |res|max) / u^2 < 2^bits, amax = 2, wmax = 1"""
    for e in range(7, 0, -1):
        if (2 * 2.0 * 1.0 * K + B_MAX + R_MAX) * 4.0 ** e < 2.0 ** bits:
            return e
    raise ValueError(f"K = {K} leaves no unit within 2^{bits}")


def _mixed(shape, bound, u2, g):
    """integers (in units of u2) of a bias / residual: half of the elements on the fine grid u2 itself, half on 2^s u2 reaching up to `bound`;
    every value has at most 10 significant bits (fp16 holds it) and is a multiple of u2"""
    n = int(min(1023, bound / u2))
    s = max(0, int(math.floor(math.log2(bound / (n * u2)))))
    i = torch.randint(-n, n + 1, shape, generator=g, dtype=torch.int64)
    coarse = torch.randint(0, 2, shape, generator=g, dtype=torch.int64)
    return i * torch.where(coarse.bool(), 2 ** s, 1)


def family_ints(M, N, K, kind, seed, bits=23):
    """dict(ia [M,K], iw [N,K], ib [N], ir [M,N] int64; sa, sw: a = ia sa, w = iw sw, bias = ib sa sw, res = ir sa sw; budget = bound of every
    partial sum + bias + residual in units of sa sw, < 2^bits)"""
    assert kind in KINDS
    g = _gen(seed)
    e = unit_exponent(K, bits)
    if kind == "small":
        # a, w multiples of 2^-10 within 2^-6 (normal fp16), the integers those of `wide` capped at 16; bias / residual: 0 or +-(64 .. 127) 2^-20,
        # normal fp16 values in [2^-14, 2^-13) on the product grid
        ra, rw, sa, sw = min(2 ** (e + 1), 16), min(2 ** e, 16), 2.0 ** -10, 2.0 ** -10
        def br(shape):
            return torch.randint(-1, 2, shape, generator=g, dtype=torch.int64) * torch.randint(64, 128, shape, generator=g, dtype=torch.int64)
        ia = torch.randint(-ra, ra + 1, (M, K), generator=g, dtype=torch.int64)
        iw = torch.randint(-rw, rw + 1, (N, K), generator=g, dtype=torch.int64)
        ib, ir = br((N,)), br((M, N))
        budget = K * ra * rw + 127 + 127
    else:
        ra, rw, sa, sw = 2 ** (e + 1), 2 ** e, 2.0 ** -e, 2.0 ** -e
        ia = torch.randint(-ra, ra + 1, (M, K), generator=g, dtype=torch.int64)
        iw = torch.randint(-rw, rw + 1, (N, K), generator=g, dtype=torch.int64)
        ib, ir = _mixed((N,), B_MAX, sa * sw, g), _mixed((M, N), R_MAX, sa * sw, g)
        budget = (K * ra * rw + int(ib.abs().max()) + int(ir.abs().max()))
        if kind == "act":
            # w scaled by 2^-j (bias and residual keep their grid: their integers grow by 2^j), j the smallest with at least 55 % of a probe block
            # of z = a w^T + bias inside |z| < 4
            pa, pw = ia[:16].double() * sa, iw[:512].double() * sw
            pb = ib[:512].double() * sa * sw
            j = 0
            while ((pa @ pw.t() * 2.0 ** -j + pb).abs() < 4).double().mean() < 0.55:
                j += 1
            sw, ib, ir = sw * 2.0 ** -j, ib * 2 ** j, ir * 2 ** j
            budget = (K * ra * rw + int(ib.abs().max()) + int(ir.abs().max()))
    assert budget < 2 ** bits, (K, kind, budget)
    return dict(ia=ia, iw=iw, ib=ib, ir=ir, sa=sa, sw=sw, budget=budget)


def family(M, N, K, kind, seed, bits=23):
    """fp64 a [M,K], w [N,K], bias [N], res [M,N]; each survives the round trip through fp16.  bits = 20 for the headed epilogues (three bits
    left for a table value or a column scale on the 2^-3 grid)."""
    f = family_ints(M, N, K, kind, seed, bits)
    u2 = f["sa"] * f["sw"]
    out = (f["ia"].double() * f["sa"], f["iw"].double() * f["sw"], f["ib"].double() * u2, f["ir"].double() * u2)
    for t in out:
        assert torch.equal(t.half().double(), t)
    return out


def dyadic_table(rows, half, seed):
    """a rotary "table" [rows][2][half] fp32 of multiples of 2^-3 within +-1 (the kernels only read the table: any values do)"""
    return torch.randint(-8, 9, (rows, 2, half), generator=_gen(seed), dtype=torch.int64).float() / 8


# ------------------------------------------------------------------------------------------------
# criteria
# ------------------------------------------------------------------------------------------------
def rne16(x64):
    """fp64 -> fp16, round to nearest even ONCE: torch narrows double to half through float, so the value has to be an fp32 number already"""
    assert torch.equal(x64.float().double(), x64), "not exactly representable in fp32: the operand budget is broken"
    return x64.float().half()


def differing(out, ref):
    """elements of `out` that are not the value `ref` holds (a NaN differs from everything; +0 and -0 are one value)"""
    return ~(out == ref)


def half_ulp_excess(out16, y64, tau):
    """mask of the elements with |out - y| > ulp / 2 + tau, ulp = 2^(max(floor(log2 |y|), -14) - 10); NaN / inf outputs are flagged"""
    m, e = torch.frexp(y64)                                       # |y| = m 2^e, m in [0.5, 1): floor(log2 |y|) = e - 1
    fl = torch.where(y64 == 0, torch.full_like(e, -14), e - 1).clamp(min=-14)
    ulp = torch.pow(2.0, (fl - 10).double())
    return ~((out16.double() - y64).abs() <= 0.5 * ulp + tau)


def within_half_ulp(out16, y64, tau):
    return not bool(half_ulp_excess(out16, y64, tau).any())


def unrounded_share(y64):
    """share of the elements whose fp16 rounding changes them"""
    return float((y64.float().half().double() != y64).double().mean())


# ------------------------------------------------------------------------------------------------
# fp64 restatements of the epilogues (include/streamchat_hip.h)
# ------------------------------------------------------------------------------------------------
def a_row_index(M, a_rows):
    """storage row of logical row m under a_rows = (grp, stride, off): (m / grp) stride + off + m % grp"""
    m = torch.arange(M)
    if a_rows is None:
        return m
    grp, stride, off = a_rows
    return (m // grp) * stride + off + m % grp


def a_store_rows(M, a_rows):
    return M if a_rows is None else int(a_row_index(M, a_rows)[-1]) + 1


def quick_gelu(z):
    return z / (1 + torch.exp(-1.702 * z))


def gelu_erf(z):
    return 0.5 * z * torch.erfc(-z * math.sqrt(0.5))              # 1 + erf(x) = erfc(-x), without the cancellation of the negative tail


def silu(z):
    return z / (1 + torch.exp(-z))


def swiglu_parts(z):
    """(gate, up) [M, N/2] from z [M, N] whose columns are interleaved quads (g_j, g_j+1, u_j, u_j+1)"""
    q = z.reshape(z.shape[0], z.shape[1] // 4, 2, 2)
    return q[:, :, 0].reshape(z.shape[0], -1), q[:, :, 1].reshape(z.shape[0], -1)


def swiglu(z):
    gate, up = swiglu_parts(z)
    return silu(gate) * up


ACT = {"none": lambda z: z, "quick_gelu": quick_gelu, "gelu": gelu_erf, "swiglu": swiglu}


def rope(z, tab, pos0, lead_cols, Dh=128):
    """rotate-half RoPE of the heads in columns [0, lead_cols) with table row pos0 + m ([pos][0] = cos, [pos][1] = sin, Dh / 2 each); columns
    beyond stay plain"""
    M, h = z.shape[0], Dh // 2
    t = tab[pos0:pos0 + M].double()
    cos, sin = t[:, None, 0], t[:, None, 1]                       # [M, 1, Dh/2]
    x = z[:, :lead_cols].reshape(M, lead_cols // Dh, Dh)
    x1, x2 = x[..., :h], x[..., h:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1).reshape(M, lead_cols)
    return torch.cat([rot, z[:, lead_cols:]], 1)


def colscale(z, scale, lead_cols):
    return torch.cat([z[:, :lead_cols] * scale, z[:, lead_cols:]], 1)


# ------------------------------------------------------------------------------------------------
# tau: what an fp32 evaluation of an activation from an EXACT z may add to half an fp16 ulp.  Derived, never fitted:
#   __expf(t) multiplies t by log2 e in fp32: relative error of the product 2^-24, of the exponential |t| 2^-24 ln 2 ... < 32 x 2^-24 = 2^-19 for
#   |t| < 32; v_exp_f32 and v_rcp_f32 are 1 ulp, the fp32 products and the division 0.5 - 1 ulp each: together below 2^-18 relative to act(z).
#   1 + erff(x / sqrt 2): erff is within a few ulp of a value near -1 .. 1, the sum has an ABSOLUTE error of a few 2^-24, times |z| / 2:
#   below 2^-20 |z|.  A residual add in fp32 rounds the sum once more, by at most half an fp32 ulp <= 2^-24 |y| (reached at a power of two);
#   like the other terms it enters with a factor of two to spare: 2^-23 |y|, 2^-12 of half an fp16 ulp.
# 2^-18 relative is 1/64 of half an fp16 ulp.  The yardstick: torch's fp32 evaluation on the CPU must use at most HALF of tau.
# ------------------------------------------------------------------------------------------------
def tau_act(act64, z64, y64=None):
    """act64 = act(z) in fp64; y64 = act(z) + residual where there is one"""
    t = 2.0 ** -18 * act64.abs() + 2.0 ** -20 * z64.abs()
    return t if y64 is None else t + 2.0 ** -23 * y64.abs()


def tau_swiglu(y64, z64):
    gate, up = swiglu_parts(z64)
    return 2.0 ** -18 * y64.abs() + 2.0 ** -20 * (gate * up).abs()


def fp32_act(z64, epi):
    """the same expressions evaluated by torch in fp32 on the CPU (the yardstick for `tau`: it must use at most half of it)"""
    z = z64.float()
    if epi == "quick_gelu":
        return z * (1.0 / (1.0 + torch.exp(-1.702 * z)))
    if epi == "gelu":
        return 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752))
    if epi == "swiglu":
        gate, up = swiglu_parts(z)
        return gate / (1.0 + torch.exp(-gate)) * up
    return z
