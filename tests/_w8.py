"""Inputs and fp64 references of the FP8 (e4m3) weight-only decode tests, shared by tests/test_gpu_w8.py (the kernels), tests/test_w8_power.py
(the CPU proof that the contract used there tells a wrong kernel from a right one) and tests/test_gpu_w8_write_bounds.py.  Everything is
generated on the CPU from a seed, so the GPU tests and the CPU power test see the SAME numbers.

The byte codes cover every finite e4m3fn code (0x7F / 0xFF are the NaNs), the row scales are spread over 2^+-8 around `2^shift`: a kernel that
decodes the bytes as e4m3fnuz (every value halved), or takes a neighbouring row's scale, is far outside the fp16 GEMV contract."""
import torch

FINITE = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)          # the 254 finite codes


def e4m3_values(codes):
    """OCP e4m3fn bytes -> fp64 values"""
    return codes.view(torch.float8_e4m3fn).double()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def random_codes(N, K, seed):
    return FINITE[torch.randint(0, 254, (N, K), generator=gen(seed))]


def spread_scales(N, seed, shift=0):
    """fp32 [N]: 2^e * (1 + u / 2), e uniform in [shift - 8, shift + 8]"""
    g = gen(seed)
    e = torch.randint(shift - 8, shift + 9, (N,), generator=g)
    return (torch.exp2(e.float()) * (1 + 0.5 * torch.rand(N, generator=g))).float()


def rmsnorm_fp16(x, g, eps):
    """the fused RMSNorm of the decode projections as the fp16 GEMV tests restate it: gamma * fp16(x * rstd), rounded to fp16 once more"""
    x, g = x.double(), g.double()
    return (g * (x * torch.rsqrt((x ** 2).mean() + eps)).half().double()).half().double()


def gemv_case(N, K, seed=0, norm=False, bias=False, res=False, swiglu=False):
    """dict(q uint8 [N, K], scale fp32 [N], x fp16 [K], gamma fp16 [K] | None, bias / res fp16 [N] | None, xh fp64 [K]: the vector the weights
    multiply, ref fp64: the GEMV's exact result).  The activation side is sized so that |y| stays far below the fp16 maximum at every K:
    sum_k q x has an rms of ~110 sqrt(K) |x|, so x (or gamma, with the norm) carries 1 / (8 sqrt(K)); SwiGLU multiplies two rows and
    takes its scales around 2^-8."""
    g = gen(1000 + seed)
    q, scale = random_codes(N, K, seed), spread_scales(N, seed + 1, shift=-8 if swiglu else 0)
    small = 1.0 / (8 * K ** 0.5)
    if norm:
        x = torch.randn(K, generator=g).half()
        gamma = ((1 + 0.1 * torch.randn(K, generator=g)) * small).half()
        xh = rmsnorm_fp16(x, gamma, 1e-6)
    else:
        x, gamma = (torch.randn(K, generator=g) * small).half(), None
        xh = x.double()
    b = (torch.randn(N, generator=g) * 10).half() if bias else None
    r = (torch.randn(N, generator=g) * 10).half() if res else None
    c = dict(q=q, scale=scale, x=x, gamma=gamma, bias=b, res=r, xh=xh, swiglu=swiglu)
    c["ref"] = reference(c)
    return c


def reference(c, values=e4m3_values, scale=None):
    """fp64 y = scale[n] * sum_k value(q[n, k]) * xh[k] (+ bias) (+ res) | SwiGLU on the (g g u u) interleave.  `values` / `scale`: what a WRONG
    kernel would use instead (tests/test_w8_power.py)."""
    s = (c["scale"] if scale is None else scale).double()
    y = s * (values(c["q"]) @ c["xh"])
    if c["bias"] is not None:
        y = y + c["bias"].double()
    if c["res"] is not None:
        y = y + c["res"].double()
    if c["swiglu"]:
        z = y.view(-1, 2, 2)
        y = (torch.nn.functional.silu(z[:, 0]) * z[:, 1]).reshape(-1)
    return y


def fp8_exact_matrix(N, K, seed=0):
    """(W fp16 [N, K], codes uint8 [N, K], e int [N]): row n = 2^e_n * e4m3 values, e_n in [-15, -10], every row holds all 254 finite codes
    (K >= 254), +-448 * 2^e_n among them.  Exact in fp16 (the smallest magnitude, 2^-9 * 2^-15, is fp16's smallest subnormal), so per-row
    e4m3 quantisation returns scale 2^e_n and the codes themselves: a model built from such weights IS its fp8 model."""
    assert K >= 254
    g = gen(seed)
    codes = FINITE[torch.randint(0, 254, (N, K), generator=g)]
    start = torch.randint(0, K - 253, (N,), generator=g)
    perm = torch.argsort(torch.rand(N, 254, generator=g), dim=1)
    codes.scatter_(1, start[:, None] + torch.arange(254)[None, :], FINITE[perm])
    e = torch.randint(-15, -9, (N,), generator=g)
    W = (e4m3_values(codes) * torch.exp2(e.double())[:, None]).half()
    assert torch.equal(W.double(), e4m3_values(codes) * torch.exp2(e.double())[:, None])
    return W, codes, e


def quantize_ref(W):
    """the specification of sc_quantize_rows_e4m3, on the CPU: (bytes uint8 [N, K], scale fp32 [N])"""
    W = W.cpu().float()
    amax = W.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
    return (W / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8), s
