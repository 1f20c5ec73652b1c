"""Inputs and fp64 references of the e4m3-weight skinny GEMM tests (sc_gemm_w8_f16), shared by tests/test_gpu_w8_gemm.py (the kernels),
tests/test_gpu_w8_gemm_write_bounds.py and tests/test_w8_gemm_power.py (the CPU proof that the two contracts used there tell a wrong kernel
from a right one).  Everything is generated on the CPU from a seed, so the GPU tests and the power test see the SAME numbers.

Two families:
  * "contract": all 254 finite codes (_w8.random_codes) with scales spread over 2^+-8 (_w8.spread_scales), activations sized as in
    _w8.gemv_case so that |y| stays far below the fp16 maximum; checked against fp64 with assert_close_fp16 at its defaults, the contract of
    the fp16 GEMM and GEMV.
  * "exact": every partial sum, in ANY order, is exact in fp32, so the fp32 accumulator holds the exact sum and the output must equal the fp64
    result rounded once - bit for bit.  Codes whose e4m3 value is an integer with |v| <= 16, power-of-two row scales 2^e_n, activations integers
    on the grid 2^-6, bias and residual integers on column n's OUTPUT grid 2^-6 2^e_n; the generator asserts the budget
    K * 16 * |a|max + |bias|max + |res|max < 2^24 in grid units.

A case always carries 32 rows of A: a row's result depends on that row alone, so the launches with fewer rows are checked against the leading
rows of the one reference."""
import torch

from tests import _w8

M_MAX = 32
GRID = 2.0 ** -6                 # the activation grid of the exact family

# the codes of the exact family: finite e4m3fn codes whose value is an integer of magnitude at most 16 (both zeros included)
_v = _w8.e4m3_values(_w8.FINITE)
INT_CODES = _w8.FINITE[(_v == _v.round()) & (_v.abs() <= 16)]
assert len(INT_CODES) == 2 * 17 and set(_w8.e4m3_values(INT_CODES).tolist()) == set(float(i) for i in range(-16, 17))


def swiglu64(z):
    """fp64 SwiGLU on the (g g u u) column interleave: [M, N] -> [M, N / 2]"""
    q = z.reshape(z.shape[0], z.shape[1] // 4, 2, 2)
    g, u = q[:, :, 0].reshape(z.shape[0], -1), q[:, :, 1].reshape(z.shape[0], -1)
    return g / (1 + torch.exp(-g)) * u


def reference(c, values=_w8.e4m3_values, scale=None, scale_bias=False, a=None):
    """fp64 (z, y): z = scale[n] * sum_k value(q[n, k]) a[m, k] + bias[n] - the epilogue's input - and y = swiglu(z) or z + res.  `values`,
    `scale`, `scale_bias`, `a`: what a WRONG kernel would use instead (tests/test_w8_gemm_power.py)."""
    s = (c["scale"] if scale is None else scale).double()
    A = (c["a"] if a is None else a).double()
    z = A @ values(c["q"]).t()
    b = c["bias"].double() if c["bias"] is not None else torch.zeros(z.shape[1], dtype=torch.float64)
    z = (z + b) * s if scale_bias else z * s + b
    if c["swiglu"]:
        return z, swiglu64(z)
    return z, (z + c["res"].double() if c["res"] is not None else z)


def contract_case(N, K, seed=0, bias=False, res=False, swiglu=False):
    """dict(q uint8 [N, K], scale fp32 [N], a fp16 [32, K], bias fp16 [N] | None, res fp16 [32, N] | None, z / ref fp64)"""
    g = _w8.gen(2000 + seed)
    q, scale = _w8.random_codes(N, K, seed), _w8.spread_scales(N, seed + 1, shift=-8 if swiglu else 0)
    a = (torch.randn(M_MAX, K, generator=g) / (8 * K ** 0.5)).half()
    b = (torch.randn(N, generator=g) * (0.01 if swiglu else 10)).half() if bias else None
    r = (torch.randn(M_MAX, N, generator=g) * 10).half() if res else None
    c = dict(q=q, scale=scale, a=a, bias=b, res=r, swiglu=swiglu)
    c["z"], c["ref"] = reference(c)
    return c


def exact_case(N, K, seed=0, bias=False, res=False, swiglu=False):
    """the exact family (module docstring); scales 2^e_n, e_n in [-6, 0] (SwiGLU: [-14, -8], so that the gates lie where the sigmoid bends)"""
    g = _w8.gen(3000 + seed)
    q = INT_CODES[torch.randint(0, len(INT_CODES), (N, K), generator=g)]
    e = torch.randint(-14, -7, (N,), generator=g) if swiglu else torch.randint(-6, 1, (N,), generator=g)
    scale = torch.exp2(e.float())
    ra = 1024
    while K * 16 * ra + 2 * 1023 >= 2 ** 24:
        ra //= 2
    ia = torch.randint(-ra, ra + 1, (M_MAX, K), generator=g, dtype=torch.int64)
    ib = torch.randint(-1023, 1024, (N,), generator=g, dtype=torch.int64) if bias else None
    ir = torch.randint(-1023, 1024, (M_MAX, N), generator=g, dtype=torch.int64) if res else None
    budget = K * 16 * int(ia.abs().max()) + (int(ib.abs().max()) if bias else 0) + (int(ir.abs().max()) if res else 0)
    assert budget < 2 ** 24, (K, budget)
    unit = GRID * scale.double()                                   # column n's output grid
    a = (ia.double() * GRID).half()
    b = (ib.double() * unit).half() if bias else None
    r = (ir.double() * unit[None, :]).half() if res else None
    assert torch.equal(a.double(), ia.double() * GRID) and (b is None or torch.equal(b.double(), ib.double() * unit))
    assert r is None or torch.equal(r.double(), ir.double() * unit[None, :])
    c = dict(q=q, scale=scale, a=a, bias=b, res=r, swiglu=swiglu, budget=budget)
    c["z"], c["ref"] = reference(c)
    assert torch.equal(c["z"].float().double(), c["z"]) and (swiglu or torch.equal(c["ref"].float().double(), c["ref"]))
    return c


# (N, K) of the kernel tests: K = 256 the generic kernel with waves that own no slice, 2048 two slices per wave, 3584 the resident-activation
# kernel (3 or 4 slices per wave), 18944 the longest rows (18 or 19 slices per wave); N = 16 one strip, 48 three, 4112 = 257 strips: one more
# than the 256 CUs, the smallest N at which the persistent kernel's workgroups own unequal numbers of strips
SHAPES = [(16, 256), (48, 256), (16, 2048), (48, 2048), (16, 3584), (48, 3584), (4112, 3584), (16, 18944), (48, 18944)]
MS = (1, 15, 16, 17, 26, 32)

# The resident-activation kernel (K = 3584, more strips than CUs) is persistent: its partial tiles are double-buffered by strip parity, the reducing
# wave rotates over the 8 waves and the next strip's weights are requested one strip ahead - all of which only matters from a workgroup's third
# strip on.  On the whole chip (4112, 3584) gives a workgroup one or two strips; on a stream masked to MASK_CUS CUs its 257 strips are 8 per
# workgroup and 9 for the first (every reducer, the parity buffers used four times each, the rotation wrapped): the path the 7B gate/up and lm_head
# launches take (9 and 38 strips per workgroup).  The tests run that shape on both streams.
MASKED_SHAPE, MASK_CUS = (4112, 3584), 32


def streams_for(N, K):
    """the streams a GPU test runs shape (N, K) on: None = the current stream, and for MASKED_SHAPE a CU-masked one as well"""
    if (N, K) != MASKED_SHAPE:
        return [None]
    from streamchat_amd import ops
    return [None, ops.masked_stream(0, MASK_CUS)]


class on_stream:
    """run the block on `stream` (None: where it is), ordered behind what the current stream holds and finished when the block ends"""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
            self.ctx = torch.cuda.stream(self.stream)
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.stream is not None:
            self.stream.synchronize()
            self.ctx.__exit__(*exc)
            torch.cuda.synchronize()
