"""CPU (torch only): the contract of tests/test_gpu_w8.py - assert_close_fp16 at its defaults against the fp64 reference on the dequantised
weights - can tell a wrong FP8 GEMV from a right one, on the GPU tests' OWN inputs (tests/_w8.py).  Three wrong kernels, restated in fp64:
  * the bytes decoded as e4m3fnuz (gfx942's format: exponent bias 8, every value halved, 0x80 a NaN);
  * scale[n + 1] used for row n;
  * the scale applied to fp16-rounded partial sums instead of once to the fp32 sum.
The first two must FAIL the check; the true reference rounded to fp16 (the most a correct kernel may lose) must PASS.  The third is an accuracy
loss of the size of fp16 rounding itself, which no end-to-end tolerance can see: it is printed, and what pins it is the kernel's structure
(one fp32 accumulator per row, gemv_w8.hip) and the bitwise decode_qkv_tab_w8 == gemv_w8(out_f32) + rope test."""
import pytest
import torch

from tests import _w8
from tests._tol import assert_close_fp16

CASES = [dict(N=37, K=1040, bias=True, res=True), dict(N=50, K=3584, norm=True, bias=True), dict(N=36, K=1040, swiglu=True)]


def _fnuz_values(codes):
    v = codes.view(torch.float8_e4m3fnuz).double()
    return torch.where(torch.isnan(v), torch.zeros_like(v), v)          # (0x80 is fnuz's NaN; a kernel would propagate it - zero is the kinder reading)


@pytest.mark.parametrize("kw", CASES, ids=lambda k: f"N{k['N']}-K{k['K']}")
def test_contract_passes_the_rounded_truth_and_fails_wrong_kernels(kw):
    c = _w8.gemv_case(**kw)
    ref = c["ref"]
    assert_close_fp16(ref.half(), ref, what="true reference rounded to fp16")
    with pytest.raises(AssertionError):
        assert_close_fp16(_w8.reference(c, values=_fnuz_values).half(), ref, what="bytes decoded as e4m3fnuz")
    with pytest.raises(AssertionError):
        assert_close_fp16(_w8.reference(c, scale=torch.roll(c["scale"], -1)).half(), ref, what="scale[n + 1] for row n")


def test_scale_before_partial_rounding_is_below_any_end_to_end_tolerance():
    c = _w8.gemv_case(N=37, K=1040, bias=True, res=True)
    vals, s = _w8.e4m3_values(c["q"]), c["scale"].double()
    y = sum((s * (vals[:, k:k + 512] @ c["xh"][k:k + 512])).half().double() for k in range(0, 1040, 512))
    y = y + c["bias"].double() + c["res"].double()
    err = ((y - c["ref"]).abs().max() / c["ref"].abs().max()).item()
    print(f"\nscale applied per fp16-rounded 512-slice partial: max err {err:.2e} of max|ref| (fp16 rounding: 4.9e-4)")
    assert err < 4e-3


def test_inputs_cover_every_finite_code_and_spread_scales():
    c = _w8.gemv_case(N=37, K=1040)
    assert len(torch.unique(c["q"])) == 254 and not bool(((c["q"] & 0x7F) == 0x7F).any())
    e = torch.log2(c["scale"])
    assert e.min() < -5 and e.max() > 5
    W, codes, ex = _w8.fp8_exact_matrix(6, 256, seed=3)
    assert all(len(torch.unique(codes[n])) == 254 for n in range(6))
    q, s = _w8.quantize_ref(W)
    assert torch.equal(q, codes) and torch.equal(s, torch.exp2(ex.float()))         # the construction round-trips: scale 2^e_n, codes unchanged
    assert int(torch.tensor(500.0).to(torch.float8_e4m3fn).view(torch.uint8)) & 0x7F == 0x7F      # why the quantiser clamps: torch turns 500 into NaN
