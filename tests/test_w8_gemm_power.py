"""The two contracts of tests/test_gpu_w8_gemm.py - assert_close_fp16 against fp64 on the contract family, bit equality on the exact family -
must REJECT a wrong kernel.  Six wrong kernels, restated on the CPU in fp64 from the inputs the GPU tests use (tests/_w8_gemm.py); the right
kernel, restated the same way, passes both.  What each contract can and cannot tell apart: tests/W8_GEMM_POWER.md."""
import pytest
import torch

from tests import _exact, _w8, _w8_gemm as G
from tests._tol import assert_close_fp16

N, M = 48, 26


def fnuz_values(codes):
    """the bytes decoded as e4m3fnuz (bias 8): every finite value halved"""
    return _w8.e4m3_values(codes) / 2


def neighbour_scale(c):
    return dict(scale=torch.roll(c["scale"], 1))


def drop_last_slice(codes):
    v = _w8.e4m3_values(codes).clone()
    v[:, -128:] = 0
    return v


def swap_halves(codes):
    """bytes 8-15 of every 16-byte piece meet the activations of bytes 0-7 and the other way round"""
    v = _w8.e4m3_values(codes)
    return v.view(v.shape[0], -1, 2, 8).flip(2).reshape(v.shape)


def rows_xor_16(c):
    a = c["a"]
    idx = torch.arange(a.shape[0]) ^ 16
    return dict(a=a[idx])


WRONG = {
    "codes decoded as e4m3fnuz": lambda c: dict(values=fnuz_values),
    "the neighbouring row's scale": neighbour_scale,
    "scale applied to the bias as well": lambda c: dict(scale_bias=True),
    "last 128-wide K slice dropped": lambda c: dict(values=drop_last_slice),
    "8-byte halves of a 16-byte piece swapped": lambda c: dict(values=swap_halves),
    "row m reads activation row m xor 16": rows_xor_16,
}


def contract_rejects(c, y):
    try:
        assert_close_fp16(y.half(), c["ref"][:M])
    except AssertionError:
        return True
    return False


def exact_rejects(c, y):
    return bool(_exact.differing(y.float().half(), _exact.rne16(c["ref"][:M])).any()) and bool(_exact.differing(y.float().double(), c["ref"][:M]).any())


@pytest.mark.parametrize("K", [256, 3584, 18944])
def test_right_kernel_passes_both(K):
    for fam, rejects in ((G.contract_case, contract_rejects), (G.exact_case, exact_rejects)):
        c = fam(N, K, seed=1, bias=True, res=True)
        assert not rejects(c, G.reference(c)[1][:M])


@pytest.mark.parametrize("K", [256, 3584, 18944])
@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_kernel_is_rejected_by_both(wrong, K):
    for fam, rejects in ((G.contract_case, contract_rejects), (G.exact_case, exact_rejects)):
        c = fam(N, K, seed=1, bias=True, res=True)
        y = G.reference(c, **WRONG[wrong](c))[1][:M]
        assert rejects(c, y), f"{fam.__name__} at K = {K} does not notice: {wrong}"


def test_exact_family_budget_and_rounding():
    for K in (256, 2048, 3584, 18944):
        c = G.exact_case(N, K, seed=1, bias=True, res=True)
        assert c["budget"] < 2 ** 24
        assert _exact.unrounded_share(c["ref"]) > 0
        # any summation order: the sum of the K slices of 128, added in reverse, is the same fp32 number
        v, a = _w8.e4m3_values(c["q"]).float(), c["a"].float()
        fwd = torch.zeros(G.M_MAX, N)
        rev = torch.zeros(G.M_MAX, N)
        for s in range(K // 128):
            fwd += a[:, s * 128:(s + 1) * 128] @ v[:, s * 128:(s + 1) * 128].t()
            r = K // 128 - 1 - s
            rev += a[:, r * 128:(r + 1) * 128] @ v[:, r * 128:(r + 1) * 128].t()
        assert torch.equal(fwd, rev) and torch.equal(fwd.double(), c["a"].double() @ _w8.e4m3_values(c["q"]).t())
