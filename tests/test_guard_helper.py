"""Host: the guarded arena of tests/_guard.py detects and locates stray writes (on CPU tensors - this is the proof that the GPU write-bound
tests can fail), and every C ABI function that takes a writable device pointer is covered by tests/test_gpu_write_bounds.py."""
import os
import re

import pytest
import torch

from tests._guard import Arena, GuardViolation, PATTERN, frozen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _elem(view, index):
    """one-element window at element `index` relative to the view's first element (may lie outside the view: that is the point)"""
    return torch.as_strided(view, (1,), (1,), view.storage_offset() + index)


def _arena(dtype=torch.float16, rows=5, cols=24, ld=32, **kw):
    a = Arena("cpu")
    v = a.out(rows, cols, dtype, ld=ld, **kw)
    return a, v


def test_pattern_reads_as_nan_and_as_an_implausible_integer():
    raw = torch.full((8,), PATTERN, dtype=torch.uint8)
    assert torch.isnan(raw.view(torch.float16)).all() and float(raw.view(torch.bfloat16)[0]) > 1e37
    assert float(raw.view(torch.float32)[0]) > 1e37 and int(raw.view(torch.int32)[0]) == 0x7E7E7E7E
    a, v = _arena()
    assert torch.isnan(v).all()                                   # an output the kernel did not write shows up too


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.int64, torch.uint8])
def test_in_bounds_writes_pass(dtype):
    a, v = _arena(dtype)
    v.fill_(1)
    assert v.shape == (5, 24) and v.stride() == (32, 1)
    a.check("in bounds")
    w = a.flat(100, dtype)
    w.fill_(3)
    a.check("in bounds, flat")


def test_write_one_element_past_the_last_row_is_located():
    a, v = _arena()
    v.fill_(1)
    _elem(v, 5 * 32).fill_(2.0)                                   # element [5, 0]: the first of the tail band
    with pytest.raises(GuardViolation) as e:
        a.check("past the end")
    assert e.value.first == (5, 0) and e.value.last == (5, 0) and e.value.count == 2 and "row 5, col 0" in str(e.value)


def test_write_into_the_gap_of_a_middle_row_is_located():
    a, v = _arena()
    v.fill_(1)
    _elem(v, 2 * 32 + 24).fill_(2.0)                              # first gap element of row 2
    _elem(v, 3 * 32 + 31).fill_(2.0)                              # last gap element of row 3
    with pytest.raises(GuardViolation) as e:
        a.check("gap")
    assert e.value.first == (2, 24) and e.value.last == (3, 31) and e.value.count == 4


def test_write_into_the_gap_of_the_last_row_is_located():
    a, v = _arena(torch.float32)
    v.fill_(1)
    _elem(v, 4 * 32 + 30).fill_(2.0)
    with pytest.raises(GuardViolation) as e:
        a.check("last row's gap")
    assert e.value.first == (4, 30) and e.value.last == (4, 30) and e.value.count == 4


def test_write_before_the_first_element_is_located():
    a, v = _arena()
    v.fill_(1)
    _elem(v, -1).fill_(2.0)
    with pytest.raises(GuardViolation) as e:
        a.check("in front")
    assert e.value.first == (-1, 31) and e.value.count == 2      # one element before [0, 0] = the last column of "row -1"


def test_single_changed_byte_and_second_block_are_reported():
    a = Arena("cpu")
    v0, v1 = a.out(3, 8, torch.float16, ld=8, name="first"), a.out(2, 4, torch.int32, ld=6, name="second")
    v0.fill_(0)
    v1.fill_(0)
    a.check("clean")
    _elem(v1, 4).view(torch.uint8)[1] = 0                         # one byte of gap element [0, 4] of the second block
    with pytest.raises(GuardViolation) as e:
        a.check("one byte")
    assert e.value.name == "second" and e.value.first == (0, 4) and e.value.count == 1


def test_requested_alignment_is_delivered():
    a = Arena("cpu")
    assert a.out(2, 8, torch.float16).data_ptr() % 256 == 0
    p = a.out(2, 8, torch.float16, align=16, misalign=8).data_ptr()
    assert p % 8 == 0 and p % 16 == 8
    assert a.out(2, 8, torch.float32, lead_bytes=0).data_ptr() % 256 == 0
    a.check("untouched")


def test_tail_band_holds_the_requested_rows():
    a = Arena("cpu")
    v = a.out(4, 8, torch.float16, ld=16, tail_rows=256)
    blk = a.blocks[0]
    assert blk.raw.numel() - (blk.start + 4 * 16 * 2) >= 256 * 16 * 2 and blk.start >= 4096
    w = a.flat(10, torch.uint8, tail_bytes=1000)
    assert w.shape == (10,) and a.blocks[1].raw.numel() - (a.blocks[1].start + 10) >= 1000


def test_frozen_detects_a_modified_input_and_passes_an_untouched_one():
    x, y = torch.randn(4, 8), torch.arange(6)
    with frozen(x, None, y[::2]):
        pass
    with pytest.raises(AssertionError, match="input 1"):
        with frozen(x, y):
            y[3] = 7
    nan = torch.full((3,), float("nan"))
    with frozen(nan):                                             # compared as integers: NaN == NaN
        pass


# ------------------------------------------------------------------------------------------------------------------------------------
def _writable_pointer_functions():
    """names of the extern "C" functions of include/streamchat_hip.h with at least one non-const pointer parameter"""
    text = open(os.path.join(ROOT, "include", "streamchat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for ret, name, args in re.findall(r"\b(int|size_t|const char\*)\s+(sc_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        params = [p.strip() for p in args.split(",")]
        if any("*" in p and not p.startswith("const ") for p in params):
            out.append(name)
    return out


def test_every_abi_function_with_a_writable_pointer_is_in_the_write_bound_module():
    from tests import test_gpu_write_bounds as W
    names = _writable_pointer_functions()
    assert len(names) >= 29 and "sc_gemm_f16" in names and "sc_kmeans_fit_cols" in names and "sc_abi_version" not in names, names
    assert set(W.EXEMPT) <= {"sc_kmeans_fit_cols", "sc_stream_create_masked", "sc_device_info"}, "the exemption list may not grow without a reason"
    missing = [n for n in names if n not in W.COVERED and n not in W.EXEMPT]
    assert not missing, f"no write-bound test for {missing}: add one to tests/test_gpu_write_bounds.py and list it in COVERED"
    assert not set(W.COVERED) & set(W.EXEMPT)
    src = open(W.__file__).read()
    for name, tests in W.COVERED.items():
        assert name in names, f"{name} is not an ABI function with a writable pointer"
        assert tests, name
        for t in tests:
            assert callable(getattr(W, t, None)), f"COVERED names {t} for {name}, which the module does not define"
        assert re.search(rf"\b{name}\b", src.split("COVERED", 1)[1].split("}", 1)[1]), f"{name} is listed but never named by a test"
