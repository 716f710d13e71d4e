"""CPU tests of prk_advance_edge_lists' C-ABI boundary (no GPU compute): the
entry point include/prk.h declares is exported, bound, refuses a NULL context
before it touches a device, and the binding fails loudly without a GPU.  The
lists it returns are checked on the GPU (tests/test_gpu_advance_lists.py).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import prk
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_advance_lists_symbol_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        assert re.search(r"\bint prk_advance_edge_lists\(prk_context \*ctx, const prk_edge \*records, "
                         r"const uint32_t \*counts,\s+uint32_t list_count, int32_t height, "
                         r"prk_edge \*records_out, int32_t \*next_out\);", f.read())
    assert "prk_advance_edge_lists" in prk.exported_symbols()
    assert hasattr(prk.lib(), "prk_advance_edge_lists")
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT prk_advance_edge_lists$", out, re.M)
    assert hasattr(prk.Renderer, "advance_edge_lists")


def test_advance_lists_null_context():
    L = prk.lib()
    rec = np.zeros((2, 27), np.uint32)
    out = np.full((2, 27), 0xA5A5A5A5, np.uint32)
    nxt = np.full(2, 77, np.int32)
    cnt = np.array([2], np.uint32)
    assert L.prk_advance_edge_lists(None, None, None, 0, 64, None, None) == abi.PRK_ERR_ARG
    assert L.prk_advance_edge_lists(None, rec.ctypes.data, cnt.ctypes.data, 1, 64, out.ctypes.data,
                                    nxt.ctypes.data) == abi.PRK_ERR_ARG
    assert (out == 0xA5A5A5A5).all() and (nxt == 77).all()  # nothing written


def test_nan_rule_of_the_gpu_tests():
    """The one comparison helper of tests/test_gpu_advance_lists.py: a NaN
    passes for the host's NaN only, every other word must be equal."""
    from test_gpu_advance_lists import same_words
    a = np.zeros((2, 27), np.uint32)
    b = a.copy()
    a[1, 21], b[1, 21] = 0xFFC00000, 0x7FC00001  # both NaNs: allowed
    same_words(b, a, "nan for nan")
    b[0, 22] = 0x7FC00000  # a NaN the host does not have
    with pytest.raises(AssertionError):
        same_words(b, a, "nan for number")
    b[0, 22], b[1, 21] = 0, 0x3F800000  # a number for the host's NaN
    with pytest.raises(AssertionError):
        same_words(b, a, "number for nan")
    b[1, 21], b[1, 13] = 0x7FC00000, 1  # an unequal number
    with pytest.raises(AssertionError):
        same_words(b, a, "unequal")
    b[1, 13], a[0, 7], b[0, 7] = 0, 0x7FC00000, 0x7FC00001  # YMin is an integer: no allowance
    with pytest.raises(AssertionError):
        same_words(b, a, "integer word")


@pytest.mark.skipif(os.environ.get("PRK_EXPECT_GPU") == "1", reason="GPU box")
def test_advance_lists_fail_loudly_without_gpu():
    """As the other compute calls (test_abi.py): no CPU fallback, the binding
    raises PRK_ERR_DEVICE."""
    if prk.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(prk.PrkError) as e:
        prk.Renderer().advance_edge_lists(np.zeros((2, 27), np.uint32), np.array([2], np.uint32), 64)
    assert e.value.code == abi.PRK_ERR_DEVICE
