"""CPU tests of prk_draw_edge_lists' C-ABI boundary (no GPU compute): the entry
point include/prk.h declares is exported, bound, and refuses a NULL context
before it touches a device.  The frames it draws are checked on the GPU
(tests/test_gpu_edge_lists.py).
"""
import os
import re
import subprocess

import numpy as np

import prk
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edge_lists_symbol_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        assert re.search(r"\bint prk_draw_edge_lists\(prk_context \*ctx, const prk_edge \*records, "
                         r"const uint32_t \*counts,\s+uint32_t list_count,", f.read())
    assert "prk_draw_edge_lists" in prk.exported_symbols()
    assert hasattr(prk.lib(), "prk_draw_edge_lists")
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT prk_draw_edge_lists$", out, re.M)
    assert hasattr(prk.Renderer, "draw_edge_lists")


def test_edge_lists_null_context():
    L = prk.lib()
    rec = np.zeros((2, 27), np.uint32)
    cnt = np.array([2], np.uint32)
    assert L.prk_draw_edge_lists(None, None, None, 0, abi.PRK_SEM_AVX, 1, 0) == abi.PRK_ERR_ARG
    assert L.prk_draw_edge_lists(None, rec.ctypes.data, cnt.ctypes.data, 1, abi.PRK_SEM_AVX, 1,
                                 0) == abi.PRK_ERR_ARG
