"""CPU tests of prk_edge_records' C-ABI boundary (no GPU compute): the entry
point include/prk.h declares is exported, bound, and checks its arguments
before it touches a device.  The records themselves are checked on the GPU
(tests/test_gpu_edge_records.py).
"""
import ctypes as C
import re
import subprocess

import prk
from prk import abi


def test_edge_records_symbol_exported():
    assert "prk_edge_records" in prk.exported_symbols()
    assert hasattr(prk.lib(), "prk_edge_records")
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT prk_edge_records$", out, re.M)
    assert hasattr(prk.Renderer, "edge_records")


def test_edge_records_null_arguments():
    L = prk.lib()
    total = C.c_uint64(7)
    # no context, no total_out: refused before anything is read
    assert L.prk_edge_records(None, 0, 0, 0, 1, None, 3, None, 0, None, C.byref(total)) == abi.PRK_ERR_ARG
    assert L.prk_edge_records(None, 0, 0, 0, 1, None, 3, None, 0, None, None) == abi.PRK_ERR_ARG
