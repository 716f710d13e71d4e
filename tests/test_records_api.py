"""CPU tests of the record handles' C-ABI boundary (no GPU compute): every
entry point include/prk.h declares is exported, bound and present on
Renderer, and refuses a NULL context before it touches a device.  What the
handles hold and draw is checked on the GPU (tests/test_gpu_records.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prk
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["prk_records_from_geometry", "prk_records_upload", "prk_records_info", "prk_records_lists",
           "prk_records_download", "prk_records_destroy", "prk_draw_records", "prk_debug_stage_bytes"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_records_symbol_declared_exported_bound(name):
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        assert re.search(r"^int %s\(prk_context \*ctx, " % name, f.read(), re.M)
    assert name in prk.exported_symbols()
    assert hasattr(prk.lib(), name)
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT %s$" % name, out, re.M)


def test_records_python_surface():
    for m in ("records_from_geometry", "records_upload", "draw_records", "stage_bytes"):
        assert hasattr(prk.Renderer, m)
    for m in ("counts", "sorted_flags", "download", "close"):
        assert hasattr(prk.Records, m)


def test_records_null_context():
    L = prk.lib()
    rec = np.zeros((2, 27), np.uint32)
    cnt = np.array([2], np.uint32)
    P = (C.c_float * 3)(0.0, 0.0, 0.0)
    h, n, t = C.c_int32(5), C.c_uint32(0), C.c_uint64(0)
    assert L.prk_records_from_geometry(None, 0, 0, 1, 1, P, 3, C.byref(h), C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
    assert L.prk_records_upload(None, rec.ctypes.data, cnt.ctypes.data, 1, C.byref(h)) == abi.PRK_ERR_ARG
    assert L.prk_records_info(None, 0, C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
    assert L.prk_records_lists(None, 0, cnt.ctypes.data, cnt.ctypes.data) == abi.PRK_ERR_ARG
    assert L.prk_records_download(None, 0, rec.ctypes.data, 2) == abi.PRK_ERR_ARG
    assert L.prk_records_destroy(None, 0) == abi.PRK_ERR_ARG
    assert L.prk_draw_records(None, 0, 0, 1, abi.PRK_SEM_AVX, 1, 0) == abi.PRK_ERR_ARG
    assert L.prk_draw_records(None, 0, 0, 0, abi.PRK_SEM_AVX, 1, 0) == abi.PRK_ERR_ARG
    assert L.prk_debug_stage_bytes(None, C.byref(t)) == abi.PRK_ERR_ARG
