"""CPU tests of the handle record walks' C-ABI boundary (no GPU compute): the
entry points include/prk.h declares are exported with the declared argument
counts, bound, named in abi.py and present on Records, and refuse a NULL
context before they touch a device.  What they compute is checked on the GPU
(tests/test_gpu_record_walks.py).
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


def declaration(name):
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        m = re.search(r"^int %s\((prk_context \*ctx, [^;]*)\);" % name, f.read(), re.M)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(abi.RECORD_WALK_ARGS))
def test_symbol_declared_exported_bound(name):
    nargs = abi.RECORD_WALK_ARGS[name]
    assert len(declaration(name)) == nargs
    assert name in prk.exported_symbols()
    f = getattr(prk.lib(), name)
    assert len(f.argtypes) == nargs and f.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT %s$" % name, out, re.M)


def test_python_surface():
    assert sorted(abi.RECORD_WALK_ARGS) == ["prk_debug_list_stats", "prk_records_advance", "prk_records_rows",
                                            "prk_records_spans"]
    for m in ("advance", "spans", "rows", "list_stats"):
        assert hasattr(prk.Records, m)
    assert abi.LIST_STATS_FIELDS == ("edge_rows", "scans", "most", "ymin0", "ymax_max")


def test_null_context():
    L = prk.lib()
    rec, nxt = np.full((2, 27), 7, np.uint32), np.full(2, 7, np.int32)
    cnt = np.full(1, 7, np.uint32)
    h, t, u = C.c_int32(5), C.c_uint64(9), C.c_uint64(9)
    stats = np.full(5, 7, np.uint64)
    assert L.prk_records_advance(None, 0, 0, 1, 64, C.byref(h), rec.ctypes.data, nxt.ctypes.data) == abi.PRK_ERR_ARG
    assert L.prk_records_advance(None, 0, 0, 0, 64, None, None, None) == abi.PRK_ERR_ARG
    assert L.prk_records_spans(None, 0, 0, 1, 64, rec.ctypes.data, 2, cnt.ctypes.data, C.byref(t)) == abi.PRK_ERR_ARG
    assert L.prk_records_spans(None, 0, 0, 1, 64, None, 0, None, None) == abi.PRK_ERR_ARG
    assert L.prk_records_rows(None, 0, 0, 1, 64, rec.ctypes.data, 2, rec.ctypes.data, 2, cnt.ctypes.data,
                              C.byref(t), C.byref(u)) == abi.PRK_ERR_ARG
    assert L.prk_debug_list_stats(None, 0, 0, 1, 64, stats.ctypes.data) == abi.PRK_ERR_ARG
    assert (rec == 7).all() and (nxt == 7).all() and cnt[0] == 7 and (stats == 7).all()
    assert (h.value, t.value, u.value) == (5, 9, 9)
