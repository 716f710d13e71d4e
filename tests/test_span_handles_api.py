"""CPU tests of the span handles' C-ABI boundary (no GPU compute): every entry
point include/prk.h declares is exported, bound and present on Renderer /
Spans, and refuses a NULL context before it touches a device.  What the
handles hold and draw is checked on the GPU (tests/test_gpu_span_handles.py).
"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import prk
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["prk_spans_from_records", "prk_spans_upload", "prk_spans_upload_rows", "prk_spans_info",
           "prk_spans_lists", "prk_spans_download", "prk_spans_destroy", "prk_draw_span_records"]


def test_span_handle_symbols_are_the_abi_list():
    assert sorted(abi.SPAN_HANDLE_ARGS) == sorted(SYMBOLS)


@pytest.mark.parametrize("name", SYMBOLS)
def test_span_handle_symbol_declared_exported_bound(name):
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        m = re.search(r"^int %s\(prk_context \*ctx, ([^;]*)\);" % name, f.read(), re.M | re.S)
    assert m, name
    assert m.group(1).count(",") + 2 == abi.SPAN_HANDLE_ARGS[name]  # (ctx and the rest)
    assert name in prk.exported_symbols()
    f = getattr(prk.lib(), name)
    assert f.restype is C.c_int and len(f.argtypes) == abi.SPAN_HANDLE_ARGS[name]
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT %s$" % name, out, re.M)


def test_span_handle_python_surface():
    for m in ("spans_upload", "spans_upload_rows", "draw_span_records"):
        assert hasattr(prk.Renderer, m)
    for m in ("counts", "download", "close"):
        assert hasattr(prk.Spans, m)
    assert "total" in inspect.getsource(prk.Spans.__init__)
    sig = inspect.signature(prk.Records.spans)
    assert sig.parameters["keep"].default is False  # (the default is the host arrays, as before)
    sig = inspect.signature(prk.Renderer.draw_span_records)
    assert [p for p in sig.parameters][1:] == ["sp", "first_span", "span_count", "semantics", "bitmap", "phong"]
    assert sig.parameters["semantics"].default == abi.PRK_SEM_AVX and sig.parameters["phong"].default is True


def test_span_handle_null_context():
    L = prk.lib()
    spans = np.zeros((2, 25), np.uint32)
    rows = np.array([[0, 2]], np.int32)
    pairs = np.zeros((2, 24), np.uint32)
    cnt = np.zeros(1, np.uint32)
    h, n, t = C.c_int32(5), C.c_uint32(0), C.c_uint64(0)
    assert L.prk_spans_from_records(None, 0, 0, 1, 64, C.byref(h), cnt.ctypes.data, C.byref(t)) == abi.PRK_ERR_ARG
    assert L.prk_spans_from_records(None, 0, 0, 0, 64, C.byref(h), None, None) == abi.PRK_ERR_ARG
    assert L.prk_spans_upload(None, spans.ctypes.data, 2, C.byref(h)) == abi.PRK_ERR_ARG
    assert L.prk_spans_upload(None, None, 0, C.byref(h)) == abi.PRK_ERR_ARG
    assert L.prk_spans_upload_rows(None, rows.ctypes.data, 1, pairs.ctypes.data, 2, C.byref(h)) == abi.PRK_ERR_ARG
    assert L.prk_spans_upload_rows(None, None, 0, None, 0, C.byref(h)) == abi.PRK_ERR_ARG
    assert L.prk_spans_info(None, 0, C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
    assert L.prk_spans_lists(None, 0, cnt.ctypes.data) == abi.PRK_ERR_ARG
    assert L.prk_spans_download(None, 0, spans.ctypes.data, 2) == abi.PRK_ERR_ARG
    assert L.prk_spans_destroy(None, 0) == abi.PRK_ERR_ARG
    assert L.prk_draw_span_records(None, 0, 0, 1, abi.PRK_SEM_AVX, 1, 0) == abi.PRK_ERR_ARG
    assert L.prk_draw_span_records(None, 0, 0, 0, abi.PRK_SEM_AVX, 1, 0) == abi.PRK_ERR_ARG
    assert h.value == 5  # (a NULL context is refused before anything is written)
