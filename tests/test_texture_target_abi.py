"""CPU tests of the render-to-texture calls' boundary (no GPU compute): the
ctypes mirror against include/prk.h, the exported symbols, NULL contexts, and
the numpy restatement of the resolve (tests/texref.py) against the header's
expression one channel at a time.  What the pass computes is checked on the
GPU (tests/test_gpu_texture_target.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prk
import texref
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prk_texture_alloc", "prk_texture_from_target", "prk_texture_download", "prk_texture_info")

CTYPES = {"prk_context *": C.c_void_p, "int32_t": C.c_int32, "void *": C.c_void_p, "int32_t *": C.POINTER(C.c_int32)}


def header():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_four_names_are_exported():
    assert sorted(abi.TEXTURE_TARGET_SIGS) == sorted(NAMES)
    for name in NAMES:
        assert name in prk.exported_symbols(), name


@pytest.mark.parametrize("name", NAMES)
def test_signature_declared_exported_bound(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header(), re.M | re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    types = [re.match(r"(.*?[ *])\w+$", p).group(1).strip() for p in params]
    assert [CTYPES[t] for t in types] == abi.TEXTURE_TARGET_SIGS[name], (name, types)
    f = getattr(prk.lib(), name)
    assert f.restype is C.c_int and list(f.argtypes) == abi.TEXTURE_TARGET_SIGS[name]
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT %s$" % name, out, re.M)


def test_python_surface_and_null_context():
    for m in ("texture_alloc", "texture_from_target", "texture_download", "texture_info"):
        assert hasattr(prk.Renderer, m)
    L = prk.lib()
    h = C.c_int32(5)
    w = C.c_int32(7)
    buf = np.full((4, 4), 9, np.uint32)
    assert L.prk_texture_alloc(None, 4, 4, C.byref(h)) == abi.PRK_ERR_ARG and h.value == 5
    assert L.prk_texture_from_target(None, 0, 0, 0, 4, 4, 1, 0, 0) == abi.PRK_ERR_ARG
    assert L.prk_texture_download(None, 0, buf.ctypes.data, 16) == abi.PRK_ERR_ARG and (buf == 9).all()
    assert L.prk_texture_info(None, 0, C.byref(w), None, None) == abi.PRK_ERR_ARG and w.value == 7


def test_texref_against_the_expression_channel_by_channel():
    rng = np.random.default_rng(1)
    px = rng.integers(0, 2**32, (8, 12), dtype=np.uint64).astype(np.uint32)
    px[0:4, 0:4] = 0xFFFFFFFF  # every channel's sum at its maximum
    px[4:8, 0:4] = 0
    assert np.array_equal(texref.resolve(px, 1), px)
    for f, shift in ((2, 2), (4, 4)):
        got = texref.resolve(px, f)
        assert got.shape == (8 // f, 12 // f)
        for y in range(8 // f):
            for x in range(12 // f):
                word = 0
                for c in range(4):
                    s = sum((int(px[f * y + j, f * x + i]) >> (8 * c)) & 255 for j in range(f) for i in range(f))
                    word |= ((s + f * f // 2) >> shift) << (8 * c)
                assert int(got[y, x]) == word, (f, y, x)
        assert got[0, 0] == 0xFFFFFFFF and got[4 // f, 0] == 0
    # rounding: a channel sum of 2 of 4 rounds up to 1, 1 of 4 down to 0; 8 of 16 up, 7 of 16 down
    one = np.zeros((4, 4), np.uint32)
    one[0, 0] = one[0, 1] = 0x01000100
    assert texref.resolve(one, 2)[0, 0] == 0x01000100
    one[0, 1] = 0
    assert texref.resolve(one, 2)[0, 0] == 0
    half = np.zeros((4, 4), np.uint32)
    half.reshape(-1)[:8] = 0x00010001
    assert texref.resolve(half, 4)[0, 0] == 0x00010001
    half.reshape(-1)[7] = 0
    assert texref.resolve(half, 4)[0, 0] == 0


def test_texref_rectangles():
    rng = np.random.default_rng(2)
    band = rng.integers(0, 2**32, (8, 16), dtype=np.uint64).astype(np.uint32)
    tex = rng.integers(0, 2**32, (7, 9), dtype=np.uint64).astype(np.uint32)
    out = texref.from_target(band, 16, (3, 18, 4, 6), 2, tex, (5, 1))
    assert np.array_equal(out[1:4, 5:7], texref.resolve(band[2:8, 3:7], 2))
    keep = np.ones(tex.shape, bool)
    keep[1:4, 5:7] = False
    assert np.array_equal(out[keep], tex[keep]) and out is not tex
    for bad in ((3, 15, 4, 2), (3, 22, 4, 4), (14, 18, 4, 2)):  # a row above the band, one below, a column past W
        with pytest.raises(AssertionError):
            texref.from_target(band, 16, bad, 2, tex)
