"""CPU tests of the visibility-feedback calls' boundary (no GPU compute): the
six symbols declared in include/prk.h, exported and bound with
abi.VISIBILITY_SIGS; NULL contexts and NULL required pointers refused before
any device call; and the numpy restatement of the definition
(tests/visref.py) on the oracle's winner map of the smoke scene.  What the
device computes is checked on the GPU (tests/test_gpu_visibility.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import prk
import visref
from prk import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prk_visibility_info", "prk_visibility_counts", "prk_visibility_groups", "prk_visibility_ids",
         "prk_visibility_device", "prk_selftest_visibility")
METHODS = ("visibility", "visibility_counts", "visibility_groups", "visibility_ids", "visibility_device")
POINTERS = (C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p))
SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


def header():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def smoke_scene():
    return scenes.random_soup(3000, 256, 256, radius=16, seed=123)


def test_the_six_names_are_exported():
    assert sorted(abi.VISIBILITY_SIGS) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert name in prk.exported_symbols(), name
        assert re.search(r"\bT %s$" % name, out, re.M), name
    for m in METHODS:
        assert hasattr(prk.Renderer, m), m
    assert callable(prk.selftest_visibility)


@pytest.mark.parametrize("name", NAMES)
def test_signature_declared_and_bound(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header(), re.M | re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    sig = abi.VISIBILITY_SIGS[name]
    assert len(params) == len(sig), (name, params)
    for p, t in zip(params, sig):
        decl = re.match(r"(.*?[ *])\w+$", p).group(1).strip()
        if decl.endswith("*"):
            assert t in POINTERS, (name, p, t)
            if t is not C.c_void_p:  # a typed scalar out: the pointee as declared
                pointee = decl.replace("const ", "")[:-1].strip()
                want = C.c_void_p if pointee.endswith("*") else SCALARS[pointee]
                assert t._type_ is want, (name, p, t)
        else:
            assert t is SCALARS[decl], (name, p, t)
    f = getattr(prk.lib(), name)
    assert f.restype is C.c_int and list(f.argtypes) == sig


def test_null_context_and_null_pointers_are_refused():
    """PRK_ERR_ARG before any device call (there is no device here), and
    nothing written -- except prk_visibility_ids' total, as its sizing
    pattern says."""
    L = prk.lib()
    n32, n64, v32 = C.c_uint32(7), C.c_uint64(7), C.c_uint32(7)
    buf = np.full(8, 9, np.uint32)
    starts = np.array([0, 1, 2], np.uint32)
    p0, p1 = C.c_void_p(5), C.c_void_p(5)
    bp, sp = buf.ctypes.data, starts.ctypes.data
    ARG = abi.PRK_ERR_ARG
    assert L.prk_visibility_info(None, C.byref(n32), C.byref(n64), C.byref(v32)) == ARG
    assert L.prk_visibility_counts(None, 0, 4, bp) == ARG
    assert L.prk_visibility_groups(None, sp, 2, bp, bp) == ARG
    assert L.prk_visibility_ids(None, bp, 8, C.byref(n64)) == ARG
    assert L.prk_visibility_device(None, C.byref(p0), C.byref(p1), C.byref(n32)) == ARG
    # a context that is never looked at: the pointer checks come first
    fake = (C.c_uint8 * 64)()
    ctx = C.addressof(fake)
    for args in ((None, C.byref(n64), C.byref(v32)), (C.byref(n32), None, C.byref(v32)),
                 (C.byref(n32), C.byref(n64), None)):
        assert L.prk_visibility_info(ctx, *args) == ARG
    assert L.prk_visibility_counts(ctx, 0, 4, None) == ARG
    assert L.prk_visibility_groups(ctx, None, 2, bp, bp) == ARG
    assert L.prk_visibility_groups(ctx, sp, 2, None, None) == ARG
    assert L.prk_visibility_ids(ctx, bp, 8, None) == ARG
    for args in ((None, C.byref(p1), C.byref(n32)), (C.byref(p0), None, C.byref(n32)), (C.byref(p0), C.byref(p1), None)):
        assert L.prk_visibility_device(ctx, *args) == ARG
    assert (n32.value, n64.value, v32.value, p0.value, p1.value) == (7, 7, 7, 5, 5) and (buf == 9).all()
    assert bytes(fake) == bytes(64)
    # the self-test: every pointer it needs, a device >= 0, id_count inside the numbering
    w = np.zeros(8, np.int32)
    outs = [np.full(9, 9, np.uint32) for _ in range(4)]
    good = [0, 8, w.ctypes.data, 8] + [o.ctypes.data for o in outs] + [C.byref(v32), C.byref(n64), C.byref(n32)]
    for k in (2, 4, 5, 6, 7, 8, 9, 10):
        bad = list(good)
        bad[k] = None
        assert L.prk_selftest_visibility(*bad) == ARG, k
    assert L.prk_selftest_visibility(*([-1] + good[1:])) == ARG
    assert L.prk_selftest_visibility(*(good[:3] + [0xFFFFFFF1] + good[4:])) == ARG
    assert all((o == 9).all() for o in outs) and (n32.value, n64.value, v32.value) == (7, 7, 7)


# ---- visref itself -----------------------------------------------------------------------------------------------------
def test_visref_on_a_hand_made_map():
    w = np.array([[-1, 2, 2, 5], [2, 0, 7, -3], [5, 5, 5, 5]], np.int32)
    v = visref.reduce(w, 7)  # (7 and -3 are outside the numbering)
    assert v.counts.tolist() == [1, 0, 3, 0, 0, 5, 0]
    assert v.pix_prefix.tolist() == [0, 1, 1, 4, 4, 4, 9, 9] and v.vis_prefix.tolist() == [0, 1, 1, 2, 2, 2, 3, 3]
    assert v.ids.tolist() == [0, 2, 5] and (v.covered, v.visible) == (9, 3)
    pix, vis = visref.groups(v, [0, 0, 3, 7, 7])
    assert pix.tolist() == [0, 4, 5, 0] and vis.tolist() == [0, 2, 1, 0]
    assert visref.runs_of(w, 2) == 2 and visref.runs_of(w, 4) == 1 and visref.runs_of(w, 1) == 8
    empty = visref.reduce(w, 0)
    assert empty.counts.shape == (0,) and empty.pix_prefix.tolist() == [0] and empty.covered == 0


def test_visref_patterns_are_what_their_names_say():
    for n in visref.SIZES:
        for m in visref.ID_COUNTS:
            for name, make in visref.PATTERNS.items():
                w = make(n, m)
                assert w.dtype == np.int32 and w.shape == (n,), (name, n, m)
            assert visref.reduce(visref.PATTERNS["none"](n, m), m).covered == 0
            assert visref.reduce(visref.PATTERNS["last_id"](n, m), m).counts[m - 1] == n
            assert visref.runs_of(visref.PATTERNS["alternating"](n, m), 2) == 0
            if n >= 4:
                assert visref.runs_of(visref.PATTERNS["spanning_run"](n, m), n - 2) == 1
    w = visref.PATTERNS["outside"](4097, 65)
    assert {-2, 65, visref.INT32_MAX, visref.INT32_MIN} <= set(w.tolist())
    assert visref.reduce(w, 65).covered == int(((w == 0) | (w == 64)).sum())
    w = visref.PATTERNS["runs"](65539, 65)
    for head in (63, 64, 252, 255, 256, 4096):
        assert w[head] != w[head - 1], head


def test_smoke_scene_in_the_oracle():
    """The numbers of the smoke scene's frame, from the oracle alone."""
    s = smoke_scene()
    win = O.render(s, semantics=abi.PRK_SEM_AVX, phong=True)[2]
    v = visref.reduce(win, s.tri_count)
    assert s.tri_count == 3000
    assert (v.covered, v.visible, s.tri_count - v.visible, int(v.counts.max())) == (61189, 2067, 933, 339)
    assert v.covered == int((win >= 0).sum()) and np.array_equal(v.ids, np.unique(win[win >= 0]))
