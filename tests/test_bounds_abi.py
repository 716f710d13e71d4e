"""CPU tests of the bounds occlusion test's boundary (no GPU compute): the six
symbols declared in include/prk.h, exported and bound with abi.BOUNDS_SIGS; the
prk_bound layout; a NULL context and NULL required pointers refused before any
device call; and the numpy restatement of the definition (tests/boundsref.py)
against a table worked by hand.  What the device computes is checked on the GPU
(tests/test_gpu_bounds.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boundsref as B
import prk
import pyref
import xform_ref as X
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prk_visibility_bounds", "prk_visibility_bounds_device", "prk_geometry_select_bounds", "prk_debug_ztiles",
         "prk_debug_bounds_ms", "prk_selftest_bounds")
STRUCTS = {"prk_select_item": abi.PrkSelectItem, "prk_select_level": abi.PrkSelectLevel, "prk_xform": abi.PrkXform,
           "prk_bound": abi.PrkBound, "prk_transform": abi.PrkTransform}
SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
f32 = np.float32


def header():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_names_are_exported():
    assert sorted(abi.BOUNDS_SIGS) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert name in prk.exported_symbols(), name
        assert re.search(r"\bT %s$" % name, out, re.M), name
    # the host functions and launchers' helpers that cross the host files stay out of the dynamic table
    for hidden in ("bounds_frame", "select_check"):
        assert not re.search(r"\b%s$" % hidden, out, re.M), hidden
    for method in ("visibility_bounds", "visibility_bounds_device", "geometry_select_bounds"):
        assert hasattr(prk.Renderer, method), method
    assert callable(prk.selftest_bounds)
    # the tables of the calls this one sits beside keep their names
    assert "prk_geometry_select_bounds" not in abi.SELECT_SIGS and "prk_visibility_bounds" not in abi.VISIBILITY_SIGS


@pytest.mark.parametrize("name", NAMES)
def test_signature_declared_and_bound(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header(), re.M | re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    sig = abi.BOUNDS_SIGS[name]
    assert len(params) == len(sig), (name, params)
    for p, t in zip(params, sig):
        decl = re.match(r"(.*?[ *])\w+$", p).group(1).strip()
        if not decl.endswith("*"):
            assert t is SCALARS[decl], (name, p, t)
            continue
        pointee = decl.replace("const ", "")[:-1].strip()
        if pointee in STRUCTS:  # a table or record: the mirrored struct
            assert t._type_ is STRUCTS[pointee], (name, p, t)
        elif t is not C.c_void_p:  # a typed scalar out (or the address of a device pointer)
            assert pointee.endswith("*") and t._type_ is C.c_void_p or t._type_ is SCALARS[pointee], (name, p, t)
        else:
            assert pointee in SCALARS or pointee == "prk_context", (name, p)
    f = getattr(prk.lib(), name)
    assert f.restype is C.c_int and list(f.argtypes) == sig


def test_struct_layout_matches_the_header():
    m = re.search(r"typedef struct prk_bound \{\s*float lo\[3\], hi\[3\];\s*uint32_t xform;\s*\} prk_bound;", header())
    assert m
    assert [f[0] for f in abi.PrkBound._fields_] == ["lo", "hi", "xform"]
    assert C.sizeof(abi.PrkBound) == 28 and abi.PrkBound.hi.offset == 12 and abi.PrkBound.xform.offset == 24
    packed = prk.pack_bounds([[1, 2, 3]], [[4, 5, 6]], [7])
    b = abi.PrkBound.from_buffer_copy(packed.tobytes())
    assert list(b.lo) == [1, 2, 3] and list(b.hi) == [4, 5, 6] and b.xform == 7


def test_null_context_and_null_pointers_are_refused():
    """PRK_ERR_ARG before any device call (there is no device here), nothing written."""
    L = prk.lib()
    ARG = abi.PRK_ERR_ARG
    bounds = prk.pack_bounds([[0, 0, 0]], [[1, 1, 1]], [0])
    xf = X.translation((0, 0, 0))[None].copy()
    bp = C.cast(bounds.ctypes.data, C.POINTER(abi.PrkBound))
    xp = C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform))
    px = np.full(1, 9, np.uint32)
    assert L.prk_visibility_bounds(None, bp, 1, xp, 1, None, px.ctypes.data) == ARG
    # a zeroed stand-in context (no camera, no target, no answer): the host checks come before any device call
    fake = (C.c_uint8 * 65536)()
    ctx = C.addressof(fake)
    assert L.prk_visibility_bounds(ctx, None, 1, xp, 1, None, px.ctypes.data) == ARG
    assert L.prk_visibility_bounds(ctx, bp, 1, None, 1, None, px.ctypes.data) == ARG
    assert L.prk_visibility_bounds(ctx, bp, 1, xp, 1, None, px.ctypes.data) == ARG  # (before any prk_set_camera)
    dp, n = C.c_void_p(5), C.c_uint32(5)
    assert L.prk_visibility_bounds_device(None, C.byref(dp), C.byref(n)) == ARG
    assert L.prk_visibility_bounds_device(ctx, None, C.byref(n)) == ARG
    assert L.prk_visibility_bounds_device(ctx, C.byref(dp), None) == ARG
    assert L.prk_visibility_bounds_device(ctx, C.byref(dp), C.byref(n)) == ARG  # (no answer)
    t = [C.c_int32(5) for _ in range(3)]
    assert L.prk_debug_ztiles(None, None, 0, *[C.byref(v) for v in t]) == ARG
    assert L.prk_debug_ztiles(ctx, None, 0, None, C.byref(t[1]), C.byref(t[2])) == ARG
    assert L.prk_debug_ztiles(ctx, None, 0, *[C.byref(v) for v in t]) == ARG
    a, b = C.c_float(3.0), C.c_float(3.0)
    assert L.prk_debug_bounds_ms(None, C.byref(a), C.byref(b)) == ARG
    assert L.prk_debug_bounds_ms(ctx, None, C.byref(b)) == ARG and L.prk_debug_bounds_ms(ctx, C.byref(a), None) == ARG
    assert L.prk_debug_bounds_ms(ctx, C.byref(a), C.byref(b)) == ARG
    items = np.array([[0, 0, 0, 1, 0]], np.uint32)
    levels = np.array([[0, 0, 1]], np.uint32)
    ip = C.cast(items.ctypes.data, C.POINTER(abi.PrkSelectItem))
    lp = C.cast(levels.ctypes.data, C.POINTER(abi.PrkSelectLevel))
    chosen, first, total = np.full(1, 9, np.int32), np.full(2, 9, np.uint32), C.c_uint64(7)
    tail = (chosen.ctypes.data, first.ctypes.data)
    assert L.prk_geometry_select_bounds(None, 0, 1, 0, ip, 1, lp, 1, xp, 1, *tail, C.byref(total)) == ARG
    assert L.prk_geometry_select_bounds(ctx, 0, 1, 0, ip, 1, lp, 1, xp, 1, *tail, None) == ARG
    assert L.prk_geometry_select_bounds(ctx, 0, 1, 0, None, 1, lp, 1, xp, 1, *tail, C.byref(total)) == ARG
    assert bytes(fake) == bytes(65536) and (px == 9).all() and (dp.value, n.value) == (5, 5)
    assert [v.value for v in t] == [5, 5, 5] and (a.value, b.value) == (3.0, 3.0)
    assert (chosen == 9).all() and (first == 9).all() and total.value == 7
    # the self-test: every pointer it needs, a device >= 0, a band inside the frame, xforms that cover the bounds
    z = np.zeros((8, 8), np.float32)
    zmin, dmg = np.full((1, 1), 9, np.float32), C.c_uint32(7)
    tr = abi.make_transform(2.0, 1.0, 8.0, 4.0, 4.0)
    good = [0, z.ctypes.data, 8, 8, 0, 8, 0, C.byref(tr), None, bp, 1, xp, 1, zmin.ctypes.data, px.ctypes.data,
            C.byref(dmg)]
    for k in (1, 7, 9, 11, 13, 14, 15):
        bad = list(good)
        bad[k] = None
        assert L.prk_selftest_bounds(*bad) == ARG, k
    for k, v in ((0, -1), (2, 0), (3, 0), (4, -1), (4, 8), (5, 9), (6, 1025), (12, 0)):
        bad = list(good)
        bad[k] = v
        assert L.prk_selftest_bounds(*bad) == ARG, (k, v)
    assert (zmin == 9).all() and (px == 9).all() and dmg.value == 7


# ---- boundsref itself -----------------------------------------------------------------------------------------------
CAM = (2.0, 1.0, 8.0, 8.0, 8.0)  # D, F, M2P, cx, cy: at z = 0, k = 1/2 and a unit of x is 4 pixels
ID = X.translation((0, 0, 0))[None]


def test_ztiles_on_a_hand_worked_band():
    """Rows 5 .. 13 of a 12-wide frame: tile row 0 holds rows 5-7, tile row 1 rows 8-13; tile column 1 is 4 wide."""
    z = np.full((9, 12), 1.0, f32)
    z[0, 3] = -2.0                       # row 5: tile (0, 0)
    z[2, 11] = np.nan                    # row 7: tile (1, 0), one NaN among ones
    z[3:, 0:8] = np.nan                  # rows 8-13 of tile (0, 1): all NaN
    z[8, 9] = -0.0                       # row 13: tile (1, 1)
    z[5, 10] = 1e-40                     # a denormal above it
    got = B.ztiles(z, 5)
    assert got.shape == (2, 2) and B.tile_shape(12, 5, 14) == (2, 2, 0)
    assert got.tolist() == [[-2.0, 1.0], [np.inf, 0.0]]
    z[8, 9] = 1e-40
    z[5, 10] = 2e-40
    assert B.ztiles(z, 5)[1, 1] == f32(1e-40) > 0  # denormals compare by value
    assert B.ztiles(np.full((1, 1), -np.inf, f32), 7).tolist() == [[-np.inf]]
    assert B.tile_shape(20, 3, 21) == (3, 3, 0) and B.tile_shape(8, 40, 200) == (20, 1, 5)


def test_projection_is_pyrefs():
    rng = np.random.default_rng(3)
    pts = X.random_values(rng, (64, 3))
    pts[:, 2] = rng.uniform(-3, 3, 64).astype(f32)

    class Cam:
        D, F, M2P, cx, cy = [f32(v) for v in CAM]

    px, py, front = B.project(CAM, pts)
    for i in range(64):
        want = pyref.project(Cam, [pts[i, 0], pts[i, 1], pts[i, 2]])
        if front[i]:
            assert (px[i], py[i]) == (want[0], want[1]) and want[2] > f32(0.2)
        else:
            assert want == [0, 0, 0]
    assert front.any() and not front.all()


def test_boundsref_on_a_hand_worked_table():
    """A 16 x 16 target, four tiles.  At z = 0 a point x lands on pixel 8 + 4x."""
    tiny = np.nextafter(f32(0), f32(1))
    zmin = np.array([[-1.0, 0.0], [0.5, tiny]], f32)
    z = np.repeat(np.repeat(zmin, 8, 0), 8, 1)
    assert np.array_equal(B.ztiles(z, 0), zmin)
    lo = np.array([[0.1, 0.1, 0.0],     # px, py in 8.4 .. 9.2: rect [7, 11)^2 over all four tiles, znear 0
                   [0.5, 0.5, -1.0],    # a point at z = -1: d = 3, px = 8 + 8 * (0.5 / 3) = 9.33: rect [8, 11)^2, one tile
                   [0.0, 0.0, 1.9],     # d = 0.1: behind the camera's plane, the whole band
                   [5.0, 0.0, 0.0],     # px = 28: off the right edge
                   [0.3, 0.3, 0.0]], f32)   # item 0 with lo and hi exchanged
    hi = np.array([[0.3, 0.3, 0.0], [0.5, 0.5, -1.0], [0.0, 0.0, 1.9], [5.0, 0.0, 0.0], [0.1, 0.1, 0.0]], f32)
    bx = B.boxes(lo, hi, np.zeros(5, int), ID, None, CAM, 16, 0, 16)
    assert bx.rect.tolist() == [[7, 11, 7, 11], [8, 11, 8, 11], [0, 16, 0, 16], [16, 16, 7, 10], [7, 11, 7, 11]]
    assert bx.whole.tolist() == [False, False, True, False, False]
    assert bx.znear.tolist() == [0.0, -1.0, f32(1.9), 0.0, 0.0]
    got = B.pixels_of(bx, zmin, 0)
    # item 0: tile (0,0) 1 px, znear 0 >= -1 passes; tile (1,0) 3 px, 0 == 0 passes (equality);
    #         tile (0,1) 3 px, 0 < 0.5 fails; tile (1,1) 9 px, 0 < the smallest positive float fails
    # item 1: 9 px of tile (1,1), -1 < tiny fails; item 2: znear 1.9 passes everywhere
    assert got.tolist() == [4, 0, 256, 0, 4]
    assert B.pixels(lo, hi, np.zeros(5, int), ID, None, CAM, z, 0).tolist() == got.tolist()
    # P moves the box as a draw's P does: item 1 lifted to z = 0.5 passes tile (1,1) ...
    up = B.boxes(lo[1:2], hi[1:2], [0], ID, (0.0, 0.0, 1.5), CAM, 16, 0, 16)
    assert up.znear.tolist() == [0.5] and B.pixels_of(up, zmin, 0)[0] > 0
    # ... a band of rows 8 .. 16 answers on its own rows: item 0 keeps tiles (0,1) and (1,1), 3 rows of them
    band = B.boxes(lo[:1], hi[:1], [0], ID, None, CAM, 16, 8, 16)
    assert band.rect.tolist() == [[7, 11, 8, 11]]
    assert B.pixels_of(band, np.array([[-1.0, 0.0]], f32), 1).tolist() == [12]
    # a NaN in the matrix: the whole band, and a NaN znear passes every tile
    bad = ID.copy()
    bad[0, 2, 2] = np.nan
    nb = B.boxes(lo[:1], hi[:1], [0], bad, None, CAM, 16, 0, 16)
    assert nb.whole.tolist() == [True] and np.isnan(nb.znear[0])
    assert B.pixels_of(nb, np.full((2, 2), np.inf, f32), 0).tolist() == [256]
