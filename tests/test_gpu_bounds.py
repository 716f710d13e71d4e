"""GPU tests: the bounds occlusion test (include/prk.h prk_visibility_bounds,
prk_geometry_select_bounds; csrc/prk_bounds.hip) -- a min-z tile map of the
target, every item's bounding box tested against it on the device, and the
select call that consumes the answer there.

Expected words come from tests/boundsref.py (the definition in numpy float32)
and, for the select call, tests/selectref.py; every word is compared.  The
self-test runs the two kernels on hand-made targets and boxes whose shapes sit
on the constants of the code: tiles of 8 x 8, a lane's 4 pixels, the 8 or 32
tiles of a wave, the 64 tiles of a trip of the test kernel.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import boundsref as B
import oracle as O
import prk
import selectref as S
import test_gpu_select as TS
import xform_ref as X
from prk import abi

pytestmark = pytest.mark.gpu

f32 = np.float32
FLT_MAX = np.finfo(f32).max
AVX, AVX_ST = abi.PRK_SEM_AVX, abi.PRK_SEM_AVX_ST
same, same_words = TS.same, TS.same_words


def same_values(got, want, label):
    """float arrays equal by value (-0.0 == +0.0; no NaN is expected on either side)."""
    assert not np.isnan(got).any() and not np.isnan(want).any(), label
    same(got, want, label)


# ---- 1. the tile map alone -------------------------------------------------------------------------------------------
ROWS = [(0, 8), (0, 9), (3, 21), (5, 6)]
CAM0 = abi.make_transform(2.0, 1.0, 8.0, 4.0, 4.0)


def fill_z(rng, rows, W, row0, nan_tile):
    z = rng.uniform(-2.0, 2.0, (rows, W)).astype(f32)
    special = np.array([-FLT_MAX, 0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan], f32)  # (1e-40: a denormal)
    at = rng.choice(rows * W, special.size, replace=False)
    z.reshape(-1)[at] = special  # the one NaN shares its tile with numbers: rows * W >= 8 > 1
    if nan_tile:  # the map's first tile, every word
        z[:8 * (row0 // 8 + 1) - row0, :8] = np.nan
    return z


@pytest.mark.parametrize("W", [8, 16, 20, 24, 264])
def test_tile_map(gpu, W):
    rng = np.random.default_rng(W)
    for row0, row1 in ROWS:
        for off in (0, 1):
            for nan_tile in (False, True):
                z = fill_z(rng, row1 - row0, W, row0, nan_tile)
                got = prk.selftest_bounds(z, row0, 24, CAM0, np.zeros((0, 7), f32), None, z_offset=off)
                label = ("W", W, "rows", row0, row1, "offset", off, "nan tile", nan_tile)
                assert got["damage"] == 0, label
                want = B.ztiles(z, row0)
                same_values(got["zmin"], want, label)
                if nan_tile:
                    assert got["zmin"][0, 0] == np.inf


# ---- 2. the test kernel alone ------------------------------------------------------------------------------------------
CAM = (2.0, 1.0, 128.0, 128.0, 128.0)
P = (0.02, -0.01, 0.03)
NAN_ROW0, NAN_ROW2 = X.translation((0, 0, 0)), X.translation((0, 0, 0))
NAN_ROW0[0, 1] = np.nan
NAN_ROW2[2, 0] = np.nan
XFORMS = np.stack([X.translation((0.01, -0.02, 0.0)), X.rotation_yx(2.0, -1.0, (0.0, 0.0, 0.05)),
                   X.translation((0.0, 0.0, -0.1)), NAN_ROW0, NAN_ROW2])
POOL = 4097


def flat_box(px0, px1, py0, py1, z):
    """lo, hi of a box flat at model z whose corners land on those pixels through XFORMS[0] and P (float64 inverse)."""
    D, F, M2P, cx, cy = CAM
    zc = z + XFORMS[0][2, 3] + P[2]
    k = F / (D - zc)
    x = [(p - cx) / (M2P * k) - XFORMS[0][0, 3] - P[0] for p in (px0, px1)]
    y = [(p - cy) / (M2P * k) - XFORMS[0][1, 3] - P[1] for p in (py0, py1)]
    return [x[0], y[0], z], [x[1], y[1], z]


def tiles_of(rect):
    x0, x1, y0, y1 = rect
    return 0 if x0 >= x1 or y0 >= y1 else ((x1 + 7) // 8 - x0 // 8) * ((y1 + 7) // 8 - y0 // 8)


@pytest.fixture(scope="module")
def pool():
    """4097 boxes on a 256 x 256 target, the named cases first, and what the definition gives for them."""
    rng = np.random.default_rng(77)
    named = [("off right", flat_box(300.5, 320.5, 100.5, 120.5, 0.0), 0, 0),
             ("off left", flat_box(-50.5, -20.5, 100.5, 120.5, 0.0), 0, 0),
             ("one tile", flat_box(17.5, 19.5, 17.5, 19.5, 0.1), 0, 1),
             ("lo and hi exchanged", flat_box(17.5, 19.5, 17.5, 19.5, 0.1)[::-1], 0, 1),
             ("63 tiles", flat_box(1.5, 68.5, 1.5, 52.5, 0.2), 0, 63),
             ("64 tiles", flat_box(1.5, 60.5, 1.5, 60.5, 0.2), 0, 64),
             ("65 tiles", flat_box(1.5, 100.5, 1.5, 36.5, 0.2), 0, 65),
             ("the whole map", flat_box(-10.5, 300.5, -10.5, 300.5, -0.3), 0, 1024),
             ("clipped left", flat_box(-20.5, 30.5, 100.5, 120.5, 0.3), 0, 4 * 4),
             ("clipped right", flat_box(230.5, 300.5, 100.5, 120.5, 0.3), 0, 4 * 4),
             ("clipped top", flat_box(100.5, 120.5, -20.5, 30.5, 0.3), 0, 4 * 4),
             ("clipped bottom", flat_box(100.5, 120.5, 230.5, 300.5, 0.3), 0, 4 * 4),
             ("behind the camera", ([-0.1, -0.1, 2.5], [0.1, 0.1, 2.6]), 0, 1024),
             ("reaching behind the camera", ([-0.1, -0.1, 0.0], [0.1, 0.1, 2.6]), 2, 1024),
             ("NaN in the matrix's x row", flat_box(17.5, 19.5, 17.5, 19.5, 0.1), 3, 1024),
             ("NaN in the matrix's z row", flat_box(17.5, 19.5, 17.5, 19.5, 0.1), 4, 1024),
             ("equal to zmin", flat_box(130.5, 150.5, 130.5, 150.5, 0.25), 0, 9),
             ("one ulp below zmin", flat_box(170.5, 190.5, 130.5, 150.5, 0.25), 0, 9)]
    lo = np.zeros((POOL, 3), f32)
    hi = np.zeros((POOL, 3), f32)
    xf = rng.integers(0, 3, POOL)
    for i, (_, (a, b), x, _) in enumerate(named):
        lo[i], hi[i], xf[i] = a, b, x
    n0 = len(named)
    c = np.stack([rng.uniform(-2.2, 2.2, POOL - n0), rng.uniform(-2.2, 2.2, POOL - n0),
                  rng.uniform(-0.8, 0.6, POOL - n0)], 1)
    half = rng.uniform(0.0, 0.25, (POOL - n0, 3)) * (rng.random((POOL - n0, 1)) < 0.7)
    lo[n0:], hi[n0:] = c - half, c + half
    bx = B.boxes(lo, hi, xf, XFORMS, P, CAM, 256, 0, 256)
    for i, (name, _, _, tiles) in enumerate(named):
        assert tiles_of(bx.rect[i].tolist()) == tiles, (name, bx.rect[i].tolist())
    names = [n for n, _, _, _ in named]
    # the target: blocks of 16 x 16 at one depth and a little noise, so that tiles pass and fail
    z = np.repeat(np.repeat(rng.uniform(-1.0, 0.7, (16, 16)), 16, 0), 16, 1) + rng.uniform(0.0, 0.01, (256, 256))
    z = z.astype(f32)
    eq, below = names.index("equal to zmin"), names.index("one ulp below zmin")
    for i, v in ((eq, bx.znear[eq]), (below, np.nextafter(bx.znear[below], f32(np.inf)))):
        x0, x1, y0, y1 = bx.rect[i].tolist()
        z[8 * (y0 // 8):8 * ((y1 + 7) // 8), 8 * (x0 // 8):8 * ((x1 + 7) // 8)] = v
    zmin = B.ztiles(z, 0)
    want = B.pixels_of(bx, zmin, 0)
    area = (bx.rect[:, 1] - bx.rect[:, 0]) * (bx.rect[:, 3] - bx.rect[:, 2])
    assert want[eq] == area[eq] > 0 and want[below] == 0  # equality passes, one ulp below does not
    assert want[names.index("NaN in the matrix's z row")] == 65536 and np.isnan(bx.znear[names.index(
        "NaN in the matrix's z row")])
    assert bx.whole[names.index("NaN in the matrix's x row")] and bx.whole[names.index("reaching behind the camera")]
    assert want[names.index("off right")] == want[names.index("off left")] == 0
    assert want[names.index("one tile")] == want[names.index("lo and hi exchanged")]
    rest = want[n0:]
    assert (rest == 0).sum() > 300 and (rest > 0).sum() > 1000 and set(xf[n0:].tolist()) == {0, 1, 2}
    partly = (want > 0) & (want < area)
    assert partly.sum() > 200  # boxes some of whose tiles pass and some fail
    return prk.pack_bounds(lo, hi, xf), z, zmin, want


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, POOL])
def test_bounds_kernel(gpu, pool, count):
    bounds, z, zmin, want = pool
    got = prk.selftest_bounds(z, 0, 256, abi.make_transform(*CAM), bounds[:count], XFORMS, P=P)
    assert got["damage"] == 0
    same_values(got["zmin"], zmin, "zmin")
    same(got["pixels"], want[:count], ("pixels", count))


def test_a_corner_exactly_at_the_projection_threshold(gpu):
    """D = 0.25 and a corner at camera z = 0.25 - 0.2f: d == 0.2f exactly, which ProjectVertex's d > 0.2 refuses, so
    the box is the whole band; the same box one ulp of d further from the camera projects."""
    cam = (0.25, 1.0, 16.0, 128.0, 128.0)
    Pz = f32(2.0 ** -6)
    cz = f32(0.25) - f32(0.2)
    assert f32(0.25) - cz == f32(0.2) and (cz - Pz) + Pz == cz
    vz = cz - Pz
    lo = np.array([[-0.1, -0.1, -1.0], [-0.1, -0.1, -1.0]], f32)
    further = vz - f32(2.0 ** -26)  # (d's ulp; a smaller step of z rounds back to d == 0.2f)
    assert f32(0.25) - (further + Pz) == np.nextafter(f32(0.2), f32(1))
    hi = np.array([[0.1, 0.1, vz], [0.1, 0.1, further]], f32)
    ident = X.translation((0, 0, 0))[None]
    bx = B.boxes(lo, hi, [0, 0], ident, (0.0, 0.0, Pz), cam, 256, 0, 256)
    assert bx.whole.tolist() == [True, False] and 0 < tiles_of(bx.rect[1].tolist()) < 1024
    z = np.random.default_rng(4).uniform(-2.0, 0.2, (256, 256)).astype(f32)
    want = B.pixels_of(bx, B.ztiles(z, 0), 0)
    got = prk.selftest_bounds(z, 0, 256, abi.make_transform(*cam), prk.pack_bounds(lo, hi, [0, 0]), ident,
                              P=(0.0, 0.0, float(Pz)))
    assert got["damage"] == 0 and want[0] == 65536
    same(got["pixels"], want, "pixels")


# ---- 3. the whole path ---------------------------------------------------------------------------------------------------
OBJECTS, FINE, FIRST_FRAME, XF = TS.OBJECTS, TS.FINE, TS.FIRST_FRAME, TS.XF
# The boxes are the numpy AABB of each object's source vertices, widened by MARGIN on every side in model units.
# A pixel of this scene is about (D - z) / M2P = 4 / 128 = 0.03 units across, so the margin is a thirtieth of a
# pixel in x and y and, in z, about 10^4 ulps of the depths drawn (|z| < 1) -- against span recurrences that
# leave the vertices' hull by a few ulps a row over at most 256 rows.  The fixture below holds the oracle alone
# to the inequality with this margin, for every object.
MARGIN = 1e-3


@dataclasses.dataclass
class World:
    s: object
    src: tuple
    items: np.ndarray      # every item without ids, one level of min_pixels 1
    levels: np.ndarray
    runs: np.ndarray
    bounds: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    oc: np.ndarray         # the oracle's full frame through the items' matrices
    oz: np.ndarray
    ow: np.ndarray
    want: np.ndarray       # boundsref on that z
    wins: np.ndarray       # per object: the pixels it wins drawn alone on top of that frame, on >=


@pytest.fixture(scope="module")
def world():
    s = TS.lod_scene()
    src = (s.vertices, s.colors, s.normals, s.uvs)
    items, levels = TS.lod_tables(1, 0, coarse=False)
    items[0, 2:4] = (0, 1)
    levels[0, 0] = 1
    runs = np.stack([levels[:, 1], levels[:, 2], levels[:, 1], items[:, 4]], 1).astype(np.uint32)
    items[:, 0:2] = 0  # no ids: every item is ruled by its box
    moved = X.apply_runs(src, (None,) * 4, runs, XF)
    st = dataclasses.replace(s, vertices=moved[0], colors=moved[1], normals=moved[2], uvs=moved[3])
    oc, oz, ow, _ = O.render(st.subset(0, FIRST_FRAME), semantics=AVX, phong=True)
    lo_o, hi_o = B.aabb(s.vertices[6:3 * FIRST_FRAME], 3 * FINE, MARGIN)
    lo_c, hi_c = B.aabb(s.vertices[:6], 6, MARGIN)
    lo, hi = np.concatenate([lo_c, lo_o]), np.concatenate([hi_c, hi_o])
    want = B.pixels(lo, hi, items[:, 4], XF, s.P, s.transform, oz, 0)
    wins = np.zeros(OBJECTS, np.int64)
    for k in range(OBJECTS):  # the object alone on top of the frame, drawn on >= (it wins its own pixels again)
        alone = O.render(st.subset(2 + FINE * k, 2 + FINE * (k + 1)), semantics=AVX_ST, phong=True, color=oc, z=oz)
        wins[k] = int((alone[2] >= 0).sum())
    # conservative, no object excused; some hidden, some not
    assert (want[1:] >= wins).all(), np.flatnonzero(want[1:] < wins)
    assert (want[1:] == 0).sum() >= 10 and (want[1:] > 0).sum() >= 10 and (wins > 150).sum() >= 10 and want[0] > 20000
    assert (wins[want[1:] == 0] == 0).all()
    return World(s, src, items, levels, runs, prk.pack_bounds(lo, hi, items[:, 4]), lo, hi, oc, oz, ow, want, wins)


def read_answer(r):
    """The library's own device array, read back through a wrapped layer (its colour words)."""
    ptr, n = r.visibility_bounds_device()
    if n == 0:
        return np.zeros(0, np.uint32)
    assert ptr
    layer = r.layer_wrap(ptr, 4 * n, ptr, n, 1)
    words = r.layer_download(layer)[0].reshape(-1).copy()
    r.layer_destroy(layer)
    return words


def full_frame(f, w):
    every = f.r.geometry_alloc()
    f.r.geometry_transform(f.g, every, w.runs, XF)
    return every, f.frame(every, FIRST_FRAME)


def test_whole_path_lossless_and_back(gpu, world):
    w = world
    with TS.Frame(w.s) as f:
        r = f.r
        every, a = full_frame(f, w)
        same(a[1].view(np.uint32), w.oz.view(np.uint32), "the frame's z against the oracle's")
        # 1. the answer, on the host and on the device, and the tile map under it
        px = r.visibility_bounds(w.bounds, XF, P=w.s.P)
        same(px, w.want, "pixels")
        same(read_answer(r), w.want, "the device array")
        zt, t0 = r.ztiles()
        assert t0 == 0
        same_values(zt, B.ztiles(a[1], 0), "the tile map")
        ms = r.bounds_ms()
        assert ms[0] > 0.0 and ms[1] > 0.0
        # 2. conservative (the oracle's own inequality, carried over by the two equalities above)
        assert (px[1:] >= w.wins).all() and (px[1:] == 0).any() and (px[1:] > 0).any()
        # 3. lossless: what the boxes drop is not in the frame
        d = r.geometry_alloc()
        total, chosen, first = r.geometry_select_bounds(f.g, d, w.items, w.levels, XF)
        sel = S.choose(w.items, w.levels, w.want)
        same(chosen, sel.chosen, "chosen")
        same(first, sel.out_first, "out_first")
        assert total == sel.total and 10 * FINE <= FIRST_FRAME - total
        same_words(r.geometry_download(d), S.emit(w.items, w.levels, XF, w.src, (None,) * 4, sel), "dst")
        b = f.frame(d, total)  # (on a cleared target)
        same(b[0], a[0], "colour")
        same(b[1].view(np.uint32), a[1].view(np.uint32), "z")
        # a later flush leaves the answer alone
        same(read_answer(r), w.want, "the device array after a flush")
        # 4. come back: the occluder gone, every object can be seen and is selected
        r.clear()
        cleared = np.full((256, 256), -FLT_MAX, f32)
        px = r.visibility_bounds(w.bounds, XF, P=w.s.P)
        same(px, B.pixels(w.lo, w.hi, w.items[:, 4], XF, w.s.P, w.s.transform, cleared, 0), "pixels on a cleared target")
        assert (px > 0).all()
        d2 = r.geometry_alloc()
        total, chosen, first = r.geometry_select_bounds(f.g, d2, w.items, w.levels, XF)
        assert total == FIRST_FRAME and (chosen == 0).all()
        same_words(r.geometry_download(d2), r.geometry_download(every), "everything selected")


def test_whole_path_mixed_items(gpu, world):
    """Items with ids take the frame's sums, items without take their boxes."""
    w = world
    items, levels = TS.lod_tables(150, 1)
    items[1 + OBJECTS // 2:, 0:2] = 0  # the later half: no ids
    counts, pp = S.frame_counts(w.ow, FIRST_FRAME)
    combined = np.where(items[:, 1] > 0, S.pixels_of(items, pix_prefix=pp), w.want.astype(np.int64))
    sel = S.choose(items, levels, combined, dst_first_tri=3)
    assert {-1, 0, 1} <= set(sel.chosen.tolist())
    with TS.Frame(w.s) as f:
        r = f.r
        every, a = full_frame(f, w)
        same(a[2], w.ow, "the frame's winners against the oracle's")
        r.visibility_bounds(w.bounds, XF, P=w.s.P)
        d = r.geometry_alloc()
        total, chosen, first = r.geometry_select_bounds(f.g, d, items, levels, XF, dst_first_tri=3)
        assert total == sel.total
        same(chosen, sel.chosen, "chosen")
        same(first, sel.out_first, "out_first")
        same_words(r.geometry_download(d), S.emit(items, levels, XF, w.src, (None,) * 4, sel), "dst")


def test_band_context(gpu, world):
    w = world
    with TS.Frame(w.s) as f:
        r = f.r
        r.target_alloc(256, 256, 40, 200)
        every, a = full_frame(f, w)
        same(a[1].view(np.uint32), w.oz[40:200].view(np.uint32), "the band's z against the oracle's rows")
        px = r.visibility_bounds(w.bounds, XF, P=w.s.P)
        same(px, B.pixels(w.lo, w.hi, w.items[:, 4], XF, w.s.P, w.s.transform, a[1], 40), "pixels of the band")
        zt, t0 = r.ztiles()
        assert t0 == 5 and zt.shape == (20, 32)
        same_values(zt, B.ztiles(a[1], 40), "the band's tile map")
        assert (px <= w.want).all() and (px < w.want).any()  # (its own rows only)


def test_refused_calls_change_nothing(gpu, world):
    w = world
    ARG, NO_TARGET, LIMIT = abi.PRK_ERR_ARG, abi.PRK_ERR_NO_TARGET, abi.PRK_ERR_LIMIT
    xf = np.ascontiguousarray(XF, f32)
    bp = C.cast(w.bounds.ctypes.data, C.POINTER(abi.PrkBound))
    xp = C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform))
    n = w.bounds.shape[0]
    with TS.Frame(w.s) as f:
        r = f.r
        L, h = r._L, r._h
        every, a = full_frame(f, w)
        d = r.geometry_alloc()
        # before any answer: nothing to select from
        with pytest.raises(prk.PrkError) as e:
            r.geometry_select_bounds(f.g, d, w.items, w.levels, XF)
        assert e.value.code == ARG and r.geometry_info(d) == (0, (False,) * 4)
        with pytest.raises(prk.PrkError):
            r.visibility_bounds_device()
        r.visibility_bounds(w.bounds, XF, P=w.s.P)
        total, _, _ = r.geometry_select_bounds(f.g, d, w.items, w.levels, XF)
        info, before, answer = r.geometry_info(d), r.geometry_download(d), r.visibility_bounds_device()
        out = np.full(n, 0x77777777, np.uint32)
        worse = w.bounds.copy()
        worse.view(np.uint32)[7, 6] = len(XF)
        wp = C.cast(worse.ctypes.data, C.POINTER(abi.PrkBound))
        cases = [("null context", ARG, lambda: L.prk_visibility_bounds(None, bp, n, xp, len(XF), None, out.ctypes.data)),
                 ("null bounds", ARG, lambda: L.prk_visibility_bounds(h, None, n, xp, len(XF), None, out.ctypes.data)),
                 ("null xforms", ARG, lambda: L.prk_visibility_bounds(h, bp, n, None, len(XF), None, out.ctypes.data)),
                 ("xform == xform_count", ARG,
                  lambda: L.prk_visibility_bounds(h, wp, n, xp, len(XF), None, out.ctypes.data)),
                 ("xform_count too small", ARG, lambda: L.prk_visibility_bounds(h, bp, n, xp, 1, None, out.ctypes.data)),
                 ("an answer of another count", ARG, lambda: r._L.prk_geometry_select_bounds(
                     h, f.g, d, 0, C.cast(w.items.ctypes.data, C.POINTER(abi.PrkSelectItem)), n - 1,
                     C.cast(w.levels.ctypes.data, C.POINTER(abi.PrkSelectLevel)), len(w.levels), xp, len(XF), None,
                     None, C.byref(C.c_uint64(0))))]
        for label, status, bad in cases:
            assert bad() == status, label
            assert (out == 0x77777777).all(), label
            assert r.visibility_bounds_device() == answer, label
            same(read_answer(r), w.want, "the answer after the refused call: " + label)
            assert r.geometry_info(d) == info, label
            same_words(r.geometry_download(d), before, "dst after the refused call: " + label)
        # contexts without a camera, without a target, and with a band of 2^32 pixels (bound, never drawn into)
        zp = r.target()[2]
        for label, status, camera, target in (("no camera", ARG, False, "own"), ("no target", NO_TARGET, True, None),
                                              ("a band of 2^32 pixels", LIMIT, True, "huge")):
            q = prk.Renderer()
            try:
                if camera:
                    q.set_camera(w.s.prk_transform(), w.s.prk_lights())
                if target == "own":
                    q.target_alloc(64, 64)
                elif target == "huge":
                    q.target_bind(zp, 65536 * 4, zp, 65536, 65536)
                assert L.prk_visibility_bounds(q._h, bp, n, xp, len(XF), None, out.ctypes.data) == status, label
                assert (out == 0x77777777).all(), label
                with pytest.raises(prk.PrkError):
                    q.visibility_bounds_device()
            finally:
                q.close()
        # no boxes: PRK_OK and an empty answer, which no item table of another size can use
        assert r.visibility_bounds(np.zeros((0, 7), f32), None).shape == (0,)
        assert r.visibility_bounds_device()[1] == 0
        with pytest.raises(prk.PrkError) as e:
            r.geometry_select_bounds(f.g, d, w.items, w.levels, XF)
        assert e.value.code == ARG
        same_words(r.geometry_download(d), before, "dst after the empty answer")
        # a new target drops the answer
        r.visibility_bounds(w.bounds, XF, P=w.s.P)
        r.target_alloc(256, 256)
        with pytest.raises(prk.PrkError):
            r.visibility_bounds_device()


def test_select_and_its_selftest_are_as_they_were(gpu, world):
    """One case of each through k_sel_choose's new parameter (NULL there)."""
    w = world
    rng = np.random.default_rng(21)
    src, xf = X.random_arrays(rng, 700), X.random_values(rng, (7, 3, 4))
    tc = rng.integers(1, 9, 130)
    items, levels, px, st = S.one_level_items(tc, rng.random(130) < 0.6, xforms=7, min_pixels=40)
    TS.check_selftest(items, levels, xf, TS.cut(src, st), "selftest", dst_first=3, item_pixels=px)
    pp = np.concatenate([[0], np.cumsum(rng.integers(0, 90, 130))]).astype(np.uint32)
    items[:, 0], items[:, 1] = np.arange(130), 1
    TS.check_selftest(items, levels, xf, TS.cut(src, st), "selftest, pix_prefix", dst_first=0, pix_prefix=pp)
    items, levels = TS.lod_tables(150, 1)
    counts, pp = S.frame_counts(w.ow, FIRST_FRAME)
    with TS.Frame(w.s) as f:
        r = f.r
        full_frame(f, w)
        for given in (None, S.pixels_of(items, pix_prefix=pp).astype(np.uint32)):
            sel = S.choose(items, levels, S.pixels_of(items, pix_prefix=pp), dst_first_tri=3)
            d = r.geometry_alloc()
            total, chosen, first = r.geometry_select(f.g, d, items, levels, XF, dst_first_tri=3, item_pixels=given)
            assert total == sel.total
            same(chosen, sel.chosen, "chosen")
            same(first, sel.out_first, "out_first")
            same_words(r.geometry_download(d), S.emit(items, levels, XF, w.src, (None,) * 4, sel), "dst")
