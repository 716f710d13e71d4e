"""GPU tests: prk_geometry_select (include/prk.h, csrc/prk_select.hip) -- cull
and pick a level of detail on the device, from a frame's per-id pixel counts
or the caller's, and write the chosen triangles packed and transformed into a
resident geometry.

Expected words come from tests/selectref.py (the definition in numpy, its
transforms through tests/xform_ref.py, its frame counts through
tests/visref.py on the oracle's winner map); every word is compared.  The
self-test runs the call's three stages on hand-made tables whose shapes sit on
the constants of the code: the emit workgroup's 64 triangles, runs of equal
starts in the search, the scan's tile of 4096 words.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import prk
import selectref as S
import xform_ref as X
from prk import abi, scenes

pytestmark = pytest.mark.gpu

NAMES = ("vertices", "colors", "normals", "uvs")
AVX = abi.PRK_SEM_AVX


def same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %r, expected %r" % (label, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, "%s: %d of %d differ; first at %d: gpu %r ref %r" % (
        label, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def same_words(got, want, label):
    """4-tuples of arrays (or None), compared as uint32 words."""
    for k in range(4):
        assert (got[k] is None) == (want[k] is None), "%s: %s present %r, expected %r" % (
            label, NAMES[k], got[k] is not None, want[k] is not None)
        if want[k] is not None:
            same(got[k].view(np.uint32), want[k].view(np.uint32), "%s: %s" % (label, NAMES[k]))


# ---- 1. the self-test: the call's stages on hand-made tables ------------------------------------------------------------
def check_selftest(items, levels, xforms, src, label, dst_first=0, slack=3, pix_prefix=None, item_pixels=None):
    px = S.pixels_of(items, pix_prefix=pix_prefix, item_pixels=item_pixels)
    want = S.choose(items, levels, px, dst_first)
    src_tris = src[0].shape[0] // 3
    worst = S.check(items, levels, len(xforms), src_tris, dst_first,
                    frame_ids=None if item_pixels is not None else len(pix_prefix) - 1)
    dst_tris = dst_first + worst + slack
    got = prk.selftest_select(items, levels, xforms, src, dst_tris, dst_first, pix_prefix=pix_prefix,
                              item_pixels=item_pixels)
    assert got["damage"] == 0, "%s: damage %d" % (label, got["damage"])
    assert got["total"] == want.total, "%s: total %d, expected %d" % (label, got["total"], want.total)
    same(got["chosen"], want.chosen, "%s: chosen" % (label,))
    same(got["out_first"], want.out_first, "%s: out_first" % (label,))
    ref = S.emit_selftest(items, levels, xforms, src, dst_tris, want)
    same_words(got["dst"], ref, label)
    # the triangles before and after the written range keep their words
    for k in range(4):
        if ref[k] is not None:
            assert (got["dst"][k][:3 * dst_first] == S.GUARD_WORD).all(), "%s: %s before" % (label, NAMES[k])
            assert (got["dst"][k][3 * (dst_first + want.total):] == S.GUARD_WORD).all(), "%s: %s after" % (
                label, NAMES[k])
    return got, want


@pytest.fixture(scope="module")
def pool():
    """Source arrays and matrices every self-test case cuts its tables from."""
    rng = np.random.default_rng(21)
    return X.random_arrays(rng, 4200), X.random_values(rng, (7, 3, 4))


def cut(src, tris, arrays=(True, True, True, True)):
    return tuple(a[:3 * tris] if on else None for a, on in zip(src, arrays))


@pytest.mark.parametrize("total", [1, 63, 64, 65, 129])
def test_selftest_totals_around_the_workgroup(gpu, pool, total):
    """Items of 1 triangle, all drawn: the total is the item count; then the
    same total from one item, and from items of 1 between dropped ones."""
    src, xf = pool
    items, levels, px, st = S.one_level_items(np.ones(total), np.ones(total), xforms=7)
    check_selftest(items, levels, xf, cut(src, st), ("ones", total), dst_first=5, item_pixels=px)
    items, levels, px, st = S.one_level_items([total], [1], xforms=7)
    check_selftest(items, levels, xf, cut(src, st), ("one item", total), dst_first=0, item_pixels=px)
    drawn = np.arange(3 * total) % 3 == 1
    items, levels, px, st = S.one_level_items(np.ones(3 * total), drawn, xforms=7)
    got, want = check_selftest(items, levels, xf, cut(src, st), ("every third", total), dst_first=64, item_pixels=px)
    assert want.total == total


@pytest.mark.parametrize("where", ["start", "middle", "end", "all"])
def test_selftest_runs_of_dropped_items(gpu, pool, where):
    """70 and more consecutive dropped items: runs of equal starts in the search."""
    src, xf = pool
    rng = np.random.default_rng(5)
    n = 300
    tc = rng.integers(1, 9, n)
    drawn = np.ones(n, bool)
    drawn[{"start": slice(0, 75), "middle": slice(100, 230), "end": slice(n - 70, n), "all": slice(0, n)}[where]] = False
    items, levels, px, st = S.one_level_items(tc, drawn, xforms=7, min_pixels=40)
    got, want = check_selftest(items, levels, xf, cut(src, st), ("dropped at the " + where,), dst_first=3,
                               item_pixels=px)
    assert (want.total == 0) == (where == "all")
    if where == "all":
        assert (got["chosen"] == -1).all() and (got["out_first"] == 3).all()


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_selftest_item_tables_around_the_scan_tile(gpu, pool, n):
    """The scan runs over n + 1 words: one tile of 4096, and one word more."""
    src, xf = pool
    rng = np.random.default_rng(n)
    drawn = rng.random(n) < 0.6
    drawn[-1] = True
    items, levels, px, st = S.one_level_items(np.ones(n), drawn, xforms=7)
    got, want = check_selftest(items, levels, xf, cut(src, st, (True, False, False, True)), ("items", n),
                               item_pixels=px)
    assert want.total == int(drawn.sum()) > 2000


@pytest.mark.parametrize("arrays", [(True, False, False, False), (True, True, False, False), (True, False, True, False),
                                    (True, False, False, True), (True, True, True, True)],
                         ids=["positions", "colors", "normals", "uvs", "all"])
def test_selftest_levels_from_pix_prefix(gpu, pool, arrays):
    """Items of several levels with unordered thresholds, counts from a
    pix_prefix; sources with and without colours, normals and uvs."""
    src, xf = pool
    rng = np.random.default_rng(8)
    n, ids_per = 150, 3
    counts = rng.integers(0, 40, n * ids_per).astype(np.uint32)
    counts[rng.random(n * ids_per) < 0.4] = 0
    pp = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    nlev = rng.integers(0, 4, n)  # (items without levels among them)
    l0 = np.concatenate([[0], np.cumsum(nlev)])
    levels = np.stack([rng.integers(0, 70, l0[-1]), rng.integers(0, 500, l0[-1]), rng.integers(0, 20, l0[-1])], 1)
    idc = rng.integers(0, ids_per + 1, n)  # (id_count == 0 among them)
    items = np.stack([ids_per * np.arange(n), idc, l0[:-1], nlev, rng.integers(0, 7, n)], 1).astype(np.uint32)
    got, want = check_selftest(items, levels.astype(np.uint32), xf, cut(src, 520, arrays), ("levels", arrays),
                               dst_first=7, pix_prefix=pp)
    assert set(want.chosen.tolist()) >= {-1, 0, 1, 2} and want.total > 300
    # exactly at and one below a threshold
    items = np.array([[0, 3, 0, 2, 0], [0, 3, 2, 2, 1]], np.uint32)
    t = int(pp[3])
    assert t > 1
    levels = np.array([[t, 0, 9], [0, 9, 2], [t + 1, 0, 9], [t, 9, 2]], np.uint32)
    got, want = check_selftest(items, levels, xf, cut(src, 11, arrays), ("thresholds", arrays), pix_prefix=pp)
    assert want.chosen.tolist() == [0, 1] and want.total == 11


def test_selftest_no_items(gpu, pool):
    src, xf = pool
    got = prk.selftest_select(np.zeros((0, 5), np.uint32), None, None, cut(src, 4), 6, 2,
                              item_pixels=np.zeros(0, np.uint32))
    assert got["damage"] == 0 and got["total"] == 0 and got["out_first"].tolist() == [2]
    assert all((a == S.GUARD_WORD).all() for a in got["dst"])


# ---- 2. the whole path: draw, ask, select, draw ---------------------------------------------------------------------------
OBJECTS, FINE, COARSE = 40, 8, 2


def lod_scene():
    """One near occluder over the left half of a 256 x 256 target (2
    triangles), then 40 objects on a grid: 8 triangles each, and after them a
    2-triangle second mesh each.  Source triangles: [0, 2) the occluder,
    [2, 322) the fine meshes, [322, 402) the coarse ones."""
    rng = np.random.default_rng(31)
    base = scenes.random_soup(1, 256, 256, seed=2)
    cam = base.transform
    tris, zs = [], []
    tris += [[(-4, -4), (128, -4), (128, 260)], [(-4, -4), (128, 260), (-4, 260)]]
    zs += [0.8, 0.8]
    centres = [(16 + 32 * (k % 8), 26 + 51 * (k // 8)) for k in range(OBJECTS)]
    for per, spread in ((FINE, 11.0), (COARSE, 7.0)):
        for cx, cy in centres:
            for _ in range(per):
                off = rng.uniform(-spread, spread, (3, 2))
                tris.append([(cx + dx, cy + dy) for dx, dy in off])
                zs.append(rng.uniform(-0.5, 0.2))
    s = np.array(tris, np.float64)
    e1, e2 = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]
    flip = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0  # (random_soup's winding)
    s[flip, 1], s[flip, 2] = s[flip, 2].copy(), s[flip, 1].copy()
    z = np.array(zs)[:, None] + rng.uniform(-0.05, 0.05, (len(zs), 3))
    x, y = scenes.unproject(s[..., 0], s[..., 1], z, cam)
    n = 3 * len(tris)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cols = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    return scenes.Scene(256, 256, np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32), cols,
                        nrm.astype(np.float32), rng.uniform(0.0, 1.0, (n, 2)).astype(np.float32), cam,
                        scenes.LIGHTS_ONE, scenes.AMBIENT_ONE, base.texture, name="lod")


def lod_tables(fine_min, coarse_min, coarse=True):
    """Item 0 the occluder (always drawn), then an item an object; its ids are
    the triangles of its fine mesh in the first frame's draw."""
    items = [[0, 2, 0, 1, 0]]
    levels = [[0, 0, 2]]
    for k in range(OBJECTS):
        items.append([2 + FINE * k, FINE, len(levels), 2 if coarse else 1, 1 + k % 3])
        levels.append([fine_min, 2 + FINE * k, FINE])
        if coarse:
            levels.append([coarse_min, 2 + FINE * OBJECTS + COARSE * k, COARSE])
    return np.array(items, np.uint32), np.array(levels, np.uint32)


XF = np.stack([X.translation((0.0, 0.0, 0.0)), X.translation((0.004, 0.0, 0.0)), X.translation((0.0, -0.004, 0.0)),
               X.rotation_yx(0.5, -0.5)])
FIRST_FRAME = 2 + FINE * OBJECTS  # triangles the first frame draws, and its ids


class Frame:
    def __init__(self, s):
        self.s = s
        self.r = r = prk.Renderer()
        r.target_alloc(s.width, s.height)
        r.clear()
        r.set_debug(True)
        r.set_camera(s.prk_transform(), s.prk_lights())
        self.tex = r.texture(s.texture)
        self.g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.close()

    def frame(self, geom, n, first=0):
        self.r.clear()
        self.r.draw(AVX, geom, n, first_tri=first, P=self.s.P, bitmap=self.tex, phong=True)
        self.r.complete_all_work()
        c, z = self.r.download()
        return c, z, self.r.winners()


@pytest.fixture(scope="module")
def lod():
    """(scene, its source arrays, the oracle's per-id counts and pix_prefix of the first frame), computed once."""
    s = lod_scene()
    win = O.render(s.subset(0, FIRST_FRAME), semantics=AVX, phong=True)[2]
    counts, pp = S.frame_counts(win, FIRST_FRAME)
    return s, (s.vertices, s.colors, s.normals, s.uvs), counts, pp


def test_lod_scene_in_the_oracle(lod):
    """What the scene is there for, met by the oracle alone: about half the
    objects hidden, some partly, the rest in full view."""
    s, src, counts, pp = lod
    per_object = counts[2:].reshape(OBJECTS, FINE).sum(1)
    assert 14 <= int((per_object == 0).sum()) <= 26 and int((per_object > 150).sum()) >= 10
    assert counts[:2].sum() > 20000
    items, levels = lod_tables(150, 1)
    sel = S.choose(items, levels, S.pixels_of(items, pix_prefix=pp))
    assert {-1, 0, 1} <= set(sel.chosen[1:].tolist()) and sel.chosen[0] == 0


def test_whole_path_from_the_frames_counts(gpu, lod):
    s, src, counts, pp = lod
    items, levels = lod_tables(150, 1)
    want = S.choose(items, levels, S.pixels_of(items, pix_prefix=pp), dst_first_tri=3)
    with Frame(s) as f:
        r = f.r
        f.frame(f.g, FIRST_FRAME)
        same(r.visibility_counts(), counts, "the frame's counts against the oracle's")
        d = r.geometry_alloc()
        total, chosen, first = r.geometry_select(f.g, d, items, levels, XF, dst_first_tri=3)
        assert total == want.total
        same(chosen, want.chosen, "chosen")
        same(first, want.out_first, "out_first")
        ref = S.emit(items, levels, XF, src, (None,) * 4, want)
        assert r.geometry_info(d) == (3 * (3 + want.total), (True,) * 4)
        same_words(r.geometry_download(d), ref, "dst")
        ms = r.select_ms()
        assert ms[0] > 0.0 and ms[1] > 0.0
        # a second call into the same dst, further on: what the first wrote stays
        items2, levels2 = lod_tables(1, 0, coarse=False)
        want2 = S.choose(items2, levels2, S.pixels_of(items2, pix_prefix=pp), dst_first_tri=400)
        total2, chosen2, first2 = r.geometry_select(f.g, d, items2, levels2, XF, dst_first_tri=400)
        assert total2 == want2.total and 100 < total2 < FIRST_FRAME
        same(first2, want2.out_first, "second call: out_first")
        ref2 = S.emit(items2, levels2, XF, src, ref, want2)
        got2 = r.geometry_download(d)
        same_words(got2, ref2, "dst after the second call")
        assert not got2[0][3 * (3 + want.total):3 * 400].view(np.uint32).any()  # (the gap: zeros of the growth)
        # the same numbers as item_pixels, after the frame is gone: the same result
        px = S.pixels_of(items, pix_prefix=pp).astype(np.uint32)
        r.target_alloc(s.width, s.height)
        with pytest.raises(prk.PrkError):
            r.visibility()
        with pytest.raises(prk.PrkError) as e:
            r.geometry_select(f.g, d, items, levels, XF)
        assert e.value.code == abi.PRK_ERR_ARG
        d3 = r.geometry_alloc()
        blind = items.copy()
        blind[:, :2] = 0xFFFFFFFF  # (first_id / id_count are not looked at)
        total3, chosen3, first3 = r.geometry_select(f.g, d3, blind, levels, XF, dst_first_tri=3, item_pixels=px)
        assert total3 == total
        same(chosen3, chosen, "item_pixels: chosen")
        same(first3, first, "item_pixels: out_first")
        same_words(r.geometry_download(d3), ref, "item_pixels: dst")


def test_lossless_culling(gpu, lod):
    """Every item one level with min_pixels = 1: the frame drawn from the
    selected geometry is the frame drawn from every item, bit for bit."""
    s, src, counts, pp = lod
    items, levels = lod_tables(1, 0, coarse=False)
    items[0, 2:4] = (0, 1)
    levels[0, 0] = 1
    runs = np.stack([levels[:, 1], levels[:, 2], levels[:, 1], items[:, 4]], 1).astype(np.uint32)
    with Frame(s) as f:
        r = f.r
        every = r.geometry_alloc()
        r.geometry_transform(f.g, every, runs, XF)
        a = f.frame(every, FIRST_FRAME)
        assert (a[2] >= 0).sum() > 30000
        d = r.geometry_alloc()
        total, chosen, first = r.geometry_select(f.g, d, items, levels, XF)  # (from frame a's counts)
        per_item = np.add.reduceat(np.bincount(a[2][a[2] >= 0], minlength=FIRST_FRAME), items[:, 0].astype(np.int64))
        same(chosen, np.where(per_item >= 1, 0, -1), "chosen: the items with a pixel")
        assert 14 * FINE <= FIRST_FRAME - total <= 26 * FINE
        b = f.frame(d, total)
    same(b[0], a[0], "colour")
    same(b[1].view(np.uint32), a[1].view(np.uint32), "z")
    # winner ids through out_first: id w of the culled frame is triangle w - out_first[i] of item i
    w = b[2].astype(np.int64)
    item = np.searchsorted(first.astype(np.int64), w, side="right") - 1
    back = np.where(w >= 0, items[:, 0].astype(np.int64)[item] + w - first.astype(np.int64)[item], -1)
    same(back, a[2], "winner ids mapped back through out_first")


# ---- 3. refused calls ---------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(gpu, lod):
    s, src, counts, pp = lod
    items, levels = lod_tables(150, 1)
    px = S.pixels_of(items, pix_prefix=pp).astype(np.uint32)
    ARG, LIMIT = abi.PRK_ERR_ARG, abi.PRK_ERR_LIMIT
    with Frame(s) as f:
        r = f.r
        L, h, g = r._L, r._h, f.g
        d = r.geometry_alloc()
        total, chosen, first = r.geometry_select(g, d, items, levels, XF, item_pixels=px)
        info = r.geometry_info(d)
        before = r.geometry_download(d)
        assert info == (3 * total, (True,) * 4) and total > 0
        zp = r.target()[2]
        wrapped = r.geometry_device(zp, None, None, None, 30)
        keep = []

        def call(ctx=h, src_=g, dst_=d, first_tri=0, it=items, nit=None, lv=levels, nlv=None, xf=XF, nxf=None,
                 pixels=px, total_ok=True):
            it = None if it is None else np.ascontiguousarray(it, np.uint32)
            lv = None if lv is None else np.ascontiguousarray(lv, np.uint32)
            xf = None if xf is None else np.ascontiguousarray(xf, np.float32)
            pixels = None if pixels is None else np.ascontiguousarray(pixels, np.uint32)
            keep[:] = [it, lv, xf, pixels]
            out = (np.full(8192, 0x77777777, np.uint32), np.full(8192, 0x77777777, np.uint32), C.c_uint64(77))
            rc = L.prk_geometry_select(
                ctx, src_, dst_, first_tri,
                None if it is None else C.cast(it.ctypes.data, C.POINTER(abi.PrkSelectItem)),
                (0 if it is None else it.shape[0]) if nit is None else nit,
                None if lv is None else C.cast(lv.ctypes.data, C.POINTER(abi.PrkSelectLevel)),
                (0 if lv is None else lv.shape[0]) if nlv is None else nlv,
                None if xf is None else C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform)),
                (0 if xf is None else xf.shape[0]) if nxf is None else nxf,
                None if pixels is None else pixels.ctypes.data, out[0].ctypes.data, out[1].ctypes.data,
                C.byref(out[2]) if total_ok else None)
            assert (out[0] == 0x77777777).all() and (out[1] == 0x77777777).all() and out[2].value == 77
            return rc

        def edited(table, row, col, value):
            t = table.copy()
            t[row, col] = value
            return t

        limit_tri = S.VERTEX_LIMIT // 3
        many = np.tile(np.array([[0, 0, 0, 1, 0]], np.uint32), (8193, 1))  # 8193 x 262144 triangles > 2^31
        big = r.geometry(np.zeros((3 * 262144, 3), np.float32))
        cases = [
            ("null context", ARG, lambda: call(ctx=None)),
            ("null total", ARG, lambda: call(total_ok=False)),
            ("src < 0", ARG, lambda: call(src_=-1)),
            ("src past the handles", ARG, lambda: call(src_=999)),
            ("dst < 0", ARG, lambda: call(dst_=-1)),
            ("dst past the handles", ARG, lambda: call(dst_=999)),
            ("src == dst", ARG, lambda: call(src_=d)),
            ("wrapped dst", ARG, lambda: call(dst_=wrapped)),
            ("null items", ARG, lambda: call(it=None, nit=3)),
            ("null levels", ARG, lambda: call(lv=None, nlv=len(levels))),
            ("null xforms", ARG, lambda: call(xf=None, nxf=4)),
            ("levels past the table", ARG, lambda: call(nlv=len(levels) - 1)),
            ("first_level wraps", ARG, lambda: call(it=edited(items, 5, 2, 0xFFFFFFFF))),
            ("xform == xform_count", ARG, lambda: call(nxf=3)),
            ("a level past the end of src", ARG, lambda: call(lv=edited(levels, len(levels) - 1, 2, COARSE + 1))),
            ("a level that starts past src", ARG, lambda: call(lv=edited(levels, 4, 1, 0xFFFFFFFF))),
            ("no frame", ARG, lambda: call(pixels=None)),
            ("worst-case end past the vertex limit", ARG, lambda: call(first_tri=limit_tri - 2 - FINE * OBJECTS + 1)),
            ("worst-case total above 2^31", LIMIT, lambda: call(src_=big, it=many, lv=[[0, 0, 262144]], pixels=many[:, 0])),
        ]
        for label, status, bad in cases:
            assert bad() == status, label
            assert r.geometry_info(d) == info, label
            same_words(r.geometry_download(d), before, "after the refused call: " + label)
        # with a frame: ids past its numbering, and the same tables accepted when inside it
        f.frame(g, FIRST_FRAME)
        assert r.visibility()[0] == FIRST_FRAME
        for label, bad in (("ids past the frame's", lambda: call(pixels=None, it=edited(items, OBJECTS, 1, FINE + 1))),
                           ("first_id past the frame's, no ids", lambda: call(pixels=None, it=edited(
                               edited(items, 3, 0, FIRST_FRAME + 1), 3, 1, 0))),
                           ("first_id + id_count wraps", lambda: call(pixels=None, it=edited(items, 3, 0, 0xFFFFFFFF)))):
            assert bad() == ARG, label
            assert r.geometry_info(d) == info, label
            same_words(r.geometry_download(d), before, "after the refused call: " + label)
        # no items: PRK_OK, total 0, out_first[0] = dst_first_tri, dst as it was
        first0, tot0 = np.full(1, 9, np.uint32), C.c_uint64(9)
        assert L.prk_geometry_select(h, g, d, 11, None, 0, None, 0, None, 0, None, None, first0.ctypes.data,
                                     C.byref(tot0)) == abi.PRK_OK
        assert tot0.value == 0 and first0.tolist() == [11] and r.geometry_info(d) == info
        # nothing chosen: the same, with every word of the answer
        none, _, first_n = r.geometry_select(g, d, items[1:], levels, XF, dst_first_tri=500,
                                             item_pixels=np.zeros(OBJECTS, np.uint32))
        assert none == 0 and (first_n == 500).all() and r.geometry_info(d) == info
        same_words(r.geometry_download(d), before, "after a call that chose nothing")
        # the worst-case end exactly at the limit passes the checks (items without a pixel: nothing is allocated)
        ok, _, _ = r.geometry_select(g, d, items[1:], levels, XF, dst_first_tri=limit_tri - FINE * OBJECTS,
                                     item_pixels=np.zeros(OBJECTS, np.uint32))
        assert ok == 0 and r.geometry_info(d) == info
