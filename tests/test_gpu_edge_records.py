"""GPU tests: prk_edge_records (FillEdgeTable's edge_info records of a batch of
objects, set up, MergeSorted and packed on the device) against the host
producer prk_fill_edge_records on zeroed memory, object by object.

Every comparison is on the records' uint32 words, so NaN payloads and -0.0
count, and the tolerance is zero: the host producer is built without
contraction and the device helpers are pinned bit for bit.  Only rows
[0, count) of the host's memory are the contract (slot `count` and the sort
scratch hold residue of skipped edges).
"""
import ctypes as C

import numpy as np
import pytest

import prk
from prk import abi, scenes

pytestmark = pytest.mark.gpu

YMAX, YMIN = 0, 7  # prk_edge words
LIGHTS = {0: ([], scenes.AMBIENT_ONE), 1: (scenes.LIGHTS_ONE, scenes.AMBIENT_ONE),
          2: (scenes.LIGHTS_TWO, scenes.AMBIENT_TWO)}


def _soup():
    """The recipe of test_abi.py::test_fill_edge_count_matches_oracle: back-
    facing triangles, the near plane, clipping on every side, horizontal edges."""
    s = scenes.random_soup(1200, 256, 192, radius=60, seed=31, centroid_margin=80)
    rng = np.random.default_rng(3)
    v = s.vertices.reshape(-1, 3, 3)
    flip = rng.random(v.shape[0]) < 0.3  # back-facing: swap two vertices
    v[flip, 1], v[flip, 2] = v[flip, 2].copy(), v[flip, 1].copy()
    v[rng.random(v.shape[0]) < 0.05, 0, 2] = 3.9  # a vertex at the near plane
    flat = rng.random(v.shape[0]) < 0.05  # a horizontal edge
    v[flat, 1, 1] = v[flat, 0, 1]
    s.vertices = v.reshape(-1, 3)
    return s


def _with_lights(s, nl):
    s.lights, s.ambient = LIGHTS[nl]
    return s


def expected(s, setup, per, normals=True, uvs=True, first=0, count=None):
    """prk_fill_edge_records per object on zeroed memory: (words, counts)."""
    T = s.tri_count if count is None else count
    tr, li = s.prk_transform(), s.prk_lights()
    rows, counts = [np.zeros((0, 27), np.uint32)], []
    for t0 in range(first, first + T, per):
        n = min(per, first + T - t0)
        sl = slice(3 * t0, 3 * (t0 + n))
        mem, c = prk.fill_edge_records(s.vertices[sl], s.colors[sl], s.normals[sl] if normals else None,
                                       s.uvs[sl] if uvs else None, s.P, tr, li, setup)
        rows.append(prk.edge_record_words(mem, c)[0])
        counts.append(c)
    return np.concatenate(rows), np.array(counts, np.uint32)


class Ctx:
    """One renderer with one scene's geometry resident."""

    def __init__(self, s, normals=True, uvs=True):
        self.s = s
        self.r = prk.Renderer()
        self.g = self.r.geometry(s.vertices, s.colors, s.normals if normals else None, s.uvs if uvs else None)

    def records(self, setup, per, lights=None, **kw):
        s = self.s
        if lights is not None:
            _with_lights(s, lights)
        self.r.set_camera(s.prk_transform(), s.prk_lights())
        return self.r.edge_records(self.g, kw.pop("count", s.tri_count), P=s.P, setup=setup, tris_per_object=per, **kw)

    def close(self):
        self.r.close()


@pytest.fixture(scope="module")
def soup(gpu):
    c = Ctx(_soup())
    yield c
    c.close()


@pytest.fixture(scope="module")
def sphere(gpu):
    V, Cc, N, UV = prk.construct_sphere()
    base = scenes.random_soup(1, 256, 256, seed=0)
    s = scenes.Scene(256, 256, V.copy(), Cc.copy(), N.copy(), UV.copy(), base.transform, scenes.LIGHTS_ONE,
                     scenes.AMBIENT_ONE, None, P=(0.0, 0.0, 2.0))
    c = Ctx(s)
    yield c
    c.close()


def same(got, want, label):
    gw, gc = got
    ww, wc = want
    assert np.array_equal(gc, wc), (label, "counts", np.nonzero(gc != wc)[0][:5])
    assert gw.shape == ww.shape, (label, gw.shape, ww.shape)
    bad = np.nonzero((gw != ww).any(1))[0]
    if bad.size:
        r = int(bad[0])
        f = np.nonzero(gw[r] != ww[r])[0]
        raise AssertionError("%s: %d of %d records differ; record %d fields %s got %s want %s" % (
            label, bad.size, gw.shape[0], r, f.tolist(), [hex(x) for x in gw[r, f]], [hex(x) for x in ww[r, f]]))


@pytest.mark.parametrize("per", [1, 5, 60, 1200])
@pytest.mark.parametrize("nl", [0, 1, 2])
@pytest.mark.parametrize("setup", [0, 1, 2, 3])
def test_soup_parity(soup, setup, nl, per):
    """Counts and every word, for every (PHONG, BITMAP) setup and 0 / 1 / 2
    lights; objects of 1 and 5 triangles (the one-wave MergeSort), 60 (180
    edges: the radix sort) and all 1200 as one object (its tie order)."""
    got = soup.records(setup, per, lights=nl)
    same(got, expected(soup.s, setup, per), "setup %d lights %d per %d" % (setup, nl, per))
    assert got[0].shape[0] > 0


@pytest.mark.parametrize("missing", ["normals", "uvs"])
def test_soup_missing_array(gpu, missing):
    """A missing vertex array reads as zeros in both producers."""
    s = _with_lights(_soup(), 2)
    kw = dict(normals=missing != "normals", uvs=missing != "uvs")
    c = Ctx(s, **kw)
    try:
        for setup, per in [(3, 60), (0, 5)]:
            same(c.records(setup, per), expected(s, setup, per, **kw), "no %s setup %d per %d" % (missing, setup, per))
    finally:
        c.close()


def test_soup_clipped_above_row_zero(soup):
    """The ClippedY branch (3993-3997) runs: some record starts at YMin == 0
    because its edge's upper vertex lies above the frame."""
    s = _with_lights(soup.s, 1)
    words, counts = soup.records(3, 1)
    D, F, M2P, cx, cy = s.transform
    v = s.vertices.reshape(-1, 3, 3).astype(np.float64)
    d = D - (v[..., 2] + s.P[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        py = np.where(d > 0.2, cy + M2P * (F / d) * (v[..., 1] + s.P[1]), 0.0)  # ProjectVertex (74-93)
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    hit = 0
    for t in np.nonzero((py.min(1) < -1.0) & (py.max(1) > 1.0) & (counts > 0))[0]:
        hit += int((words[off[t]:off[t + 1], YMIN] == 0).sum())
    assert hit > 0


@pytest.mark.parametrize("setup", [3, 0])
@pytest.mark.parametrize("per", [2208, 16])
def test_sphere_ties(sphere, setup, per):
    """ConstructSphere's rings share YMin: MergeSort's tie order decides the
    result, as one object (the radix sort's path bits) and as 16-triangle
    objects (the one-wave sort)."""
    assert sphere.s.tri_count == 2208
    got = sphere.records(setup, per)
    same(got, expected(sphere.s, setup, per), "sphere setup %d per %d" % (setup, per))
    ymin = got[0][:, YMIN]
    assert np.unique(ymin).size < ymin.size  # ties exist


def test_records_do_not_depend_on_the_target(gpu):
    """No target, a 64x32 target, the 256x192 target: the same records.  The
    frame path's sort key clamps YMin to the frame height, which would tie the
    edges that start at distinct rows >= 32 of a 32-row frame."""
    s = _with_lights(_soup(), 1)
    c = Ctx(s)
    try:
        a = c.records(3, 1200)
        c.r.target_alloc(64, 32)
        b = c.records(3, 1200)
        c.r.target_alloc(256, 192)
        d = c.records(3, 1200)
    finally:
        c.close()
    assert np.unique(a[0][:, YMIN][a[0][:, YMIN].view(np.int32) >= 32]).size >= 2
    same(b, a, "64x32 target")
    same(d, a, "256x192 target")
    same(a, expected(s, 3, 1200), "no target")


def _frame(s, sem, phong, textured, per, setup, from_records):
    r = prk.Renderer()
    try:
        r.target_alloc(s.width, s.height)
        r.clear()
        r.set_camera(s.prk_transform(), s.prk_lights())
        tex = r.texture(s.texture) if textured else None
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        if from_records:
            words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=setup, tris_per_object=per)
            o = 0
            for n in counts:
                r.draw_edges(words[o:o + n], semantics=sem, bitmap=tex, phong=phong)
                o += int(n)
            assert o == words.shape[0] > 0
        else:
            r.draw(sem, g, s.tri_count, P=s.P, bitmap=tex, phong=phong, tris_per_object=per, setup=setup)
        r.complete_all_work()
        return r.download()
    finally:
        r.close()


@pytest.mark.parametrize("sem,phong,textured,setup", [(abi.PRK_SEM_AVX, True, True, 3),
                                                     (abi.PRK_SEM_SCALAR, False, False, 0)])
def test_round_trip(gpu, sem, phong, textured, setup):
    """Every object drawn from its returned records (prk_draw_edges) gives the
    frame of the whole-object draw, colour and z (the winner ids differ by
    construction: an edge-list draw counts as one id)."""
    s = scenes.random_soup(300, 128, 96, radius=24, seed=12, centroid_margin=20)
    c0, z0 = _frame(s, sem, phong, textured, 20, setup, False)
    c1, z1 = _frame(s, sem, phong, textured, 20, setup, True)
    assert (c0 != scenes.CLEAR_COLOR).any()
    assert np.array_equal(z1.view(np.uint32), z0.view(np.uint32))
    assert np.array_equal(c1, c0)


def _raw(r, g, tri_count, per, setup, records, capacity, counts):
    total = C.c_uint64(12345)
    rc = r._L.prk_edge_records(r._h, g, 0, tri_count, per, None, setup,
                               None if records is None else records.ctypes.data, capacity,
                               None if counts is None else counts.ctypes.data, C.byref(total))
    return rc, total.value


def test_interface_edges(gpu):
    s = scenes.random_soup(15, 128, 96, radius=24, seed=5)
    v = s.vertices.reshape(-1, 3, 3)
    v[5:10, 1], v[5:10, 2] = v[5:10, 2].copy(), v[5:10, 1].copy()  # the second object: all back-facing
    s.vertices = v.reshape(-1, 3)
    r = prk.Renderer()
    try:
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        cnt = np.zeros(3, np.uint32)
        rec = np.zeros((45, 27), np.uint32)
        # before any prk_set_camera
        assert _raw(r, g, 15, 5, 3, rec, 45, cnt)[0] == abi.PRK_ERR_ARG
        r.set_camera(s.prk_transform(), s.prk_lights())
        # an all-back-facing object: count 0, its neighbours' offsets right
        got = r.edge_records(g, 15, P=s.P, setup=3, tris_per_object=5)
        want = expected(s, 3, 5)
        same(got, want, "back-facing object")
        assert got[1][1] == 0 and got[1][0] > 0 and got[1][2] > 0
        total = int(got[1].sum())
        # records == NULL: the same counts and total
        rc, tot = _raw(r, g, 15, 5, 3, None, 0, cnt)
        assert (rc, tot) == (abi.PRK_OK, total) and np.array_equal(cnt, got[1])
        # a buffer one record short: refused, the total still reported
        rc, tot = _raw(r, g, 15, 5, 3, rec, total - 1, cnt)
        assert (rc, tot) == (abi.PRK_ERR_ARG, total)
        rc, tot = _raw(r, g, 15, 5, 3, rec, total, cnt)
        assert (rc, tot) == (abi.PRK_OK, total) and np.array_equal(rec[:total], want[0])
        # argument checks
        assert _raw(r, g, 15, 0, 3, rec, 45, cnt)[0] == abi.PRK_ERR_ARG
        assert _raw(r, g, 15, 5, 4, rec, 45, cnt)[0] == abi.PRK_ERR_ARG
        assert _raw(r, g, 15, 5, -1, rec, 45, cnt)[0] == abi.PRK_ERR_ARG
        assert _raw(r, g, 16, 5, 3, rec, 48, cnt)[0] == abi.PRK_ERR_ARG
        assert _raw(r, g + 1, 15, 5, 3, rec, 45, cnt)[0] == abi.PRK_ERR_ARG
        assert _raw(r, g, 0, 5, 3, rec, 45, cnt) == (abi.PRK_OK, 0)
        # a sub-range of the geometry
        sub = r.edge_records(g, 7, first_tri=3, P=s.P, setup=1, tris_per_object=4)
        same(sub, expected(s, 1, 4, first=3, count=7), "sub-range")
    finally:
        r.close()


def test_recorded_draws_survive(gpu):
    """Draws recorded before the call still produce the same frame after it,
    and the frame in flight before it is not disturbed."""
    s = scenes.random_soup(600, 128, 96, radius=20, seed=21)

    def frame(call):
        r = prk.Renderer()
        try:
            r.target_alloc(s.width, s.height)
            r.clear()
            r.set_camera(s.prk_transform(), s.prk_lights())
            tex = r.texture(s.texture)
            g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
            r.draw(abi.PRK_SEM_AVX, g, 300, bitmap=tex, phong=True, tris_per_object=10)
            r.complete_all_work()  # a frame in flight
            r.draw(abi.PRK_SEM_AVX, g, 200, first_tri=300, bitmap=tex, phong=True, tris_per_object=10)
            r.draw(abi.PRK_SEM_AVX, g, 100, first_tri=500, bitmap=tex, phong=True)
            st0 = r.stats() if call else None
            if call:
                w, c = r.edge_records(g, s.tri_count, setup=3, tris_per_object=10)
                assert w.shape[0] == int(c.sum()) > 0
                st1 = r.stats()
                assert st1 == st0
            r.complete_all_work()
            return r.download()
        finally:
            r.close()

    c0, z0 = frame(False)
    c1, z1 = frame(True)
    assert (c0 != scenes.CLEAR_COLOR).any()
    assert np.array_equal(z1.view(np.uint32), z0.view(np.uint32))
    assert np.array_equal(c1, c0)
