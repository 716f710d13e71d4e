"""GPU tests: prk_advance_edge_lists (what DrawModel* leaves in every list of a
batch, walked on the device) against the host call prk_advance_edge_records,
list by list on zero-Next edge_info memory, and against the oracle's walk
(oracle.advance_edges), which the library's host code is itself held to.

Every comparison is on the records' uint32 words and on the Next indices.
One allowance (prk.h): where the expected word is a NaN, the device's word
must be a NaN, of any sign and payload (Normalize of a zero normal is
inf * 0, whose default NaN differs between x86 and gfx950); every other word
must be equal, and a NaN where none is expected fails (same_words).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import prk
from prk import abi, scenes

pytestmark = pytest.mark.gpu

YMAX, XMIN, GRAD, YMIN, LEFT = 0, 1, 4, 7, 12  # prk_edge words
INT_WORDS = (YMAX, YMIN, LEFT)
LIGHTS = {0: ([], scenes.AMBIENT_ONE), 1: (scenes.LIGHTS_ONE, scenes.AMBIENT_ONE)}


def is_nan(w):
    return ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)


def same_words(got, want, label):
    """got == want word for word, but a NaN where (and only where) the
    expected float word is a NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (label, got.shape, want.shape)
    isf = np.ones(27, bool)
    isf[list(INT_WORDS)] = False
    wn = is_nan(want) & isf
    ok = np.where(wn, is_nan(got), got == want)
    bad = np.nonzero(~ok.all(1))[0]
    if bad.size:
        r = int(bad[0])
        f = np.nonzero(~ok[r])[0]
        raise AssertionError("%s: %d of %d records differ; record %d fields %s got %s want %s" % (
            label, bad.size, got.shape[0], r, f.tolist(), [hex(x) for x in got[r, f]], [hex(x) for x in want[r, f]]))


def _lists(words, counts):
    o = 0
    for n in counts:
        yield words[o:o + int(n)]
        o += int(n)


def host_advance(words, counts, height):
    """prk_advance_edge_records on each list as a zero-Next edge_info array."""
    outs, nxts = [np.zeros((0, 27), np.uint32)], [np.zeros(0, np.int32)]
    for w in _lists(words, counts):
        n = w.shape[0]
        mem = np.zeros((max(1, n), prk.EDGE_INFO_STRIDE), np.uint8)
        mem[:n, :108] = np.ascontiguousarray(w).view(np.uint8).reshape(n, 108)
        prk.advance_edge_records(mem, n, height)
        ow, on = prk.edge_record_words(mem, n)
        outs.append(ow)
        nxts.append(on)
    return np.concatenate(outs), np.concatenate(nxts)


def oracle_advance(words, counts, height):
    outs, nxts = [np.zeros((0, 27), np.uint32)], [np.zeros(0, np.int32)]
    for w in _lists(words, counts):
        if w.shape[0]:
            ow, on = O.advance_edges(w, height)
            outs.append(ow)
            nxts.append(on)
    return np.concatenate(outs), np.concatenate(nxts)


def check(r, words, counts, height, label, oracle=False):
    """The device's lists against the host's (and the oracle's); returns them."""
    gw, gn = r.advance_edge_lists(words, counts, height)
    hw, hn = host_advance(words, counts, height)
    same_words(gw, hw, label + " vs host")
    assert np.array_equal(gn, hn), (label, "Next vs host", np.nonzero(gn != hn)[0][:5])
    if oracle:
        ow, on = oracle_advance(words, counts, height)
        same_words(gw, ow, label + " vs oracle")
        assert np.array_equal(gn, on), (label, "Next vs oracle", np.nonzero(gn != on)[0][:5])
    return gw, gn


def _soup():
    """The recipe of test_gpu_edge_records.py: back-facing triangles, the near
    plane, clipping on every side, horizontal edges."""
    s = scenes.random_soup(1200, 256, 192, radius=60, seed=31, centroid_margin=80)
    rng = np.random.default_rng(3)
    v = s.vertices.reshape(-1, 3, 3)
    flip = rng.random(v.shape[0]) < 0.3
    v[flip, 1], v[flip, 2] = v[flip, 2].copy(), v[flip, 1].copy()
    v[rng.random(v.shape[0]) < 0.05, 0, 2] = 3.9
    flat = rng.random(v.shape[0]) < 0.05
    v[flat, 1, 1] = v[flat, 0, 1]
    s.vertices = v.reshape(-1, 3)
    return s


class Ctx:
    """One renderer with one scene's geometry resident, and its records."""

    def __init__(self, s):
        self.s = s
        self.r = prk.Renderer()
        self.g = self.r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        self.cache = {}

    def records(self, setup, per, lights=None, P=None):
        key = (setup, per, lights, P)
        if key not in self.cache:
            s = self.s
            if lights is not None:
                s.lights, s.ambient = LIGHTS[lights]
            self.r.set_camera(s.prk_transform(), s.prk_lights())
            self.cache[key] = self.r.edge_records(self.g, s.tri_count, P=s.P if P is None else P, setup=setup,
                                                  tris_per_object=per)
        return self.cache[key]

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
    c = Ctx(scenes.Scene(256, 256, V.copy(), Cc.copy(), N.copy(), UV.copy(), base.transform, scenes.LIGHTS_ONE,
                         scenes.AMBIENT_ONE, None, P=(0.0, 0.0, 2.0)))
    yield c
    c.close()


@pytest.mark.parametrize("height", [192, 96, 0])
@pytest.mark.parametrize("per", [1, 5, 60])
def test_soup_batches(soup, per, height):
    """Lists of 1, 5 and 60 triangles' edges (empty lists of back-facing
    objects among them), the full frame, half of it, and no rows at all."""
    words, counts = soup.records(3, per, lights=1)
    assert words.shape[0] > 0 and ((counts == 0).any() or per > 1)
    gw, gn = check(soup.r, words, counts, height, "soup per %d height %d" % (per, height), oracle=True)
    if height > 0:
        assert (gw != words).any() and (gn >= 0).any()  # the walk stepped and linked edges
    else:
        assert np.array_equal(gw, words) and (gn == -1).all()


@pytest.mark.parametrize("nl", [0, 1])
@pytest.mark.parametrize("setup", [0, 1, 2])
@pytest.mark.parametrize("per", [1, 5, 60])
def test_soup_setups(soup, per, setup, nl):
    """FillEdgeTable's other setups: records without normals (a zero normal
    normalises to NaN on the first step) and without UV gradients."""
    words, counts = soup.records(setup, per, lights=nl)
    gw, _ = check(soup.r, words, counts, 192, "soup per %d setup %d lights %d" % (per, setup, nl), oracle=per == 60)
    assert (gw != words).any()
    if not (setup & abi.PRK_SETUP_PHONG):
        assert is_nan(gw[:, 21:24]).any()  # the NaN normals do come up


@pytest.mark.parametrize("P,height", [((0.0, 0.0, 2.0), 256), ((0.0, 0.0, 2.0), 128), ((0.0, 0.0, 3.6), 256)])
def test_sphere_one_list(sphere, P, height):
    """ConstructSphere as one list: many pairs a row, both swaps; and through
    the near plane."""
    words, counts = sphere.records(3, 2208, P=P)
    if P[2] == 2.0:
        assert words.shape[0] == 2072
    assert counts.tolist() == [words.shape[0]]
    gw, gn = check(sphere.r, words, counts, height, "sphere P %s height %d" % (P, height), oracle=True)
    assert (gw != words).any() and (gn >= 0).any()


def edge(ymin, ymax, x, g, left, k=0):
    """One prk_edge with every steppable field alive (k varies them)."""
    f = np.zeros(27, np.float32)
    f[XMIN], f[GRAD] = x, g
    f[2], f[5] = 1.0 + k, 0.0625          # ZMin, ZGradient
    f[3], f[6] = 0.25, 0.001 * (k + 1)    # OneOverZMin, OneOverZGradient
    f[8], f[9], f[10], f[11] = 0.1, 0.2, 0.003, -0.004  # UMin, VMin, UGradient, VGradient
    f[13:17] = (0.5, 0.25, 0.125, 1.0)    # MinColor
    f[17:21] = (0.01, -0.01, 0.002, 0.0)  # ColorGradient
    f[21:24] = (0.0, 0.6, 0.8)            # MinNormal
    f[24:27] = (0.01 * (k + 1), -0.02, 0.005)  # NormalGradient
    w = f.view(np.uint32).copy()
    w[YMAX], w[YMIN], w[LEFT] = ymax, ymin, left
    return w


HAND_HEIGHT = 40
HAND_LISTS = [
    ("empty first", []),
    ("one edge", [edge(0, 10, 5.0, 0.5, 1)]),
    # the pair's X cross on the third row: the first pair swaps, the head moves (P3)
    ("first pair swaps", [edge(0, 12, 0.0, 2.0, 1), edge(0, 12, 10.0, -2.0, 0, 1)]),
    # the second pair's left edge crosses under the first pair's right edge (3843-3853)
    ("second swap", [edge(0, 8, 0.0, 0.0, 1), edge(0, 8, 10.0, 3.0, 0, 1), edge(0, 8, 12.0, -3.0, 1, 2),
                     edge(0, 8, 30.0, 0.0, 0, 3)]),
    ("empty middle", []),
    # equal XMin and Gradient: Left orders them (3663-3667), the second goes first
    ("left tie", [edge(2, 9, 7.0, 0.25, 1), edge(2, 9, 7.0, 0.25, 0, 1)]),
    # the list runs empty for rows 5..19, then takes new edges
    ("gap", [edge(0, 5, 1.0, 1.0, 1), edge(0, 5, 9.0, 0.0, 0, 1), edge(20, 30, 3.0, 0.5, 1, 2),
             edge(20, 30, 8.0, -0.25, 0, 3)]),
    # the later edges start on exactly the row the earlier ones expire on: the
    # earlier ones are still linked when the later ones are inserted between them
    ("segment trap", [edge(0, 10, 0.0, 0.0, 1), edge(0, 10, 20.0, 0.0, 0, 1), edge(10, 20, 5.0, 0.0, 1, 2),
                      edge(10, 20, 25.0, 0.0, 0, 3)]),
    ("starts at height", [edge(HAND_HEIGHT, 60, 1.0, 0.0, 1), edge(HAND_HEIGHT + 5, 60, 4.0, 0.0, 0, 1)]),
    ("ymax past height", [edge(30, 100, 2.0, 0.5, 1), edge(30, 100, 50.0, -0.5, 0, 1)]),
    ("empty last", []),
]


def hand_batch():
    counts = np.array([len(l) for _, l in HAND_LISTS], np.uint32)
    words = np.array([e for _, l in HAND_LISTS for e in l], np.uint32).reshape(-1, 27)
    off = dict(zip([n for n, _ in HAND_LISTS], np.concatenate([[0], np.cumsum(counts.astype(np.int64))[:-1]]).tolist()))
    return words, counts, off


def test_hand_made_lists(gpu):
    words, counts, off = hand_batch()
    r = prk.Renderer()
    try:
        gw, gn = check(r, words, counts, HAND_HEIGHT, "hand-made", oracle=True)
    finally:
        r.close()
    X = gw[:, XMIN].view(np.float32)

    def part(name, a):
        o = off[name]
        return a[o:o + len(dict(HAND_LISTS)[name])]

    # never paired: nothing stepped, no link
    assert np.array_equal(part("one edge", gw), part("one edge", words)) and part("one edge", gn).tolist() == [-1]
    # after the crossing the second edge heads the list
    assert part("first pair swaps", gn).tolist() == [-1, 0]
    assert part("first pair swaps", X).tolist() == [24.0, -14.0]
    assert part("second swap", gn).tolist() == [3, -1, 0, 1]  # X order: edges 2, 0, 3, 1
    assert part("left tie", gn).tolist() == [-1, 0]
    assert part("gap", gn).tolist() == [-1, -1, -1, 2]  # (the second pair crossed too)
    assert part("gap", X).tolist() == [6.0, 9.0, 8.0, 5.5]
    # the expired second edge keeps the link to the edge inserted after it
    assert part("segment trap", gn).tolist() == [-1, 3, 3, -1]
    assert np.array_equal(part("starts at height", gw), part("starts at height", words))
    assert part("starts at height", gn).tolist() == [-1, -1]
    assert part("ymax past height", X).tolist() == [2.0 + 0.5 * 10, 50.0 - 0.5 * 10]  # rows 30..39 only


def test_long_list_of_short_edges(gpu):
    """2100 edges, two a row: as many as the crowd test_refusals sees refused,
    but no insertion meets more than the row before, so the list is walked."""
    stair = np.array([edge(i // 2, i // 2 + 1, 3.0 + 40.0 * (i & 1), 0.5, (i + 1) & 1, i & 3) for i in range(2100)],
                     np.uint32)
    r = prk.Renderer()
    try:
        gw, gn = check(r, stair, np.array([2100], np.uint32), 4096, "stair", oracle=True)
    finally:
        r.close()
    assert (gw[:, XMIN].view(np.float32) == np.tile([3.5, 43.5], 1050)).all()  # every pair stepped once


def _raw(r, words, counts, height, out, nxt, nlist=None):
    return r._L.prk_advance_edge_lists(r._h, None if words is None else words.ctypes.data,
                                       None if counts is None else counts.ctypes.data,
                                       len(counts) if nlist is None else nlist, height,
                                       None if out is None else out.ctypes.data,
                                       None if nxt is None else nxt.ctypes.data)


def test_in_place_and_no_next(gpu):
    words, counts, _ = hand_batch()
    r = prk.Renderer()
    try:
        gw, gn = r.advance_edge_lists(words, counts, HAND_HEIGHT)
        buf = words.copy()
        assert _raw(r, buf, counts, HAND_HEIGHT, buf, None) == abi.PRK_OK  # records_out is records, no next_out
        assert np.array_equal(buf, gw) and (buf != words).any()
        out = np.zeros_like(words)
        nxt = np.full(words.shape[0], 99, np.int32)
        assert _raw(r, words, counts, HAND_HEIGHT, out, nxt) == abi.PRK_OK
        assert np.array_equal(out, gw) and np.array_equal(nxt, gn)
        # nothing to walk
        assert _raw(r, None, None, HAND_HEIGHT, None, None, nlist=0) == abi.PRK_OK
        assert _raw(r, None, np.zeros(3, np.uint32), HAND_HEIGHT, None, None) == abi.PRK_OK
    finally:
        r.close()


def test_refusals(gpu):
    """Every refusal leaves the output buffers as they were."""
    good = np.array([edge(0, 10, 0.0, 1.0, 1), edge(0, 10, 9.0, 0.0, 0, 1), edge(4, 12, 3.0, 0.0, 1, 2)], np.uint32)
    counts = np.array([0, 3], np.uint32)

    def variant(row, word, value):
        w = good.copy()
        w[row, word] = np.array([value], np.int32).view(np.uint32)[0]
        return w

    # 257 edges over 65536 rows: 2^24 + 2^16 edge-rows, over the one-thread cap
    long_list = np.array([edge(0, 65536, float(i), 0.0, i & 1) for i in range(257)], np.uint32)
    crowd = np.array([edge(0, 1, float(i), 0.0, i & 1) for i in range(2100)], np.uint32)
    cases = [
        ("YMin out of order", variant(1, YMIN, 5), counts, 64, abi.PRK_ERR_UNSUPPORTED),
        ("YMin < 0", variant(0, YMIN, -1), counts, 64, abi.PRK_ERR_UNSUPPORTED),
        ("Left = 2", variant(1, LEFT, 2), counts, 64, abi.PRK_ERR_UNSUPPORTED),
        ("height -1", good, counts, -1, abi.PRK_ERR_ARG),
        ("height 65537", good, counts, 65537, abi.PRK_ERR_LIMIT),
        ("over the edge-row cap", long_list, np.array([257], np.uint32), 65536, abi.PRK_ERR_LIMIT),
        # one row, but every insertion scans all the edges before it: 2.2 M list steps
        ("insertion scans over the cap", crowd, np.array([2100], np.uint32), 64, abi.PRK_ERR_LIMIT),
    ]
    r = prk.Renderer()
    try:
        for label, w, cnt, height, status in cases:
            out = np.full_like(w, 0xA5A5A5A5)
            nxt = np.full(w.shape[0], 77, np.int32)
            assert _raw(r, w, cnt, height, out, nxt) == status, label
            assert (out == 0xA5A5A5A5).all() and (nxt == 77).all(), label
        out = np.full_like(good, 0xA5A5A5A5)
        assert _raw(r, good, None, 64, out, None, nlist=2) == abi.PRK_ERR_ARG
        assert _raw(r, None, counts, 64, out, None) == abi.PRK_ERR_ARG
        assert _raw(r, good, counts, 64, None, None) == abi.PRK_ERR_ARG
        assert (out == 0xA5A5A5A5).all()
        # ... and the same lists are taken once they are inside the rule
        check(r, good, counts, 64, "accepted")
    finally:
        r.close()


def test_recorded_draws_and_stats_survive(gpu):
    """A call between the recording of a draw and its flush: the same frame,
    the same prk_stats."""
    s = scenes.random_soup(120, 64, 64, radius=12, seed=9)
    words, counts, _ = hand_batch()

    def frame(call):
        r = prk.Renderer()
        try:
            r.target_alloc(s.width, s.height)
            r.clear()
            r.set_camera(s.prk_transform(), s.prk_lights())
            tex = r.texture(s.texture)
            g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
            r.draw(abi.PRK_SEM_AVX, g, s.tri_count, P=s.P, bitmap=tex, phong=True, tris_per_object=6)
            if call:
                st0 = r.stats()
                gw, _ = r.advance_edge_lists(words, counts, HAND_HEIGHT)
                assert (gw != words).any()
                assert r.stats() == st0
            r.complete_all_work()
            c, z = r.download()
            return c, z, r.stats()["triangles"]
        finally:
            r.close()

    c0, z0, t0 = frame(False)
    c1, z1, t1 = frame(True)
    assert (c0 != scenes.CLEAR_COLOR).any() and t0 == s.tri_count
    assert np.array_equal(z1.view(np.uint32), z0.view(np.uint32))
    assert np.array_equal(c1, c0)
    assert t1 == t0
