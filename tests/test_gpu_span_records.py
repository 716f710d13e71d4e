"""GPU tests: prk_span_records (the work records DrawModelOptimized(RenderQueue)
queues for every list of a batch, from the device's list walk) against
tests/spanref.py, the Python restatement of the reference's walk that
tests/test_span_records_api.py holds to the oracle.

Every comparison is on the spans' 25 uint32 words and on the counts.  One
allowance (prk.h): where the expected MinColor / MinNormal word is a NaN, the
device's word must be a NaN, of any sign and payload; every other word, Row
included, must be equal, and a NaN where none is expected fails (same_spans).
The hand-made batch and the Phong + Bitmap batches are compared with no
allowance at all where the expectation holds no NaN in those words.
"""
import numpy as np
import pytest

import prk
import spanref
from prk import abi, scenes

pytestmark = pytest.mark.gpu

YMAX, XMIN, GRAD, YMIN, LEFT = 0, 1, 4, 7, 12  # prk_edge words
# prk_span words: an end is XMin ZMin OneOverZMin UMin VMin MinColor[4] MinNormal[3]
S_LEFT_X, S_RIGHT_X, S_ROW = 0, 12, 24
NAN_WORDS = [o + k for o in (0, 12) for k in range(5, 12)]  # MinColor, MinNormal of both ends
NORMAL_WORDS = [o + k for o in (0, 12) for k in range(9, 12)]
LIGHTS = {0: ([], scenes.AMBIENT_ONE), 1: (scenes.LIGHTS_ONE, scenes.AMBIENT_ONE)}


def is_nan(w):
    return ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)


def same_spans(got, want, label):
    """got == want word for word, but a NaN where (and only where) the
    expected MinColor / MinNormal word is a NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (label, got.shape, want.shape)
    allow = np.zeros(25, bool)
    allow[NAN_WORDS] = True
    wn = is_nan(want) & allow
    ok = np.where(wn, is_nan(got), got == want)
    bad = np.nonzero(~ok.all(1))[0]
    if bad.size:
        r = int(bad[0])
        f = np.nonzero(~ok[r])[0]
        raise AssertionError("%s: %d of %d spans differ; span %d words %s got %s want %s" % (
            label, bad.size, got.shape[0], r, f.tolist(), [hex(x) for x in got[r, f]], [hex(x) for x in want[r, f]]))


def check(r, words, counts, height, label):
    """The device's spans and counts against spanref's; returns both."""
    gs, gc = r.span_records(words, counts, height)
    ws, wc, _, _ = spanref.walk_batch(words, counts, height)
    assert gc.dtype == np.uint32 and np.array_equal(gc, wc), (label, "counts", np.nonzero(gc != wc)[0][:5])
    same_spans(gs, ws, label)
    return gs, gc, ws


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


def _sphere_scene():
    V, Cc, N, UV = prk.construct_sphere()
    base = scenes.random_soup(1, 256, 256, seed=0)
    return scenes.Scene(256, 256, V.copy(), Cc.copy(), N.copy(), UV.copy(), base.transform, scenes.LIGHTS_ONE,
                        scenes.AMBIENT_ONE, None, P=(0.0, 0.0, 2.0))


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
    c = Ctx(_sphere_scene())
    yield c
    c.close()


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
ODD_THIRD_X = 77.0  # the odd list's last edge: no span holds this XMin
HAND_LISTS = [
    ("empty first", []),
    ("one edge", [edge(0, 10, 5.0, 0.5, 1)]),
    # the pair's X cross on the third row: the first pair swaps, the head moves (P3)
    ("first pair swaps", [edge(0, 12, 0.0, 2.0, 1), edge(0, 12, 10.0, -2.0, 0, 1)]),
    # the second pair's left edge crosses under the first pair's right edge (3843-3853)
    ("second swap", [edge(0, 8, 0.0, 0.0, 1), edge(0, 8, 10.0, 3.0, 0, 1), edge(0, 8, 12.0, -3.0, 1, 2),
                     edge(0, 8, 30.0, 0.0, 0, 3)]),
    # equal XMin and Gradient: Left orders them (3663-3667), the second goes first
    ("left tie", [edge(2, 9, 7.0, 0.25, 1), edge(2, 9, 7.0, 0.25, 0, 1)]),
    # the list runs empty for rows 5..19, then takes new edges
    ("gap", [edge(0, 5, 1.0, 1.0, 1), edge(0, 5, 9.0, 0.0, 0, 1), edge(20, 30, 3.0, 0.5, 1, 2),
             edge(20, 30, 8.0, -0.25, 0, 3)]),
    # the later edges start on exactly the row the earlier ones expire on
    ("segment trap", [edge(0, 10, 0.0, 0.0, 1), edge(0, 10, 20.0, 0.0, 0, 1), edge(10, 20, 5.0, 0.0, 1, 2),
                      edge(10, 20, 25.0, 0.0, 0, 3)]),
    ("starts at height", [edge(HAND_HEIGHT, 60, 1.0, 0.0, 1), edge(HAND_HEIGHT + 5, 60, 4.0, 0.0, 0, 1)]),
    ("ymax past height", [edge(30, 100, 2.0, 0.5, 1), edge(30, 100, 50.0, -0.5, 0, 1)]),
    # three edges: the third is listed on every row and never paired
    ("odd list", [edge(3, 9, 1.0, 0.0, 1), edge(3, 9, 6.0, 0.0, 0, 1), edge(3, 9, ODD_THIRD_X, 0.0, 1, 2)]),
    ("empty last", []),
]


def hand_batch():
    counts = np.array([len(l) for _, l in HAND_LISTS], np.uint32)
    words = np.array([e for _, l in HAND_LISTS for e in l], np.uint32).reshape(-1, 27)
    return words, counts


def test_hand_made_lists(gpu):
    words, counts = hand_batch()
    ws, wc, _, _ = spanref.walk_batch(words, counts, HAND_HEIGHT)
    r = prk.Renderer()
    try:
        gs, gc = r.span_records(words, counts, HAND_HEIGHT)
    finally:
        r.close()
    assert np.array_equal(gc, wc)
    assert np.array_equal(gs, ws)  # all 25 words equal: no allowance
    names = [n for n, _ in HAND_LISTS]
    off = np.concatenate([[0], np.cumsum(gc.astype(np.int64))])

    def part(name):
        o = names.index(name)
        return gs[off[o]:off[o + 1]]

    F = lambda a: a.view(np.float32)  # noqa: E731
    assert gc[names.index("empty first")] == 0 and gc[names.index("empty last")] == 0
    assert part("one edge").shape[0] == 0 and part("starts at height").shape[0] == 0
    p = part("first pair swaps")
    assert p.shape[0] == 12 and p[:, S_ROW].tolist() == list(range(12))
    assert F(p[:3, S_LEFT_X]).tolist() == [0.0, 2.0, 4.0]
    assert F(p[:3, S_RIGHT_X]).tolist() == [10.0, 8.0, 6.0]
    # the step after row 2 crosses them (6, 4): from row 3 on the second edge is Left
    assert F(p[3:, S_LEFT_X]).tolist() == [4.0 - 2.0 * k for k in range(9)]
    assert F(p[3:, S_RIGHT_X]).tolist() == [6.0 + 2.0 * k for k in range(9)]
    assert F(p[3, 1:2]).tolist() == [2.0 + 3 * 0.0625]  # Left.ZMin is the second edge's (k = 1), stepped thrice
    g = part("gap")
    assert g.shape[0] == 15 and not ((g[:, S_ROW] >= 5) & (g[:, S_ROW] < 20)).any()
    y = part("ymax past height")
    assert y[:, S_ROW].tolist() == list(range(30, 40))
    o = part("odd list")
    assert o[:, S_ROW].tolist() == list(range(3, 9))
    assert not (F(o[:, [S_LEFT_X, S_RIGHT_X]]) == ODD_THIRD_X).any()
    assert part("second swap").shape[0] == 16  # two pairs a row, eight rows


@pytest.mark.parametrize("height", [192, 96, 0])
@pytest.mark.parametrize("per", [1, 5, 60])
def test_soup_batches(soup, per, height):
    """Lists of 1, 5 and 60 triangles' edges (empty lists of back-facing
    objects among them), the full frame, half of it, and no rows at all.
    per 1: 1200 lists, so the count scan and the pack's list lookup cross
    workgroups; the totals leave the last 16-byte piece part filled."""
    words, counts = soup.records(3, per, lights=1)
    assert words.shape[0] > 0 and ((counts == 0).any() or per > 1)
    assert per > 1 or counts.shape[0] > 256
    gs, gc, ws = check(soup.r, words, counts, height, "soup per %d height %d" % (per, height))
    assert not is_nan(ws[:, NAN_WORDS]).any()  # Phong + Bitmap: the allowance was not used
    if height > 0:
        assert gs.shape[0] % 4 != 0 and gs.shape[0] > 256
    else:
        assert gs.shape[0] == 0 and (gc == 0).all()


@pytest.mark.parametrize("nl", [0, 1])
@pytest.mark.parametrize("setup", [0, 1, 2])
def test_soup_setups(soup, setup, nl):
    """FillEdgeTable's other setups: records without normals (a zero normal
    normalises to NaN on the first step) and without UV gradients."""
    words, counts = soup.records(setup, 5, lights=nl)
    gs, _, _ = check(soup.r, words, counts, 192, "soup setup %d lights %d" % (setup, nl))
    assert gs.shape[0] > 0
    if not (setup & abi.PRK_SETUP_PHONG):
        assert is_nan(gs[:, NORMAL_WORDS]).any()  # the NaN normals do come up


@pytest.mark.parametrize("height", [256, 128])
def test_sphere_one_list(sphere, height):
    """ConstructSphere as one list: many pairs a row, both swaps."""
    words, counts = sphere.records(3, 2208)
    assert counts.tolist() == [2072]
    gs, gc, ws = check(sphere.r, words, counts, height, "sphere height %d" % height)
    assert not is_nan(ws).any()
    rows = gs[:, S_ROW].view(np.int32)
    assert (np.diff(rows) >= 0).all() and np.bincount(rows).max() > 8


def test_spans_draw_the_lists_frame(gpu):
    """Composition: draw_spans of the device's spans is draw_edge_lists of
    the lists they came from (z bits and colours; ids number differently)."""
    s = scenes.random_soup(120, 64, 64, radius=12, seed=9, textured=True)

    def frame(use_spans):
        r = prk.Renderer()
        try:
            r.target_alloc(s.width, s.height)
            r.clear()
            r.set_camera(s.prk_transform(), s.prk_lights())
            tex = r.texture(s.texture)
            g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
            words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=6)
            if use_spans:
                spans, sc = r.span_records(words, counts, s.height)
                assert spans.shape[0] == int(sc.sum()) > 0
                r.draw_spans(spans, abi.PRK_SEM_AVX, bitmap=tex, phong=True)
            else:
                r.draw_edge_lists(words, counts, abi.PRK_SEM_AVX, bitmap=tex, phong=True)
            r.complete_all_work()
            return r.download()
        finally:
            r.close()

    ca, za = frame(False)
    cb, zb = frame(True)
    assert (ca != scenes.CLEAR_COLOR).any()
    assert np.array_equal(zb.view(np.uint32), za.view(np.uint32))
    assert np.array_equal(cb, ca)


def _raw(r, words, counts, height, spans, capacity, sc, total, nlist=None):
    import ctypes as C
    return r._L.prk_span_records(r._h, None if words is None else words.ctypes.data,
                                 None if counts is None else counts.ctypes.data,
                                 len(counts) if nlist is None else nlist, height,
                                 None if spans is None else spans.ctypes.data, capacity,
                                 None if sc is None else sc.ctypes.data,
                                 None if total is None else C.cast(total.ctypes.data, C.POINTER(C.c_uint64)))


def test_calling_pattern(gpu):
    words, counts = hand_batch()
    ws, wc, _, _ = spanref.walk_batch(words, counts, HAND_HEIGHT)
    n = ws.shape[0]
    r = prk.Renderer()
    try:
        # the count alone
        sc = np.full(counts.shape[0], 99, np.uint32)
        total = np.full(1, 99, np.uint64)
        assert _raw(r, words, counts, HAND_HEIGHT, None, 0, sc, total) == abi.PRK_OK
        assert total[0] == n and np.array_equal(sc, wc)
        # a short buffer: the totals, and the buffer as it was
        spans = np.full((n, 25), 0xA5A5A5A5, np.uint32)
        sc[:], total[0] = 99, 99
        assert _raw(r, words, counts, HAND_HEIGHT, spans, n - 1, sc, total) == abi.PRK_ERR_ARG
        assert total[0] == n and np.array_equal(sc, wc) and (spans == 0xA5A5A5A5).all()
        # room to spare: the spans, nothing past them; no span_counts asked for
        spans = np.full((n + 2, 25), 0xA5A5A5A5, np.uint32)
        total[0] = 99
        assert _raw(r, words, counts, HAND_HEIGHT, spans, n + 2, None, total) == abi.PRK_OK
        assert total[0] == n and np.array_equal(spans[:n], ws) and (spans[n:] == 0xA5A5A5A5).all()
        # nothing to walk
        total[0] = 99
        assert _raw(r, None, None, HAND_HEIGHT, None, 0, None, total, nlist=0) == abi.PRK_OK and total[0] == 0
        sc3, total[0] = np.full(3, 99, np.uint32), 99
        assert _raw(r, None, np.zeros(3, np.uint32), HAND_HEIGHT, spans, n + 2, sc3, total) == abi.PRK_OK
        assert total[0] == 0 and (sc3 == 0).all() and (spans[n:] == 0xA5A5A5A5).all()
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
        for fill in (True, False):
            for label, w, cnt, height, status in cases:
                spans = np.full((64, 25), 0xA5A5A5A5, np.uint32)
                sc = np.full(cnt.shape[0], 77, np.uint32)
                total = np.full(1, 99, np.uint64)
                assert _raw(r, w, cnt, height, spans if fill else None, 64 if fill else 0, sc, total) == status, label
                assert (spans == 0xA5A5A5A5).all() and (sc == 77).all() and total[0] == 0, label
        spans = np.full((64, 25), 0xA5A5A5A5, np.uint32)
        sc = np.full(2, 77, np.uint32)
        total = np.full(1, 99, np.uint64)
        assert _raw(r, good, None, 64, spans, 64, sc, total, nlist=2) == abi.PRK_ERR_ARG
        assert _raw(r, None, counts, 64, spans, 64, sc, total) == abi.PRK_ERR_ARG
        assert _raw(r, good, counts, 64, spans, 64, sc, None) == abi.PRK_ERR_ARG
        assert (spans == 0xA5A5A5A5).all() and (sc == 77).all()
        # ... and the same lists are taken once they are inside the rule
        gs, gc, _ = check(r, good, counts, 64, "accepted")
        assert gc.tolist() == [0, gs.shape[0]] and gs.shape[0] > 0
    finally:
        r.close()


def test_recorded_draws_and_stats_survive(gpu):
    """A call between the recording of a draw and its flush: the same frame,
    the same prk_stats."""
    s = scenes.random_soup(120, 64, 64, radius=12, seed=9)
    words, counts = hand_batch()

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
                gs, gc = r.span_records(words, counts, HAND_HEIGHT)
                assert gs.shape[0] > 0
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
