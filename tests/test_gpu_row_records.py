"""GPU tests: prk_row_records (the row work DrawModelOptimizedLines queues for
every list of a batch, from the device's list walk) against tests/rowref.py,
the Python restatement of that row loop which tests/test_row_records_api.py
holds to spanref; and prk_draw_rows against prk_draw_spans.

Rows ([k, 2] int32: RowIndex, EdgeCount) and row counts are compared with
plain equality, always.  Pairs ([m, 24] uint32) carry prk.h's one allowance:
where the expected MinColor / MinNormal word is a NaN, the device's word must
be a NaN, of any sign and payload; every other word must be equal, and a NaN
where none is expected fails (same_pairs).  The hand-made lists and the Phong
+ Bitmap batches hold no NaN in those words and are compared with no
allowance at all.
"""
import ctypes as C

import numpy as np
import pytest

import prk
import rowref
from prk import abi, scenes
from test_gpu_span_records import LEFT, LIGHTS, YMIN, Ctx, _soup, _sphere_scene, edge, is_nan

pytestmark = pytest.mark.gpu

# prk_row_pair words: 10 interleaved scalars, LeftMinColor, RightMinColor, LeftMinNormal, RightMinNormal
P_LEFT_X, P_RIGHT_X = 0, 1
NAN_WORDS = list(range(10, 24))
NORMAL_WORDS = list(range(18, 24))
CANARY = 0xA5A5A5A5


def same_pairs(got, want, label):
    """got == want word for word, but a NaN where (and only where) the
    expected MinColor / MinNormal word is a NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (label, got.shape, want.shape)
    allow = np.zeros(24, bool)
    allow[NAN_WORDS] = True
    wn = is_nan(want) & allow
    ok = np.where(wn, is_nan(got), got == want)
    bad = np.nonzero(~ok.all(1))[0]
    if bad.size:
        r = int(bad[0])
        f = np.nonzero(~ok[r])[0]
        raise AssertionError("%s: %d of %d pairs differ; pair %d words %s got %s want %s" % (
            label, bad.size, got.shape[0], r, f.tolist(), [hex(x) for x in got[r, f]], [hex(x) for x in want[r, f]]))


def check(r, words, counts, height, label, exact=False):
    """The device's rows, pairs and counts against rowref's; returns both."""
    gr, gp, gc = r.row_records(words, counts, height)
    wr, wp, wc = rowref.walk_batch(words, counts, height)
    assert gc.dtype == np.uint32 and np.array_equal(gc, wc), (label, "row counts", np.nonzero(gc != wc)[0][:5])
    assert gr.dtype == np.int32 and gr.shape == wr.shape, (label, gr.shape, wr.shape)
    assert np.array_equal(gr, wr), (label, "rows", np.nonzero((gr != wr).any(1))[0][:5])
    if exact:
        assert np.array_equal(gp, wp), label
    else:
        same_pairs(gp, wp, label)
    return gr, gp, gc, wp


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


HAND_HEIGHT = 64
HAND_LISTS = [
    ("empty", []),
    ("one edge", [edge(4, 11, 5.0, 0.5, 1)]),
    ("triangle", [edge(2, 20, 10.0, -0.25, 1), edge(2, 12, 10.0, 1.0, 0, 1), edge(12, 20, 20.0, -1.5, 0, 2)]),
    # two triangles, the rows 10..29 between them empty
    ("y gap", [edge(0, 10, 1.0, 0.0, 1), edge(0, 10, 9.0, -0.5, 0, 1), edge(0, 4, 1.0, 1.0, 0, 2),
               edge(30, 38, 3.0, 0.5, 1, 3), edge(30, 38, 8.0, 0.25, 0, 4), edge(30, 33, 3.0, 2.0, 0, 5)]),
    # three edges listed at once: one pair, the third unpaired; then it alone (rows 9..13: EdgeCount 0)
    ("three active", [edge(3, 9, 1.0, 0.0, 1), edge(3, 9, 6.0, 0.0, 0, 1), edge(3, 14, 40.0, 0.0, 1, 2)]),
    # the pair's X cross on the third row: Left / Right are the edges before the swap
    ("crossing", [edge(0, 12, 0.0, 2.0, 1), edge(0, 12, 10.0, -2.0, 0, 1)]),
    ("clipped by height", [edge(50, 100, 2.0, 0.5, 1), edge(50, 100, 50.0, -0.5, 0, 1)]),
    ("starts at height", [edge(HAND_HEIGHT, 80, 1.0, 0.0, 1), edge(HAND_HEIGHT + 5, 80, 4.0, 0.0, 0, 1)]),
    ("empty last", []),
]


def hand_batch():
    counts = np.array([len(l) for _, l in HAND_LISTS], np.uint32)
    words = np.array([e for _, l in HAND_LISTS for e in l], np.uint32).reshape(-1, 27)
    return words, counts


def test_hand_made_lists(gpu):
    words, counts = hand_batch()
    r = prk.Renderer()
    try:
        gr, gp, gc, _ = check(r, words, counts, HAND_HEIGHT, "hand", exact=True)
        zr, zp, zc, _ = check(r, words, counts, 0, "hand height 0", exact=True)
    finally:
        r.close()
    assert zr.shape[0] == 0 and zp.shape[0] == 0 and (zc == 0).all()
    names = [n for n, _ in HAND_LISTS]
    roff = np.concatenate([[0], np.cumsum(gc.astype(np.int64))])
    poff = np.concatenate([[0], np.cumsum(gr[:, 1].astype(np.int64))])

    def part(name):
        o = names.index(name)
        rows = gr[roff[o]:roff[o + 1]]
        return rows, gp[poff[roff[o]]:poff[roff[o + 1]]]

    F = lambda a: a.view(np.float32)  # noqa: E731
    for name in ("empty", "empty last", "starts at height"):
        assert part(name)[0].shape[0] == 0, name
    rows, pairs = part("one edge")
    assert rows.tolist() == [[y, 0] for y in range(4, 11)] and pairs.shape[0] == 0
    rows, pairs = part("triangle")
    assert rows.tolist() == [[y, 1] for y in range(2, 20)] and pairs.shape[0] == 18
    rows, pairs = part("y gap")
    assert rows[:, 0].tolist() == list(range(0, 10)) + list(range(30, 38))
    # the third edge of each triangle is listed unpaired while it lasts
    assert rows[:, 1].tolist() == [1] * 18
    rows, pairs = part("three active")
    assert rows.tolist() == [[y, 1] for y in range(3, 9)] + [[y, 0] for y in range(9, 14)]
    assert not (F(pairs[:, [P_LEFT_X, P_RIGHT_X]]) == 40.0).any()
    rows, pairs = part("crossing")
    assert rows.tolist() == [[y, 1] for y in range(12)]
    assert F(pairs[:3, P_LEFT_X]).tolist() == [0.0, 2.0, 4.0] and F(pairs[:3, P_RIGHT_X]).tolist() == [10.0, 8.0, 6.0]
    # the step after row 2 crosses them (6, 4): from row 3 on the second edge is Left
    assert F(pairs[3:, P_LEFT_X]).tolist() == [4.0 - 2.0 * k for k in range(9)]
    assert F(pairs[3:, P_RIGHT_X]).tolist() == [6.0 + 2.0 * k for k in range(9)]
    rows, pairs = part("clipped by height")
    assert rows.tolist() == [[y, 1] for y in range(50, 64)]


@pytest.mark.parametrize("height", [192, 96, 0])
@pytest.mark.parametrize("per", [1, 5, 60])
def test_soup_batches(soup, per, height):
    """Lists of 1, 5 and 60 triangles' edges (empty lists of back-facing
    objects among them).  per 1: 1200 lists, so both scans and both list
    lookups of the pack cross workgroups.  Phong + Bitmap: plain equality."""
    words, counts = soup.records(3, per, lights=1)
    assert per > 1 or counts.shape[0] > 256
    gr, gp, gc, wp = check(soup.r, words, counts, height, "soup per %d height %d" % (per, height), exact=True)
    assert not is_nan(wp[:, NAN_WORDS]).any()
    if height > 0:
        assert gp.shape[0] > 256 and gr.shape[0] > 256
        # a triangle's rows pair two of its three edges: one pair a row, never more for per 1
        assert per > 1 or (gr[:, 1] <= 1).all()
    else:
        assert gp.shape[0] == 0 and gr.shape[0] == 0 and (gc == 0).all()


@pytest.mark.parametrize("nl", [0, 1])
@pytest.mark.parametrize("setup", [0, 1, 2])
def test_soup_setups(soup, setup, nl):
    """FillEdgeTable's other setups: records without normals (a zero normal
    normalises to NaN on the first step) and without UV gradients."""
    words, counts = soup.records(setup, 5, lights=nl)
    gr, gp, _, _ = check(soup.r, words, counts, 192, "soup setup %d lights %d" % (setup, nl))
    assert gp.shape[0] > 0
    if not (setup & abi.PRK_SETUP_PHONG):
        assert is_nan(gp[:, NORMAL_WORDS]).any()  # the NaN normals do come up


def test_sphere_one_list(sphere):
    """ConstructSphere as one list: many pairs a row, both swaps."""
    words, counts = sphere.records(3, 2208)
    assert counts.tolist() == [2072]
    gr, gp, gc, wp = check(sphere.r, words, counts, 256, "sphere", exact=True)
    assert gc.tolist() == [gr.shape[0]] and (np.diff(gr[:, 0]) > 0).all() and gr[:, 1].max() > 8


def _raw(r, words, counts, height, rows, rcap, pairs, pcap, rc, nrow, npair, nlist=None):
    p64 = lambda a: None if a is None else C.cast(a.ctypes.data, C.POINTER(C.c_uint64))  # noqa: E731
    d = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return r._L.prk_row_records(r._h, d(words), d(counts), len(counts) if nlist is None else nlist, height,
                                d(rows), rcap, d(pairs), pcap, d(rc), p64(nrow), p64(npair))


def _crowd(n):
    """n edges of one row, X strictly descending in index order: every
    insertion is at the head, so the walk is n (n - 1) / 2 + n list steps by
    the host's bound and short in fact."""
    return np.array([edge(3, 4, float(n - i), 0.0, i & 1) for i in range(n)], np.uint32)


def test_the_1000_pair_line(gpu):
    assert 2002 * 2001 // 2 + 2002 < 1 << 21  # inside the step cap: the refusal below is the walk's
    r = prk.Renderer()
    try:
        w = _crowd(2000)
        gr, gp, gc, _ = check(r, w, np.array([2000], np.uint32), 64, "1000 pairs", exact=True)
        assert gr.tolist() == [[3, 1000]] and gp.shape[0] == 1000 and gc.tolist() == [1]
        w, cnt = _crowd(2002), np.array([2002], np.uint32)
        for fill in (True, False):
            rows = np.full((8, 2), CANARY, np.uint32)
            pairs = np.full((1100, 24), CANARY, np.uint32)
            rc, nrow, npair = np.full(1, 77, np.uint32), np.full(1, 99, np.uint64), np.full(1, 98, np.uint64)
            st = _raw(r, w, cnt, 64, rows if fill else None, 8 if fill else 0, pairs if fill else None,
                      1100 if fill else 0, rc, nrow, npair)
            assert st == abi.PRK_ERR_UNSUPPORTED, fill
            assert (rows == CANARY).all() and (pairs == CANARY).all()
            assert rc[0] == 77 and nrow[0] == 99 and npair[0] == 98
    finally:
        r.close()


def test_calling_pattern(gpu):
    words, counts = hand_batch()
    wr, wp, wc = rowref.walk_batch(words, counts, HAND_HEIGHT)
    nr, npr = wr.shape[0], wp.shape[0]
    r = prk.Renderer()
    try:
        rc, nrow, npair = np.full(counts.shape[0], 99, np.uint32), np.full(1, 99, np.uint64), np.full(1, 99, np.uint64)
        # sizing only
        assert _raw(r, words, counts, HAND_HEIGHT, None, 0, None, 0, rc, nrow, npair) == abi.PRK_OK
        assert nrow[0] == nr and npair[0] == npr and np.array_equal(rc, wc)
        # exact capacities; no row_counts asked for
        rows, pairs = np.full((nr + 2, 2), CANARY, np.uint32), np.full((npr + 2, 24), CANARY, np.uint32)
        nrow[0] = npair[0] = 99
        assert _raw(r, words, counts, HAND_HEIGHT, rows, nr, pairs, npr, None, nrow, npair) == abi.PRK_OK
        assert nrow[0] == nr and npair[0] == npr
        assert np.array_equal(rows[:nr].view(np.int32), wr) and np.array_equal(pairs[:npr], wp)
        assert (rows[nr:] == CANARY).all() and (pairs[npr:] == CANARY).all()  # nothing past them
        # each capacity one short: the totals, and both arrays as they were
        for rcap, pcap in ((nr - 1, npr), (nr, npr - 1)):
            rows[:], pairs[:], rc[:] = CANARY, CANARY, 99
            nrow[0] = npair[0] = 99
            assert _raw(r, words, counts, HAND_HEIGHT, rows, rcap, pairs, pcap, rc, nrow, npair) == abi.PRK_ERR_ARG
            assert nrow[0] == nr and npair[0] == npr and np.array_equal(rc, wc)
            assert (rows == CANARY).all() and (pairs == CANARY).all()
        # one array NULL
        rc[:] = 99
        nrow[0] = npair[0] = 99
        assert _raw(r, words, counts, HAND_HEIGHT, rows, nr, None, 0, rc, nrow, npair) == abi.PRK_ERR_ARG
        assert _raw(r, words, counts, HAND_HEIGHT, None, 0, pairs, npr, rc, nrow, npair) == abi.PRK_ERR_ARG
        assert (rows == CANARY).all() and (pairs == CANARY).all() and (rc == 99).all() and nrow[0] == npair[0] == 99
        # nothing to walk
        assert _raw(r, None, None, HAND_HEIGHT, None, 0, None, 0, None, nrow, npair, nlist=0) == abi.PRK_OK
        assert nrow[0] == 0 and npair[0] == 0
        rc3 = np.full(3, 99, np.uint32)
        nrow[0] = npair[0] = 99
        assert _raw(r, None, np.zeros(3, np.uint32), HAND_HEIGHT, rows, nr, pairs, npr, rc3, nrow, npair) == abi.PRK_OK
        assert nrow[0] == 0 and npair[0] == 0 and (rc3 == 0).all() and (rows == CANARY).all()
    finally:
        r.close()


def test_refusals(gpu):
    """The table of test_gpu_span_records.py::test_refusals for this call:
    every refusal leaves every output as it was."""
    good = np.array([edge(0, 10, 0.0, 1.0, 1), edge(0, 10, 9.0, 0.0, 0, 1), edge(4, 12, 3.0, 0.0, 1, 2)], np.uint32)
    counts = np.array([0, 3], np.uint32)

    def variant(row, word, value):
        w = good.copy()
        w[row, word] = np.array([value], np.int32).view(np.uint32)[0]
        return w

    # 257 edges over 65536 rows: 2^24 + 2^16 edge-rows, over the one-thread cap
    long_list = np.array([edge(0, 65536, float(i), 0.0, i & 1) for i in range(257)], np.uint32)
    # one row, X ascending: every insertion scans all the edges before it, 2.2 M list steps
    crowd = np.array([edge(0, 1, float(i), 0.0, i & 1) for i in range(2100)], np.uint32)
    cases = [
        ("YMin out of order", variant(1, YMIN, 5), counts, 64, abi.PRK_ERR_UNSUPPORTED),
        ("YMin < 0", variant(0, YMIN, -1), counts, 64, abi.PRK_ERR_UNSUPPORTED),
        ("Left = 2", variant(1, LEFT, 2), counts, 64, abi.PRK_ERR_UNSUPPORTED),
        ("height -1", good, counts, -1, abi.PRK_ERR_ARG),
        ("height 65537", good, counts, 65537, abi.PRK_ERR_LIMIT),
        ("over the edge-row cap", long_list, np.array([257], np.uint32), 65536, abi.PRK_ERR_LIMIT),
        ("insertion scans over the cap", crowd, np.array([2100], np.uint32), 64, abi.PRK_ERR_LIMIT),
    ]
    r = prk.Renderer()
    try:
        def outputs(nlist):
            return (np.full((64, 2), CANARY, np.uint32), np.full((64, 24), CANARY, np.uint32),
                    np.full(nlist, 77, np.uint32), np.full(1, 99, np.uint64), np.full(1, 98, np.uint64))

        def untouched(rows, pairs, rc, nrow, npair):
            return ((rows == CANARY).all() and (pairs == CANARY).all() and (rc == 77).all() and nrow[0] == 99 and
                    npair[0] == 98)

        for fill in (True, False):
            for label, w, cnt, height, status in cases:
                rows, pairs, rc, nrow, npair = outputs(cnt.shape[0])
                st = _raw(r, w, cnt, height, rows if fill else None, 64 if fill else 0, pairs if fill else None,
                          64 if fill else 0, rc, nrow, npair)
                assert st == status, (label, fill, st)
                assert untouched(rows, pairs, rc, nrow, npair), (label, fill)
        rows, pairs, rc, nrow, npair = outputs(2)
        assert _raw(r, good, None, 64, rows, 64, pairs, 64, rc, nrow, npair, nlist=2) == abi.PRK_ERR_ARG
        assert _raw(r, None, counts, 64, rows, 64, pairs, 64, rc, nrow, npair) == abi.PRK_ERR_ARG
        assert _raw(r, good, counts, 64, rows, 64, pairs, 64, rc, None, npair) == abi.PRK_ERR_ARG
        assert _raw(r, good, counts, 64, rows, 64, pairs, 64, rc, nrow, None) == abi.PRK_ERR_ARG
        assert untouched(rows, pairs, rc, nrow, npair)
        # ... and the same lists are taken once they are inside the rule
        gr, gp, gc, _ = check(r, good, counts, 64, "accepted", exact=True)
        assert gc.tolist() == [0, 12] and gr[:, 0].tolist() == list(range(12)) and gp.shape[0] == 10
    finally:
        r.close()


DRAW_SCENE = dict(n=160, width=128, height=96, radius=14, seed=9)


def _draw_frame(how, bad=None):
    """One frame of a soup's lists at 128x96, drawn from their row records,
    their span records or the lists themselves: (colour, z, winners)."""
    d = DRAW_SCENE
    s = scenes.random_soup(d["n"], d["width"], d["height"], radius=d["radius"], seed=d["seed"], textured=True)
    r = prk.Renderer()
    try:
        r.target_alloc(s.width, s.height)
        r.clear()
        r.set_debug(True)  # (winner ids)
        r.set_camera(s.prk_transform(), s.prk_lights())
        tex = r.texture(s.texture)
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=6)
        if how == "rows":
            rows, pairs, rc = r.row_records(words, counts, s.height)
            assert pairs.shape[0] == int(rows[:, 1].sum()) > 0 and rows.shape[0] == int(rc.sum())
            if bad is not None:
                bad(r, rows, pairs, tex)
            r.draw_rows(rows, pairs, abi.PRK_SEM_AVX, bitmap=tex, phong=True)
        elif how == "spans":
            spans, _ = r.span_records(words, counts, s.height)
            r.draw_spans(spans, abi.PRK_SEM_AVX, bitmap=tex, phong=True)
        else:
            r.draw_edge_lists(words, counts, abi.PRK_SEM_AVX, bitmap=tex, phong=True)
        r.complete_all_work()
        c, z = r.download()
        return c, z, r.winners(), r.stats()["triangles"]
    finally:
        r.close()


def test_rows_draw_the_spans_frame(gpu):
    def refused(r, rows, pairs, tex):
        """Draws that must record nothing: the frame after them is the same."""
        L, h = r._L, r._h
        rp, pp, nr, npr = rows.ctypes.data, pairs.ctypes.data, rows.shape[0], pairs.shape[0]
        assert L.prk_draw_rows(h, rp, nr, pp, npr - 1, abi.PRK_SEM_AVX, 1, tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_rows(h, rp, nr - 1, pp, npr, abi.PRK_SEM_AVX, 1, tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_rows(h, None, nr, pp, npr, abi.PRK_SEM_AVX, 1, tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_rows(h, rp, nr, None, npr, abi.PRK_SEM_AVX, 1, tex) == abi.PRK_ERR_ARG
        neg = rows.copy()
        neg[0, 0] = -1
        assert L.prk_draw_rows(h, neg.ctypes.data, nr, pp, npr, abi.PRK_SEM_AVX, 1, tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_rows(h, rp, nr, pp, npr, abi.PRK_SEM_SCALAR, 1, tex) == abi.PRK_ERR_UNSUPPORTED
        assert L.prk_draw_rows(h, rp, 0, pp, 0, abi.PRK_SEM_AVX, 1, tex) == abi.PRK_OK
        assert L.prk_draw_rows(h, rp, nr, pp, npr, 77, 1, tex) == abi.PRK_ERR_ARG

    cr, zr, wr, tr = _draw_frame("rows", bad=refused)
    cs, zs, ws, ts = _draw_frame("spans")
    cl, zl, _, _ = _draw_frame("lists")
    assert (cs != scenes.CLEAR_COLOR).any()
    assert np.array_equal(zr.view(np.uint32), zs.view(np.uint32)) and np.array_equal(cr, cs)
    assert np.array_equal(wr, ws) and tr == ts  # one id per pair, none for a row without pairs
    assert np.array_equal(zr.view(np.uint32), zl.view(np.uint32)) and np.array_equal(cr, cl)


def test_recorded_draws_and_stats_survive(gpu):
    """A prk_row_records call between the recording of a draw and its flush:
    the same frame, the same prk_stats."""
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
                gr, gp, _ = r.row_records(words, counts, HAND_HEIGHT)
                assert gr.shape[0] > 0 and gp.shape[0] > 0
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
