"""GPU tests: span handles (prk_spans_*, prk_draw_span_records) -- packed
prk_span records that stay on the device -- against prk_records_spans and
prk_draw_spans of the same spans from host memory.

The scene is the soup of test_gpu_span_records.py::test_spans_draw_the_lists_frame
(120 triangles, 64x64, six triangles an object: 20 lists, 1165
spans).  Every frame comparison is on bits (same_frame: z as uint32, colours
equal, winners equal) between the handle route and prk_draw_spans in a
renderer of its own.  k_span_handle_walk's workgroup is 256 spans
(prk_records.hip kHandleSpans): the lengths of test 3 are the issue's.
"""
import ctypes as C

import numpy as np
import pytest

import prk
from prk import abi, scenes
from test_gpu_edge_lists import AVX, AVX_ST, YMIN, Frame, same_frame
from test_gpu_records import offsets

pytestmark = pytest.mark.gpu

H = 64
S_ROW = 24  # prk_span word
PER = 6     # triangles an object


def scene():
    return scenes.random_soup(120, 64, H, radius=12, seed=9, textured=True)


@pytest.fixture(scope="module")
def base(gpu):
    """The soup's records as 6-triangle objects and the spans their walk
    queues over 64 rows, in host memory (prk_records_download / _spans)."""
    s = scene()
    with Frame(s, True) as f:
        rec = f.r.records_from_geometry(f.g, s.tri_count, P=s.P, setup=3, tris_per_object=PER)
        words, counts = rec.download(), rec.counts()
        spans, sc = rec.spans(H)
    assert counts.size == 20 and spans.shape[0] == int(sc.sum()) == 1165, (counts.size, spans.shape)
    for a in (words, counts, spans, sc):
        a.setflags(write=False)
    return s, words, counts, spans, sc


def draw_h(f, sp, mode=AVX, first=0, count=None):
    f.r.draw_span_records(sp, first, count, semantics=mode[0], bitmap=f.tex, phong=mode[1])


def draw_s(f, spans, mode=AVX):
    f.r.draw_spans(spans, semantics=mode[0], bitmap=f.tex, phong=mode[1])


def next_frame(f):
    out = f.done()
    f.r.clear()
    return out


# ---- 1. contents -----------------------------------------------------------------------------------------------------
def test_contents(base):
    s, words, counts, spans, sc = base
    with Frame(s, True) as f:
        rec = f.r.records_upload(words, counts)
        for height in (64, 32, 0):
            for a, n in ((0, None), (3, 9)):
                want, wc = rec.spans(height, a, n)
                sp = rec.spans(height, a, n, keep=True)
                label = "height %d lists %s" % (height, (a, n))
                assert (sp.list_count, sp.total) == (wc.size, want.shape[0]), label
                assert np.array_equal(sp.counts(), wc), label
                got = sp.download()
                assert got.dtype == np.uint32 and np.array_equal(got, want), label
                assert (height > 0) == (sp.total > 0), label
                sp.close()
        assert np.array_equal(rec.spans(H)[0], spans)
        # the optional outputs
        h, t = C.c_int32(-1), C.c_uint64(0)
        cnt = np.full(9, 77, np.uint32)
        assert f.r._L.prk_spans_from_records(f.r._h, rec.handle, 3, 9, H, C.byref(h), cnt.ctypes.data,
                                             C.byref(t)) == abi.PRK_OK
        assert h.value >= 0 and np.array_equal(cnt, sc[3:12]) and t.value == int(sc[3:12].sum())

        up = f.r.spans_upload(spans)
        assert (up.list_count, up.total) == (1, spans.shape[0]) and up.counts().tolist() == [spans.shape[0]]
        assert np.array_equal(up.download(), spans)
        empty = f.r.spans_upload(spans[:0])
        assert (empty.list_count, empty.total) == (1, 0) and empty.download().shape == (0, 25)

        rows, pairs, _ = rec.rows(H)
        assert pairs.shape[0] == spans.shape[0]
        ur = f.r.spans_upload_rows(rows, pairs)
        assert (ur.list_count, ur.total) == (1, spans.shape[0])
        assert np.array_equal(ur.download(), spans)
        none = f.r.spans_upload_rows(rows[:0], pairs[:0])
        assert (none.list_count, none.total) == (1, 0)


# ---- 2. draw parity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [AVX, AVX_ST], ids=["avx", "avx_st"])
def test_draw_parity(base, mode):
    s, words, counts, spans, sc = base
    with Frame(s, True) as f:
        rec = f.r.records_upload(words, counts)
        sp = rec.spans(H, keep=True)
        draw_h(f, sp, mode)
        h = f.done()
    with Frame(s, True) as f:
        draw_s(f, spans, mode)
        b = f.done()
    assert (h[0] != scenes.CLEAR_COLOR).any() and h[2].max() >= 900
    same_frame(h, b, "span handle against draw_spans")


# ---- 3. workgroup and alignment edges --------------------------------------------------------------------------------
LENGTHS = (0, 1, 3, 4, 255, 256, 257, 513)


@pytest.mark.parametrize("first", range(5))
def test_ranges_at_every_alignment(base, first):
    s, _, _, spans, _ = base
    part = spans[300:900]  # (600 spans from the middle rows of the frame)
    ranges = [(first, n) for n in LENGTHS]
    if first == 0:
        ranges += [(599, 1), (0, 600)]
    with Frame(s, True) as f, Frame(s, True) as g:
        sp = f.r.spans_upload(part)
        assert sp.total == 600
        for a, n in ranges:
            draw_h(f, sp, AVX, a, n)
            h = next_frame(f)
            draw_s(g, part[a:a + n])
            b = next_frame(g)
            if n == 0:
                assert (h[0] == scenes.CLEAR_COLOR).all() and (h[2] == -1).all()
            else:
                assert h[2].max() < n and (n < 255 or (h[2] >= 0).any()), (a, n)
            same_frame(h, b, "spans [%d, %d) of 600" % (a, a + n))


# ---- 4. rows outside the target --------------------------------------------------------------------------------------
OUT_ROWS = (-1, 0, H - 1, H, 0x7FFFFFF0, 15, 16, 47, 48, 30)


@pytest.mark.parametrize("band", [None, (16, 48)], ids=["full", "band"])
def test_rows_outside_the_target(base, band):
    s, _, _, spans, _ = base
    with Frame(s, True) as f:  # a span that covers pixels when drawn alone
        draw_s(f, spans)
        w = f.done()[2]
    k = int(np.bincount(w[w >= 0]).argmax())
    hand = np.repeat(spans[k:k + 1], len(OUT_ROWS), axis=0)
    hand[:, S_ROW] = np.array(OUT_ROWS, np.int64).astype(np.uint32)
    lo, hi = band if band else (0, H)
    inside = {i for i, r in enumerate(OUT_ROWS) if lo <= r < hi}
    with Frame(s, True, rows=band) as f, Frame(s, True, rows=band) as g:
        sp = f.r.spans_upload(hand)
        draw_h(f, sp)
        h = f.done()
        draw_s(g, hand)
        b = g.done()
    assert h[0].shape[0] == hi - lo
    assert set(np.unique(h[2]).tolist()) - {-1} == inside, (np.unique(h[2]), inside)
    for i in inside:  # every span on its own row of the target, and nowhere else
        assert set(np.nonzero((h[2] == i).any(1))[0].tolist()) == {OUT_ROWS[i] - lo}
    same_frame(h, b, "hand-made rows, %s target" % (band,))


# ---- 5. mixed pass and reuse -----------------------------------------------------------------------------------------
def test_mixed_pass_and_reuse(base):
    s, words, counts, spans, sc = base
    so = offsets(sc)

    def frame(handles):
        with Frame(s, True) as f:
            rec = f.r.records_upload(words, counts)
            one = rec.spans(H, 5, 8, keep=True)
            two = f.r.spans_upload(spans[500:1100])
            d1, d2 = one.download(), two.download()
            assert np.array_equal(d1, spans[so[5]:so[13]]) and one.total > 0

            def handle(sp, d, a=0, n=None):
                n = sp.total - a if n is None else n
                if handles:
                    draw_h(f, sp, AVX, a, n)
                else:
                    draw_s(f, d[a:a + n])

            f.objects(AVX, PER, first=0, count=30)
            draw_s(f, spans[:500])
            handle(one, d1)
            f.r.draw_records(rec, 12, 4, semantics=AVX[0], bitmap=f.tex, phong=True)
            handle(two, d2, 3, 500)
            handle(one, d1)
            first = next_frame(f)
            later = []
            for _ in range(2):  # the same handle in two consecutive frames
                handle(one, d1)
                later.append(next_frame(f))
            return first, later, 30 + 500 + one.total + 4 + 500 + one.total

    h, hl, ids = frame(True)
    b, bl, _ = frame(False)
    got = np.unique(h[2])
    assert got.max() < ids and (got < 30).any() and (got >= 30 + 500).any()
    same_frame(h, b, "mixed pass")
    assert (hl[0][0] != scenes.CLEAR_COLOR).any()
    same_frame(hl[0], bl[0], "the handle alone")
    same_frame(hl[1], hl[0], "the handle alone, the next frame")


# ---- 6. composition --------------------------------------------------------------------------------------------------
def test_composition_with_draw_records(base):
    s, words, counts, _, _ = base
    with Frame(s, True) as f:
        rec = f.r.records_upload(words, counts)
        draw_h(f, rec.spans(H, keep=True))
        h = next_frame(f)
        f.r.draw_records(rec, semantics=AVX[0], bitmap=f.tex, phong=True)
        b = f.done()
    assert (h[0] != scenes.CLEAR_COLOR).any()
    same_frame(h, b, "spans of the handle against draw_records of it", winners=False)  # (ids number differently)


# ---- 7. no span bytes staged -----------------------------------------------------------------------------------------
def test_handle_draw_stages_no_spans(base):
    s, _, _, spans, _ = base
    part = spans[300:900]
    with Frame(s, True) as f:
        sp = f.r.spans_upload(part)
        draw_h(f, sp, AVX, 0, 10)
        next_frame(f)
        few = f.r.stage_bytes()
        draw_h(f, sp)
        next_frame(f)
        many = f.r.stage_bytes()
        draw_s(f, part)
        f.done()
        host = f.r.stage_bytes()
    print("staging bytes: handle draw of 10 spans %d, of 600 spans %d, draw_spans of 600 %d" % (few, many, host))
    assert few == many
    assert 0 < many < 60000
    assert host >= 60000


# ---- 8. made before any target exists --------------------------------------------------------------------------------
def test_made_before_any_target(base):
    s, words, counts, spans, sc = base
    r = prk.Renderer()
    try:
        r.set_camera(s.prk_transform(), s.prk_lights())
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        rec = r.records_from_geometry(g, s.tri_count, P=s.P, setup=3, tris_per_object=PER)
        sp = rec.spans(H, keep=True)
        assert np.array_equal(sp.download(), spans) and np.array_equal(sp.counts(), sc)
        r.target_alloc(s.width, s.height)
        r.clear()
        r.set_debug(True)
        tex = r.texture(s.texture)
        r.draw_spans(spans[:300], abi.PRK_SEM_AVX, bitmap=tex, phong=True)  # a recorded draw ...
        before = dict(r.stats())
        again = rec.spans(H, 2, 5, keep=True)  # ... that a handle made meanwhile leaves alone
        assert again.total == int(sc[2:7].sum())
        assert dict(r.stats()) == before
        r.draw_span_records(sp, bitmap=tex)
        r.complete_all_work()
        h = r.download() + (r.winners(),)
    finally:
        r.close()
    with Frame(s, True) as f:
        draw_s(f, spans[:300])
        draw_s(f, spans)
        b = f.done()
    same_frame(h, b, "handle made before the target")


# ---- 9. lifetime and errors ------------------------------------------------------------------------------------------
def test_lifetime_and_errors(base):
    s, words, counts, spans, sc = base
    part = spans[300:900]
    with Frame(s, True) as f:
        L, ctx = f.r._L, f.r._h
        draw_s(f, part)
        want = next_frame(f)
        sp = f.r.spans_upload(part)
        other = f.r.spans_upload(part[:7])
        draw_h(f, sp)  # recorded before every refused call below
        n, t, h = C.c_uint32(0), C.c_uint64(0), C.c_int32(5)
        buf = np.empty((600, 25), np.uint32)
        for bad in (-1, 99):
            assert L.prk_draw_span_records(ctx, bad, 0, 1, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG
            assert L.prk_spans_info(ctx, bad, C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
            assert L.prk_spans_lists(ctx, bad, None) == abi.PRK_ERR_ARG
            assert L.prk_spans_download(ctx, bad, buf.ctypes.data, 600) == abi.PRK_ERR_ARG
            assert L.prk_spans_destroy(ctx, bad) == abi.PRK_ERR_ARG
            assert L.prk_spans_from_records(ctx, bad, 0, 1, H, C.byref(h), None, None) == abi.PRK_ERR_ARG
            assert h.value == -1
        dead = other.handle
        other.close()
        assert L.prk_draw_span_records(ctx, dead, 0, 1, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG
        assert L.prk_spans_info(ctx, dead, None, None) == abi.PRK_ERR_ARG
        assert L.prk_spans_destroy(ctx, dead) == abi.PRK_ERR_ARG
        assert L.prk_spans_info(ctx, sp.handle, None, None) == abi.PRK_OK
        # ranges
        assert L.prk_draw_span_records(ctx, sp.handle, 590, 11, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG  # 601 > 600
        assert L.prk_draw_span_records(ctx, sp.handle, 601, 0, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_span_records(ctx, sp.handle, 0xFFFFFFFF, 2, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_span_records(ctx, sp.handle, 600, 0, AVX[0], 1, f.tex) == abi.PRK_OK  # nothing recorded
        assert L.prk_draw_span_records(ctx, sp.handle, 0, 600, 77, 1, f.tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_span_records(ctx, sp.handle, 0, 600, AVX[0], 1, f.tex + 5) == abi.PRK_ERR_ARG
        assert L.prk_spans_download(ctx, sp.handle, buf.ctypes.data, 599) == abi.PRK_ERR_ARG
        assert L.prk_spans_upload(ctx, None, 3, C.byref(h)) == abi.PRK_ERR_ARG and h.value == -1
        # PRK_ERR_UNSUPPORTED exactly where prk_draw_spans gives it
        cases = [(abi.PRK_SEM_SCALAR, 1, f.tex), (abi.PRK_SEM_SCALAR, 0, -1), (AVX[0], 1, -1), (AVX[0], 0, f.tex),
                 (AVX_ST[0], 0, f.tex), (AVX_ST[0], 1, -1)]
        for sem, phong, tex in cases:
            assert L.prk_draw_spans(ctx, part.ctypes.data, 600, sem, phong, tex) == abi.PRK_ERR_UNSUPPORTED
            assert L.prk_draw_span_records(ctx, sp.handle, 0, 600, sem, phong, tex) == abi.PRK_ERR_UNSUPPORTED
        # a record handle with an unsorted list
        ymin = words[:, YMIN].view(np.int32)
        o = offsets(counts)
        i = next(j for j in range(1, words.shape[0]) if j not in o and ymin[j] > ymin[j - 1])  # (inside a list)
        sw = words.copy()
        sw[[i - 1, i], YMIN] = words[[i, i - 1], YMIN]
        rec = f.r.records_upload(sw, counts)
        k = int(np.searchsorted(o, i, side="right")) - 1
        assert rec.sorted_flags()[k] == 0
        h.value = 5
        assert L.prk_spans_from_records(ctx, rec.handle, 0, counts.size, H, C.byref(h), None,
                                        C.byref(t)) == abi.PRK_ERR_UNSUPPORTED
        assert h.value == -1
        assert L.prk_records_spans(ctx, rec.handle, 0, counts.size, H, None, 0, None,
                                   C.byref(t)) == abi.PRK_ERR_UNSUPPORTED
        h.value = 5
        assert L.prk_spans_from_records(ctx, rec.handle, 0, counts.size + 1, H, C.byref(h), None,
                                        None) == abi.PRK_ERR_ARG and h.value == -1
        assert L.prk_spans_from_records(ctx, rec.handle, 0, 1, -1, C.byref(h), None, None) == abi.PRK_ERR_ARG
        assert L.prk_spans_from_records(ctx, rec.handle, 0, 1, H, None, None, None) == abi.PRK_ERR_ARG
        # prk_draw_rows' argument checks
        rows = np.array([[3, 2]], np.int32)
        pairs = np.zeros((3, 24), np.uint32)
        assert L.prk_spans_upload_rows(ctx, rows.ctypes.data, 1, pairs.ctypes.data, 3, C.byref(h)) == abi.PRK_ERR_ARG
        rows[0] = (-3, 3)
        assert L.prk_spans_upload_rows(ctx, rows.ctypes.data, 1, pairs.ctypes.data, 3, C.byref(h)) == abi.PRK_ERR_ARG
        assert h.value == -1
        # a recorded, unflushed draw names the handle
        assert L.prk_spans_destroy(ctx, sp.handle) == abi.PRK_ERR_ARG
        got = next_frame(f)  # the flush draws what was recorded before the refusals, unchanged
        same_frame(got, want, "after refused calls")
        draw_h(f, sp)
        assert L.prk_spans_destroy(ctx, sp.handle) == abi.PRK_ERR_ARG
        f.r.reset_draws()
        assert L.prk_spans_destroy(ctx, sp.handle) == abi.PRK_OK
        assert L.prk_spans_info(ctx, sp.handle, C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
        c, z, w = f.done()
        assert (c == scenes.CLEAR_COLOR).all() and (w == -1).all()
        # ... and after the flush that drew it
        sp2 = f.r.spans_upload(part)
        draw_h(f, sp2)
        got = f.done()
        same_frame(got, want, "a second handle of the same spans")
        assert L.prk_spans_destroy(ctx, sp2.handle) == abi.PRK_OK
