"""GPU tests: record handles (prk_records_*, prk_draw_records) -- edge lists
that stay on the device -- against prk_edge_records / prk_draw_edge_lists of
the same lists from host memory, and against the whole-object draw.

Every comparison is on bits (same_frame: z as uint32, colours equal, winners
equal).  A whole-object draw numbers its winners by triangle and a batch by
list, so an object frame's winners are compared as triangle // per.
"""
import ctypes as C

import numpy as np
import pytest

import prk
from prk import abi, scenes
from test_gpu_edge_lists import (AVX, AVX_ST, SC_GOURAUD, YMIN, Frame, large_objects, same_frame, soup_scene,
                                 sphere_scene)

pytestmark = pytest.mark.gpu

YMAX, LEFT = 0, 12  # prk_edge words


def rule(words, counts):
    """prk_draw_edge_lists' sorted rule per list, as prk.h states it."""
    ymin, ymax = words[:, YMIN].view(np.int32).astype(np.int64), words[:, YMAX].view(np.int32).astype(np.int64)
    out, o = [], 0
    for n in counts.tolist():
        a, b, left = ymin[o:o + n], ymax[o:o + n], words[o:o + n, LEFT]
        prev = np.concatenate([[0], a[:-1]]) if n else a
        out.append(int(bool((a >= prev).all() and (b >= a).all() and (left <= 1).all())))
        o += n
    return np.array(out, np.uint32)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts.astype(np.int64))])


def make_batch(pool, counts):
    """Lists of `counts` real records each: consecutive slices of the pool
    repeated, every slice sorted by YMin (stable) -- inside the sorted rule."""
    total = int(counts.sum())
    src = np.tile(pool, (total // pool.shape[0] + 1, 1))[:total]
    off = offsets(counts)
    parts = []
    for o in range(counts.size):
        w = src[off[o]:off[o + 1]]
        parts.append(w[np.argsort(w[:, YMIN].view(np.int32), kind="stable")])
    return np.ascontiguousarray(np.concatenate(parts)), counts


@pytest.fixture(scope="module")
def soup(gpu):
    """The soup's records as 20-triangle objects (AVX setup), from the host call."""
    s = soup_scene()
    with Frame(s, True) as f:
        words, counts = f.records(3, 20)
    return s, words, counts


def handle_frame(f, rec, mode, first=0, count=None):
    f.r.draw_records(rec, first, count, semantics=mode[0], bitmap=f.tex, phong=mode[1])


def both_frames(f, words, counts, mode=AVX):
    """(frame of the uploaded handle, frame of the host batch, flags) on one context."""
    rec = f.r.records_upload(words, counts)
    flags = rec.sorted_flags()
    assert np.array_equal(rec.counts(), counts) and (rec.list_count, rec.total) == (counts.size, words.shape[0])
    f.r.clear()
    handle_frame(f, rec, mode)
    h = f.done()
    rec.close()
    f.r.clear()
    f.batch(words, counts, mode)
    return h, f.done(), flags


# ---- 1. round trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [AVX, AVX_ST, SC_GOURAUD], ids=["avx", "avx_st", "scalar_gouraud"])
def test_round_trip(gpu, mode):
    s = soup_scene()
    with Frame(s, mode[2]) as f:
        words, counts = f.records(mode[3], 20)
        rec = f.r.records_from_geometry(f.g, s.tri_count, P=s.P, setup=mode[3], tris_per_object=20)
        assert (rec.list_count, rec.total) == (15, words.shape[0]) and rec.total > 0
        assert np.array_equal(rec.counts(), counts)
        assert np.array_equal(rec.download(), words)
        assert np.array_equal(rec.sorted_flags(), rule(words, counts)) and rec.sorted_flags().all()
        handle_frame(f, rec, mode)
        h = f.done()
        f.r.clear()
        f.batch(words, counts, mode)
        b = f.done()
        f.r.clear()
        f.objects(mode, 20)
        oc, oz, ow = f.done()
    assert (h[0] != scenes.CLEAR_COLOR).any()
    same_frame(h, b, "handle against draw_edge_lists of its records")
    same_frame(h, (oc, oz, np.where(ow >= 0, ow // 20, -1)), "handle against the 20-triangle objects")


# ---- 2. the rule kernel ----------------------------------------------------------------------------------------------
RULE_COUNTS = np.array([0, 1, 63, 64, 65, 0, 255, 257, 1, 300], np.uint32)


def rule_variants(words, counts):
    """(label, words) with one violation each; flat record indices: list 6 is
    [193, 448), list 7 [448, 705), list 9 [706, 1006)."""
    off = offsets(counts)
    ymin = words[:, YMIN].view(np.int32)

    def decreasing(e):
        w = words.copy()
        assert off.tolist().count(e) == 0 and ymin[e - 1] > 0  # (not a list's first edge)
        w[e, YMIN] = np.uint32(ymin[e - 1] - 1)
        return w

    neg = words.copy()
    neg[off[3], YMIN] = np.uint32(0xFFFFFFFF)  # list 3's first edge: YMin -1
    ymax = words.copy()
    ymax[500, YMAX] = np.uint32(np.int64(ymin[500]) - 1 & 0xFFFFFFFF)
    left = words.copy()
    left[900, LEFT] = 2
    return [("clean", words), ("first edge negative", neg), ("last edge decreasing", decreasing(int(off[5]) - 1)),
            ("lane 0 of a wave", decreasing(320)), ("thread 0 of a workgroup", decreasing(256)),
            ("thread 0 of the last workgroup", decreasing(768)), ("YMax < YMin", ymax), ("Left == 2", left)]


def test_rule_kernel(soup):
    s, pool, _ = soup
    words, counts = make_batch(pool, RULE_COUNTS)
    assert rule(words, counts).all()
    off = offsets(counts)
    ymin = words[:, YMIN].view(np.int32)
    # a list that starts below the previous list's last YMin is still sorted
    assert ymin[off[4]] < ymin[off[4] - 1] and ymin[off[9]] < ymin[off[9] - 1]
    with Frame(s, True) as f:
        for label, w in rule_variants(words, counts):
            want = rule(w, counts)
            assert int((want == 0).sum()) == (0 if label == "clean" else 1), label
            h, b, flags = both_frames(f, w, counts)
            assert np.array_equal(flags, want), "%s: flags %s, rule %s" % (label, flags, want)
            assert (h[0] != scenes.CLEAR_COLOR).any()
            same_frame(h, b, "rule variant '%s'" % label)


# ---- 3. sub-ranges and alignment -------------------------------------------------------------------------------------
SUB_COUNTS = np.array([5, 4, 5, 5, 0, 9, 70, 0, 3, 300, 2], np.uint32)
# (first_list, list_count): record offsets 0, 5, 14 and 19 -- 0, 1, 2 and 3 mod 4 -- each ending before
# the last list (two of them over more than one workgroup of 256 records); then a single empty list
SUB_RANGES = [(0, 6), (1, 9), (3, 7), (5, 5), (4, 1)]


def test_sub_ranges_at_every_alignment(soup):
    s, pool, _ = soup
    words, counts = make_batch(pool, SUB_COUNTS)
    off = offsets(counts)
    assert [int(off[a]) % 4 for a, _ in SUB_RANGES[:4]] == [0, 1, 2, 3]
    assert all(a + n < counts.size for a, n in SUB_RANGES)
    with Frame(s, True) as f:
        rec = f.r.records_upload(words, counts)
        for a, n in SUB_RANGES:
            f.r.clear()
            handle_frame(f, rec, AVX, a, n)
            h = f.done()
            f.r.clear()
            f.batch(words[off[a]:off[a + n]], counts[a:a + n], AVX)
            b = f.done()
            if (a, n) == (4, 1):
                assert (h[0] == scenes.CLEAR_COLOR).all() and (h[2] == -1).all()
            else:
                assert (h[0] != scenes.CLEAR_COLOR).any() and h[2].max() < n
            same_frame(h, b, "lists [%d, %d)" % (a, a + n))


# ---- 4. one large list -----------------------------------------------------------------------------------------------
def test_large_list_takes_a_parallel_walk(gpu):
    s = sphere_scene()
    with Frame(s, True) as f:
        rec = f.r.records_from_geometry(f.g, s.tri_count, P=s.P, setup=3, tris_per_object=s.tri_count)
        assert rec.list_count == 1 and rec.total >= 144 and rec.sorted_flags().tolist() == [1]
        words = rec.download()
        handle_frame(f, rec, AVX)
        h = f.done()
        routes = f.r.walk_routes()
    assert large_objects(routes) == 1, routes
    with Frame(s, True) as f:
        f.objects(AVX, s.tri_count)
        oc, oz, ow = f.done()
    assert (h[0] != scenes.CLEAR_COLOR).any() and set(np.unique(h[2])) == {-1, 0}
    same_frame(h, (oc, oz, np.where(ow >= 0, 0, -1)), "sphere handle against the object draw")

    # one YMin swapped with its successor's (both records stay inside their own row range): unsorted
    ymin, ymax = words[:, YMIN].view(np.int32), words[:, YMAX].view(np.int32)
    i = int(np.flatnonzero((ymin[:-1] < ymin[1:]) & (ymin[1:] <= ymax[:-1]))[0])
    sw = words.copy()
    sw[[i, i + 1], YMIN] = words[[i + 1, i], YMIN]
    counts = np.array([sw.shape[0]], np.uint32)
    assert rule(sw, counts).tolist() == [0]
    base = scenes.random_soup(1, 64, 64, seed=0)
    small = scenes.Scene(64, 64, s.vertices, s.colors, s.normals, s.uvs, base.transform, scenes.LIGHTS_ONE,
                         scenes.AMBIENT_ONE, base.texture, P=s.P)
    with Frame(small, True) as f:
        h2, b2, flags = both_frames(f, sw, counts)
        routes = f.r.walk_routes()
    assert flags.tolist() == [0]
    assert large_objects(routes) == 0, routes
    same_frame(h2, b2, "unsorted sphere list, handle against draw_edge_lists")


# ---- 5. mixed pass and re-use ----------------------------------------------------------------------------------------
def test_mixed_pass_and_reuse(gpu):
    s = scenes.with_ties(scenes.random_soup(400, 128, 96, radius=20, seed=61, centroid_margin=10), seed=61)
    assert s.tri_count == 600

    def frame(handles):
        with Frame(s, True) as f:
            A = f.r.records_from_geometry(f.g, 160, first_tri=240, P=s.P, setup=3, tris_per_object=8)
            B = f.r.records_from_geometry(f.g, 40, first_tri=400, P=s.P, setup=3)
            assert A.list_count == 20 and B.list_count == 1
            aw, ac, bw, bc = A.download(), A.counts(), B.download(), B.counts()
            ao = offsets(ac)
            host = f.records(3, 20, first=440, count=160)
            e = f.records(3, None, first=560, count=40)

            def lists(rec, w, cnt, off, a, n):
                if handles:
                    handle_frame(f, rec, AVX, a, n)
                else:
                    f.batch(w[off[a]:off[a + n]], cnt[a:a + n], AVX)

            f.objects(AVX, 8, first=0, count=240)
            lists(A, aw, ac, ao, 0, 7)
            f.batch(host[0], host[1], AVX)
            lists(A, aw, ac, ao, 3, 12)
            lists(B, bw, bc, offsets(bc), 0, 1)
            f.r.draw_edges(e[0], semantics=AVX[0], bitmap=f.tex, phong=True)
            first = f.done()
            later = []
            for _ in range(2):  # the same handle in a second and a third frame
                f.r.clear()
                lists(A, aw, ac, ao, 0, 20)
                later.append(f.done())
            return first, later

    h, hl = frame(True)
    b, bl = frame(False)
    ids = set(np.unique(h[2]).tolist())
    assert any(0 <= i < 240 for i in ids) and any(240 <= i < 247 for i in ids) and any(i >= 247 for i in ids)
    same_frame(h, b, "mixed pass")
    assert (hl[0][0] != scenes.CLEAR_COLOR).any()
    same_frame(hl[0], bl[0], "the handle alone, second frame")
    same_frame(hl[1], hl[0], "the handle alone, third frame against the second")


def test_handle_made_before_any_target(soup):
    s, words, counts = soup
    r = prk.Renderer()
    try:
        r.set_camera(s.prk_transform(), s.prk_lights())
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        rec = r.records_from_geometry(g, s.tri_count, P=s.P, setup=3, tris_per_object=20)
        assert np.array_equal(rec.download(), words) and np.array_equal(rec.counts(), counts)
        r.target_alloc(s.width, s.height)
        r.clear()
        r.set_debug(True)
        tex = r.texture(s.texture)
        r.draw_records(rec, bitmap=tex)
        r.complete_all_work()
        h = r.download() + (r.winners(),)
    finally:
        r.close()
    with Frame(s, True) as f:
        f.batch(words, counts, AVX)
        b = f.done()
    same_frame(h, b, "handle made before the target")


# ---- 6. a band target ------------------------------------------------------------------------------------------------
def test_band_target(soup):
    s, words, counts = soup
    with Frame(s, True, rows=(32, 64)) as f:
        h, b, _ = both_frames(f, words, counts)
    assert h[0].shape[0] == 32 and (h[0] != scenes.CLEAR_COLOR).any()
    same_frame(h, b, "rows [32, 64) of the frame")


# ---- 7. no record staging --------------------------------------------------------------------------------------------
def test_handle_draw_stages_no_records(soup):
    s, words, counts = soup
    total = words.shape[0]
    with Frame(s, True) as f:
        rec = f.r.records_upload(words, counts)
        handle_frame(f, rec, AVX)
        f.done()
        staged_handle = f.r.stage_bytes()
        f.r.clear()
        f.batch(words, counts, AVX)
        f.done()
        staged_host = f.r.stage_bytes()
    print("staging bytes: handle %d, host batch %d, records %d" % (staged_handle, staged_host, 108 * total))
    assert 0 < staged_handle < 108 * total
    assert staged_host >= 108 * total


# ---- 8. lifetime and errors ------------------------------------------------------------------------------------------
def test_lifetime_and_errors(soup):
    s, words, counts = soup
    with Frame(s, True) as f:
        L, ctx = f.r._L, f.r._h
        f.batch(words, counts, AVX)
        want = f.done()
        f.r.clear()
        rec = f.r.records_upload(words, counts)
        other = f.r.records_upload(words[:int(counts[0])], counts[:1])
        handle_frame(f, rec, AVX)  # recorded before every refused call below
        n, t = C.c_uint32(0), C.c_uint64(0)
        buf = np.empty((rec.total, 27), np.uint32)
        for bad in (-1, 99):
            assert L.prk_draw_records(ctx, bad, 0, 1, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG
            assert L.prk_records_info(ctx, bad, C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
            assert L.prk_records_lists(ctx, bad, None, None) == abi.PRK_ERR_ARG
            assert L.prk_records_download(ctx, bad, buf.ctypes.data, rec.total) == abi.PRK_ERR_ARG
            assert L.prk_records_destroy(ctx, bad) == abi.PRK_ERR_ARG
        dead = other.handle
        other.close()
        assert L.prk_draw_records(ctx, dead, 0, 1, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG
        assert L.prk_records_destroy(ctx, dead) == abi.PRK_ERR_ARG
        assert L.prk_draw_records(ctx, rec.handle, 10, 6, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG  # 16 > 15 lists
        assert L.prk_draw_records(ctx, rec.handle, 16, 0, AVX[0], 1, f.tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_records(ctx, rec.handle, 15, 0, AVX[0], 1, f.tex) == abi.PRK_OK  # nothing recorded
        assert L.prk_draw_records(ctx, rec.handle, 0, 15, 77, 1, f.tex) == abi.PRK_ERR_ARG
        assert L.prk_draw_records(ctx, rec.handle, 0, 15, AVX[0], 1, f.tex + 5) == abi.PRK_ERR_ARG
        assert L.prk_records_download(ctx, rec.handle, buf.ctypes.data, rec.total - 1) == abi.PRK_ERR_ARG
        # PRK_ERR_UNSUPPORTED exactly where prk_draw_edge_lists gives it
        wp, cp = words.ctypes.data, counts.ctypes.data
        for sem, phong, tex in [(AVX[0], 1, -1), (AVX[0], 0, f.tex), (AVX_ST[0], 0, f.tex), (AVX_ST[0], 1, -1)]:
            assert L.prk_draw_edge_lists(ctx, wp, cp, 15, sem, phong, tex) == abi.PRK_ERR_UNSUPPORTED
            assert L.prk_draw_records(ctx, rec.handle, 0, 15, sem, phong, tex) == abi.PRK_ERR_UNSUPPORTED
        # a recorded, unflushed draw names the handle
        assert L.prk_records_destroy(ctx, rec.handle) == abi.PRK_ERR_ARG
        got = f.done()  # the flush draws what was recorded before the errors, unchanged
        same_frame(got, want, "after refused calls")
        handle_frame(f, rec, AVX)
        assert L.prk_records_destroy(ctx, rec.handle) == abi.PRK_ERR_ARG
        f.r.reset_draws()
        assert L.prk_records_destroy(ctx, rec.handle) == abi.PRK_OK
        assert L.prk_records_info(ctx, rec.handle, C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
        f.r.clear()
        c, z, w = f.done()
        assert (c == scenes.CLEAR_COLOR).all() and (w == -1).all()
