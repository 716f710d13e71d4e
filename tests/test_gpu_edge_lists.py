"""GPU tests: prk_draw_edge_lists (a batch of edge_info lists in one call, the
sorted ones on the walks of triangle objects) against prk_draw_edges list by
list, against the whole-object draw the records came from, and against the
oracle.

Every comparison is on bits: z as uint32, colours equal, winners equal.  A
loop of prk_draw_edges calls takes no id for an empty list and the batch takes
one for every list (prk.h), so a loop's winners are renumbered to the batch's
ids before they are compared (loop_to_batch_ids).
"""
import numpy as np
import pytest

import oracle as O
import prk
from prk import abi, scenes
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

YMIN = 7  # prk_edge word

# (semantics, phong, textured, FillEdgeTable setup)
AVX = (abi.PRK_SEM_AVX, True, True, 3)
AVX_ST = (abi.PRK_SEM_AVX_ST, True, True, 3)
SC_GOURAUD = (abi.PRK_SEM_SCALAR, False, False, 0)
SC_PHONG = (abi.PRK_SEM_SCALAR, True, False, 1)


def soup_scene():
    return scenes.random_soup(300, 128, 96, radius=24, seed=12, centroid_margin=20)


def sphere_scene():
    V, Cc, N, UV = prk.construct_sphere()
    base = scenes.random_soup(1, 256, 256, seed=0)
    return scenes.Scene(256, 256, V.copy(), Cc.copy(), N.copy(), UV.copy(), base.transform, scenes.LIGHTS_ONE,
                        scenes.AMBIENT_ONE, base.texture, P=(0.0, 0.0, 2.0))


class Frame:
    """A renderer with the scene's target, camera, texture and geometry; the
    frame and its winners after the recorded draws."""

    def __init__(self, s, textured, rows=None):
        self.s = s
        self.r = r = prk.Renderer()
        if rows is None:
            r.target_alloc(s.width, s.height)
        else:
            r.target_alloc(s.width, s.height, rows[0], rows[1])
        r.clear()
        r.set_debug(True)
        r.set_camera(s.prk_transform(), s.prk_lights())
        self.tex = r.texture(s.texture) if textured else None
        self.g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.close()

    def records(self, setup, per, first=0, count=None, P=None):
        n = self.s.tri_count - first if count is None else count
        return self.r.edge_records(self.g, n, first_tri=first, P=self.s.P if P is None else P, setup=setup,
                                   tris_per_object=per)

    def batch(self, words, counts, mode):
        self.r.draw_edge_lists(words, counts, semantics=mode[0], bitmap=self.tex, phong=mode[1])

    def loop(self, words, counts, mode):
        o = 0
        for n in counts:
            self.r.draw_edges(words[o:o + int(n)], semantics=mode[0], bitmap=self.tex, phong=mode[1])
            o += int(n)

    def objects(self, mode, per, first=0, count=None):
        n = self.s.tri_count - first if count is None else count
        self.r.draw(mode[0], self.g, n, first_tri=first, P=self.s.P, bitmap=self.tex, phong=mode[1],
                    tris_per_object=per, setup=mode[3])

    def done(self):
        self.r.complete_all_work()
        c, z = self.r.download()
        return c, z, self.r.winners()


def same_frame(got, want, label, winners=True):
    nz = int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum())
    nc = int((got[0] != want[0]).sum())
    nw = int((got[2] != want[2]).sum()) if winners else 0
    assert (nz, nc, nw) == (0, 0, 0), "%s: z %d, colours %d, winners %d pixels differ" % (label, nz, nc, nw)


def loop_to_batch_ids(w, steps):
    """Winners of a pass whose batches were drawn as loops of draw_edges calls,
    renumbered as the pass with the batches numbers them.  steps: ("ids", n)
    for a draw that takes n ids either way, ("lists", counts) for a batch."""
    table, b = [], 0  # loop id -> batch id
    for kind, v in steps:
        if kind == "ids":
            table += list(range(b, b + v))
            b += v
        else:
            table += [b + o for o in range(len(v)) if v[o] > 0]
            b += len(v)
    table = np.array(table + [-1], np.int32)
    assert w.max() < table.size - 1
    return table[w]  # (-1, no winner, reads the last entry)


# ---- 1. round trip, small lists --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup_frames(gpu):
    """Per mode: the records of the soup as 20-triangle objects, and the
    frames of the batch, of the loop and of the object draw."""
    cache = {}

    def get(mode):
        if mode not in cache:
            s = soup_scene()
            with Frame(s, mode[2]) as f:
                words, counts = f.records(mode[3], 20)
                f.batch(words, counts, mode)
                b = f.done()
            with Frame(s, mode[2]) as f:
                f.loop(words, counts, mode)
                lp = f.done()
            with Frame(s, mode[2]) as f:
                f.objects(mode, 20)
                ob = f.done()
            cache[mode] = (words, counts, b, lp, ob)
        return cache[mode]

    return get


@pytest.mark.parametrize("mode", [AVX, AVX_ST, SC_GOURAUD], ids=["avx", "avx_st", "scalar_gouraud"])
def test_round_trip_small_lists(soup_frames, mode):
    words, counts, b, lp, ob = soup_frames(mode)
    assert counts.size == 15 and counts.max() > 0 and int(counts.sum()) == words.shape[0]
    assert (b[0] != scenes.CLEAR_COLOR).any()
    lw = loop_to_batch_ids(lp[2], [("lists", counts)])
    same_frame(b, (lp[0], lp[1], lw), "batch against the loop of draw_edges")
    same_frame(b, ob, "batch against the 20-triangle objects", winners=False)
    assert set(np.unique(b[2])) <= set(range(-1, 15))


# ---- 2. one large sorted list ----------------------------------------------------------------------------------------
WALKS = {
    "default": {},
    "rows0": {"PRK_OBJ_ROWS": "0"},
    "wave": {"PRK_OBJ_BIG_MIN": "0", "PRK_OBJ_ROWS": "0", "PRK_OBJ_BIG": "0"},
    "big": {"PRK_OBJ_BIG_MIN": "0", "PRK_OBJ_ROWS": "0", "PRK_OBJ_HUGE_EDGES": "100", "PRK_OBJ_LDSWALK": "1"},
    "bigmem": {"PRK_OBJ_BIG_MIN": "0", "PRK_OBJ_ROWS": "0", "PRK_OBJ_HUGE_EDGES": "100", "PRK_OBJ_LDSWALK": "0"},
}


@pytest.fixture(scope="module")
def sphere_frames(gpu):
    """Per mode: the sphere's records as one object and the frame of its
    whole-object draw (default walks)."""
    cache = {}

    def get(mode):
        if mode not in cache:
            s = sphere_scene()
            with Frame(s, mode[2]) as f:
                words, counts = f.records(mode[3], None)
                f.objects(mode, s.tri_count)
                ob = f.done()
            assert counts.tolist() == [words.shape[0]] and words.shape[0] >= 144  # (a large object: DESIGN §4.4.2)
            assert (np.diff(words[:, YMIN].view(np.int32)) >= 0).all()
            cache[mode] = (s, words, counts, ob)
        return cache[mode]

    return get


def large_objects(routes):
    return sum(routes["slots"]) + routes["huge_lds"] + routes["huge_mem"] + routes["wave"]


@pytest.mark.parametrize("walk", sorted(WALKS))
@pytest.mark.parametrize("mode", [AVX, SC_PHONG], ids=["avx", "scalar_phong"])
def test_large_sorted_list(sphere_frames, mode, walk, monkeypatch):
    s, words, counts, ob = sphere_frames(mode)
    for k, v in WALKS[walk].items():
        monkeypatch.setenv(k, v)
    with Frame(s, mode[2]) as f:
        f.batch(words, counts, mode)
        b = f.done()
        routes = f.r.walk_routes()
        st = f.r.stats()
    assert (b[0] != scenes.CLEAR_COLOR).any()
    same_frame(b, ob, "sphere from its records, %s walks" % walk, winners=False)
    assert np.array_equal(b[2] >= 0, ob[2] >= 0) and set(np.unique(b[2])) == {-1, 0}
    assert large_objects(routes) == 1, routes
    assert st["objects_chunked"] + st["objects_walked"] == 1
    if walk == "wave":
        assert routes["wave"] == 1
    if walk in ("big", "bigmem"):
        assert routes["huge_lds" if walk == "big" else "huge_mem"] == 1 and routes["sized_huge"] == 1


# ---- 3. against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [abi.PRK_SEM_AVX, abi.PRK_SEM_AVX_ST])
def test_one_list_batch_against_the_oracle(gpu, sem):
    s = scenes.random_soup(60, 256, 256, radius=60, seed=43, textured=True, centroid_margin=40)
    words = O.fill_edge_table_words(s, 0, 60)
    with Frame(s, True) as f:
        f.batch(words, np.array([words.shape[0]], np.uint32), (sem, True, True, 3))
        c, z, w = f.done()
        st = f.r.stats()
    compare((c, z, w, st), O.render_edges(s, words, semantics=sem), label="one-list batch")


# ---- 4. unsorted input -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sphere", "forty"])
def test_unsorted_list_is_walked_as_draw_edges_walks_it(sphere_frames, which):
    s, words, _, _ = sphere_frames(AVX)
    if which == "forty":
        words = words[::words.shape[0] // 40][:40]  # (every 80th or so: still sorted, many rows)
    perm = words[np.random.default_rng(7).permutation(words.shape[0])]
    assert (np.diff(perm[:, YMIN].view(np.int32)) < 0).any()
    counts = np.array([perm.shape[0]], np.uint32)
    with Frame(s, True) as f:
        f.batch(perm, counts, AVX)
        b = f.done()
        routes = f.r.walk_routes()
        st = f.r.stats()
    with Frame(s, True) as f:
        f.loop(perm, counts, AVX)
        lp = f.done()
    assert (lp[0] != scenes.CLEAR_COLOR).any()
    same_frame(b, lp, "unsorted %s list" % which)
    assert large_objects(routes) == 0 and routes["sized_huge"] == 0, routes
    assert st["objects_chunked"] + st["objects_walked"] == 0


# ---- 5. mixed pass and order -----------------------------------------------------------------------------------------
def test_mixed_pass_keeps_submission_order(gpu):
    s = scenes.with_ties(scenes.random_soup(400, 128, 96, radius=20, seed=61, centroid_margin=10), seed=61)
    assert s.tri_count == 600

    def frame(batched):
        with Frame(s, True) as f:
            a = f.records(3, 8, first=240, count=160)
            e = f.records(3, None, first=400, count=40)
            c = f.records(3, 20, first=440, count=160)
            f.objects(AVX, 8, first=0, count=240)
            (f.batch if batched else f.loop)(a[0], a[1], AVX)
            f.r.draw_edges(e[0], semantics=AVX[0], bitmap=f.tex, phong=True)
            (f.batch if batched else f.loop)(c[0], c[1], AVX)
            return f.done(), [("ids", 240), ("lists", a[1]), ("ids", 1), ("lists", c[1])]

    b, steps = frame(True)
    lp, _ = frame(False)
    assert e_nonempty(steps)
    ids = set(np.unique(b[2]).tolist())
    assert any(i < 240 for i in ids if i >= 0) and any(240 <= i < 260 for i in ids)  # objects and lists both win pixels
    assert any(i > 260 for i in ids)
    same_frame(b, (lp[0], lp[1], loop_to_batch_ids(lp[2], steps)), "mixed pass")


def e_nonempty(steps):
    return all(int(np.sum(v)) > 0 for k, v in steps if k == "lists")


# ---- 6. ids and empties ----------------------------------------------------------------------------------------------
def interface_scene():
    s = scenes.random_soup(15, 128, 96, radius=24, seed=5)
    v = s.vertices.reshape(-1, 3, 3)
    v[5:10, 1], v[5:10, 2] = v[5:10, 2].copy(), v[5:10, 1].copy()  # the second object: all back-facing
    s.vertices = v.reshape(-1, 3)
    return s


@pytest.mark.parametrize("mode,want", [(AVX, {-1, 0, 1}), (AVX_ST, {-1, 1, 3})], ids=["avx", "avx_st"])
def test_ids_and_empty_lists(gpu, mode, want):
    """One prk_draw_edges call of the third list takes id 0, so the batch's
    base is 1 and its lists take 1, 2 (empty), 3.  Strict '>' (AVX) leaves the
    third list's pixels with the earlier draw of the same list, id 0; '>='
    (AVX_ST) gives them to the batch, id 3."""
    s = interface_scene()

    def frame(batched, refused_calls):
        with Frame(s, True) as f:
            words, counts = f.records(3, 5)
            assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
            third = words[int(counts[0]):]
            f.r.draw_edges(third, semantics=mode[0], bitmap=f.tex, phong=True)
            if refused_calls:
                L, h = f.r._L, f.r._h
                wp, cp = words.ctypes.data, counts.ctypes.data
                assert L.prk_draw_edge_lists(h, None, None, 0, mode[0], 1, f.tex) == abi.PRK_OK
                assert L.prk_draw_edge_lists(h, wp, cp, 0, mode[0], 1, f.tex) == abi.PRK_OK
                assert L.prk_draw_edge_lists(h, wp, None, 3, mode[0], 1, f.tex) == abi.PRK_ERR_ARG
                assert L.prk_draw_edge_lists(h, None, cp, 3, mode[0], 1, f.tex) == abi.PRK_ERR_ARG
                assert L.prk_draw_edge_lists(h, wp, cp, 3, 77, 1, f.tex) == abi.PRK_ERR_ARG
                assert L.prk_draw_edge_lists(h, wp, cp, 3, mode[0], 1, f.tex + 5) == abi.PRK_ERR_ARG
                assert L.prk_draw_edge_lists(h, wp, cp, 3, mode[0], 1, -1) == abi.PRK_ERR_UNSUPPORTED  # no texture
                assert L.prk_draw_edge_lists(h, wp, cp, 3, mode[0], 0, f.tex) == abi.PRK_ERR_UNSUPPORTED  # no Phong
            if batched:
                f.batch(words, counts, mode)
            else:
                f.loop(words, counts, mode)
            return f.done(), counts

    b, counts = frame(True, False)
    assert set(np.unique(b[2]).tolist()) == want
    lp, _ = frame(False, False)
    same_frame(b, (lp[0], lp[1], loop_to_batch_ids(lp[2], [("ids", 1), ("lists", counts)])), "batch with an empty list")
    # calls that record nothing: the frame and its ids as without them
    same_frame(frame(True, True)[0], b, "after refused and empty calls")


def test_reset_draws_drops_recorded_lists(gpu):
    s = soup_scene()
    with Frame(s, True) as f:
        words, counts = f.records(3, 20)
        f.batch(words, counts, AVX)
        f.r.reset_draws()
        c, z, w = f.done()
    assert (c == scenes.CLEAR_COLOR).all() and (w == -1).all()


# ---- 7. bands --------------------------------------------------------------------------------------------------------
def test_two_bands_stack_to_the_frame(soup_frames):
    words, counts, full, _, _ = soup_frames(AVX)
    s = soup_scene()
    parts = []
    for rows in [(0, 41), (41, 96)]:
        with Frame(s, True, rows=rows) as f:
            f.batch(words, counts, AVX)
            parts.append(f.done())
    stacked = tuple(np.concatenate([parts[0][k], parts[1][k]]) for k in range(3))
    same_frame(stacked, full, "two row bands")


# ---- 8. two frames on one context ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["soup", "sphere"])
def test_two_frames_on_one_context(soup_frames, sphere_frames, which):
    if which == "soup":
        s = soup_scene()
        words, counts, want = soup_frames(AVX)[:3]
    else:
        s, words, counts, ob = sphere_frames(AVX)
        want = None
    with Frame(s, True) as f:
        f.batch(words, counts, AVX)
        a = f.done()
        f.r.clear()
        f.batch(words, counts, AVX)
        b = f.done()
    assert (a[0] != scenes.CLEAR_COLOR).any()
    same_frame(b, a, "the second frame of the %s batch" % which)
    if want is not None:
        same_frame(a, want, "the first frame")
    else:
        same_frame(a, ob, "the first frame against the object draw", winners=False)
