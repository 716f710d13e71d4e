"""GPU tests: visibility feedback (include/prk.h prk_visibility_*,
csrc/prk_visibility.hip) -- the winner map of a frame reduced on the device to
per-id pixel counts, their prefix sums and the list of visible ids.

Expected words come from tests/visref.py (np.bincount over the definition),
fed the oracle's winner map and the same frame's prk_download_winners; every
word is compared.  The self-test runs the same kernels on hand-made maps whose
sizes sit on the histogram's constants (a lane's 4 words, a wave's 64 lanes,
the 256-word segment, the 4096-word chunk a wave walks) and on the scans' one-
and two-launch forms, and reports the atomic adds the histogram issued: run
aggregation is asserted, not assumed.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import prk
import visref
from prk import abi, scenes

pytestmark = pytest.mark.gpu

AVX = (abi.PRK_SEM_AVX, True, True)
SC_GOURAUD = (abi.PRK_SEM_SCALAR, False, False)

SCENES = {
    "general": ((3000, 256, 256), dict(radius=16, seed=123)),
    "long_runs": ((200, 256, 256), dict(radius=120, seed=5)),
    "many_ids": ((40000, 128, 128), dict(radius=3, seed=9)),
}


def first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d differ; first at %d: gpu %d ref %d" % (bad.size, want.size, bad[0], int(got[bad[0]]),
                                                            int(want[bad[0]]))


def same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %r, expected %r" % (label, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %s" % (label, first_bad(got.reshape(-1), want.reshape(-1)))


def refused(call, code=abi.PRK_ERR_ARG):
    with pytest.raises(prk.PrkError) as e:
        call()
    assert e.value.code == code


class Frame:
    """A renderer with the scene's target, camera, texture and geometry, the
    winner map on."""

    def __init__(self, s, mode=AVX, rows=None):
        self.s, self.mode = s, mode
        self.r = r = prk.Renderer()
        r0, r1 = (0, s.height) if rows is None else rows
        r.target_alloc(s.width, s.height, r0, r1)
        r.clear()
        r.set_debug(True)
        r.set_camera(s.prk_transform(), s.prk_lights())
        self.tex = r.texture(s.texture) if mode[2] else None
        self.g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.close()

    def draw(self, first=0, count=None, per=1):
        n = self.s.tri_count - first if count is None else count
        self.r.draw(self.mode[0], self.g, n, first_tri=first, P=self.s.P, bitmap=self.tex, phong=self.mode[1],
                    tris_per_object=per)

    def flush(self):
        self.r.complete_all_work()


def check_answer(r, want, label):
    """Every call of the frame's answer against a visref.Vis."""
    m = want.counts.shape[0]
    same(r.visibility(), (m, want.covered, want.visible), label + ": info")
    same(r.visibility_counts(), want.counts, label + ": counts")
    same(r.visibility_ids(), want.ids, label + ": ids")
    same(r.visibility_ids(), np.flatnonzero(r.visibility_counts()), label + ": ids are the nonzero counts")


# ---- 1. the self-test: sizes and patterns ---------------------------------------------------------------------------
def check_selftest(w, m, label):
    got = prk.selftest_visibility(w, m)
    want = visref.reduce(w, m)
    assert got["damage"] == 0, "%s: damage %d" % (label, got["damage"])
    same(got["counts"], want.counts, "%s counts" % (label,))
    same(got["pix_prefix"], want.pix_prefix, "%s pix_prefix" % (label,))
    same(got["vis_prefix"], want.vis_prefix, "%s vis_prefix" % (label,))
    assert got["visible"] == want.visible, label
    same(got["ids"], want.ids, "%s ids" % (label,))
    assert got["atomics"] <= w.shape[0], "%s: %d atomic adds for %d words" % (label, got["atomics"], w.shape[0])
    return got


@pytest.mark.parametrize("m", visref.ID_COUNTS)
@pytest.mark.parametrize("n", visref.SIZES)
def test_selftest_sizes_and_patterns(gpu, n, m):
    for name in sorted(visref.PATTERNS):
        check_selftest(visref.PATTERNS[name](n, m), m, (name, n, m))


def test_selftest_no_words_no_ids(gpu):
    got = check_selftest(np.zeros(0, np.int32), 65, ("empty map", 0, 65))
    assert got["atomics"] == 0 and not got["counts"].any()
    got = prk.selftest_visibility(np.arange(-3, 300, dtype=np.int32), 0)
    assert got["damage"] == 0 and got["visible"] == 0 and got["atomics"] == 0
    assert got["pix_prefix"].tolist() == [0] and got["vis_prefix"].tolist() == [0] and got["counts"].shape == (0,)


def test_selftest_chunk_boundaries(gpu):
    """Runs that end, begin and pass over the ends of the 4096-word chunks."""
    rng = np.random.default_rng(7)
    n, m = 3 * 4096 + 517, 300
    w = rng.integers(0, m, n).astype(np.int32)
    w[4000:4096] = 5      # ends with the first chunk
    w[4096:4200] = 5      # ... and goes on in the second (one run of 200 for the definition, two adds)
    w[8192:8192 + 700] = 9  # begins with the third chunk, passes two segments
    w[12000:] = 299       # over the last chunk boundary into the tail
    got = check_selftest(w, m, ("chunks", n, m))
    assert got["counts"][299] >= n - 12000


# ---- 2. aggregation is real ---------------------------------------------------------------------------------------------
def test_one_id_is_added_by_the_run(gpu):
    n = 65536
    for ident, m in ((0, 1), (69999, 70000)):
        got = check_selftest(np.full(n, ident, np.int32), m, ("one id", n, m))
        assert got["counts"][ident] == n
        assert 1 <= got["atomics"] <= n // 64, got["atomics"]


def test_alternating_ids_add_once_a_word_at_most(gpu):
    n = 65536
    got = check_selftest(visref.PATTERNS["alternating"](n, 2), 2, ("alternating", n, 2))
    assert got["atomics"] <= n and got["counts"].tolist() == [n // 2, n // 2]
    got = check_selftest(visref.PATTERNS["id_and_none"](n, 2), 2, ("id_and_none", n, 2))
    assert got["atomics"] <= n // 2 and got["counts"].tolist() == [0, n // 2]


# ---- 3. frames against the oracle -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_frames():
    """Per scene: (scene, the oracle's winner map, its visref), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            args, kw = SCENES[name]
            s = scenes.random_soup(*args, **kw)
            win = O.render(s, semantics=abi.PRK_SEM_AVX, phong=True)[2]
            cache[name] = (s, win, visref.reduce(win, s.tri_count))
        return cache[name]

    return get


def test_scene_conditions_hold_in_the_oracle(oracle_frames):
    """What each scene is there for, met by the oracle alone."""
    s, win, v = oracle_frames("general")
    assert v.visible >= 500 and s.tri_count - v.visible >= 500
    s, win, v = oracle_frames("long_runs")
    assert int(v.counts.max()) >= 5000 and visref.runs_of(win, 65) >= 50
    s, win, v = oracle_frames("many_ids")
    assert s.tri_count > 4096 and v.visible >= 5000


@pytest.mark.parametrize("name", sorted(SCENES))
def test_frame_counts_equal_the_oracle(gpu, oracle_frames, name):
    s, win, want = oracle_frames(name)
    with Frame(s) as f:
        f.draw()
        f.flush()
        check_answer(f.r, want, name)
        mine = f.r.winners()
        same(mine, win, name + ": winner map")
        check_answer(f.r, visref.reduce(mine, s.tri_count), name + " (own winners)")
        assert f.r.visibility()[1] == int((win >= 0).sum())


def test_scalar_semantics_odd_width(gpu):
    """A 101 x 37 target (rows of 404 bytes: the map's rows start at every
    alignment of a lane's four words) and a Gouraud soup."""
    s = scenes.random_soup(60, 101, 37, radius=12, seed=3)
    win = O.render(s, semantics=abi.PRK_SEM_SCALAR, phong=False)[2]
    want = visref.reduce(win, s.tri_count)
    assert want.visible >= 10
    with Frame(s, SC_GOURAUD) as f:
        f.draw()
        f.flush()
        check_answer(f.r, want, "gouraud 101x37")
        same(f.r.winners(), win, "gouraud 101x37: winner map")


# ---- 4. mixed passes in one flush -----------------------------------------------------------------------------------------
def test_mixed_passes_in_one_flush(gpu):
    """prk_draw of 100 triangles, prk_draw_objects of 160 in objects of 8,
    prk_draw_edge_lists of five lists, one of them empty: 100 + 160 + 5 ids."""
    s = scenes.random_soup(300, 128, 96, radius=24, seed=12, centroid_margin=20)
    with Frame(s) as f:
        r = f.r
        words, counts = r.edge_records(f.g, 40, first_tri=260, P=s.P, setup=3, tris_per_object=10)
        assert counts.shape == (4,) and (counts > 0).all()
        lists = np.array([counts[0], 0, counts[1], counts[2], counts[3]], np.uint32)
        f.draw(0, 100)
        f.draw(100, 160, per=8)
        r.draw_edge_lists(words, lists, semantics=abi.PRK_SEM_AVX, bitmap=f.tex, phong=True)
        f.flush()
        m = 100 + 160 + 5
        assert r.visibility()[0] == m
        win = r.winners()
        want = visref.reduce(win, m)
        assert int(win.max()) < m and want.covered == int((win >= 0).sum())
        check_answer(r, want, "mixed")
        got = r.visibility_counts()
        assert got[:100].any() and got[100:260].any() and got[260:].any()
        assert got[260 + 1] == 0  # the empty list's id
        # an object's pixels carry its first triangle's id
        assert not got[100:260].reshape(20, 8)[:, 1:].any()
        pix, vis = r.visibility_groups(np.array([0, 100, 260, 265], np.uint32))
        same(pix, [got[:100].sum(), got[100:260].sum(), got[260:].sum()], "mixed: the draws' pixels")
        same(vis, [(got[:100] > 0).sum(), (got[100:260] > 0).sum(), (got[260:] > 0).sum()], "mixed: the draws' ids")


# ---- 5. groups, ranges, sizing ------------------------------------------------------------------------------------------------
def test_groups_ranges_and_sizing(gpu, oracle_frames):
    s, win, want = oracle_frames("general")
    m = s.tri_count
    with Frame(s) as f:
        f.draw()
        f.flush()
        r = f.r
        rng = np.random.default_rng(4)
        cuts = np.sort(rng.integers(0, m + 1, 40))
        cases = {
            "empty groups": np.concatenate([[0, 0, 0], cuts, cuts[-1:], [m, m]]),
            "one group": np.array([0, m]),
            "a group an id": np.arange(m + 1),
            "inside": np.array([17, 17, 900, 2999]),
            "no group": np.array([m]),
        }
        for label, st in cases.items():
            pix, vis = r.visibility_groups(st)
            wp, wv = visref.groups(want, st)
            same(pix, wp, label + ": pixels")
            same(vis, wv, label + ": visible")
        pix, vis = r.visibility_groups(cases["one group"])
        assert (int(pix[0]), int(vis[0])) == (want.covered, want.visible)
        # either output alone
        st = np.ascontiguousarray(cases["empty groups"], np.uint32)
        g = st.shape[0] - 1
        only = np.full(g, 0xFFFFFFFF, np.uint32)
        L, h = r._L, r._h
        assert L.prk_visibility_groups(h, st.ctypes.data, g, only.ctypes.data, None) == abi.PRK_OK
        same(only, visref.groups(want, st)[0], "pixels alone")
        assert L.prk_visibility_groups(h, st.ctypes.data, g, None, only.ctypes.data) == abi.PRK_OK
        same(only, visref.groups(want, st)[1], "visible alone")
        # bad starts: nothing written
        only[:] = 7
        for bad in ([0, 5, 4, m], [0, m + 1], [m + 1, m + 1], [3, 2]):
            b = np.array(bad, np.uint32)
            refused(lambda: r.visibility_groups(b))
            assert L.prk_visibility_groups(h, b.ctypes.data, b.shape[0] - 1, only.ctypes.data, only.ctypes.data) == \
                abi.PRK_ERR_ARG
        assert (only == 7).all()
        # ranges of ids
        same(r.visibility_counts(0, 0), np.zeros(0, np.uint32), "no ids")
        same(r.visibility_counts(m, 0), np.zeros(0, np.uint32), "no ids at the end")
        same(r.visibility_counts(1234, 777), want.counts[1234:2011], "ids 1234 ...")
        same(r.visibility_counts(m - 1), want.counts[m - 1:], "the last id")
        refused(lambda: r.visibility_counts(m, 1))
        refused(lambda: r.visibility_counts(1, m))
        refused(lambda: r.visibility_counts(0xFFFFFFFF, 2))
        # the id list's sizing: the total always, the list only with room for all of it
        ids = np.full(want.visible, 0xFFFFFFFF, np.uint32)
        total = C.c_uint64(99)
        assert L.prk_visibility_ids(h, ids.ctypes.data, want.visible - 1, C.byref(total)) == abi.PRK_ERR_ARG
        assert total.value == want.visible and (ids == 0xFFFFFFFF).all()
        total = C.c_uint64(99)
        assert L.prk_visibility_ids(h, None, 0, C.byref(total)) == abi.PRK_OK and total.value == want.visible
        assert L.prk_visibility_ids(h, ids.ctypes.data, want.visible, C.byref(total)) == abi.PRK_OK
        same(ids, want.ids, "ids at the exact capacity")


# ---- 6. bands --------------------------------------------------------------------------------------------------------------------
def test_two_bands_sum_to_the_frame(gpu, oracle_frames):
    s, win, want = oracle_frames("general")
    total = np.zeros(s.tri_count, np.uint64)
    covered = 0
    for rank in range(2):
        rows = prk.band_rows(s.height, rank, 2)
        with Frame(s, rows=rows) as f:
            f.draw()
            f.flush()
            band = visref.reduce(win[rows[0]:rows[1]], s.tri_count)
            check_answer(f.r, band, "band %d" % rank)
            assert 0 < band.covered < want.covered
            total += f.r.visibility_counts()
            covered += f.r.visibility()[1]
    same(total.astype(np.uint32), want.counts, "the bands' sum")
    assert covered == want.covered


# ---- 7. lifecycle ----------------------------------------------------------------------------------------------------------------
def test_lifecycle(gpu, oracle_frames):
    s, win, want = oracle_frames("general")
    with Frame(s) as f:
        r = f.r
        refused(r.visibility)  # no flush yet
        total = C.c_uint64(99)
        assert r._L.prk_visibility_ids(r._h, None, 0, C.byref(total)) == abi.PRK_ERR_ARG and total.value == 0
        f.draw()
        f.flush()
        check_answer(r, want, "first")
        check_answer(r, want, "again")  # the same words from the kept result
        # the library's own arrays, read back through a wrapped layer: colour = counts, z = pix_prefix
        cp, pp, m = r.visibility_device()
        assert m == s.tri_count and cp and pp and cp != pp
        layer = r.layer_wrap(cp, 4 * m, pp, m, 1)
        c, z = r.layer_download(layer)
        same(c.reshape(-1), want.counts, "device counts")
        same(z.view(np.uint32).reshape(-1), want.pix_prefix[:m], "device pix_prefix")
        r.layer_destroy(layer)
        layer = r.layer_wrap(cp, 4, pp + 4 * m, 1, 1)
        assert int(r.layer_download(layer)[1].view(np.uint32)[0, 0]) == want.covered  # the prefix's last word
        r.layer_destroy(layer)
        # a second flush replaces the answer
        r.clear()
        f.draw(500, 700)
        f.flush()
        sub = visref.reduce(O.render(s.subset(500, 1200), semantics=abi.PRK_SEM_AVX, phong=True)[2], 700)
        assert 0 < sub.visible < want.visible
        check_answer(r, sub, "second flush")
        same(visref.reduce(r.winners(), 700).counts, sub.counts, "second flush: own winners")
        # merging another layer in does not change it: winner ids are not merged
        other = r.layer_alloc(s.width, s.height)
        r.layer_from_target(other)
        r.clear()
        f.draw(0, 500)
        f.flush()
        first = visref.reduce(O.render(s.subset(0, 500), semantics=abi.PRK_SEM_AVX, phong=True)[2], 500)
        r.target_from_layer(other, rule=abi.PRK_MERGE_GREATER)  # (before the frame's first query)
        check_answer(r, first, "after a merge")
        r.target_from_layer(other, rule=abi.PRK_MERGE_COPY)
        check_answer(r, first, "after a second merge")
        # an empty flush is no frame
        f.flush()
        refused(r.visibility)
        refused(r.visibility_counts)
        refused(r.visibility_ids)
        refused(lambda: r.visibility_groups([0, 1]))
        refused(r.visibility_device)
        # a flush without the winner map is none either, and debug mode brings it back
        r.set_debug(False)
        r.clear()
        f.draw()
        f.flush()
        refused(r.visibility)
        r.set_debug(True)
        refused(r.visibility)  # (the flag counts at the flush)
        r.clear()
        f.draw()
        f.flush()
        check_answer(r, want, "debug on again")
        # a new target: no frame until the next flush
        r.target_alloc(s.width, s.height)
        refused(r.visibility)
