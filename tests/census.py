"""The sizes of a whole-object draw's active edge list, counted on the CPU,
and the comb scenes (prk.scenes.comb) the huge-object walk tests render.

census() restates k_obj_maxact (prk_spans.hip) on the oracle's edge table:
FirstRow, the rows the walk visits, the most entries listed at once, the
entries over all rows, and the new edges per row.  The host picks an
object's walk from these (prk_span_pass.hip: LDS slot classes up to 1022 entries,
the huge-object walk in LDS up to 9200 entries and below 16000 rows, in
device memory beyond, one wave when the rows outgrow the histogram), and
Renderer.walk_routes() reports them as the device counted them.

A scene's figures cannot be had from comb()'s parameters alone (rounding
decides each edge's first row), so every builder here drops triangles by the
per-triangle edge rows until the census of the FINAL scene shows the wanted
figure; tests assert the census, never the recipe.
"""
import dataclasses
import functools

import numpy as np

import oracle as O
from prk import abi, scenes

INT32_MAX = 2**31 - 1
MAXACT_ROWS = 16000   # k_obj_maxact's histogram (kMaxactRows): rows + 1 beyond it are not counted
WINDOW = 1024         # new edges one insertion batch takes (kBigThreads)
LDS_CAP = 9200        # k_obj_walk_lds's list (kLdsCap)
SLOT_CAP = 1022       # the largest LDS slot class of the workgroup walk
W, H = 512, 96
TALL_W, TALL_H = 64, 16064


def census(scene, rows=None):
    """k_obj_maxact's sizes of `scene` drawn as one object into rows
    [rows[0], rows[1]) (default: the frame).  first: FirstRow; rows: min(max
    YMax, H, row1) - FirstRow; most: the peak of the difference histogram
    over those rows; ents: the sum over edges of their listed rows; new[q] /
    listed[q]: edges entering / listed on row first + q; edges: the table's
    length; ns: the longest scan of the device-memory walk (window_scans).
    (The kernel reports most = rows = INT32_MAX, ents = 0 once rows
    + 1 > 16000: device_sizes() below.)"""
    w = O.fill_edge_table_words(scene, 0, scene.tri_count)
    y0 = w[:, 7].view(np.int32).astype(np.int64)
    y1 = w[:, 0].view(np.int32).astype(np.int64)
    assert len(w) and (np.diff(y0) >= 0).all()  # sorted by YMin: E[0].YMin is FirstRow
    row1 = scene.height if rows is None else rows[1]
    first = int(y0[0])
    max_y = int(min(y1.max(), scene.height, row1))
    n = max_y - first
    out = dict(first=first, rows=n, edges=len(w), most=0, ents=0, ns=0, new=np.zeros(0, np.int64),
               listed=np.zeros(0, np.int64))
    if n <= 0:
        return out
    ins = y0 < max_y  # (the others are never inserted)
    a, b = y0[ins], y1[ins]
    h = np.zeros(n + 2, np.int64)
    np.add.at(h, a - first, 1)
    np.add.at(h, np.minimum(np.maximum(a, b), max_y - 1) - first + 1, -1)
    listed = np.cumsum(h)[:n]
    new = np.bincount(a - first, minlength=n)[:n]
    out.update(most=int(listed.max()), ents=int(np.maximum(0, np.minimum(b, max_y) - a).sum()),
               ns=int(window_scans(listed, new).max()), new=new, listed=listed)
    return out


def window_scans(listed, new):
    """Per row, the longest scan k_obj_walk_big's big_insert_expire makes (its
    ns; up to 8192 it scans from registers, beyond it reloads).  A row starts
    with the listed - new entries the row before left; its new edges go in
    1024 at a time, window j scanning the list before it and the tail gap:
    listed - new + 1024 j + 1.  The last window is the one that holds fewer
    than 1024 edges and expires as well; when none does (no new edges, or an
    exact multiple of 1024) expiry runs alone over all `listed` entries.  So
    a row's longest scan is `listed` itself only when new % 1024 is 0 or 1,
    and stays below it otherwise: below `most` on a peak row that many edges
    enter."""
    listed, new = np.asarray(listed, np.int64), np.asarray(new, np.int64)
    last = (new - 1) // WINDOW  # the last non-empty window (new > 0)
    return np.where(new % WINDOW == 0, listed, listed - new + WINDOW * last + 1)


def device_sizes(c):
    """(most, rows, ents) as k_obj_maxact / k_maxact_huge_fin report census c."""
    if c["rows"] + 1 > MAXACT_ROWS:
        return (INT32_MAX, INT32_MAX, 0)
    return (c["most"], c["rows"], c["ents"])


def busiest(c):
    """(row, new edges) of the census row most edges enter on."""
    q = int(np.argmax(c["new"]))
    return c["first"] + q, int(c["new"][q])


def _per_triangle(scene):
    tri, y0, y1 = O.edge_rows_per_triangle(scene)
    return tri.astype(np.int64), y0.astype(np.int64), y1.astype(np.int64)


def trim_new_edges(scene, want):
    """`scene` less the latest triangles that bring the new-edge count of its
    busiest row down to exactly `want`."""
    tri, y0, _ = _per_triangle(scene)
    row = int(np.argmax(np.bincount(y0)))
    per = np.bincount(tri[y0 == row], minlength=scene.tri_count)
    over = int(per.sum()) - want
    assert over >= 0, (scene.name, int(per.sum()), want)
    keep = np.ones(scene.tri_count, bool)
    for t in range(scene.tri_count - 1, -1, -1):
        if over and 0 < per[t] <= over:
            keep[t] = False
            over -= int(per[t])
    assert over == 0, (scene.name, want)
    return scenes.select_triangles(scene, np.nonzero(keep)[0])


def trim_most(scene, want, figure="most"):
    """`scene` less the latest triangles that bring the peak list length
    (census most; figure="ns": the longest scan, census ns) down to exactly
    `want`.
    most: a triangle listed on the peak's row takes its entries there off.
    ns: a row's scan is its old entries (listed since a row before) + 1 + the
    windows before the last, or all its entries when expiry runs alone.  A
    scanline crosses a triangle twice or not at all, so the old entries are
    even and a window row's scan odd: an even excess goes by dropping
    triangles that are old on the peak's row (two entries each), and an odd
    one by dropping the triangles whose edges enter on that row until expiry
    runs alone there (the scan is then the old entries themselves)."""
    tri, y0, y1 = _per_triangle(scene)
    max_y = min(int(y1.max()), scene.height)
    lo, hi = y0, np.minimum(np.maximum(y0, y1), max_y - 1)
    alive = y0 < max_y
    keep = np.ones(scene.tri_count, bool)
    for _ in range(4000):
        h = np.zeros(max_y + 2, np.int64)
        np.add.at(h, lo[alive], 1)
        np.add.at(h, hi[alive] + 1, -1)
        fig = np.cumsum(h)[:max_y]
        if figure == "ns":
            fig = window_scans(fig, np.bincount(lo[alive], minlength=max_y)[:max_y])
        p = int(np.argmax(fig))
        over = int(fig[p]) - want
        assert over >= 0, (scene.name, int(fig[p]), want)
        if over == 0:
            break
        if figure == "ns" and over % 2:
            cand = np.unique(tri[alive & (lo == p)])  # (none: expiry alone, an even scan, and an odd `want`)
        else:
            per = np.bincount(tri[alive & (lo < p if figure == "ns" else lo <= p) & (p <= hi)],
                              minlength=scene.tri_count)
            if figure == "ns":
                per[tri[alive & (lo == p)]] = 0
            # a triangle of the excess's parity first (few have 1 or 3 entries on a row), then the latest
            cand = np.nonzero((per > 0) & (per <= over) & (per % 2 == over % 2))[0]
        assert len(cand), (scene.name, want, p, over)
        t = int(cand[-1])
        keep[t] = False
        alive &= tri != t
    return scenes.select_triangles(scene, np.nonzero(keep)[0])


def untextured(scene):
    """(DrawModel, PRK_SEM_SCALAR, is drawn without the texture here, as the other whole-object tests do.)"""
    return dataclasses.replace(scene, texture=None)


# ---- the scenes -------------------------------------------------------------
# A background group entering at row 3 is listed before each comb's busy rows,
# so the new edges interleave with listed ones.

@functools.lru_cache(maxsize=None)
def window_scene(k):
    """A: one row takes exactly k new edges (k around the insertion window of
    1024 and its multiples) into a list of ~500."""
    s = scenes.comb([(250, 3, 30, 92), (k // 2 + 24, 10, 40, 94), (120, 22, 60, 94)], W, H, seed=1000 + k)
    return trim_new_edges(s, k)


B_GROUPS = [(600, 3, 30, 92), (1250, 10, 40, 94), (350, 20, 50, 94), (250, 31, 60, 94)]


@functools.lru_cache(maxsize=None)
def lds_scene(ties=False):
    """B: the LDS walk over several windows: 2500 edges on one row, 700 more
    ten rows later into the long list, most in (4096, 9200]; with ties, every
    second triangle twice (equal keys: the order is by arrival)."""
    if not ties:
        return scenes.comb(B_GROUPS, W, H, seed=41)
    s = scenes.comb([(g[0] * 4 // 5,) + g[1:] for g in B_GROUPS], W, H, seed=42)
    return scenes.with_ties(s, seed=42)


@functools.lru_cache(maxsize=None)
def handover_scene(most):
    """C: most == 9200 (the last list k_obj_walk_lds takes) / 9201 (the first
    k_obj_walk_big takes unforced)."""
    s = scenes.comb([(1500, 3, 14, 94), (2000, 10, 50, 94), (1300, 18, 60, 94)], W, H, seed=43)
    return trim_most(s, most)


@functools.lru_cache(maxsize=None)
def reload_scene(ns):
    """D: a tied scene whose longest scan (census ns) is the last the
    device-memory walk makes from registers (8192) / the first it reloads
    (8193)."""
    s = scenes.comb([(900, 3, 14, 94), (1300, 10, 50, 94), (680, 18, 60, 94)], W, H, seed=44)
    return trim_most(scenes.with_ties(s, seed=44), ns, figure="ns")


@functools.lru_cache(maxsize=None)
def big_scene():
    """D: most of 11k to 14k (k_obj_walk_big unforced) and more than 2 * 8192
    edges (F: three histogram workgroups and more)."""
    return scenes.comb([(1500, 3, 40, 94), (3000, 10, 50, 94), (1100, 18, 60, 94), (400, 30, 70, 94)], W, H, seed=45)


TALL_GROUPS = [(620, 20, 100, 2000), (40, 20, 8000, 15990), (1, 20, 16015, 16015)]


@functools.lru_cache(maxsize=None)
def tall_scene(stretched=False):
    """Tall frames: a comb whose longest sliver ends 15995 rows below its apex
    (just inside the LDS walk's 16-bit row packing and the histogram), and the
    same comb stretched by 1 % about the apex row, past the frame's bottom
    (rows >= 16000: no histogram, most = INT32_MAX)."""
    f = 1.01 if stretched else 1.0
    g = [(n, a, a + (lo - a) * f, a + (hi - a) * f) for n, a, lo, hi in TALL_GROUPS]
    return scenes.comb(g, TALL_W, TALL_H, seed=46)


BAND = (40, 75)  # rows rendered of B / D in the band cases: FirstRow + 10 lies well above, row 75 inside


SCENES = {  # the catalogue by name: what the tests' parameters and the shared references are keyed by
    "window_1023": (window_scene, 1023), "window_1024": (window_scene, 1024), "window_1025": (window_scene, 1025),
    "window_2048": (window_scene, 2048), "window_2049": (window_scene, 2049),
    "lds": (lds_scene, False), "lds_ties": (lds_scene, True),
    "handover_9200": (handover_scene, 9200), "handover_9201": (handover_scene, 9201),
    "reload_8192": (reload_scene, 8192), "reload_8193": (reload_scene, 8193),
    "big": (big_scene,), "tall": (tall_scene, False), "tall_stretched": (tall_scene, True),
}


def scene(name):
    f = SCENES[name]
    return f[0](*f[1:])


def check_lds_scene(c):
    """B's census: most in (4096, 9200]; a row of more than 2048 new edges;
    several hundred more, less than a window, 8 to 12 rows later into a list
    of thousands; a row of odd length."""
    assert 4096 < c["most"] <= LDS_CAP
    row, new = busiest(c)
    q = row - c["first"]
    assert new > 2048
    assert 300 <= c["new"][q + 8: q + 13].max() < WINDOW and c["listed"][q + 7] > 3000
    assert (c["listed"] % 2 == 1).sum() >= 1


def check_band(c):
    """E's census: the band starts 25 rows and more below the rows where the
    groups enter (first + 10) and ends inside the object."""
    assert c["first"] + 10 + 25 <= BAND[0] and c["rows"] == BAND[1] - c["first"] and c["most"] > 4096


@functools.lru_cache(maxsize=None)
def reference(name, sem):
    """The oracle's frame of scene `name` of SCENES drawn as one object;
    shared, never written to."""
    s = scene(name)
    if sem == abi.PRK_SEM_SCALAR:
        s = untextured(s)
    out = O.render(s, semantics=sem, phong=sem != abi.PRK_SEM_SCALAR, threads=1, tris_per_object=s.tri_count)
    for a in out[:3]:
        a.setflags(write=False)
    return out
