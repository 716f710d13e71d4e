"""GPU tests: the tile binning (cpu-renderer_amd/csrc/prk_bin.hip) equals its
definition, tests/binref.py -- read back with prk_debug_bins.

Every case is one frame with the debug flag on.  For each: tri_n and the
tile ranges equal binref word for word; tri_off is the exclusive scan of
tri_n and its last word is the entry count everywhere it is kept; pair_tri
names each pair's triangle; every tile's bin is exactly the reference's set
of (triangle, pair) -- none missing, none twice, pair = tri_off + the entry's
position in for_each_entry order; and within each window of 2048 slots of a
bin the entries are grouped by binref's row class, ascending.  The order
within a class is free (the kernel says so) and is not asserted.

What the device leaves unwritten is not compared: the pad words of a triangle
without entries, and, in a row band (binned through run lists), everything
of a triangle that is not listed.

The counting sort's band chunks of `per` runs reach their cap of 64 only at
2048 * 64 * 128 triangles a frame (PRK_BAND_MIN_CHUNKS), far past what a test
frame can hold.  test_bands runs at per = 1; test_bands_several_runs_a_chunk
reaches per = 2 and 3, each with a last chunk of fewer runs (band_per in the
read-back says so)."""
import numpy as np
import pytest

import bincases
import binref
import oracle as O
import prk
from prk import abi, scenes

pytestmark = pytest.mark.gpu
AVX, SCALAR = abi.PRK_SEM_AVX, abi.PRK_SEM_SCALAR


def soup(n, W, H, sem, seed, box=None, radius=2.5, flip=False):
    """n small triangles with their centres uniform over `box` (x0, y0, x1, y1;
    default: the frame and a margin around it)."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = box or (-6, -6, W + 6, H + 6)
    c = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], 1)
    s = c[:, None, :] + rng.uniform(-radius, radius, (n, 3, 2))
    z = rng.uniform(-0.8, 0.8, (n, 1)) + rng.uniform(-0.1, 0.1, (n, 3))
    sc = bincases.screen_scene(s, z, seed, W=W, H=H)
    if flip:  # back-facing: every triangle culled
        v = sc.vertices.reshape(n, 3, 3)
        v[:, [1, 2]] = v[:, [2, 1]]
        sc.vertices = v.reshape(-1, 3).copy()
    sc.texture = scenes.random_texture(rng, 16, 16)
    return sc


def frames(plan, W, H, rows=None, tile=None):
    """Draw the scenes of `plan` [(scene, semantics)] one frame each into one
    W x H target (clear, draw, flush) and read the last frame's bins back:
    (debug_bins dict, stats, colour, z, entry counts of every frame)."""
    r = prk.Renderer(0)
    try:
        r0, r1 = (0, H) if rows is None else rows
        r.target_alloc(W, H, r0, r1)
        if tile:
            r.set_tile(*tile)
        r.set_debug(True)
        counts = []
        for scene, sem in plan:
            r.clear()
            r.set_camera(scene.prk_transform(), scene.prk_lights())
            g = r.geometry(scene.vertices, scene.colors, scene.normals, scene.uvs)
            tex = r.texture(scene.texture)
            for first, count, s in binref.draws_of(scene, sem):
                r.draw(s, g, count, first_tri=first, P=scene.P, bitmap=tex, phong=True)
            r.complete_all_work()
            if scene is not plan[-1][0]:
                counts.append(r.stats()["bin_entries"])
        b = r.debug_bins()
        st = r.stats()
        counts.append(st["bin_entries"])
        r.synchronize()
        col, z = r.download()
        return b, st, col, z, counts
    finally:
        r.close()


def check(b, st, scene, sem, W, H, rows=None):
    """Every assertion of this module's docstring, for one read-back."""
    row0, row1 = (0, H) if rows is None else rows
    tr = binref.tile_ranges(scene, binref.draws_of(scene, sem), W, H, row0, row1, (b["tile_w"], b["tile_h"]))
    T = tr["tri_n"].shape[0]
    ntiles = tr["tiles_x"] * tr["tiles_y"]
    assert (b["tiles_x"], b["tiles_y"], b["tri_count"], b["row0"], b["row1"]) == (tr["tiles_x"], tr["tiles_y"], T, row0, row1)
    has = tr["tri_n"] > 0
    listed = b["listed"].astype(bool)
    assert (b["band_per"] > 0) == (rows is not None and (row0 > 0 or row1 < H))
    assert (listed == (has if b["band_per"] else np.ones(T, bool))).all(), np.nonzero(listed != has)[0][:8]
    # the ranges and counts, word for word
    bad = np.nonzero(b["tri_n"] != tr["tri_n"])[0]
    assert bad.size == 0, (bad[:8], b["tri_n"][bad[:8]], tr["tri_n"][bad[:8]], b["ranges"][bad[:8]], tr["ranges"][bad[:8]])
    bad = np.nonzero((b["ranges"][:, :6] != tr["ranges"][:, :6]).any(1) | (has & (b["ranges"][:, 6:] != tr["ranges"][:, 6:]).any(1)))[0]
    assert bad.size == 0, (bad[:8], b["ranges"][bad[:8]], tr["ranges"][bad[:8]])
    # pair numbering
    total = int(tr["tri_n"].sum())
    scan = np.concatenate([[0], np.cumsum(tr["tri_n"].astype(np.int64))])
    assert (b["tri_off"][:-1][listed] == scan[:-1][listed]).all()
    assert int(b["tri_off"][T]) == int(b["offs"][ntiles]) == b["entry_count"] == st["bin_entries"] == total
    assert (b["pair_tri"] == np.repeat(np.arange(T), tr["tri_n"])).all()
    # the bins: a permutation of the reference's pairs, each in its own tile
    g, tile, cls = binref.entries(tr)
    offs = b["offs"].astype(np.int64)
    assert offs[0] == 0 and (np.diff(offs) >= 0).all()
    assert (np.diff(offs) == np.bincount(tile, minlength=ntiles)).all()
    bg, bj = b["bins"][:, 0].astype(np.int64), b["bins"][:, 1].astype(np.int64)
    assert (np.sort(bj) == np.arange(total)).all(), "a pair missing or binned twice"
    slot_tile = np.searchsorted(offs, np.arange(total), side="right") - 1
    assert (g[bj] == bg).all() and (tile[bj] == slot_tile).all()
    # classes ascend within each window of a bin
    window = (np.arange(total) - offs[slot_tile]) // binref.CLASS_WINDOW
    same = (slot_tile[1:] == slot_tile[:-1]) & (window[1:] == window[:-1])
    assert (np.diff(cls[bj])[same] >= 0).all()
    return tr


def one(scene, sem, W, H, rows=None, tile=(32, 8)):
    b, st, col, z, _ = frames([(scene, sem)], W, H, rows, tile)
    assert b["rerun"] == 0
    assert (b["tile_w"], b["tile_h"]) == tuple(tile)
    return check(b, st, scene, sem, W, H, rows), b


# T around a chunk of 4096, and 7, 8, 9, 16 and 17 chunks (a tail chunk of one triangle where T = 4096 k + 1).
# k_cs_colscan cuts the chunks into 16 segments of ceil(chunks / 16): only at exactly 16 chunks (T = 16 * 4096) does
# its last segment hold a chunk -- with fewer, or with 17 (segments of two), segment 15 is empty.  So that case's
# diff(offs) == bincount(tile) in check() is the one guard against a column scan that loses its last segment (a
# mutation not tried on a device: it leaves bin slots unwritten for the raster kernels to read).
@pytest.mark.parametrize("T", [1, 4095, 4096, 4097, 6 * 4096 + 1, 8 * 4096, 8 * 4096 + 1, 16 * 4096, 16 * 4096 + 1])
def test_chunks(gpu, T):
    tr, _ = one(soup(T, 256, 64, AVX, seed=T, box=(20, 10, 200, 50) if T == 1 else None), AVX, 256, 64)
    assert tr["tri_n"].sum() > 0


def test_all_culled(gpu):
    tr, b = one(soup(5000, 256, 64, AVX, seed=3, flip=True), AVX, 256, 64)
    assert b["entry_count"] == 0 and not tr["live"].any()


@pytest.mark.parametrize("n", [2500, 6000])
def test_one_crowded_tile(gpu, n):
    """More than 2048 and more than 4096 entries in one bin: several class windows."""
    tr, b = one(soup(n, 256, 64, AVX, seed=n, box=(40, 10, 56, 13), radius=1.5), AVX, 256, 64)
    assert np.diff(b["offs"].astype(np.int64)).max() > (2048 if n < 4096 else 4096)


@pytest.mark.parametrize("W,H,tile,ntiles", [(64, 64, (64, 64), 1), (504, 8, (8, 8), 63), (512, 8, (8, 8), 64),
                                             (520, 8, (8, 8), 65)])
def test_tile_counts(gpu, W, H, tile, ntiles):
    tr, b = one(soup(3000, W, H, AVX, seed=ntiles), AVX, W, H, tile=tile)
    assert b["tiles_x"] * b["tiles_y"] == ntiles


@pytest.mark.parametrize("sem", [AVX, SCALAR])
def test_tile_height_not_a_power_of_two(gpu, sem):
    tr, b = one(soup(5000, 256, 64, sem, seed=12, radius=9.0), sem, 256, 64, tile=(64, 12))
    assert b["tiles_y"] == 6


def right_edge(n, W, H, seed):
    """Scalar triangles whose largest x lies in [W - 0.5, W): spans that end at MaxX == W on every row."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-4, H + 2, n)
    h = rng.uniform(3, 14, n)
    xm = W - rng.uniform(0.01, 0.49, n)
    s = np.stack([np.stack([xm - rng.uniform(3, 20, n), y], 1), np.stack([xm, y + h * rng.uniform(0.2, 0.8, n)], 1),
                  np.stack([xm - rng.uniform(0, 1.5, n), y + h], 1)], 1)
    sc = bincases.screen_scene(s, rng.uniform(-0.8, 0.8, (n, 1)) + rng.uniform(-0.1, 0.1, (n, 3)), seed, W=W, H=H)
    sc.texture = scenes.random_texture(rng, 16, 16)
    return sc


@pytest.mark.parametrize("rows", [None, (8, 24), (37, 64)])
def test_scalar_row_overflow(gpu, rows):
    """Scalar spans ending at MaxX == W on the last row of a tile, of the band
    and of the frame: the column-0 tile one row down gets its entry."""
    sc = right_edge(1500, 256, 64, seed=21)
    tr, b = one(sc, SCALAR, 256, 64, rows=rows)
    assert (tr["ranges"][:, 4] <= tr["ranges"][:, 5]).sum() > 100
    need, nt = binref.needed(sc, SCALAR, 256, 64, *(rows or (0, 64)), (32, 8))
    assert (need % nt % b["tiles_x"] == 0).any() and np.isin(need, binref.entry_keys(tr)).all()


def test_mixed_semantics_one_pass(gpu):
    sc = soup(9000, 256, 64, AVX, seed=31, radius=5.0)
    sc.draws = [(0, 3000, sc.texture, AVX), (3000, 3000, sc.texture, SCALAR), (6000, 3000, sc.texture, abi.PRK_SEM_AVX_ST)]
    one(sc, AVX, 256, 64)


@pytest.mark.parametrize("T", [2047, 2048, 2049, 20000])
@pytest.mark.parametrize("rows", [(37, 91), (300, 301)])
def test_bands(gpu, rows, T):
    """Row bands bin through run lists of 2048 triangles (kRecRun)."""
    tr, b = one(soup(T, 64, 512, AVX, seed=T + rows[0], box=(-4, rows[0] - 30, 68, rows[1] + 30), radius=4.0), AVX,
                64, 512, rows=rows)
    assert 0 < (tr["tri_n"] > 0).sum() < T
    assert b["band_per"] == 1


# per = min(2 * (H // band rows), runs // 128, 64) runs a chunk (prk_cs_band_runs_per_chunk): 257 runs make 128
# chunks of 2 and a tail chunk of one run, 385 runs 128 chunks of 3 and a tail of one.  The triangles lie all over
# the frame, so a run lists few of its 2048 and a chunk's triangles come from each of its runs' lists.
@pytest.mark.parametrize("rows,runs,per", [((37, 91), 257, 2), ((300, 301), 385, 3)])
def test_bands_several_runs_a_chunk(gpu, rows, runs, per):
    """A band's counting-sort chunks of more than one run, the last chunk
    short of `per`: chunk_tris' prefix over the runs' counts and chunk_tri's
    search in it (the two heavier frames of this module, half a million
    triangles and more: fewer do not reach per > 1)."""
    T = runs * 2048 - 1000
    tr, b = one(soup(T, 64, 512, AVX, seed=runs, radius=4.0), AVX, 64, 512, rows=rows)
    assert b["band_per"] == per and (runs + per - 1) // per == 129 and runs % per == 1
    listed = (tr["tri_n"] > 0).reshape(-1)
    per_run = np.bincount(np.nonzero(listed)[0] // 2048, minlength=runs)
    assert (per_run > 0).sum() > runs // 2 and per_run[-1] > 0  # most runs, and the tail chunk's, list something


def test_band_nothing_touches(gpu):
    tr, b = one(soup(5000, 64, 512, AVX, seed=5, box=(0, 0, 64, 100)), AVX, 64, 512, rows=(300, 301))
    assert b["entry_count"] == 0


def test_over_capacity_rerun(gpu):
    """A small frame sizes the scratch; a frame with more than four times its
    entries overflows it and is re-run: the read-back answers for the re-run."""
    small = soup(2000, 256, 64, AVX, seed=41)
    big = soup(3000, 256, 64, AVX, seed=42, radius=60.0)
    b, st, _, _, counts = frames([(small, AVX), (small, AVX), (big, AVX)], 256, 64, tile=(8, 8))
    assert counts[2] > 4 * counts[1] and counts[2] > 70000, counts
    assert b["rerun"] == 1
    check(b, st, big, AVX, 256, 64)


def test_refused_without_a_debug_flush(gpu):
    """PRK_ERR_ARG before any flush and after a flush made without debug."""
    sc = soup(100, 256, 64, AVX, seed=51)
    r = prk.Renderer(0)
    try:
        r.target_alloc(256, 64)
        r.clear()
        r.set_camera(sc.prk_transform(), sc.prk_lights())
        g, tex = r.geometry(sc.vertices, sc.colors, sc.normals, sc.uvs), r.texture(sc.texture)
        for debug, ok in ((None, False), (False, False), (True, True), (False, False)):
            if debug is not None:
                r.set_debug(debug)
                r.draw(AVX, g, sc.tri_count, P=sc.P, bitmap=tex, phong=True)
                r.complete_all_work()
            if ok:
                assert r.debug_bins()["tri_count"] == sc.tri_count
            else:
                with pytest.raises(prk.PrkError) as e:
                    r.debug_bins()
                assert e.value.code == abi.PRK_ERR_ARG
    finally:
        r.close()


@pytest.fixture(scope="module")
def hostile():
    scene, cls = bincases.hostile(bincases.P_OFF)
    return scene, cls, binref.spans_of(scene)


@pytest.mark.parametrize("sem", [AVX, SCALAR])
def test_hostile_frame(gpu, hostile, sem):
    """tests/test_binref.py's hostile triangles, whole frame at 64 x 16064: the
    device's bins equal binref's, hold every pair the oracle side needs, and
    the frame is the oracle's."""
    scene, cls, spans = hostile
    W, H = bincases.W, bincases.H
    b, st, col, z, _ = frames([(scene, sem)], W, H, tile=(32, 8))
    tr = check(b, st, scene, sem, W, H)
    need, ntiles = binref.needed(scene, sem, W, H, 0, H, (32, 8), spans)
    offs = b["offs"].astype(np.int64)
    slot_tile = np.searchsorted(offs, np.arange(b["entry_count"]), side="right") - 1
    have = np.unique(b["bins"][:, 0].astype(np.int64) * ntiles + slot_tile)
    assert np.isin(need, have).all()
    oc, oz, _, _ = O.render(scene, semantics=sem, phong=True)
    assert (z.view(np.uint32) == oz.view(np.uint32)).all()
    assert (col == oc).all()
