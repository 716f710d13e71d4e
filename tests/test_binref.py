"""The tile range covers every pixel a triangle stores to (host, no GPU).

binref.tile_ranges restates tri_tile_range_proj (cpu-renderer_amd/csrc/prk_bin.hip);
binref.needed lists the (triangle, tile) pairs a triangle actually stores to,
from the oracle's edge records, spanref's walk and the references' own span
clamps.  The column bound (the slack of DESIGN.md §4.1) and the scalar
row-overflow tiles are claims about edge-DDA values; this holds them to
needed <= entries(tile_ranges) with no exception, on the hostile triangles of
tests/bincases.py, for the three semantics, five tiles, the whole frame and
four bands.  tests/test_gpu_bins.py holds the device to binref."""
import numpy as np
import pytest

import bincases
import binref
import pyref
from prk import abi

SEMS = {"avx": abi.PRK_SEM_AVX, "avx_st": abi.PRK_SEM_AVX_ST, "scalar": abi.PRK_SEM_SCALAR}
_cache = {}


def hostile(shifted):
    """The hostile scene (P = 0 or bincases.P_OFF), its classes and its spans, made once."""
    if shifted not in _cache:
        scene, cls = bincases.hostile(bincases.P_OFF if shifted else (0.0, 0.0, 0.0))
        _cache[shifted] = (scene, cls, binref.spans_of(scene))
    return _cache[shifted]


def pixels(sem, shifted):
    """binref.span_pixels of the hostile scene, made once per semantics."""
    if (sem, shifted) not in _cache:
        scene, _, spans = hostile(shifted)
        _cache[sem, shifted] = binref.span_pixels(spans, SEMS[sem], bincases.W, bincases.H)
    return _cache[sem, shifted]


def test_project_is_pyref_project():
    scene, _, _ = hostile(True)
    ctx = pyref.Cam(scene)
    proj = binref.project(scene, np.arange(scene.tri_count))
    P = [np.float32(v) for v in scene.P]
    for t in range(scene.tri_count):
        for k in range(3):
            want = pyref.project(ctx, [scene.vertices[3 * t + k][i] + P[i] for i in range(3)])
            assert [float(v) for v in want] == proj[t, k].tolist(), (t, k)


@pytest.mark.parametrize("shifted", [False, True], ids=["P0", "P"])
def test_cull_is_pyref_edge_table(shifted):
    """The restated cull keeps a triangle exactly when pyref.edge_table does,
    both ways and for every triangle.  edge_table also returns no edge for a
    kept triangle all of whose edges it skips (an edge whose upper end is
    not below row 0, a horizontal edge): a kept triangle with a vertex below
    row 0 and two distinct y must give edges.  With the front faces
    mirrored (two vertices swapped) the cull must drop what it kept."""
    scene, _, _ = hostile(shifted)
    ctx = pyref.Ctx(scene, abi.PRK_SEM_AVX, True)
    proj = binref.project(scene, np.arange(scene.tri_count))
    front = binref.front_facing(proj)
    back = binref.front_facing(proj[:, [0, 2, 1]])
    assert front.any() and not (front & back).any()
    with np.errstate(all="ignore"):
        for t in range(scene.tri_count):
            edges = pyref.edge_table(ctx, t)
            if edges:
                assert front[t], t
            y = proj[t, :, 1]
            if front[t] and y.max() > 0 and y.max() != y.min():
                assert edges, t
    mirrored = scene.subset(0, scene.tri_count)
    v = mirrored.vertices.reshape(-1, 3, 3)
    v[:, [1, 2]] = v[:, [2, 1]]
    mirrored.vertices = v.reshape(-1, 3).copy()
    mctx = pyref.Ctx(mirrored, abi.PRK_SEM_AVX, True)
    with np.errstate(all="ignore"):
        for t in np.nonzero(front)[0].tolist():
            assert not pyref.edge_table(mctx, t), t


@pytest.mark.parametrize("shifted", [False, True], ids=["P0", "P"])
@pytest.mark.parametrize("sem", sorted(SEMS))
def test_every_class_draws(sem, shifted):
    """Each hostile class still has triangles that store pixels after the cull."""
    scene, cls, spans = hostile(shifted)
    keys, ntiles = binref.needed(scene, SEMS[sem], bincases.W, bincases.H, 0, bincases.H, (32, 8), pixels=pixels(sem, shifted))
    drawn = np.unique(keys // ntiles)
    for name, idx in cls.items():
        assert np.isin(idx, drawn).any(), name
    assert np.isin(cls["far_1e+07"], drawn).sum() >= 4 and np.isin(cls["tall"], drawn).sum() >= 4


@pytest.mark.parametrize("shifted", [False, True], ids=["P0", "P"])
@pytest.mark.parametrize("tile", bincases.TILES, ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("sem", sorted(SEMS))
def test_needed_within_range(sem, tile, shifted):
    scene, cls, spans = hostile(shifted)
    W, H = bincases.W, bincases.H
    for row0, row1 in [(0, H)] + bincases.BANDS:
        tr = binref.tile_ranges(scene, binref.draws_of(scene, SEMS[sem]), W, H, row0, row1, tile)
        need, ntiles = binref.needed(scene, SEMS[sem], W, H, row0, row1, tile, pixels=pixels(sem, shifted))
        missing = need[~np.isin(need, binref.entry_keys(tr))]
        assert missing.size == 0, (sem, tile, (row0, row1), [(int(k // ntiles), int(k % ntiles)) for k in missing[:8]],
                                   [n for n, i in cls.items() if np.isin(missing // ntiles, i).any()])
        assert need.size > 0, (row0, row1)


def test_print_column_margins(capsys):
    """The smallest distance between a column a span end rounds to and the
    range's own columns before their clamp, per semantics: a measurement,
    printed and recorded in DESIGN.md §4.1, not asserted."""
    for sem in sorted(SEMS):
        m = np.inf
        for shifted in (False, True):
            scene, _, spans = hostile(shifted)
            tr = binref.tile_ranges(scene, binref.draws_of(scene, SEMS[sem]), bincases.W, bincases.H, 0, bincases.H,
                                    (8, 8))
            live = tr["live"][spans[0]]
            m = min(m, binref.column_margin(tr, tuple(a[live] for a in spans), SEMS[sem]))
        with capsys.disabled():
            print("column margin %s: %.4f px" % (sem, m))
        assert np.isfinite(m)
