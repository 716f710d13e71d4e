"""CPU tests of the comb scenes (tests/census.py) that the huge-object walk
tests in test_gpu_parity.py render: each scene's census shows the figure its
GPU test is about, and the oracle renders it as one object.  The figures
stand here next to the scenes; the GPU tests assert the same properties and
compare the device's own sizes (Renderer.walk_routes) with the census.

Where a walk's list sizes decide its path (prk_spans.hip, prk_span_pass.hip):
  new edges on a row  < 1024: one insertion window; == 1024: a full window,
                      then an empty one; > 1024: several
  most                <= 1022: an LDS slot class; <= 9200 (and rows < 16000):
                      k_obj_walk_lds; beyond: k_obj_walk_big
  ns                  the longest scan of a window (census.window_scans; at
                      most `most`): <= 8192 k_obj_walk_big scans from
                      registers, more: it reloads
  rows + 1            > 16000: no histogram, most = INT32_MAX, one wave
  edges               > 8192: more than one workgroup in k_maxact_huge_part
"""
import numpy as np
import pytest

import census as Cn
import oracle as O
from prk import abi, scenes


def _renders(s, sem=abi.PRK_SEM_AVX):
    """The oracle draws the scene as one object and covers pixels with it."""
    col, z, win, st = O.render(s, semantics=sem, phong=True, threads=1, tris_per_object=s.tri_count)
    assert st["spans"] > 0 and (win >= 0).sum() > 0, s.name
    assert np.isfinite(z[win >= 0]).all()


def test_census_on_a_known_table():
    """census() on a hand-made case: one triangle, apex in row 10, base in
    rows 20 / 30 -- edges [10, 20), [10, 30), [20, 30)."""
    s = scenes.comb([(1, 10, 20, 20)], 64, 64, seed=0, kink=0.0)
    v = s.vertices.reshape(1, 3, 3).copy()
    D, F, M2P, cx, cy = s.transform
    z = v[0, :, 2]
    scr = np.array([[30.0, 10.0], [26.0, 20.0], [34.0, 30.0]])
    e1, e2 = scr[1] - scr[0], scr[2] - scr[0]
    if e1[0] * e2[1] - e1[1] * e2[0] > 0:
        scr[[1, 2]] = scr[[2, 1]]
    v[0, :, 0] = (scr[:, 0] - cx) * (D - z) / M2P / F
    v[0, :, 1] = (scr[:, 1] - cy) * (D - z) / M2P / F
    s.vertices = v.reshape(-1, 3).astype(np.float32)
    c = Cn.census(s)
    assert (c["first"], c["rows"], c["edges"]) == (10, 20, 3)
    # listed through YMax inclusive in the histogram (k_obj_maxact), [YMin, YMax) in the entries
    assert c["most"] == 3 and c["ents"] == 10 + 20 + 10
    assert list(np.nonzero(c["new"])[0]) == [0, 10] and c["new"][0] == 2 and c["new"][10] == 1
    assert list(c["listed"][[0, 9, 10, 11, 19]]) == [2, 2, 3, 2, 2]
    b = Cn.census(s, rows=(0, 25))  # a band clips the rows and the entries at row1
    assert (b["rows"], b["most"], b["ents"]) == (15, 3, 10 + 15 + 5)
    assert c["ns"] == 3 and b["ns"] == 3  # rows 11.. and 21..: expiry alone over 2; row 20: 2 old + 1
    assert Cn.device_sizes(c) == (3, 20, 40)
    assert Cn.device_sizes(dict(c, rows=15999)) == (3, 15999, 40)
    assert Cn.device_sizes(dict(c, rows=16000)) == (Cn.INT32_MAX, Cn.INT32_MAX, 0)


def test_window_scans():
    """The scan lengths of a row's insertion windows, by hand: a list of 5000
    that `new` edges enter (listed counts them)."""
    listed = lambda new: 5000 + new  # noqa: E731
    for new, want in [(0, 5000),            # expiry alone: the whole list
                      (1, 5001),            # one window: 5000 old + the tail gap
                      (1023, 5001),
                      (1024, 6024),         # a full window (5001), then expiry alone over all 6024
                      (1025, 6025),         # windows of 1024 and 1: the second scans 6024 + 1
                      (2047, 6025),
                      (2048, 7048),
                      (2049, 7049)]:
        assert Cn.window_scans([listed(new)], [new])[0] == want, new


def test_per_triangle_rows_make_the_object_table():
    """The per-triangle edge rows the builders select by are the whole
    object's table, edge for edge."""
    s = Cn.lds_scene(False)
    tri, y0, y1 = O.edge_rows_per_triangle(s)
    w = O.fill_edge_table_words(s, 0, s.tri_count).view(np.int32)
    assert sorted(zip(y0.tolist(), y1.tolist())) == sorted(zip(w[:, 7].tolist(), w[:, 0].tolist()))
    assert tri.max() == s.tri_count - 1 and (np.diff(tri) >= 0).all()


@pytest.mark.parametrize("k", [1023, 1024, 1025, 2048, 2049])
def test_window_scenes(k):
    """A: most 1777 to 2822, rows 92; the busiest row (10) takes exactly k."""
    s = Cn.window_scene(k)
    c = Cn.census(s)
    row, new = Cn.busiest(c)
    assert new == k and c["listed"][row - c["first"] - 1] > 200  # into a list already several hundred long
    assert Cn.SLOT_CAP < c["most"] <= Cn.LDS_CAP and c["rows"] < Cn.MAXACT_ROWS
    assert (c["new"] >= Cn.WINDOW).sum() == (1 if k >= Cn.WINDOW else 0)
    _renders(s)


@pytest.mark.parametrize("ties", [False, True])
def test_lds_scenes(ties):
    """B: most 4912 (5888 with ties), rows 92; row 10 takes 2463 (2971) new
    edges and row 20 685 (807) into a list of thousands; 32 (39) rows of odd
    length."""
    s = Cn.lds_scene(ties)
    c = Cn.census(s)
    Cn.check_lds_scene(c)
    if ties:  # exact duplicates: every second triangle of the base scene twice
        v = s.vertices.reshape(s.tri_count, 9)
        assert len(np.unique(v, axis=0)) == s.tri_count * 2 // 3
    # the band of the E cases: well below the busy rows, ending inside the object
    b = Cn.census(s, rows=Cn.BAND)
    Cn.check_band(b)
    assert b["most"] == c["most"] and b["ents"] < c["ents"]
    _renders(s)
    _renders(Cn.untextured(s), abi.PRK_SEM_SCALAR)


@pytest.mark.parametrize("most", [9200, 9201])
def test_handover_scenes(most):
    """C: most exactly 9200 / 9201 (rows 92, 3792 / 3796 new edges on row 10)."""
    s = Cn.handover_scene(most)
    c = Cn.census(s)
    assert c["most"] == most and (most <= Cn.LDS_CAP) == (most == 9200)
    _renders(s)


@pytest.mark.parametrize("ns", [8192, 8193])
def test_reload_scenes(ns):
    """D: tied scenes whose longest scan is exactly 8192 / 8193 entries, on
    row 19 (8192: expiry alone over the 8192 listed; 8193: 10 new edges
    into 8192 old ones); most 8259, rows 92, ~3680 new edges on row 10."""
    s = Cn.reload_scene(ns)
    c = Cn.census(s)
    assert c["ns"] == ns and ns <= c["most"] <= Cn.LDS_CAP
    scans = Cn.window_scans(c["listed"], c["new"])
    assert (scans == ns).sum() >= 1 and (c["new"][scans == ns] % Cn.WINDOW == 0).all() == (ns == 8192)
    v = s.vertices.reshape(s.tri_count, 9)
    assert len(np.unique(v, axis=0)) < s.tri_count * 0.7  # (ties)
    _renders(s)


def test_big_scene():
    """D / F: most 12017, rows 92, 5896 new edges on row 10, scans of up to
    12001 entries, 18000 edges (three histogram workgroups of 8192)."""
    s = Cn.big_scene()
    c = Cn.census(s)
    assert 11000 <= c["most"] <= 14000 and c["edges"] > 2 * 8192 and c["ns"] > 8192
    Cn.check_band(Cn.census(s, rows=Cn.BAND))
    _renders(s)


def test_catalogue():
    """Every scene the GPU tests name exists and is built once."""
    for name in Cn.SCENES:
        assert Cn.scene(name) is Cn.scene(name) and Cn.scene(name).tri_count >= 64


def test_tall_scenes():
    """Tall frames (64 x 16064): most 1341 (1303 new edges on row 20); rows
    15996, and 16045 for the stretched object, which reaches the frame's
    bottom."""
    s = Cn.tall_scene(False)
    c = Cn.census(s)
    assert 15990 <= c["rows"] <= 15999 and c["most"] > 1024
    assert Cn.device_sizes(c) == (c["most"], c["rows"], c["ents"])
    t = Cn.tall_scene(True)
    d = Cn.census(t)
    assert d["rows"] >= 16000 and d["first"] + d["rows"] == Cn.TALL_H and d["most"] > 1024
    assert Cn.device_sizes(d) == (Cn.INT32_MAX, Cn.INT32_MAX, 0)
    assert s.tri_count == t.tri_count and d["first"] == c["first"]
    _renders(s)
    _renders(t)
