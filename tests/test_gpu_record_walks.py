"""GPU tests: the record walks of a handle (prk_records_advance, prk_records_spans,
prk_records_rows; prk_debug_list_stats) -- DESIGN §4.4.8.

The statistics the device computes where the records are (k_list_stats,
k_list_most) are held to the closed forms of liststats.py, which
test_list_stats_rule.py holds to the host pass's sweeps.  The three calls are
held to their host-input calls on the same lists (download() + counts()):
np.array_equal on uint32 words -- the same kernels run on the same inputs --
and the same routes (prk_debug_list_routes).
"""
import ctypes as C

import numpy as np
import pytest

import prk
import test_gpu_advance_lists as A
import test_gpu_row_records as RW
import test_gpu_span_records as SP
from liststats import expected_rows
from prk import abi, scenes
from test_gpu_edge_lists import AVX, YMIN, Frame, same_frame, soup_scene
from test_gpu_long_lists import CANARY, crowd, five_groups
from test_gpu_records import RULE_COUNTS, SUB_COUNTS, SUB_RANGES, make_batch, offsets, rule

pytestmark = pytest.mark.gpu

edge = A.edge
HUGE = str(1 << 62)
THREAD_ONLY = (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def fr(gpu):
    """The soup with a target: geometry, texture, and its records as 20-triangle objects."""
    s = soup_scene()
    with Frame(s, True) as f:
        f.words, f.counts = f.records(3, 20)
        assert f.counts.size == 15 and (f.counts > 0).all()
        yield f


@pytest.fixture(scope="module")
def sphere(gpu):
    c = A.Ctx(SP._sphere_scene())
    c.words, c.counts = c.records(3, 2208)
    assert c.counts.tolist() == [2072]
    yield c
    c.close()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, label):
    assert len(got) == len(want), label
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(u32(g), u32(w)), "%s: output %d differs" % (label, k)


def parity(r, rec, words, counts, height, label, first=0, n=None):
    """Lists [first, first + n) of the handle through the three calls against
    the host-input calls on that slice of its records; returns the routes."""
    off = offsets(counts)
    n = counts.size - first if n is None else n
    w = np.ascontiguousarray(words[off[first]:off[first + n]])
    c = np.ascontiguousarray(counts[first:first + n])
    label = "%s, lists [%d, %d) height %d" % (label, first, first + n, height)
    assert w.shape[0] > 0, label  # (the routes of an empty batch are the previous call's)
    routes = []
    for name, host, handle in (("advance", r.advance_edge_lists, rec.advance), ("spans", r.span_records, rec.spans),
                               ("rows", r.row_records, rec.rows)):
        want = host(w, c, height)
        routes.append(r.list_routes())
        got = handle(height, first, n)
        assert r.list_routes() == routes[-1], (label, name)
        same(got, want, "%s %s" % (label, name))
    assert routes[0] == routes[1] == routes[2], label
    return routes[0]


def misaligned(counts):
    """The first list past list 0 whose record offset is no multiple of 4."""
    off = offsets(counts)
    return next(a for a in range(1, counts.size) if off[a] % 4)


def prefixed(words, counts, lead=1):
    """Three short lists in front, of `lead`, 1 and 1 edges: lists 1, 2 and 3
    begin at records lead, lead + 1 and lead + 2."""
    front = [edge(0, 10, 5.0 + k, 0.5, (k + 1) & 1, k) for k in range(lead)]
    front += [edge(1, 7, 9.0, -0.5, 0, 1), edge(2, 30, 3.0, 0.25, 1, 2)]
    return (np.concatenate([np.array(front, np.uint32), words]),
            np.concatenate([[lead, 1, 1], counts]).astype(np.uint32))


def mixed_batch():
    hw, hc, _ = A.hand_batch()
    sw, sc = SP.hand_batch()
    return np.concatenate([hw, five_groups(), sw]), np.concatenate([hc, [5000], sc]).astype(np.uint32)


# ---- 1. statistics ---------------------------------------------------------------------------------------------------
def check_stats(rec, words, counts, label, min_steps, ranges=((0, None),)):
    ymax = words[:, 0].view(np.int32)
    top = int(ymax.max())
    off = offsets(counts)
    for first, n in ranges:
        n = counts.size - first if n is None else n
        w, c = words[off[first]:off[first + n]], counts[first:first + n]
        for height in (0, max(1, top // 2), top + 3):
            got = rec.list_stats(height, first, n)
            want = expected_rows(w, c, height, min_steps)
            bad = np.argwhere(got != want)
            assert bad.size == 0, "%s lists [%d, %d) height %d: list %d field %s got %d want %d" % (
                label, first, first + n, height, bad[0][0], abi.LIST_STATS_FIELDS[bad[0][1]], got[tuple(bad[0])],
                want[tuple(bad[0])])


@pytest.mark.parametrize("steps", [None, "0"], ids=["default", "forced"])
def test_statistics(fr, sphere, monkeypatch, steps):
    """Default routing: only lists past the threshold have a `most`; forced:
    every list with an edge is a candidate, so k_list_most runs for all."""
    min_steps = 3432
    if steps is not None:
        monkeypatch.setenv("PRK_ADV_WG_MIN_STEPS", steps)
        min_steps = int(steps)
    r = fr.r
    batches = [("soup", fr.words, fr.counts, ((0, None), (misaligned(fr.counts), 9))),
               ("rule batch", *make_batch(fr.words, RULE_COUNTS), ((0, None),)),
               ("sub batch", *make_batch(fr.words, SUB_COUNTS), SUB_RANGES),
               ("crowds", np.array(crowd(62, 1, 3) + crowd(63, 1, 3) + crowd(1022, 1, 3) + crowd(1023, 1, 3), np.uint32),
                np.array([62, 63, 1022, 1023], np.uint32), ((0, None), (1, 3), (2, 2))),
               ("sphere", sphere.words, sphere.counts, ((0, None),))]
    assert [int(offsets(batches[2][2])[a]) % 4 for a, _ in SUB_RANGES[:4]] == [0, 1, 2, 3]
    seen_most = 0
    for label, words, counts, ranges in batches:
        rec = r.records_upload(words, counts)
        assert rec.sorted_flags().all()
        check_stats(rec, words, counts, label, min_steps, ranges)
        seen_most += int((rec.list_stats(int(words[:, 0].view(np.int32).max()))[:, 2] > 0).sum())
        rec.close()
    assert seen_most >= (30 if steps == "0" else 2)  # (default: the 1022 / 1023 crowds and the sphere at least)


# ---- 2. parity of the three calls ------------------------------------------------------------------------------------
ROUTING = [None, "0", HUGE]
ROUTING_IDS = ["default", "forced", "thread-only"]


def set_routing(monkeypatch, steps):
    if steps is not None:
        monkeypatch.setenv("PRK_ADV_WG_MIN_STEPS", steps)


@pytest.mark.parametrize("steps", ROUTING, ids=ROUTING_IDS)
@pytest.mark.parametrize("source", ["upload", "geometry"])
def test_parity_soup(fr, monkeypatch, steps, source):
    set_routing(monkeypatch, steps)
    words, counts = fr.words, fr.counts
    if source == "upload":
        words, counts = prefixed(words, counts)
        rec = fr.r.records_upload(words, counts)
    else:
        s = fr.s
        rec = fr.r.records_from_geometry(fr.g, s.tri_count, P=s.P, setup=3, tris_per_object=20)
        assert np.array_equal(rec.download(), words)
    a = misaligned(counts)
    for height in (96, 40):
        routes = parity(fr.r, rec, words, counts, height, "soup " + source)
        parity(fr.r, rec, words, counts, height, "soup " + source, a, counts.size - a - 2)
    if steps == "0":
        assert routes["thread"] == 0 and sum(routes["slots"]) == counts.size
    if steps == HUGE:
        assert routes == dict(thread=counts.size, slots=THREAD_ONLY)
    rec.close()


@pytest.mark.parametrize("steps", ROUTING, ids=ROUTING_IDS)
@pytest.mark.parametrize("source", ["upload", "geometry"])
def test_parity_sphere_one_list(sphere, monkeypatch, steps, source):
    set_routing(monkeypatch, steps)
    r, words, counts = sphere.r, sphere.words, sphere.counts
    if source == "upload":
        words, counts = prefixed(words, counts)
        rec = r.records_upload(words, counts)
    else:
        s = sphere.s
        rec = r.records_from_geometry(sphere.g, s.tri_count, P=s.P, setup=3, tris_per_object=2208)
        assert np.array_equal(rec.download(), words)
    routes = parity(r, rec, words, counts, 256, "sphere " + source)
    if steps != HUGE:  # the workgroup walk, past the 126 class
        small = 3 if steps == "0" and source == "upload" else 0  # (the one-edge lists in front)
        assert sum(routes["slots"][2:]) == 1 and sum(routes["slots"][:2]) == small
    else:
        assert routes["slots"] == THREAD_ONLY
    if source == "upload":
        for first in (1, 2, 3):  # the long list from records 1, 2 and 3 of the handle's buffer
            parity(r, rec, words, counts, 128, "sphere upload", first, counts.size - first)
    rec.close()


@pytest.mark.parametrize("steps", [None, "0"], ids=ROUTING_IDS[:2])
def test_parity_mixed_batch(gpu, monkeypatch, steps):
    """Short lists around five_groups(): its edge-rows are few and its
    edge-rows + n (n - 1) / 2 pass 2^21, so its cost is formed from the exact
    insertion scans -- the branch that needs `scans` -- and it is routed to
    the largest class by default."""
    set_routing(monkeypatch, steps)
    words, counts = prefixed(*mixed_batch(), lead=2)
    long_one = int(np.flatnonzero(counts == 5000)[0])
    r = prk.Renderer()
    try:
        rec = r.records_upload(words, counts)
        st = rec.list_stats(A.HAND_HEIGHT)[long_one]
        assert st[0] == 5000 and st[0] + 5000 * 4999 // 2 > 1 << 21 and st[1] == 5 * (1000 * 999 // 2), st
        routes = parity(r, rec, words, counts, A.HAND_HEIGHT, "mixed")
        if steps is None:
            assert routes == dict(thread=counts.size - 1, slots=(0, 0, 0, 0, 1))
        for first in (1, 2, 3):
            parity(r, rec, words, counts, A.HAND_HEIGHT, "mixed", first, long_one - first + 2)
        # the long list alone (test_long_list_over_the_thread_cap's), from record offset 3 mod 4
        assert offsets(counts)[long_one] % 4
        routes = parity(r, rec, words, counts, 64, "five groups", long_one, 1)
        assert routes == dict(thread=0, slots=(0, 0, 0, 0, 1))
    finally:
        r.close()


def test_parity_five_groups_thread_only(gpu, monkeypatch):
    """Without a route the exact cost refuses the list, as the host pass does."""
    monkeypatch.setenv("PRK_ADV_WG_MIN_STEPS", HUGE)
    words, counts = five_groups(), np.array([5000], np.uint32)
    r = prk.Renderer()
    try:
        rec = r.records_upload(words, counts)
        out, nxt = np.full_like(words, CANARY), np.full(5000, 77, np.int32)
        assert A._raw(r, words, counts, 64, out, nxt) == abi.PRK_ERR_LIMIT
        assert r._L.prk_records_advance(r._h, rec.handle, 0, 1, 64, None, out.ctypes.data,
                                        nxt.ctypes.data) == abi.PRK_ERR_LIMIT
        assert (out == CANARY).all() and (nxt == 77).all()
    finally:
        r.close()


def test_parity_scans_decide_under_the_cap(gpu, monkeypatch):
    """41 groups of 50 edges, each group alone on its row, and no route:
    edge-rows + n (n - 1) / 2 pass 2^21, the exact scans (41 * 50 * 49 / 2)
    do not, so the thread walk takes the list -- by the device's scans as by
    the host's sweep."""
    monkeypatch.setenv("PRK_ADV_WG_MIN_STEPS", HUGE)
    words = np.array([edge(2 * g, 2 * g + 1, float(k), 0.0, (k + 1) & 1, k & 3) for g in range(41) for k in range(50)],
                     np.uint32)
    words, counts = prefixed(words, np.array([2050], np.uint32))
    r = prk.Renderer()
    try:
        rec = r.records_upload(words, counts)
        st = rec.list_stats(128)[3]
        assert st.tolist() == [2050, 41 * (50 * 49 // 2), 0, 0, 81], st
        assert st[0] + 2050 * 2049 // 2 > 1 << 21
        routes = parity(r, rec, words, counts, 128, "41 groups of 50")
        assert routes == dict(thread=4, slots=THREAD_ONLY)
        parity(r, rec, words, counts, 128, "41 groups of 50", 3, 1)
    finally:
        r.close()


@pytest.mark.parametrize("n,slots", [(62, (1, 0, 0, 0, 0)), (63, (0, 1, 0, 0, 0)), (1022, (0, 0, 0, 0, 1)),
                                     (1023, THREAD_ONLY)])
def test_parity_class_edges(gpu, monkeypatch, n, slots):
    monkeypatch.setenv("PRK_ADV_WG_MIN_STEPS", "0")
    words, counts = prefixed(np.array(crowd(n, 1, 3), np.uint32), np.array([n], np.uint32))
    r = prk.Renderer()
    try:
        rec = r.records_upload(words, counts)
        routes = parity(r, rec, words, counts, 64, "%d listed" % n, 3, 1)
        assert routes == dict(thread=int(n == 1023), slots=slots)
        parity(r, rec, words, counts, 64, "%d listed" % n, 2, 2)
    finally:
        r.close()


# ---- 3. sizing and capacity ------------------------------------------------------------------------------------------
def p64(a):
    return C.cast(a.ctypes.data, C.POINTER(C.c_uint64))


def test_sizing_and_short_capacity(fr):
    r, L, ctx = fr.r, fr.r._L, fr.r._h
    words, counts = fr.words, fr.counts
    nl = counts.size
    rec = r.records_upload(words, counts)
    h = rec.handle
    hs, hsc = r.span_records(words, counts, 96)
    hr, hp, hrc = r.row_records(words, counts, 96)
    assert hs.shape[0] > 1 and hr.shape[0] > 1 and hp.shape[0] > 1
    # the sizing calls
    sc, total = np.full(nl, 99, np.uint32), np.full(1, 99, np.uint64)
    assert L.prk_records_spans(ctx, h, 0, nl, 96, None, 0, sc.ctypes.data, p64(total)) == abi.PRK_OK
    assert np.array_equal(sc, hsc) and total[0] == hs.shape[0]
    rc, nrow, npair = np.full(nl, 99, np.uint32), np.full(1, 99, np.uint64), np.full(1, 99, np.uint64)
    assert L.prk_records_rows(ctx, h, 0, nl, 96, None, 0, None, 0, rc.ctypes.data, p64(nrow),
                              p64(npair)) == abi.PRK_OK
    assert np.array_equal(rc, hrc) and (nrow[0], npair[0]) == (hr.shape[0], hp.shape[0])
    # one short: PRK_ERR_ARG, the counts and totals written, the arrays untouched
    spans = np.full((hs.shape[0], 25), CANARY, np.uint32)
    sc[:], total[:] = 99, 99
    assert L.prk_records_spans(ctx, h, 0, nl, 96, spans.ctypes.data, hs.shape[0] - 1, sc.ctypes.data,
                               p64(total)) == abi.PRK_ERR_ARG
    assert (spans == CANARY).all() and np.array_equal(sc, hsc) and total[0] == hs.shape[0]
    for rcap, pcap in ((hr.shape[0] - 1, hp.shape[0]), (hr.shape[0], hp.shape[0] - 1)):
        rows, pairs = np.full(hr.shape, CANARY, np.uint32), np.full(hp.shape, CANARY, np.uint32)
        rc[:], nrow[:], npair[:] = 99, 99, 99
        assert L.prk_records_rows(ctx, h, 0, nl, 96, rows.ctypes.data, rcap, pairs.ctypes.data, pcap, rc.ctypes.data,
                                  p64(nrow), p64(npair)) == abi.PRK_ERR_ARG
        assert (rows == CANARY).all() and (pairs == CANARY).all() and np.array_equal(rc, hrc)
        assert (nrow[0], npair[0]) == (hr.shape[0], hp.shape[0])
    # rows without pairs (or the reverse) is refused as prk_row_records refuses it
    rows = np.full(hr.shape, CANARY, np.uint32)
    assert L.prk_records_rows(ctx, h, 0, nl, 96, rows.ctypes.data, hr.shape[0], None, 0, rc.ctypes.data, p64(nrow),
                              p64(npair)) == abi.PRK_ERR_ARG
    assert (rows == CANARY).all()
    # Next alone, and the records alone
    hw, hn = r.advance_edge_lists(words, counts, 96)
    nxt = np.full(words.shape[0], 77, np.int32)
    assert L.prk_records_advance(ctx, h, 0, nl, 96, None, None, nxt.ctypes.data) == abi.PRK_OK
    assert np.array_equal(nxt, hn)
    out = np.full_like(words, CANARY)
    assert L.prk_records_advance(ctx, h, 0, nl, 96, None, out.ctypes.data, None) == abi.PRK_OK
    assert np.array_equal(out, hw)
    rec.close()


# ---- 4. advanced_out -------------------------------------------------------------------------------------------------
def test_advanced_handle(fr):
    r, L, ctx = fr.r, fr.r._L, fr.r._h
    words, counts = fr.words, fr.counts
    rec = r.records_upload(words, counts)
    hw, hn = r.advance_edge_lists(words, counts, 40)
    assert (hw != words).any()
    adv = rec.advance(40, keep=True, host=False)
    assert isinstance(adv, prk.Records) and adv.handle != rec.handle
    assert (adv.list_count, adv.total) == (counts.size, words.shape[0])
    assert np.array_equal(adv.download(), hw) and np.array_equal(rec.download(), words)
    assert np.array_equal(adv.counts(), counts)
    assert np.array_equal(adv.sorted_flags(), rule(hw, counts)) and adv.sorted_flags().all()
    # the frame of the new handle against the frame of the host call's records
    r.reset_draws()
    r.clear()
    r.draw_records(adv, semantics=AVX[0], bitmap=fr.tex, phong=True)
    got = fr.done()
    r.clear()
    fr.batch(hw, counts, AVX)
    want = fr.done()
    assert (got[0] != scenes.CLEAR_COLOR).any()
    same_frame(got, want, "draw_records of the advanced handle")
    # again, with the host outputs beside the handle: the host call applied twice
    hw2, hn2 = r.advance_edge_lists(hw, counts, 40)
    gw2, gn2, adv2 = adv.advance(40, keep=True, host=True)
    same((gw2, gn2, adv2.download()), (hw2, hn2, hw2), "advanced twice")
    # a sub-range: a handle of those lists alone
    a = 4
    off = offsets(counts)
    part = rec.advance(40, a, 6, keep=True, host=False)
    assert np.array_equal(part.counts(), counts[a:a + 6]) and np.array_equal(part.download(), hw[off[a]:off[a + 6]])
    # lists without a record
    none = rec.advance(40, 3, 0, keep=True, host=False)
    assert (none.list_count, none.total) == (0, 0)
    # a failed call makes no handle
    live = [rec, adv, adv2, part, none]
    nxt_handle = max(x.handle for x in live) + 1
    n, t = C.c_uint32(0), C.c_uint64(0)
    for height, first, nl, status in ((-1, 0, 15, abi.PRK_ERR_ARG), (65537, 0, 15, abi.PRK_ERR_LIMIT),
                                      (40, 10, 6, abi.PRK_ERR_ARG)):
        h = C.c_int32(5)
        assert L.prk_records_advance(ctx, rec.handle, first, nl, height, C.byref(h), None, None) == status
        assert h.value == -1
        assert L.prk_records_info(ctx, nxt_handle, C.byref(n), C.byref(t)) == abi.PRK_ERR_ARG
    for x in live[1:]:
        x.close()
    rec.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
class Outputs:
    """Canaried outputs of the three calls and the statistics."""

    def __init__(self, nrec, nlist):
        self.out, self.nxt = np.full((max(nrec, 1), 27), CANARY, np.uint32), np.full(max(nrec, 1), 77, np.int32)
        self.spans, self.sc = np.full((16, 25), CANARY, np.uint32), np.full(max(nlist, 1), 77, np.uint32)
        self.rows, self.pairs = np.full((8, 2), CANARY, np.uint32), np.full((16, 24), CANARY, np.uint32)
        self.rc = np.full(max(nlist, 1), 77, np.uint32)
        self.total, self.nrow, self.npair = (np.full(1, 99, np.uint64) for _ in range(3))
        self.stats = np.full((max(nlist, 1), 5), 99, np.uint64)
        self.h = C.c_int32(5)

    def call(self, r, handle, first, n, height, pair_capacity=16):
        L, ctx = r._L, r._h
        return (L.prk_records_advance(ctx, handle, first, n, height, C.byref(self.h), self.out.ctypes.data,
                                      self.nxt.ctypes.data),
                L.prk_records_spans(ctx, handle, first, n, height, self.spans.ctypes.data, 16, self.sc.ctypes.data,
                                    p64(self.total)),
                L.prk_records_rows(ctx, handle, first, n, height, self.rows.ctypes.data, 8, self.pairs.ctypes.data,
                                   pair_capacity, self.rc.ctypes.data, p64(self.nrow), p64(self.npair)),
                L.prk_debug_list_stats(ctx, handle, first, n, height, self.stats.ctypes.data))

    def untouched(self, label):
        assert (self.out == CANARY).all() and (self.nxt == 77).all() and self.h.value == -1, label
        assert (self.spans == CANARY).all() and (self.sc == 77).all() and self.total[0] == 0, label  # (0, as the host call)
        assert (self.rows == CANARY).all() and (self.pairs == CANARY).all() and (self.rc == 77).all(), label
        assert (self.nrow[0], self.npair[0]) == (99, 99) and (self.stats == 99).all(), label


def test_refusals(fr):
    r, L, ctx = fr.r, fr.r._L, fr.r._h
    words, counts = fr.words, fr.counts
    off = offsets(counts)
    # list 6 unsorted: one YMin swapped with its successor's
    ymin = words[:, YMIN].view(np.int32)
    i = int(off[6]) + int(np.flatnonzero(np.diff(ymin[off[6]:off[7]]) > 0)[0])
    sw = words.copy()
    sw[[i, i + 1], YMIN] = words[[i + 1, i], YMIN]
    rec = r.records_upload(sw, counts)
    assert rec.sorted_flags().tolist() == [1] * 6 + [0] + [1] * 8
    four = (abi.PRK_ERR_UNSUPPORTED,) * 4
    for first, n in ((0, 15), (6, 1), (2, 5)):
        o = Outputs(words.shape[0], 15)
        assert o.call(r, rec.handle, first, n, 96) == four
        o.untouched("unsorted list in [%d, %d)" % (first, first + n))
    for first, n in ((0, 6), (7, 8)):  # the same handle, the unsorted list outside the range
        w, c = sw[off[first]:off[first + n]], counts[first:first + n]
        same(rec.advance(96, first, n), r.advance_edge_lists(w, c, 96), "beside the unsorted list: advance")
        same(rec.spans(96, first, n), r.span_records(w, c, 96), "beside the unsorted list: spans")
        same(rec.rows(96, first, n), r.row_records(w, c, 96), "beside the unsorted list: rows")
    # arguments
    ok = r.records_upload(words, counts)
    dead = r.records_upload(words[:int(counts[0])], counts[:1])
    dead_handle = dead.handle
    dead.close()
    arg, lim = (abi.PRK_ERR_ARG,) * 4, (abi.PRK_ERR_LIMIT,) * 4
    for label, handle, first, n, height, want in (
            ("height < 0", ok.handle, 0, 15, -1, arg), ("height > 65536", ok.handle, 0, 15, 65537, lim),
            ("a destroyed handle", dead_handle, 0, 1, 96, arg), ("no such handle", 9999, 0, 1, 96, arg),
            ("a negative handle", -1, 0, 1, 96, arg), ("a range past the end", ok.handle, 10, 6, 96, arg),
            ("a range that starts past the end", ok.handle, 16, 0, 96, arg)):
        o = Outputs(words.shape[0], 15)
        assert o.call(r, handle, first, n, height) == want, label
        o.untouched(label)
    assert L.prk_records_advance(ctx, ok.handle, 0, 15, 96, None, None, None) == abi.PRK_ERR_ARG
    assert L.prk_records_advance(ctx, ok.handle, 0, 0, 96, None, None, None) == abi.PRK_ERR_ARG
    # no lists, and a handle of none: PRK_OK, zero totals
    empty = r.records_upload(np.zeros((0, 27), np.uint32), np.zeros(0, np.uint32))
    for handle, first in ((ok.handle, 15), (ok.handle, 4), (empty.handle, 0)):
        o = Outputs(0, 0)
        o.h = C.c_int32(5)
        assert o.call(r, handle, first, 0, 96) == (abi.PRK_OK,) * 4
        assert (o.total[0], o.nrow[0], o.npair[0]) == (0, 0, 0) and (o.spans == CANARY).all()
        made = prk.Records(r, o.h.value)
        assert (made.list_count, made.total) == (0, 0)
        made.close()
    # the limits of the walk: 2^21 edge-rows; 2100 edges on a row (the exact scans pass the cap, no class holds them)
    long_list = np.array([edge(0, 65536, float(k), 0.0, k & 1) for k in range(257)], np.uint32)
    one_row = np.array([edge(0, 1, float(k), 0.0, k & 1) for k in range(2100)], np.uint32)
    for label, w, height in (("257 x 65536", long_list, 65536), ("2100 on one row", one_row, 64)):
        cnt = np.array([w.shape[0]], np.uint32)
        assert A._raw(r, w, cnt, height, np.empty_like(w), None) == abi.PRK_ERR_LIMIT, label
        big = r.records_upload(w, cnt)
        o = Outputs(w.shape[0], 1)
        got = o.call(r, big.handle, 0, 1, height)
        assert got[:3] == (abi.PRK_ERR_LIMIT,) * 3 and got[3] == abi.PRK_OK, label  # (the statistics are no walk)
        o.stats[:] = 99
        o.untouched(label)
        big.close()
    # a row of more than 1000 pairs: the walk finds it
    w, cnt = RW._crowd(2002), np.array([2002], np.uint32)
    big = r.records_upload(w, cnt)
    o = Outputs(2002, 1)
    pairs = np.full((1100, 24), CANARY, np.uint32)
    assert L.prk_records_rows(ctx, big.handle, 0, 1, 64, o.rows.ctypes.data, 8, pairs.ctypes.data, 1100,
                              o.rc.ctypes.data, p64(o.nrow), p64(o.npair)) == abi.PRK_ERR_UNSUPPORTED
    assert (o.rows == CANARY).all() and (pairs == CANARY).all() and o.rc[0] == 77
    assert (o.nrow[0], o.npair[0]) == (99, 99)
    for x in (rec, ok, empty, big):
        x.close()


# ---- 6. no side effects ----------------------------------------------------------------------------------------------
def test_no_side_effects(fr):
    r = fr.r
    words, counts = fr.words, fr.counts
    rec = r.records_upload(words, counts)
    r.reset_draws()
    r.clear()
    r.draw_records(rec, semantics=AVX[0], bitmap=fr.tex, phong=True)
    want = fr.done()
    assert (want[0] != scenes.CLEAR_COLOR).any()
    r.clear()
    r.draw_records(rec, semantics=AVX[0], bitmap=fr.tex, phong=True)  # recorded, not flushed
    before = r.stats()
    gw, gn = rec.advance(96)
    adv = rec.advance(96, 2, 9, keep=True, host=False)
    gs, gc = rec.spans(96)
    gr, gp, grc = rec.rows(96)
    rec.list_stats(96)
    assert r.stats() == before
    assert (gw != words).any() and gs.shape[0] > 0 and gr.shape[0] > 0
    assert np.array_equal(rec.download(), words)
    same_frame(fr.done(), want, "the frame recorded before the walks")
    adv.close()
    rec.close()
