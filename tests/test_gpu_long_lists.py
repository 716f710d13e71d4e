"""GPU tests: the workgroup walk of long lists in prk_advance_edge_lists,
prk_span_records and prk_row_records (k_adv_walk_wg / k_span_walk_wg /
k_row_walk_wg: one workgroup a list, the list an ordered array of LDS slots).

PRK_ADV_WG_MIN_STEPS=0 sends every list that fits a slot class through that
walk, so the hand-made lists, the soup and the sphere of the three calls' own
test modules are checked again, by those modules' checkers: the host call
prk_advance_edge_records and the oracle (records, Next), spanref (spans) and
rowref (rows, pairs).  Every case reads prk_debug_list_routes (list_routes)
to make sure the lists it means to test took a slot class.
"""
import numpy as np
import pytest

import prk
import test_gpu_advance_lists as A
import test_gpu_row_records as RW
import test_gpu_span_records as SP
from prk import abi

pytestmark = pytest.mark.gpu

edge = A.edge
CANARY = 0xA5A5A5A5
END_WORDS = [1, 2, 3, 8, 9, 13, 14, 15, 16, 21, 22, 23]  # prk_edge words of a prk_span end


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("PRK_ADV_WG_MIN_STEPS", "0")


@pytest.fixture(scope="module")
def rdr(gpu):
    r = prk.Renderer()
    yield r
    r.close()


@pytest.fixture(scope="module")
def soup(gpu):
    c = A.Ctx(A._soup())
    yield c
    c.close()


@pytest.fixture(scope="module")
def sphere(gpu):
    c = A.Ctx(SP._sphere_scene())
    yield c
    c.close()


def all_routed(r, counts, label, slots=None):
    """Every list with an edge took a slot class (`slots`: these counts)."""
    lr = r.list_routes()
    assert lr["thread"] == int((counts == 0).sum()), (label, lr)
    assert sum(lr["slots"]) == int((counts > 0).sum()), (label, lr)
    if slots is not None:
        assert lr["slots"] == tuple(slots), (label, lr)
    return lr


def count_spans(r, words, counts, height):
    sc = np.full(counts.shape[0], 99, np.uint32)
    total = np.full(1, 99, np.uint64)
    assert SP._raw(r, words, counts, height, None, 0, sc, total) == abi.PRK_OK
    return sc, int(total[0])


def count_rows(r, words, counts, height):
    rc = np.full(counts.shape[0], 99, np.uint32)
    nrow, npair = np.full(1, 99, np.uint64), np.full(1, 99, np.uint64)
    assert RW._raw(r, words, counts, height, None, 0, None, 0, rc, nrow, npair) == abi.PRK_OK
    return rc, int(nrow[0]), int(npair[0])


def three_calls(r, words, counts, height, label, slots=None, oracle=True, exact=False):
    """The batch through all three calls, each against its module's checker;
    the counting variants against the filling ones; the routes of each."""
    gw, gn = A.check(r, words, counts, height, label, oracle=oracle)
    all_routed(r, counts, label + " advance", slots)
    gs, gc, _ = SP.check(r, words, counts, height, label)
    all_routed(r, counts, label + " spans", slots)
    sc, total = count_spans(r, words, counts, height)
    all_routed(r, counts, label + " span counts", slots)
    assert np.array_equal(sc, gc) and total == gs.shape[0], label
    gr, gp, grc, _ = RW.check(r, words, counts, height, label, exact=exact)
    all_routed(r, counts, label + " rows", slots)
    rc, nrow, npair = count_rows(r, words, counts, height)
    all_routed(r, counts, label + " row counts", slots)
    assert np.array_equal(rc, grc) and nrow == gr.shape[0] and npair == gp.shape[0], label
    return gw, gn


def test_hand_made_lists(rdr, forced):
    words, counts, off = A.hand_batch()
    n = int((counts > 0).sum())
    gw, gn = three_calls(rdr, words, counts, A.HAND_HEIGHT, "advance's hand lists", slots=(n, 0, 0, 0, 0), exact=True)
    o = off["segment trap"]
    assert gn[o:o + 4].tolist() == [-1, 3, 3, -1]  # the expired second edge keeps its link
    o = off["gap"]
    assert gn[o:o + 4].tolist() == [-1, -1, -1, 2]
    o = off["one edge"]
    assert np.array_equal(gw[o], words[o]) and gn[o] == -1
    for mod, name in ((SP, "spans' hand lists"), (RW, "rows' hand lists")):
        w, c = mod.hand_batch()
        three_calls(rdr, w, c, mod.HAND_HEIGHT, name, slots=(int((c > 0).sum()), 0, 0, 0, 0), exact=True)
        three_calls(rdr, w, c, 0, name + " height 0", exact=True)


@pytest.mark.parametrize("height", [192, 0])
@pytest.mark.parametrize("per", [5, 60])
def test_soup_batches(soup, forced, per, height):
    words, counts = soup.records(3, per, lights=1)
    assert (counts > 62).any() or per == 5  # 60 triangles a list: past the first class
    gw, gn = three_calls(soup.r, words, counts, height, "soup per %d height %d" % (per, height))
    if height:
        assert (gw != words).any() and (gn >= 0).any()
    else:
        assert np.array_equal(gw, words) and (gn == -1).all()


def test_soup_without_normals(soup, forced):
    """A non-Phong setup: zero normals normalise to NaN on the first step (the
    NaN allowance of the checkers), and NaN-free keys all the same."""
    words, counts = soup.records(0, 5, lights=0)
    gw, _ = three_calls(soup.r, words, counts, 192, "soup setup 0", oracle=False)
    assert A.is_nan(gw[:, 21:24]).any()


@pytest.mark.parametrize("height", [256, 128])
def test_sphere_one_list(sphere, forced, height):
    words, counts = sphere.records(3, 2208)
    assert counts.tolist() == [2072]
    three_calls(sphere.r, words, counts, height, "sphere height %d" % height)
    assert sum(sphere.r.list_routes()["slots"][:2]) == 0  # more than 126 edges listed at once


def crowd(n, ymin=0, ymax=3, k0=0):
    """n edges starting on one row in scrambled X order, gradients that cross
    neighbours on the rows after."""
    order = [(i * 37 + 11) % n for i in range(n)] if n % 37 else list(range(n))[::-1]
    return [edge(ymin, ymax, 4.0 * order[i], (1.5 if order[i] % 3 == 0 else -0.75), i & 1, (i + k0) & 3)
            for i in range(n)]


WINDOW_CASES = [
    # more new edges on one row than a wave, a batch insert of far more than two
    ("70 on one row", crowd(70), (0, 1, 0, 0, 0)),
    ("62 listed", crowd(62), (1, 0, 0, 0, 0)),
    ("63 listed", crowd(63), (0, 1, 0, 0, 0)),
    # the second row's edges cross the 128-thread read-ahead window of the 126 class
    ("window crossing", crowd(100, 0, 1) + crowd(60, 2, 5, 1), (0, 1, 0, 0, 0)),
    # later edges start on the row the first ones expire on: 40 + 30 listed at once
    ("insert among expiring", crowd(40, 0, 2) + crowd(30, 2, 4, 2), (0, 1, 0, 0, 0)),
    ("1022 listed", crowd(1022, 1, 3), (0, 0, 0, 0, 1)),
]


@pytest.mark.parametrize("name", [c[0] for c in WINDOW_CASES])
def test_window_and_class_edges(rdr, forced, name):
    _, edges, slots = next(c for c in WINDOW_CASES if c[0] == name)
    words = np.array(edges, np.uint32)
    three_calls(rdr, words, np.array([words.shape[0]], np.uint32), 64, name, slots=slots, exact=True)


def test_1023_listed_stays_on_the_thread_walk(rdr, forced):
    words = np.array(crowd(1023, 1, 3), np.uint32)
    counts = np.array([1023], np.uint32)
    A.check(rdr, words, counts, 64, "1023 listed", oracle=True)
    assert rdr.list_routes() == dict(thread=1, slots=(0, 0, 0, 0, 0))
    SP.check(rdr, words, counts, 64, "1023 listed")
    assert rdr.list_routes() == dict(thread=1, slots=(0, 0, 0, 0, 0))
    RW.check(rdr, words, counts, 64, "1023 listed", exact=True)
    assert rdr.list_routes() == dict(thread=1, slots=(0, 0, 0, 0, 0))


def five_groups():
    """Five groups of 1000 edges, group g on row 2 g alone: 5000 edge-rows,
    but about 2.5 M insertion-scan steps for a thread."""
    return np.array([edge(2 * g, 2 * g + 1, float(i), 0.0, (i + 1) & 1, i & 3) for g in range(5) for i in range(1000)],
                    np.uint32)


def five_groups_expect(words):
    """Each edge is listed on one row only: 500 pairs a row, each pair two
    input records as they came, in list order (X ascending == input order)."""
    spans = np.zeros((2500, 25), np.uint32)
    spans[:, 0:12] = words[0::2][:, END_WORDS]
    spans[:, 12:24] = words[1::2][:, END_WORDS]
    spans[:, 24] = np.repeat(2 * np.arange(5), 500)
    rows = np.array([[2 * g, 500] for g in range(5)], np.int32)
    pairs = np.zeros((2500, 24), np.uint32)
    L, R = spans[:, 0:12], spans[:, 12:24]
    pairs[:, 0:10:2], pairs[:, 1:10:2] = L[:, 0:5], R[:, 0:5]
    pairs[:, 10:14], pairs[:, 14:18] = L[:, 5:9], R[:, 5:9]
    pairs[:, 18:21], pairs[:, 21:24] = L[:, 9:12], R[:, 9:12]
    return spans, rows, pairs


def check_five_groups(r, words, counts, o, gw, gn, gs, gc, gr, gp, grc):
    """List o of the batch is five_groups(): its part of every output."""
    e0 = int(counts[:o].sum())
    hw, hn = A.host_advance(words[e0:e0 + 5000], np.array([5000], np.uint32), 64)
    A.same_words(gw[e0:e0 + 5000], hw, "five groups vs host")
    assert np.array_equal(gn[e0:e0 + 5000], hn)
    assert (hn[:4000] == -1).all() and hn[4000:].tolist() == list(range(4001, 5000)) + [-1]
    spans, rows, pairs = five_groups_expect(words[e0:e0 + 5000])
    s0 = int(gc[:o].sum())
    assert gc[o] == 2500 and np.array_equal(gs[s0:s0 + 2500], spans)
    r0 = int(grc[:o].sum())
    assert grc[o] == 5 and np.array_equal(gr[r0:r0 + 5], rows)
    p0 = int(gr[:r0, 1].sum())
    assert np.array_equal(gp[p0:p0 + 2500], pairs)


def test_long_list_over_the_thread_cap(rdr):
    """Default routing.  Without the workgroup walk all three calls refuse
    this list (PRK_ERR_LIMIT: the insertion scans pass the one-thread cap)."""
    words = five_groups()
    counts = np.array([5000], np.uint32)
    want = dict(thread=0, slots=(0, 0, 0, 0, 1))
    gw, gn = rdr.advance_edge_lists(words, counts, 64)
    assert rdr.list_routes() == want
    gs, gc = rdr.span_records(words, counts, 64)
    assert rdr.list_routes() == want
    gr, gp, grc = rdr.row_records(words, counts, 64)
    assert rdr.list_routes() == want
    check_five_groups(rdr, words, counts, 0, gw, gn, gs, gc, gr, gp, grc)
    assert count_spans(rdr, words, counts, 64)[1] == 2500
    assert count_rows(rdr, words, counts, 64)[1:] == (5, 2500)


def test_mixed_batch(rdr):
    """Default routing: short lists around one long list; both routes in one
    batch, the packed outputs, counts and scans right across the boundary."""
    hw, hc, _ = A.hand_batch()
    sw, sc = SP.hand_batch()
    words = np.concatenate([hw, five_groups(), sw])
    counts = np.concatenate([hc, [5000], sc]).astype(np.uint32)
    o = hc.shape[0]
    want = dict(thread=counts.shape[0] - 1, slots=(0, 0, 0, 0, 1))
    gw, gn = rdr.advance_edge_lists(words, counts, A.HAND_HEIGHT)
    assert rdr.list_routes() == want
    gs, gc = rdr.span_records(words, counts, A.HAND_HEIGHT)
    assert rdr.list_routes() == want
    gr, gp, grc = rdr.row_records(words, counts, A.HAND_HEIGHT)
    assert rdr.list_routes() == want
    check_five_groups(rdr, words, counts, o, gw, gn, gs, gc, gr, gp, grc)
    # the short lists on either side: as the same batch without the long list
    short_w = np.concatenate([hw, sw])
    short_c = np.concatenate([hc, sc]).astype(np.uint32)
    e1 = hw.shape[0]
    xw, xn = A.host_advance(short_w, short_c, A.HAND_HEIGHT)
    assert np.array_equal(np.concatenate([gw[:e1], gw[e1 + 5000:]]), xw)
    assert np.array_equal(np.concatenate([gn[:e1], gn[e1 + 5000:]]), xn)
    ws, wc, _, _ = SP.spanref.walk_batch(short_w, short_c, A.HAND_HEIGHT)
    assert np.array_equal(np.concatenate([gc[:o], gc[o + 1:]]), wc)
    s0 = int(gc[:o].sum())
    assert np.array_equal(np.concatenate([gs[:s0], gs[s0 + 2500:]]), ws)
    wr, wp, wrc = RW.rowref.walk_batch(short_w, short_c, A.HAND_HEIGHT)
    assert np.array_equal(np.concatenate([grc[:o], grc[o + 1:]]), wrc)
    r0 = int(grc[:o].sum())
    assert np.array_equal(np.concatenate([gr[:r0], gr[r0 + 5:]]), wr)
    p0 = int(gr[:r0, 1].sum())
    assert np.array_equal(np.concatenate([gp[:p0], gp[p0 + 2500:]]), wp)


def test_refusals_unchanged(rdr, forced):
    """The caps the workgroup walk does not lift, with every list that fits
    sent to it; every refusal leaves the outputs as they were."""
    long_list = np.array([edge(0, 65536, float(i), 0.0, i & 1) for i in range(257)], np.uint32)
    one_row = np.array([edge(0, 1, float(i), 0.0, i & 1) for i in range(2100)], np.uint32)
    r = rdr
    for label, w, height in (("257 x 65536", long_list, 65536), ("2100 on one row", one_row, 64)):
        cnt = np.array([w.shape[0]], np.uint32)
        out, nxt = np.full_like(w, CANARY), np.full(w.shape[0], 77, np.int32)
        assert A._raw(r, w, cnt, height, out, nxt) == abi.PRK_ERR_LIMIT, label
        assert (out == CANARY).all() and (nxt == 77).all(), label
        spans = np.full((16, 25), CANARY, np.uint32)
        sc, total = np.full(1, 77, np.uint32), np.full(1, 99, np.uint64)
        assert SP._raw(r, w, cnt, height, spans, 16, sc, total) == abi.PRK_ERR_LIMIT, label
        assert (spans == CANARY).all() and sc[0] == 77 and total[0] == 0, label  # (total_out: 0 on every refusal)
        rows, pairs = np.full((8, 2), CANARY, np.uint32), np.full((16, 24), CANARY, np.uint32)
        rc, nrow, npair = np.full(1, 77, np.uint32), np.full(1, 99, np.uint64), np.full(1, 98, np.uint64)
        assert RW._raw(r, w, cnt, height, rows, 8, pairs, 16, rc, nrow, npair) == abi.PRK_ERR_LIMIT, label
        assert (rows == CANARY).all() and (pairs == CANARY).all() and rc[0] == 77, label
    w, cnt = RW._crowd(2002), np.array([2002], np.uint32)
    rows, pairs = np.full((8, 2), CANARY, np.uint32), np.full((1100, 24), CANARY, np.uint32)
    rc, nrow, npair = np.full(1, 77, np.uint32), np.full(1, 99, np.uint64), np.full(1, 98, np.uint64)
    assert RW._raw(r, w, cnt, 64, rows, 8, pairs, 1100, rc, nrow, npair) == abi.PRK_ERR_UNSUPPORTED
    assert (rows == CANARY).all() and (pairs == CANARY).all()
    assert rc[0] == 77 and nrow[0] == 99 and npair[0] == 98
