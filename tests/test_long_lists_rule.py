"""CPU test: the rule by which the workgroup walk of the record calls
(k_adv_walk_wg, prk_records.hip) gives every record its final Next.

That walk keeps a list as an ordered array, not as links, so an edge's Next --
which the reference leaves in the caller's edge_info memory -- has to be read
off the array.  The rule, modelled here exactly as the kernel
applies it:

* on a row, after that row's insertions, take the list as it stands before
  the removal: an expiring entry with no staying entry before it (the leading
  run of expiring entries, the head expiry 3715-3720) gets -1; any other
  expiring entry keeps the index of its successor in that list, whether the
  successor expires too or not (3722-3749 never writes the removed edge's own
  pointer); the last entry has -1;
* after the last walked row every entry still listed gets its successor's
  index, the last -1;
* edges never inserted keep -1.

The model is held to oracle.advance_edges -- Next and the stepped X -- on a
few hundred seeded random sorted lists: at most 40 edges and 30 rows,
quarter-integer X and Gradient (float32 steps are exact), with X / Gradient /
Left ties, zero-row edges, gaps, odd lists, edges that start on the row others
expire on, and heights that cut the walk.
"""
import numpy as np

import oracle as O

YMAX, XMIN, GRAD, YMIN, LEFT = 0, 1, 4, 7, 12  # prk_edge words


def edge(ymin, ymax, x, g, left):
    f = np.zeros(27, np.float32)
    f[XMIN], f[GRAD] = x, g
    f[2], f[3] = 1.0, 0.25
    f[13:17] = 0.5
    f[21:24] = (0.0, 0.6, 0.8)
    w = f.view(np.uint32).copy()
    w[YMAX], w[YMIN], w[LEFT] = ymax, ymin, left
    return w


def model(words, height):
    """(Next, X) of the list after the array walk."""
    n = words.shape[0]
    wi = words.view(np.int32)
    ymin, ymax, left = wi[:, YMIN], wi[:, YMAX], wi[:, LEFT]
    x = words[:, XMIN].view(np.float32).copy()
    g = words[:, GRAD].view(np.float32)
    nxt = np.full(n, -1, np.int32)
    max_y = min(int(ymax.max()), height)

    def before(a, b):  # 3663-3667
        return x[a] < x[b] or (x[a] == x[b] and (g[a] < g[b] or (g[a] == g[b] and left[a] < left[b])))

    lst, ins, row = [], 0, int(ymin[0])
    while row < max_y:
        while ins < n and ymin[ins] == row:  # insertion: before the first entry it sorts before, else the tail
            p = next((q for q, e in enumerate(lst) if before(ins, e)), len(lst))
            lst.insert(p, ins)
            ins += 1
        kept = []
        for q, e in enumerate(lst):  # expiry, on the list before the removal
            if ymax[e] <= row:
                nxt[e] = -1 if (not kept or q + 1 == len(lst)) else lst[q + 1]
            else:
                kept.append(e)
        lst = kept
        if not lst:  # the rows before the next insertion are skipped
            row = max(row + 1, int(ymin[ins])) if ins < n else max_y
            continue
        pairs = len(lst) // 2
        for e in lst[:2 * pairs]:  # the unpaired odd entry is not stepped
            x[e] = np.float32(x[e] + g[e])
        a = [lst[2 * k] for k in range(pairs)]
        b = [lst[2 * k + 1] for k in range(pairs)]
        for k in range(pairs):  # 3831-3841
            if x[a[k]] > x[b[k]]:
                a[k], b[k] = b[k], a[k]
        na, nb = list(a), list(b)
        for k in range(1, pairs):  # 3843-3853: pair k's first entry against pair k - 1's second
            if x[b[k - 1]] > x[a[k]]:
                na[k], nb[k - 1] = b[k - 1], a[k]
        lst = [e for k in range(pairs) for e in (na[k], nb[k])] + lst[2 * pairs:]
        row += 1
    for q, e in enumerate(lst):
        nxt[e] = lst[q + 1] if q + 1 < len(lst) else -1
    return nxt, x


def random_list(rng):
    n = int(rng.integers(1, 41))
    rows = int(rng.integers(2, 31))
    y0 = np.sort(rng.integers(0, rows, n))
    if rng.random() < 0.5:  # a gap: the list runs empty, then takes new edges
        cut = int(rng.integers(0, rows))
        y0 = np.where(y0 >= cut, y0 + 6, y0)
    span = rng.integers(0, 9, n)  # 0: a zero-row edge
    if rng.random() < 0.5:  # edges that start on the row others expire on
        ends = y0 + span
        pick = rng.random(n) < 0.4
        starts = rng.choice(ends, n)
        y0 = np.sort(np.where(pick, starts, y0))
    xs = rng.integers(0, 24, n) / 4.0 if rng.random() < 0.5 else rng.integers(0, 200, n) / 4.0
    gs = rng.integers(-8, 9, n) / 4.0
    if rng.random() < 0.3:
        gs[:] = 0.0  # X ties stay ties: Left orders them
    lf = rng.integers(0, 2, n)
    words = np.array([edge(int(y0[i]), int(y0[i] + span[i]), float(xs[i]), float(gs[i]), int(lf[i]))
                      for i in range(n)], np.uint32)
    top = int((y0 + span).max())
    height = [top + 5, top, max(0, top - int(rng.integers(1, 6))), int(y0[0]), 0][int(rng.integers(0, 5))]
    return words, height


def test_array_rule_gives_the_reference_next():
    rng = np.random.default_rng(20261020)
    seen = dict(ties=0, zero=0, gap=0, odd=0, trap=0, cut=0, linked=0)
    for _ in range(400):
        words, height = random_list(rng)
        ow, on = O.advance_edges(words, height)
        ox = ow[:, XMIN].view(np.float32)
        mn, mx = model(words, height)
        assert np.array_equal(mn, on), (words.view(np.int32)[:, [YMIN, YMAX, LEFT]].tolist(), height,
                                        mn.tolist(), on.tolist())
        assert np.array_equal(mx, ox)
        wi = words.view(np.int32)
        key = [(int(a), int(b), int(c)) for a, b, c in zip(words[:, XMIN], words[:, GRAD], wi[:, YMIN])]
        seen["ties"] += len(set(key)) < len(key)
        seen["zero"] += bool((wi[:, YMIN] == wi[:, YMAX]).any())
        seen["gap"] += bool((np.diff(wi[:, YMIN]) > 5).any())
        seen["odd"] += words.shape[0] % 2
        seen["trap"] += bool(np.isin(wi[:, YMIN], wi[:, YMAX]).any())
        seen["cut"] += height < int(wi[:, YMAX].max())
        seen["linked"] += bool((on >= 0).any())
    assert all(v >= 20 for v in seen.values()), seen


def test_hand_cases():
    # the expired second edge keeps the link to the edge inserted after it
    trap = np.array([edge(0, 10, 0.0, 0.0, 1), edge(0, 10, 20.0, 0.0, 0), edge(10, 20, 5.0, 0.0, 1),
                     edge(10, 20, 25.0, 0.0, 0)], np.uint32)
    assert model(trap, 40)[0].tolist() == [-1, 3, 3, -1] == O.advance_edges(trap, 40)[1].tolist()
    # all expire at once (a later edge keeps the walk going): every entry is in the leading run
    both = np.array([edge(0, 3, 0.0, 0.0, 1), edge(0, 3, 4.0, 0.0, 0)], np.uint32)
    later = np.concatenate([both, edge(5, 9, 1.0, 0.0, 1)[None]])
    assert model(later, 40)[0].tolist() == [-1, -1, -1] == O.advance_edges(later, 40)[1].tolist()
    # the walk ends before row max YMax, and before `height`: the survivors stay linked
    assert model(both, 40)[0].tolist() == [1, -1] == O.advance_edges(both, 40)[1].tolist()
    assert model(both, 2)[0].tolist() == [1, -1] == O.advance_edges(both, 2)[1].tolist()
    # never walked
    assert model(both, 0)[0].tolist() == [-1, -1] == O.advance_edges(both, 0)[1].tolist()
