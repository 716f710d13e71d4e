"""The checker of prk_row_records: a Python restatement of the row loop of
DrawModelOptimizedLines (projekt.cpp:3398-3611) over packed prk_edge words,
which returns the buffer_line_render_work records that walk queues -- one a
row, RowIndex and EdgeCount, and its thread_edge_info pairs in their
interleaved layout (projekt.h:39-88).

The walk is written out here in its own right, not taken from spanref: the
whole-list insertion scan of every row (3406-3465: no cursor, no sorted-list
shortcut), the head expiry (3467-3472) with the project's pin (an emptied list
skips the row: the reference dereferences NULL there, so no record is queued),
the removal (3474-3501), the pairing with both swaps and P3 (3518-3602), and a
row record at the end of every row that is not skipped (3604-3609), paired or
not.  Only the stepped values are shared: an edge's fields depend on how
often it was stepped alone, and spanref._states holds state k of every edge.
tests/test_row_records_api.py holds the result to spanref's spans.
"""
import numpy as np

from spanref import GRAD, LEFT, YMAX, YMIN, _states

# thread_edge_info word w as (end, word of the end's twelve): an end is XMin
# ZMin OneOverZMin UMin VMin MinColor[4] MinNormal[3] (spanref.END_WORDS)
PAIR_WORDS = ([(h, k) for k in range(5) for h in (0, 1)] + [(0, k) for k in range(5, 9)] +
              [(1, k) for k in range(5, 9)] + [(0, k) for k in range(9, 12)] + [(1, k) for k in range(9, 12)])
assert len(PAIR_WORDS) == 24
MAX_ROW_PAIRS = 1000  # ThreadEdges[1000] (3403)


def _rows_of_list(X, G, L, ymin, ymax, height):
    """One list: X[e][k] is XMin of edge e after k steps.  Returns the queue
    [(row, [(cur, cur's steps, next, next's steps), ...])]."""
    n = len(G)
    if n == 0:
        return []
    steps = [0] * n
    nxt = [-1] * n  # FillEdgeTable leaves every Next NULL (4094)
    queue = []

    def x(e):
        return X[e][steps[e]]

    def before(a, b):  # 3417-3421 / 3434-3438
        return x(a) < x(b) or (x(a) == x(b) and (G[a] < G[b] or (G[a] == G[b] and L[a] < L[b])))

    first_row = ymin[0]  # 3373-3396
    max_row = ymax[0]
    for e in range(1, n):
        if max_row < ymax[e]:
            max_row = ymax[e]
    max_y = first_row + (max_row - first_row)
    if max_y > height:
        max_y = height
    head = tail = -1
    for row in range(first_row, max_y):
        thread_edges = []
        for cur in range(n):  # 3406-3465
            if ymin[cur] != row:
                continue
            if head < 0:
                head = tail = cur
            elif before(cur, head):
                nxt[cur] = head
                head = cur
            else:
                compared = previous = head
                while compared != tail:
                    compared = nxt[compared]
                    if before(cur, compared):
                        nxt[cur] = compared
                        nxt[previous] = cur
                        compared = tail
                    else:
                        previous = compared
                if previous == compared:
                    nxt[tail] = cur
                    tail = cur
        while head >= 0 and ymax[head] <= row:  # 3467-3472
            removed = head
            head = nxt[head]
            nxt[removed] = -1
        if head < 0:  # the pin: the row is skipped, nothing is queued
            tail = -1
            continue
        previous = checked = head  # 3474-3501
        while checked != tail:
            checked = nxt[checked]
            if ymax[checked] <= row:
                if checked == tail:
                    tail = previous
                    nxt[tail] = -1
                    checked = tail
                else:
                    nxt[previous] = nxt[checked]
                    checked = previous
            previous = checked
        prev_cur = prev_next = -1  # 3503-3602
        cur, nx = head, nxt[head]
        while nx >= 0:
            thread_edges.append((cur, steps[cur], nx, steps[nx]))  # 3521-3544: before the step
            steps[cur] += 1  # 3546-3564
            steps[nx] += 1
            if x(cur) > x(nx):  # 3566-3576
                nxt[cur] = nxt[nx]
                nxt[nx] = cur
                if prev_next >= 0:
                    nxt[prev_next] = nx
                else:
                    head = nx  # P3
                if tail == nx:
                    tail = cur  # P3
                cur = nx
                nx = nxt[cur]
            if prev_next >= 0 and x(prev_next) > x(cur):  # 3578-3588
                nxt[prev_next] = nxt[cur]
                nxt[cur] = prev_next
                nxt[prev_cur] = cur
                prev_next = cur
                cur = nxt[prev_next]
            prev_cur, prev_next = cur, nx
            if nxt[nx] >= 0:
                cur = nxt[nx]
                nx = nxt[cur]
            else:
                nx = -1
        queue.append((row, thread_edges))  # 3604-3609
    return queue


def walk_batch(words, counts, height):
    """Every list of a packed batch: (rows int32 [k, 2]: RowIndex, EdgeCount;
    pairs uint32 [m, 24] in prk_row_pair layout, queue order; row_counts
    uint32 [nlist]).  A row of more than MAX_ROW_PAIRS pairs raises
    OverflowError: the reference writes past ThreadEdges there."""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
    counts = np.asarray(counts, np.int64).reshape(-1)
    assert int(counts.sum()) == words.shape[0]
    T = _states(words, height)
    X = T[:, :, 0].T.tolist()
    f, i = words.view(np.float32), words.view(np.int32)
    G, L = f[:, GRAD].tolist(), i[:, LEFT].tolist()
    ymin, ymax = i[:, YMIN].tolist(), i[:, YMAX].tolist()
    rows, ends, row_counts = [], [], []
    e0 = 0
    for n in counts.tolist():
        e1 = e0 + n
        q = _rows_of_list(X[e0:e1], G[e0:e1], L[e0:e1], ymin[e0:e1], ymax[e0:e1], height)
        for row, te in q:
            if len(te) > MAX_ROW_PAIRS:
                raise OverflowError("row %d holds %d pairs" % (row, len(te)))
            rows.append((row, len(te)))
            ends += [(a + e0, ka, b + e0, kb) for a, ka, b, kb in te]
        row_counts.append(len(q))
        e0 = e1
    q = np.array(ends, np.int64).reshape(-1, 4)
    both = np.empty((q.shape[0], 2, 12), np.uint32)
    both[:, 0] = T[q[:, 1], q[:, 0]].view(np.uint32)
    both[:, 1] = T[q[:, 3], q[:, 2]].view(np.uint32)
    pairs = np.empty((q.shape[0], 24), np.uint32)
    for w, (h, k) in enumerate(PAIR_WORDS):
        pairs[:, w] = both[:, h, k]
    return np.array(rows, np.int32).reshape(-1, 2), pairs, np.array(row_counts, np.uint32)


def as_spans(rows, pairs):
    """The pairs regrouped as prk_span words [m, 25]: what DoBufferLineRenderWork
    hands FillLinesOptimized, de-interleaved, each on its row's RowIndex."""
    rows = np.asarray(rows, np.int32).reshape(-1, 2)
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 24)
    assert int(rows[:, 1].astype(np.int64).sum()) == pairs.shape[0]
    spans = np.empty((pairs.shape[0], 25), np.uint32)
    for w, (h, k) in enumerate(PAIR_WORDS):
        spans[:, 12 * h + k] = pairs[:, w]
    spans[:, 24] = np.repeat(rows[:, 0], rows[:, 1]).view(np.uint32)
    return spans
