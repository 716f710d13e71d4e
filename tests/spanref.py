"""The checker of prk_span_records: a Python restatement of the reference's
list walk (projekt.cpp:3654-3869) over packed prk_edge words, which returns
the work records DrawModelOptimized(RenderQueue) queues (3756-3809) beside
the list the walk leaves.  tests/test_span_records_api.py holds its advanced
words and links to the oracle's own walk (oracle.advance_edges) and its spans
to the oracle's frames.

The walk is the reference's, with the oracle's pins (P3: the first pair's swap
moves the head and the tail; an emptied list skips the row): the whole-list
insertion scan of every row (no cursor, no sorted-list shortcut), the head
expiry, the 3722-3749 removal, the pairing with both swaps.  The arithmetic is
numpy float32.  An edge's fields depend only on how often it was stepped, so
the steps (3811-3829, Normalize through pyref.norm_rcp) are taken for all
edges of a batch at once -- state k of every edge, k up to the most rows an
edge can be listed on -- and the walk, in plain Python, counts each edge's
steps and reads XMin from its state.
"""
import numpy as np

from pyref import norm_rcp

YMAX, XMIN, ZMIN, WMIN, GRAD, ZGRAD, WGRAD, YMIN, UMIN, VMIN, UGRAD, VGRAD, LEFT = range(13)
COLOR, CGRAD, NORMAL, NGRAD = slice(13, 17), slice(17, 21), slice(21, 24), slice(24, 27)
# prk_span_end's twelve words as prk_edge words
END_WORDS = [XMIN, ZMIN, WMIN, UMIN, VMIN, 13, 14, 15, 16, 21, 22, 23]


def _states(words, height):
    """T[k, e]: the twelve span-end words of edge e after k steps (float32)."""
    f = words.view(np.float32)
    i = words.view(np.int32)
    rows = np.maximum(0, np.minimum(i[:, YMAX], height) - i[:, YMIN])
    K = int(rows.max()) if rows.size else 0
    T = np.empty((K + 1, words.shape[0], 12), np.float32)
    cur = f[:, END_WORDS].copy()
    T[0] = cur
    g = f[:, [GRAD, ZGRAD, WGRAD, UGRAD, VGRAD]].copy()
    cg, ng = f[:, CGRAD].copy(), f[:, NGRAD].copy()
    with np.errstate(all="ignore"):
        for k in range(1, K + 1):
            nxt = np.empty_like(cur)
            nxt[:, 0] = cur[:, 0] + g[:, 0]   # XMin += Gradient
            nxt[:, 1] = cur[:, 1] + g[:, 1]   # ZMin += ZGradient
            nxt[:, 5:9] = cur[:, 5:9] + cg    # MinColor += ColorGradient
            v = cur[:, 9:12] + ng             # MinNormal = Normalize(MinNormal + NormalGradient)
            n = norm_rcp([v[:, 0], v[:, 1], v[:, 2]])
            nxt[:, 9], nxt[:, 10], nxt[:, 11] = n[0], n[1], n[2]
            nxt[:, 3] = cur[:, 3] + g[:, 3]   # UMin, VMin, OneOverZMin
            nxt[:, 4] = cur[:, 4] + g[:, 4]
            nxt[:, 2] = cur[:, 2] + g[:, 2]
            T[k] = cur = nxt
    return T


def _walk_list(X, G, L, ymin, ymax, height):
    """One list: X[e][k] is XMin of edge e after k steps.  Returns the queue
    [(cur, cur's steps, next, next's steps, row)], the steps and the links."""
    n = len(G)
    steps, nxt = [0] * n, [-1] * n
    queue = []
    if n == 0:
        return queue, steps, nxt

    def before(a, b):
        ax, bx = X[a][steps[a]], X[b][steps[b]]
        return ax < bx or (ax == bx and (G[a] < G[b] or (G[a] == G[b] and L[a] < L[b])))

    ym = np.asarray(ymin)
    head = tail = -1
    for row in range(ymin[0], min(max(ymax), height)):
        for c in np.nonzero(ym == row)[0].tolist():  # 3654-3713, the whole list in index order
            if head >= 0:
                if before(c, head):
                    nxt[c] = head
                    head = c
                else:
                    cmp_, prev = head, head
                    while cmp_ != tail:
                        cmp_ = nxt[cmp_]
                        if before(c, cmp_):
                            nxt[c] = cmp_
                            nxt[prev] = c
                            cmp_ = tail
                        else:
                            prev = cmp_
                    if prev == cmp_:
                        nxt[tail] = c
                        tail = c
            else:
                head = tail = c
        while head >= 0 and ymax[head] <= row:  # 3715-3720
            rm = head
            head = nxt[head]
            nxt[rm] = -1
        if head < 0:  # pin: the reference dereferences NULL
            tail = -1
            continue
        prev = chk = head  # 3722-3749
        while chk != tail:
            chk = nxt[chk]
            if ymax[chk] <= row:
                if chk == tail:
                    tail = prev
                    nxt[tail] = -1
                    chk = tail
                else:
                    nxt[prev] = nxt[chk]
                    chk = prev
            prev = chk
        pcur = pnext = -1  # 3751-3869
        cur, nx = head, nxt[head]
        while nx >= 0:
            queue.append((cur, steps[cur], nx, steps[nx], row))  # 3756-3809
            steps[cur] += 1  # 3811-3829
            steps[nx] += 1
            if X[cur][steps[cur]] > X[nx][steps[nx]]:  # 3831-3841
                nxt[cur] = nxt[nx]
                nxt[nx] = cur
                if pnext >= 0:
                    nxt[pnext] = nx
                else:
                    head = nx  # P3
                if tail == nx:
                    tail = cur  # P3
                cur = nx
                nx = nxt[cur]
            if pnext >= 0 and X[pnext][steps[pnext]] > X[cur][steps[cur]]:  # 3843-3853
                nxt[pnext] = nxt[cur]
                nxt[cur] = pnext
                nxt[pcur] = cur
                pnext = cur
                cur = nxt[pnext]
            pcur, pnext = cur, nx
            if nxt[nx] >= 0:
                cur = nxt[nx]
                nx = nxt[cur]
            else:
                nx = -1
    return queue, steps, nxt


def walk_batch(words, counts, height):
    """Every list of a packed batch: (span_words uint32 [k, 25], span_counts
    uint32 [nlist], advanced_words uint32 [n, 27], next int32 [n], an index
    within the record's own list or -1)."""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
    counts = np.asarray(counts, np.int64).reshape(-1)
    assert int(counts.sum()) == words.shape[0]
    T = _states(words, height)
    X = T[:, :, 0].T.tolist()
    f, i = words.view(np.float32), words.view(np.int32)
    G, L = f[:, GRAD].tolist(), i[:, LEFT].tolist()
    ymin, ymax = i[:, YMIN].tolist(), i[:, YMAX].tolist()
    queue, steps, links, span_counts = [], [], [], []
    e0 = 0
    for n in counts.tolist():
        e1 = e0 + n
        q, s, l = _walk_list(X[e0:e1], G[e0:e1], L[e0:e1], ymin[e0:e1], ymax[e0:e1], height)
        queue += [(a + e0, ka, b + e0, kb, row) for a, ka, b, kb, row in q]
        steps += s
        links += l
        span_counts.append(len(q))
        e0 = e1
    q = np.array(queue, np.int64).reshape(-1, 5)
    spans = np.empty((q.shape[0], 25), np.uint32)
    spans[:, 0:12] = T[q[:, 1], q[:, 0]].view(np.uint32)
    spans[:, 12:24] = T[q[:, 3], q[:, 2]].view(np.uint32)
    spans[:, 24] = q[:, 4].astype(np.int32).view(np.uint32)
    adv = words.copy()
    if words.shape[0]:
        adv[:, END_WORDS] = T[np.array(steps, np.int64), np.arange(words.shape[0])].view(np.uint32)
    return spans, np.array(span_counts, np.uint32), adv, np.array(links, np.int32).reshape(-1)


def walk(words, height):
    """One list: (span_words [k, 25], advanced_words [n, 27], next [n])."""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
    spans, _, adv, nxt = walk_batch(words, [words.shape[0]], height)
    return spans, adv, nxt
