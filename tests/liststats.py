"""The per-list walk statistics of the handle record walks (prk_records_advance
/ _spans / _rows), twice:

  stats_formula   the closed forms the device kernels evaluate (k_list_stats,
                  k_list_most), in NumPy;
  stats_sweep     a literal port of prk_record_api.hip's list_walk_steps and
                  list_most_listed -- the heap sweeps of the host-input calls
                  -- without their early exits.

Both take one sorted list as int arrays (ymin non-decreasing, 0 <= ymin <=
ymax) and a height, and return (edge_rows, scans, most, ymin0, ymax_max).
tests/test_list_stats_rule.py holds the two to each other.
"""
import heapq

import numpy as np

CAP = 1 << 21          # kAdvMaxSteps
MIN_STEPS = 3432       # kAdvWgMinSteps
YMAX, YMIN = 0, 7      # prk_edge words


def stats_formula(ymin, ymax, height):
    ymin, ymax = np.asarray(ymin, np.int64), np.asarray(ymax, np.int64)
    n = ymin.shape[0]
    if n == 0:
        return 0, 0, 0, 0, 0
    edge_rows = int(np.maximum(0, np.minimum(ymax, height) - ymin).sum())
    m = int(np.searchsorted(ymin, height, side="left"))  # the records with YMin < height: a prefix
    a, b = ymin[:m], ymax[:m]
    ub = np.searchsorted(a, b, side="right")             # #{i < m : YMin[i] <= YMax[j]}
    scans = int((ub - np.arange(m) - 1).sum())
    # #{j < m : YMin[j] <= YMin[i] <= YMax[j]}: those begun by row YMin[i] less those ended before it
    begun = np.searchsorted(a, a, side="right")
    ended = np.searchsorted(np.sort(b), a, side="left")
    most = int((begun - ended).max()) if m else 0
    return edge_rows, scans, most, int(ymin[0]), int(ymax.max())


def stats_sweep(ymin, ymax, height):
    n = len(ymin)
    edge_rows = sum(max(0, min(int(ymax[i]), height) - int(ymin[i])) for i in range(n))
    scans, most, heap = 0, 0, []
    i = 0
    while i < n and ymin[i] < height:  # (the walk ends at `height`)
        while heap and heap[0] < ymin[i]:
            heapq.heappop(heap)
        scans += len(heap)             # list_walk_steps: before the push
        heapq.heappush(heap, int(ymax[i]))
        most = max(most, len(heap))    # list_most_listed: after it
        i += 1
    return edge_rows, scans, most, (int(ymin[0]) if n else 0), (int(max(ymax)) if n else 0)


def cost(edge_rows, scans, n):
    """list_walk_steps' value, from the exact scans."""
    allp = n * (n - 1) // 2
    if edge_rows > CAP or edge_rows + allp <= CAP:
        return edge_rows + allp
    return edge_rows + scans


def expected_rows(words, counts, height, min_steps=MIN_STEPS):
    """prk_debug_list_stats' rows for a batch of packed records: int64
    [nlist, 5]; most is 0 unless the list is a route candidate."""
    out, o = np.zeros((len(counts), 5), np.int64), 0
    for l, n in enumerate(int(c) for c in counts):
        w = words[o:o + n]
        o += n
        er, sc, most, y0, ym = stats_formula(w[:, YMIN].view(np.int32), w[:, YMAX].view(np.int32), height)
        cand = n > 0 and cost(er, sc, n) >= min_steps and er <= CAP
        out[l] = (er, sc, most if cand else 0, y0, ym)
    return out
