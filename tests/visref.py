"""Visibility feedback (include/prk.h prk_visibility_*), written from the
definition in numpy: the counts of a winner map's words per id, their prefix
sums, the ids that won a pixel, and group sums as prefix differences.  The
winner-word patterns the GPU tests feed prk_selftest_visibility live here too.
"""
import collections

import numpy as np

Vis = collections.namedtuple("Vis", "counts pix_prefix vis_prefix ids covered visible")

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


def reduce(winners, id_count):
    """The definition: words in [0, id_count) counted per id (np.bincount);
    every other word -- -1, or any id the frame did not hand out -- ignored."""
    w = np.asarray(winners).astype(np.int64).reshape(-1)
    m = int(id_count)
    inside = w[(w >= 0) & (w < m)]
    counts = np.bincount(inside, minlength=m)[:m].astype(np.uint64)
    assert int(counts.sum()) < 2**32
    flags = (counts != 0).astype(np.uint64)
    pix = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    vis = np.concatenate([[0], np.cumsum(flags)]).astype(np.uint32)
    ids = np.flatnonzero(counts).astype(np.uint32)
    return Vis(counts.astype(np.uint32), pix, vis, ids, int(pix[m]), int(vis[m]))


def groups(v, starts):
    """(pixels, visible) of the id ranges [starts[g], starts[g + 1])."""
    st = np.asarray(starts, np.int64)
    assert st.ndim == 1 and st.shape[0] >= 1 and (np.diff(st) >= 0).all() and 0 <= st[0] and st[-1] <= v.counts.shape[0]
    return v.pix_prefix[st[1:]] - v.pix_prefix[st[:-1]], v.vis_prefix[st[1:]] - v.vis_prefix[st[:-1]]


def runs_of(winners, at_least):
    """How many maximal runs of equal words, in 1-D order, are `at_least` long or longer."""
    w = np.asarray(winners).reshape(-1)
    if w.shape[0] == 0:
        return 0
    heads = np.flatnonzero(np.concatenate([[True], w[1:] != w[:-1]]))
    return int((np.diff(np.concatenate([heads, [w.shape[0]]])) >= at_least).sum())


# ---- winner-word patterns: n int32 words over id_count ids --------------------------
def _rng(name, n, m):
    return np.random.default_rng([sorted(PATTERNS).index(name), n, m])


def p_none(n, m):
    return np.full(n, -1, np.int32)


def p_first_id(n, m):
    return np.zeros(n, np.int32)


def p_last_id(n, m):
    return np.full(n, m - 1, np.int32)


def p_alternating(n, m):
    """Strictly alternating two ids (with one id: that id and -1)."""
    a, b = (0, m - 1) if m > 1 else (0, -1)
    return np.where(np.arange(n) % 2 == 0, a, b).astype(np.int32)


def p_id_and_none(n, m):
    return np.where(np.arange(n) % 2 == 0, m - 1, -1).astype(np.int32)


def p_random(n, m):
    return _rng("random", n, m).integers(0, m, n).astype(np.int32)


def p_runs(n, m):
    """Runs of random length 1..130 of random ids (-1 among them), then runs
    placed so that heads fall on lanes 0 and 63 of a wave (words 0, 63, 64,
    252 of a 256-word segment, a lane holding four) and on words 255 / 256."""
    rng = _rng("runs", n, m)
    w = np.repeat(rng.integers(-1, m, n), rng.integers(1, 131, n))[:n].astype(np.int32)
    for head in (63, 64, 252, 255, 256, 511, 512, 4095, 4096):
        if head + 1 < n:
            end = min(n, head + int(rng.integers(1, 131)))
            w[head:end] = (w[head - 1] + 1) % m if m > 1 else (-1 if w[head - 1] == 0 else 0)
    return w


def p_spanning_run(n, m):
    """One run over the whole array but its first and last word."""
    w = np.full(n, m - 1, np.int32)
    w[0] = w[-1] = -1 if m == 1 else 0
    return w


def p_outside(n, m):
    """Ids of the frame mixed with words outside [0, id_count): all ignored."""
    rng = _rng("outside", n, m)
    pool = np.array([-2, m, INT32_MAX, INT32_MIN, 0, m - 1], np.int64)
    return pool[rng.integers(0, len(pool), n)].astype(np.int32)


PATTERNS = {"none": p_none, "first_id": p_first_id, "last_id": p_last_id, "alternating": p_alternating,
            "id_and_none": p_id_and_none, "random": p_random, "runs": p_runs, "spanning_run": p_spanning_run,
            "outside": p_outside}
SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 65539)
ID_COUNTS = (1, 2, 65, 4096, 4097, 70000)  # the scans of id_count + 1 words: one launch up to 4096, two above
