"""CPU test: the closed forms of the per-list walk statistics (what k_list_stats
and k_list_most evaluate for the handle record walks) against
literal ports of the host pass's heap sweeps (prk_record_api.hip list_walk_steps and
list_most_listed, without their early exits) -- liststats.py holds both.  The
proof of the formulas by exhaustion; the device is held to the closed forms in
tests/test_gpu_record_walks.py.
"""
import numpy as np
import pytest

from liststats import stats_formula, stats_sweep
from prk import abi

FIELDS = abi.LIST_STATS_FIELDS  # prk_debug_list_stats' words

HAND = {
    "empty": ([], []),
    "one edge": ([3], [9]),
    "one edge of no rows": ([3], [3]),
    "all equal YMin": ([5] * 7, [6, 9, 5, 30, 7, 5, 12]),
    "YMax == YMin throughout": ([0, 0, 2, 2, 2, 8], [0, 0, 2, 2, 2, 8]),
    "nested": ([0, 1, 2, 3, 4], [20, 15, 10, 6, 4]),
    "disjoint": ([0, 4, 8, 12], [2, 6, 10, 14]),
    "touching (YMax == the next YMin)": ([0, 3, 6, 9], [3, 6, 9, 12]),
    "ties then a gap": ([1, 1, 1, 40, 40], [5, 2, 1, 41, 90]),
    "a long edge over short ones": ([0, 1, 1, 2, 5, 5, 9], [100, 1, 3, 2, 7, 5, 9]),
}


def heights(ymin, ymax):
    top = max(ymax) if len(ymax) else 0
    inside = sorted({0, 1, top // 2, top, top + 1, top + 50} | set(ymin) | {y + 1 for y in ymin})
    return inside


def compare(ymin, ymax, height, label):
    got = stats_formula(ymin, ymax, height)
    want = stats_sweep(ymin, ymax, height)
    assert got == want, "%s height %d: %s" % (label, height, {f: (g, w) for f, g, w in zip(FIELDS, got, want)
                                                               if g != w})


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_lists(name):
    assert len(FIELDS) == 5
    ymin, ymax = HAND[name]
    for h in heights(ymin, ymax):
        compare(ymin, ymax, h, name)


def test_known_values():
    """Figures worked by hand, so that the two statements cannot be wrong alike."""
    # nested: every earlier edge is still linked at each insertion: 0 + 1 + 2 + 3 + 4
    assert stats_formula(*HAND["nested"], 64) == (20 + 14 + 8 + 3 + 0, 10, 5, 0, 20)
    # disjoint: no edge is linked when the next begins
    assert stats_formula(*HAND["disjoint"], 64) == (8, 0, 1, 0, 14)
    # touching: an edge leaves on row YMax after that row's insertions, so it is met once
    assert stats_formula(*HAND["touching (YMax == the next YMin)"], 64) == (12, 3, 2, 0, 12)
    # height 4 cuts the touching list after its second edge
    assert stats_formula(*HAND["touching (YMax == the next YMin)"], 4) == (3 + 1, 1, 2, 0, 12)
    assert stats_formula(*HAND["nested"], 0) == (0, 0, 0, 0, 20)


def test_random_sorted_lists():
    rng = np.random.default_rng(20260)
    for k in range(400):
        n = int(rng.integers(0, 301))
        span = int(rng.choice([1, 4, 40, 400]))
        ymin = np.sort(rng.integers(0, span + 1, n))
        ymax = ymin + rng.integers(0, int(rng.choice([1, 3, 30, 300])) + 1, n)
        top = int(ymax.max()) if n else 0
        for h in (0, int(rng.integers(0, top + 2)), top + 7):
            compare(ymin.tolist(), ymax.tolist(), h, "random list %d (%d edges)" % (k, n))
