"""The span path's radix sort and exclusive scans (csrc/prk_sort.hip) on the
GPU against their definitions in numpy (tests/sortref.py): every output word
equal, and the damage word of prk_selftest_sort / prk_selftest_scan zero --
the inputs unchanged, nothing written past n outputs or past the temp size
the query returned.

Sort: the sizes sit on the code's constants (wave segments of 256 / 1024
items, tiles of 1024 / 4096, the switch at 262144, more than 256 long tiles);
end_bit runs through 0 .. 8 passes at one short-tile and one long-tile size,
and the size list runs at 3, 4 and 8 passes.  Each key family aims at one
mistake (sortref.py says which); the values are random with duplicates.  The
order is by whole 8-bit digits (csrc/prk_launch.h): `mid_bits` would fail a
sort that masked its last digit to end_bit, `high_bits` one that looked
above its last digit.

Scan: both widths at every size (a thread's 16 items, a wave's 1024, the
4096 tile, 256 / 257 / 258 tiles: one and two trips of the loop over the tile
sums), sums that wrap 2^32 and 2^64, and for width 64 sums that carry from
the low half into the high half inside a wave, between waves and between
tiles.

What these tests see, tried on mutated builds of prk_sort.hip (values only,
the scatter's store bounds-checked in those builds): the rank inside a peer
group reversed (626 tests fail: every sort with a repeated digit in a wave
round), the high half dropped from wave_incl_u64's add (79: every width-64
family whose sums pass 2^32, from n = 63 up), k_scan_down reading the tile
sums in one trip only (21: every non-zero family from 258 tiles up -- 256 and
257 tiles still fit one trip), a neighbouring pass's histogram row (680:
every sort of two passes or more), and one pass fewer in k_rs_upsweep (608).
"""
import numpy as np
import pytest

import prk
import sortref as R

pytestmark = pytest.mark.gpu

SIZE_END_BITS = (17, 26, 64)  # 3, 4 and 8 passes: both ping-pong parities
FAMILIES = sorted(R.SORT_FAMILIES)


def first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d differ; first at %d: gpu %x ref %x" % (bad.size, want.size, bad[0], int(got[bad[0]]),
                                                            int(want[bad[0]]))


def check_sort(keys, end_bit, label, repeats=1):
    vals = R.sort_vals(keys.shape[0], label)
    k, v, damage = prk.selftest_sort(keys, vals, end_bit, repeats)
    wk, wv = R.sort_ref(keys, vals, end_bit)
    assert damage == 0, "%s: damage %d" % (label, damage)
    assert np.array_equal(k, wk), "%s keys: %s" % (label, first_bad(k, wk))
    assert np.array_equal(v, wv), "%s vals: %s" % (label, first_bad(v, wv))
    return k, v, vals


@pytest.mark.parametrize("end_bit", R.END_BITS)
@pytest.mark.parametrize("n", [R.SORT_SIZE_SHORT, R.SORT_SIZE_LONG])
@pytest.mark.parametrize("family", FAMILIES)
def test_sort_every_pass_count(family, n, end_bit):
    check_sort(R.SORT_FAMILIES[family](n, end_bit), end_bit, (family, n, end_bit))


@pytest.mark.parametrize("end_bit", SIZE_END_BITS)
@pytest.mark.parametrize("n", R.SORT_SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_sort_every_size(family, n, end_bit):
    check_sort(R.SORT_FAMILIES[family](n, end_bit), end_bit, (family, n, end_bit))


@pytest.mark.parametrize("end_bit", [b for b in R.END_BITS if b])
@pytest.mark.parametrize("n", [R.SORT_SIZE_SHORT, R.SORT_SIZE_LONG])
def test_sort_one_digit_differs(n, end_bit):
    for q in range(R.passes(end_bit)):
        check_sort(R.keys_digit(n, end_bit, q), end_bit, ("digit", n, end_bit, q))


@pytest.mark.parametrize("n", [1, 257, 1025, 5003, 262144, 262145, 266241, 1100003])
@pytest.mark.parametrize("pads", ["tail", "interleaved"])
@pytest.mark.parametrize("layout", ["H", "31"])
def test_sort_mergesort_keys(layout, pads, n):
    keys, end_bit, real = R.keys_merge(n, layout, pads)
    k, v, vals = check_sort(keys, end_bit, ("merge", layout, pads, n, end_bit))
    total = int(real.sum())
    # every pad after every real key, in input order
    assert (k[:total] != R.ALL_ONES).all() and (k[total:] == R.ALL_ONES).all()
    assert np.array_equal(v[total:], vals[~real])
    assert (k[1:total] > k[:total - 1]).all()  # (object, YMin, path) is unique


@pytest.mark.parametrize("end_bit", [9, 26, 64])
@pytest.mark.parametrize("n", [1025, R.SORT_SIZE_SHORT, R.SORT_SIZE_LONG, 1100003])
@pytest.mark.parametrize("family", ["equal", "uniform"])
def test_sort_repeated_on_one_temp(family, n, end_bit):
    """Three sorts on the temp buffer the one before left: stale histograms,
    tickets and look-back status words would show."""
    check_sort(R.SORT_FAMILIES[family](n, end_bit), end_bit, (family, n, end_bit, "x3"), repeats=3)


def test_sort_repeated_mergesort_keys():
    keys, end_bit, _ = R.keys_merge(R.SORT_SIZE_LONG, "H", "tail")
    check_sort(keys, end_bit, ("merge", "x3", end_bit), repeats=3)


# ---- scans ------------------------------------------------------------------------
def check_scan(x, width, label):
    out, damage = prk.selftest_scan(x, width)
    want = R.scan_ref(x, width)
    assert damage == 0, "%s: damage %d" % (label, damage)
    assert out.dtype == want.dtype
    assert np.array_equal(out, want), "%s: %s" % (label, first_bad(out, want))
    return out


SCAN_CASES = [(w, f) for w in (32, 64) for f in sorted(R.SCAN_FAMILIES[w])]


@pytest.mark.parametrize("n", R.SCAN_SIZES)
@pytest.mark.parametrize("width,family", SCAN_CASES)
def test_scan(width, family, n):
    x = R.SCAN_FAMILIES[width][family](n, width)
    out = check_scan(x, width, (width, family, n))
    if family == "one":
        assert np.array_equal(out, np.arange(n, dtype=out.dtype))
    if family == "zero":
        assert not out.any()


@pytest.mark.parametrize("n", [4095, 4096, 8192, 1048576, 1052672])
@pytest.mark.parametrize("width,family", SCAN_CASES)
def test_scan_callers_form(width, family, n):
    """n + 1 values, the last one 0: out[n] is the total (every call site)."""
    x = np.concatenate([R.SCAN_FAMILIES[width][family](n, width), np.zeros(1, R.scan_dtype(width))])
    out = check_scan(x, width, (width, family, n, "+1"))
    assert int(out[n]) == sum(x.tolist()) % (1 << width)


@pytest.mark.parametrize("n", [s for s in R.SCAN_SIZES if s])
@pytest.mark.parametrize("width", [32, 64])
def test_scan_single_value(width, n):
    """One non-zero value at p: zero up to p and the value after it -- each
    position reaches every later one and no earlier one."""
    for p in R.scan_single_positions(n):
        out = check_scan(R.scan_single(n, width, p), width, (width, "single", n, p))
        assert not out[:p + 1].any() and (out[p + 1:] == R.SCAN_SINGLE_VALUE[width]).all(), (width, n, p)
