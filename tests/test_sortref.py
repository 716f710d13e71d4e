"""CPU tests of tests/sortref.py, the host definitions tests/test_gpu_sort_scan.py
holds the span path's radix sort and scans to: sort_ref equals Python's sorted
with an index tiebreak on every key family, scan_ref equals a loop over Python
ints, the families have the shapes their names promise, and prk_selftest_sort /
prk_selftest_scan refuse bad arguments and fail loudly without a GPU.
"""
import ctypes as C
import os

import numpy as np
import pytest

import prk
import sortref as R
from prk import abi

SMALL_N = (0, 1, 2, 5, 67, 300)
SMALL_END_BITS = (0, 1, 8, 9, 26, 41, 57, 64)


def plain_sort(keys, vals, end_bit):
    """sorted() on (masked key, index): the definition, with Python ints."""
    mask = (1 << (8 * ((end_bit + 7) // 8))) - 1
    ks = [int(k) for k in keys]
    order = sorted(range(len(ks)), key=lambda i: (ks[i] & mask, i))
    return [ks[i] for i in order], [int(vals[i]) for i in order]


def check_sort_ref(keys, end_bit, label):
    vals = R.sort_vals(len(keys), label)
    k, v = R.sort_ref(keys, vals, end_bit)
    wk, wv = plain_sort(keys, vals, end_bit)
    assert k.dtype == np.uint64 and v.dtype == np.uint32
    assert [int(x) for x in k] == wk and [int(x) for x in v] == wv, label


@pytest.mark.parametrize("family", sorted(R.SORT_FAMILIES))
def test_sort_ref_is_sorted_with_index_tiebreak(family):
    for n in SMALL_N:
        for end_bit in SMALL_END_BITS:
            check_sort_ref(R.SORT_FAMILIES[family](n, end_bit), end_bit, (family, n, end_bit))


def test_sort_ref_digit_and_merge_families():
    for n in SMALL_N:
        for end_bit in SMALL_END_BITS:
            for q in range(R.passes(end_bit)):
                check_sort_ref(R.keys_digit(n, end_bit, q), end_bit, ("digit", n, end_bit, q))
        for layout in ("H", "31"):
            for pads in ("tail", "interleaved"):
                keys, end_bit, _ = R.keys_merge(n, layout, pads)
                check_sort_ref(keys, end_bit, ("merge", n, layout, pads))


def test_order_mask_is_whole_digits():
    assert [R.passes(b) for b in R.END_BITS] == [0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 6, 7, 7, 8, 8]
    assert R.order_mask(0) == 0 and R.order_mask(1) == 0xFF and R.order_mask(26) == 0xFFFFFFFF
    assert R.order_mask(57) == R.order_mask(64) == 0xFFFFFFFFFFFFFFFF
    # bits 26 .. 31 order the pairs at end_bit = 26; bit 32 does not
    keys = np.array([1 << 26, 0, 1 << 32, 0], np.uint64)
    k, v = R.sort_ref(keys, np.arange(4), 26)
    assert v.tolist() == [1, 2, 3, 0] and k.tolist() == [0, 1 << 32, 0, 1 << 26]


def test_family_shapes():
    n = 3000
    for end_bit in (9, 26, 64):
        m = R.order_mask(end_bit)
        assert np.unique(R.keys_equal(n, end_bit)).size == 1
        a = R.keys_alt2(n, end_bit)
        assert np.unique(a).size == 2 and (a[0] & m) > (a[1] & m) and (a[::2] == a[0]).all()
        r = R.keys_runs64(n, end_bit) & m
        edges = np.flatnonzero(r[1:] != r[:-1]) + 1
        assert (edges == np.arange(64, n, 64)).all()  # every run is exactly 64 long, on a multiple of 64
        for q in range(R.passes(end_bit)):
            d = R.keys_digit(n, end_bit, q)
            assert np.unique(d & ~(np.uint64(0xFF) << np.uint64(8 * q))).size == 1 and np.unique(d).size > 100
        s = R.keys_sorted(n, end_bit)
        assert (s[1:] >= s[:-1]).all() and (R.keys_reverse(n, end_bit) == s[::-1]).all()
        assert (R.keys_uniform(n, end_bit) >> np.uint64(end_bit - 1)).max() == 1
        h = R.keys_high_bits(n, end_bit)
        assert np.unique(h & m).size < n // 2  # ties under the mask ...
        if end_bit < 57:
            assert np.unique(h & ~m).size > n // 2  # ... that the bits above would reorder
            hk, _ = R.sort_ref(h, np.arange(n), end_bit)
            assert not (hk == np.sort(h)).all()
        mid = R.keys_mid_bits(n, end_bit)
        assert (mid & ~m).max() == 0
        if end_bit % 8:
            # the other reading of end_bit (a mask of end_bit bits) gives another order
            idx = np.argsort(mid & R.low_mask(end_bit), kind="stable")
            assert not (mid[idx] == R.sort_ref(mid, np.arange(n), end_bit)[0]).all()
    v = R.sort_vals(n, "x")
    assert v.dtype == np.uint32 and np.unique(v).size < n and not (v == np.arange(n)).all()


def test_merge_keys_shape():
    for layout, ybits in (("H", 11), ("31", 31)):
        for pads in ("tail", "interleaved"):
            slots = 9001
            keys, end_bit, real = R.keys_merge(slots, layout, pads)
            pad = keys == R.ALL_ONES
            assert (pad == ~real).all()
            assert slots / 3 - 1 <= pad.sum() <= 2 * slots / 3 + 1
            if pads == "tail":
                assert not pad[:real.sum()].any()
            else:
                assert pad[2::3].all() and not pad[0::3].any()
            k = keys[real]
            assert (k >> np.uint64(end_bit)).max() == 0 and (k & np.uint64(1)).max() == 0  # below every pad key
            assert end_bit > ybits + 2
            # the pads sorted last in input order, the real keys by their whole value
            sk, sv = R.sort_ref(keys, np.arange(slots), end_bit)
            assert (sk[:real.sum()] != R.ALL_ONES).all() and (sk[real.sum():] == R.ALL_ONES).all()
            assert (sv[real.sum():] == np.flatnonzero(pad)).all()
            assert (sk[:real.sum()] == np.sort(k)).all()


def test_merge_path_orders_like_mergesort():
    """The reference's MergeSort on equal keys (run of two kept, Half1 before
    Half0) against the path order."""
    def mergesort(a):
        if len(a) <= 1:
            return a
        if len(a) == 2:
            return a
        h0 = len(a) // 2
        return mergesort(a[h0:]) + mergesort(a[:h0])  # equal keys: every Half1 entry first
    for n in (1, 2, 3, 5, 8, 13, 64, 100, 199):
        pbits = R.bitlen(n) + 1
        p = R.merge_path(np.arange(n), np.full(n, n), pbits)
        assert (p & np.uint64(1)).max() == 0 and np.unique(p).size == n
        assert np.argsort(p, kind="stable").tolist() == mergesort(list(range(n))), n


def plain_scan(x, width):
    out, acc = [], 0
    for v in x:
        out.append(acc % (1 << width))
        acc += int(v)
    return out


@pytest.mark.parametrize("width", [32, 64])
def test_scan_ref_is_the_plain_loop(width):
    for n in (0, 1, 2, 65, 257, 4097, 9000):
        for name, fam in R.SCAN_FAMILIES[width].items():
            x = fam(n, width)
            got = R.scan_ref(x, width)
            assert got.dtype == R.scan_dtype(width) and x.dtype == R.scan_dtype(width)
            assert [int(v) for v in got] == plain_scan(x, width), (name, n)
        for p in R.scan_single_positions(n):
            x = R.scan_single(n, width, p)
            assert [int(v) for v in R.scan_ref(x, width)] == plain_scan(x, width), ("single", n, p)
    # the sums of these families do pass 2^width / 2^32 at these sizes
    assert sum(int(v) for v in R.scan_random(9000, width)) >> width
    if width == 64:
        assert sum(int(v) for v in R.scan_below40(64, 64)) >> 32 and sum(int(v) for v in R.scan_edge32(3, 64)) >> 32


def test_sizes_sit_on_the_kernels_boundaries():
    s = set(R.SORT_SIZES)
    for b in (64, R.WAVE_SEG_SHORT, R.TILE_SHORT, R.SMALL_MAX):
        assert {b - 1, b, b + 1} <= s
    assert {R.SMALL_MAX + R.TILE_LONG, R.SMALL_MAX + R.TILE_LONG + 1} <= s
    assert max(s) > 256 * R.TILE_LONG and max(s) < 1200000
    assert R.SORT_SIZE_SHORT <= R.SMALL_MAX < R.SORT_SIZE_LONG
    c = set(R.SCAN_SIZES)
    for b in (64, 256, R.SCAN_TILE, 2 * R.SCAN_TILE):
        assert {b - 1, b, b + 1} <= c
    assert {256 * R.SCAN_TILE, 256 * R.SCAN_TILE + 1, 257 * R.SCAN_TILE + 1} <= c and max(c) < 1400000


def test_selftest_sort_scan_argument_errors():
    L = prk.lib()
    k = np.zeros(64, np.uint64)
    v = np.zeros(64, np.uint32)
    pk, pv = C.c_void_p(k.ctypes.data), C.c_void_p(v.ctypes.data)
    d = C.c_uint32(0)
    pd = C.byref(d)
    sort, scan = L.prk_selftest_sort, L.prk_selftest_scan
    assert sort(-1, 64, 26, pk, pv, 1, pk, pv, pd) == abi.PRK_ERR_ARG
    assert sort(0, 64, 26, None, pv, 1, pk, pv, pd) == abi.PRK_ERR_ARG
    assert sort(0, 64, 26, pk, None, 1, pk, pv, pd) == abi.PRK_ERR_ARG
    assert sort(0, 64, 26, pk, pv, 1, None, pv, pd) == abi.PRK_ERR_ARG
    assert sort(0, 64, 26, pk, pv, 1, pk, None, pd) == abi.PRK_ERR_ARG
    assert sort(0, 64, 26, pk, pv, 1, pk, pv, None) == abi.PRK_ERR_ARG
    assert sort(0, 64, 26, pk, pv, 0, pk, pv, pd) == abi.PRK_ERR_ARG  # no repeats
    for width in (0, 8, 16, 33, 128, -32):
        assert scan(0, width, 64, pk, pk, pd) == abi.PRK_ERR_ARG
    assert scan(-1, 32, 64, pk, pk, pd) == abi.PRK_ERR_ARG
    assert scan(0, 32, 64, None, pk, pd) == abi.PRK_ERR_ARG
    assert scan(0, 64, 64, pk, None, pd) == abi.PRK_ERR_ARG
    assert scan(0, 64, 64, pk, pk, None) == abi.PRK_ERR_ARG
    if prk.device_count() > 0:
        assert sort(prk.device_count(), 64, 26, pk, pv, 1, pk, pv, pd) == abi.PRK_ERR_ARG
        assert scan(prk.device_count(), 32, 64, pk, pk, pd) == abi.PRK_ERR_ARG


def test_selftest_sort_refuses_sizes_before_touching_memory():
    """end_bit = 65 and n = 2^30: the status of hipErrorInvalidValue, with
    64-element arrays behind the pointers -- nothing is allocated or read."""
    L = prk.lib()
    k = np.zeros(64, np.uint64)
    v = np.zeros(64, np.uint32)
    pk, pv = C.c_void_p(k.ctypes.data), C.c_void_p(v.ctypes.data)
    d = C.c_uint32(0x5A5A5A5A)
    assert L.prk_selftest_sort(0, 64, 65, pk, pv, 1, pk, pv, C.byref(d)) == abi.PRK_ERR_DEVICE
    assert L.prk_selftest_sort(0, 1 << 30, 26, pk, pv, 1, pk, pv, C.byref(d)) == abi.PRK_ERR_DEVICE
    assert L.prk_selftest_sort(0, 0xFFFFFFFF, 64, pk, pv, 1, pk, pv, C.byref(d)) == abi.PRK_ERR_DEVICE
    assert d.value == 0x5A5A5A5A and not k.any() and not v.any()


@pytest.mark.skipif(os.environ.get("PRK_EXPECT_GPU") == "1", reason="GPU box")
def test_selftest_sort_scan_fail_loudly_without_gpu():
    if prk.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(prk.PrkError) as e:
        prk.selftest_sort(np.zeros(64, np.uint64), np.zeros(64, np.uint32), 26)
    assert e.value.code == abi.PRK_ERR_DEVICE
    for width in (32, 64):
        with pytest.raises(prk.PrkError) as e:
            prk.selftest_scan(np.zeros(64, np.uint64), width)
        assert e.value.code == abi.PRK_ERR_DEVICE
