"""The device argument of the self-tests that count the devices (ops, sort,
scan, visibility, select, bounds), with every other argument valid and one
element long: a device past the count is PRK_ERR_DEVICE where there is no
device at all and PRK_ERR_ARG where there is one, a negative device is
PRK_ERR_ARG everywhere.  No kernel runs, so the test needs no GPU and holds on
a machine with one as well.
"""
import ctypes as C

import numpy as np
import pytest

import prk
import xform_ref as X
from prk import abi

FAR = 1 << 20  # no machine has this many devices


def _calls():
    """name -> (function, arguments with the device first, the arrays they point into)."""
    L = prk.lib()
    u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
    dmg = C.c_uint32(7)
    calls = {}
    # ops: op 0 reads a and b
    a, b, out0 = u32(7), u32(3), u32(9)
    calls["ops"] = (L.prk_selftest_ops,
                    [0, 0, 1, a.ctypes.data, b.ctypes.data, None, None, out0.ctypes.data, None, None, None], (a, b, out0))
    keys, vals, ko, vo = np.array([5], np.uint64), u32(1), np.array([9], np.uint64), u32(9)
    calls["sort"] = (L.prk_selftest_sort, [0, 1, 64, keys.ctypes.data, vals.ctypes.data, 1, ko.ctypes.data,
                                           vo.ctypes.data, C.byref(dmg)], (keys, vals, ko, vo))
    x, y = u32(4), u32(9)
    calls["scan"] = (L.prk_selftest_scan, [0, 32, 1, x.ctypes.data, y.ctypes.data, C.byref(dmg)], (x, y))
    win = np.array([0], np.int32)
    counts, ids, pix, vis = u32(9), u32(9), u32(9, 9), u32(9, 9)
    nvis, nat = C.c_uint32(7), C.c_uint64(7)
    calls["visibility"] = (L.prk_selftest_visibility,
                           [0, 1, win.ctypes.data, 1, counts.ctypes.data, pix.ctypes.data, vis.ctypes.data,
                            ids.ctypes.data, C.byref(nvis), C.byref(nat), C.byref(dmg)], (win, counts, ids, pix, vis))
    items, levels = u32(0, 1, 0, 1, 0).reshape(1, 5), u32(0, 0, 1).reshape(1, 3)
    xf = X.translation((0, 0, 0))[None].copy()
    ip = C.cast(items.ctypes.data, C.POINTER(abi.PrkSelectItem))
    lp = C.cast(levels.ctypes.data, C.POINTER(abi.PrkSelectLevel))
    xp = C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform))
    px, chosen, first, total = u32(5), np.array([9], np.int32), u32(9, 9), C.c_uint64(7)
    src, dst = np.zeros((3, 3), np.float32), np.full((3, 3), 9, np.float32)
    calls["select"] = (L.prk_selftest_select,
                       [0, None, 0, ip, 1, lp, 1, xp, 1, px.ctypes.data, src.ctypes.data, None, None, None, 1, 0, 1,
                        dst.ctypes.data, None, None, None, chosen.ctypes.data, first.ctypes.data, C.byref(total),
                        C.byref(dmg)], (items, levels, xf, px, chosen, first, src, dst))
    bounds = prk.pack_bounds([[0, 0, 0]], [[1, 1, 1]], [0])
    bp = C.cast(bounds.ctypes.data, C.POINTER(abi.PrkBound))
    z, zmin, bpx = np.zeros((8, 8), np.float32), np.full((1, 1), 9, np.float32), u32(9)
    tr = abi.make_transform(2.0, 1.0, 8.0, 4.0, 4.0)
    calls["bounds"] = (L.prk_selftest_bounds,
                       [0, z.ctypes.data, 8, 8, 0, 8, 0, C.byref(tr), None, bp, 1, xp, 1, zmin.ctypes.data,
                        bpx.ctypes.data, C.byref(dmg)], (bounds, z, zmin, bpx, tr, xf))
    return calls, dmg


NAMES = ("ops", "sort", "scan", "visibility", "select", "bounds")


def test_every_counting_self_test_is_covered():
    assert tuple(_calls()[0]) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_a_device_past_the_count(name):
    calls, dmg = _calls()
    fn, args, _keep = calls[name]
    want = abi.PRK_ERR_DEVICE if prk.device_count() == 0 else abi.PRK_ERR_ARG
    assert fn(*([FAR] + args[1:])) == want
    assert dmg.value == 7  # (nothing written)


@pytest.mark.parametrize("name", NAMES)
def test_a_negative_device(name):
    calls, dmg = _calls()
    fn, args, _keep = calls[name]
    assert fn(*([-1] + args[1:])) == abi.PRK_ERR_ARG
    assert dmg.value == 7
