"""CPU tests of prk_geometry_select's boundary (no GPU compute): the symbols
declared in include/prk.h, exported and bound with abi.SELECT_SIGS; a NULL
context and NULL required pointers refused before any device call; and the
numpy restatement of the definition (tests/selectref.py) against a table
worked by hand.  What the device computes is checked on the GPU
(tests/test_gpu_select.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prk
import selectref as S
import xform_ref as X
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prk_geometry_select", "prk_selftest_select", "prk_debug_select_ms")
STRUCTS = {"prk_select_item": abi.PrkSelectItem, "prk_select_level": abi.PrkSelectLevel, "prk_xform": abi.PrkXform}
SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}


def header():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_names_are_exported():
    assert sorted(abi.SELECT_SIGS) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert name in prk.exported_symbols(), name
        assert re.search(r"\bT %s$" % name, out, re.M), name
    # the host functions that cross the host files stay out of the dynamic table
    for hidden in ("select_check", "vis_ready", "geometry_grow"):
        assert not re.search(r"\b%s$" % hidden, out, re.M), hidden
    assert hasattr(prk.Renderer, "geometry_select") and callable(prk.selftest_select)


@pytest.mark.parametrize("name", NAMES)
def test_signature_declared_and_bound(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header(), re.M | re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    sig = abi.SELECT_SIGS[name]
    assert len(params) == len(sig), (name, params)
    for p, t in zip(params, sig):
        decl = re.match(r"(.*?[ *])\w+$", p).group(1).strip()
        if not decl.endswith("*"):
            assert t is SCALARS[decl], (name, p, t)
            continue
        pointee = decl.replace("const ", "")[:-1].strip()
        if pointee in STRUCTS:  # a table: the mirrored struct, and its size as the header's fields give it
            assert t._type_ is STRUCTS[pointee], (name, p, t)
        elif t is not C.c_void_p:  # a typed scalar out
            assert t._type_ is SCALARS[pointee], (name, p, t)
        else:
            assert pointee in SCALARS or pointee == "prk_context", (name, p)
    f = getattr(prk.lib(), name)
    assert f.restype is C.c_int and list(f.argtypes) == sig


def test_struct_layouts_match_the_header():
    h = header()
    for name, cls in (("prk_select_level", abi.PrkSelectLevel), ("prk_select_item", abi.PrkSelectItem)):
        m = re.search(r"typedef struct %s \{\s*uint32_t ([^;]*);\s*\} %s;" % (name, name), h)
        assert m, name
        fields = [f.strip() for f in m.group(1).split(",")]
        assert fields == [f[0] for f in cls._fields_], name
        assert C.sizeof(cls) == 4 * len(fields)


def test_null_context_and_null_pointers_are_refused():
    """PRK_ERR_ARG before any device call (there is no device here), nothing written."""
    L = prk.lib()
    ARG = abi.PRK_ERR_ARG
    items = np.array([[0, 1, 0, 1, 0]], np.uint32)
    levels = np.array([[0, 0, 1]], np.uint32)
    xf = X.translation((0, 0, 0))[None].copy()
    ip = C.cast(items.ctypes.data, C.POINTER(abi.PrkSelectItem))
    lp = C.cast(levels.ctypes.data, C.POINTER(abi.PrkSelectLevel))
    xp = C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform))
    px = np.array([5], np.uint32)
    chosen, first = np.full(1, 9, np.int32), np.full(2, 9, np.uint32)
    total = C.c_uint64(7)
    tail = (px.ctypes.data, chosen.ctypes.data, first.ctypes.data)
    assert L.prk_geometry_select(None, 0, 1, 0, ip, 1, lp, 1, xp, 1, *tail, C.byref(total)) == ARG
    # a context that is never looked at: the pointer checks come first
    fake = (C.c_uint8 * 64)()
    ctx = C.addressof(fake)
    assert L.prk_geometry_select(ctx, 0, 1, 0, ip, 1, lp, 1, xp, 1, *tail, None) == ARG
    assert L.prk_geometry_select(ctx, 0, 1, 0, None, 1, lp, 1, xp, 1, *tail, C.byref(total)) == ARG
    a, b = C.c_float(3.0), C.c_float(3.0)
    assert L.prk_debug_select_ms(None, C.byref(a), C.byref(b)) == ARG
    assert L.prk_debug_select_ms(ctx, None, C.byref(b)) == ARG and L.prk_debug_select_ms(ctx, C.byref(a), None) == ARG
    assert bytes(fake) == bytes(64) and total.value == 7 and (a.value, b.value) == (3.0, 3.0)
    # the self-test: every pointer it needs, a device >= 0, tables that hold together
    src = np.zeros((3, 3), np.float32)
    dst = np.full((3, 3), 9, np.float32)
    dmg = C.c_uint32(7)
    good = [0, None, 0, ip, 1, lp, 1, xp, 1, px.ctypes.data, src.ctypes.data, None, None, None, 1, 0, 1,
            dst.ctypes.data, None, None, None, chosen.ctypes.data, first.ctypes.data, C.byref(total), C.byref(dmg)]
    for k in (3, 5, 7, 10, 17, 21, 22, 23, 24):
        bad = list(good)
        bad[k] = None
        assert L.prk_selftest_select(*bad) == ARG, k
    assert L.prk_selftest_select(*([-1] + good[1:])) == ARG
    no_counts = list(good)
    no_counts[9] = None  # neither item_pixels nor pix_prefix
    assert L.prk_selftest_select(*no_counts) == ARG
    for k, v in ((14, 0), (16, 0), (8, 0), (6, 0)):  # src too short, dst too short, xform / levels past their tables
        bad = list(good)
        bad[k] = v
        assert L.prk_selftest_select(*bad) == ARG, k
    assert (dst == 9).all() and (chosen == 9).all() and (first == 9).all() and total.value == 7 and dmg.value == 7


# ---- selectref itself -----------------------------------------------------------------------------------------------
# levels: (min_pixels, src_first_tri, tri_count)
LEVELS = np.array([[100, 0, 8],    # 0: item 0, 1, 5 -- fine
                   [10, 8, 2],     # 1:                 coarse
                   [1, 10, 4],     # 2: item 2 -- unordered thresholds: 1, 50, 0
                   [50, 14, 6],    # 3
                   [0, 20, 1],     # 4
                   [0, 21, 3],     # 5: item 3 -- always drawn
                   [7, 24, 5]], np.uint32)  # 6: item 6 -- its ids are an empty range
# items: (first_id, id_count, first_level, level_count, xform)
ITEMS = np.array([[0, 2, 0, 2, 0],    # ids 0, 1: 100 pixels -- a threshold equal to the count passes
                  [2, 1, 0, 2, 1],    # id 2: 9 pixels -- one below the coarse threshold: dropped
                  [3, 2, 2, 3, 0],    # ids 3, 4: 60 pixels -- the first pass is level 0 (>= 1), not the 50 behind it
                  [5, 1, 5, 1, 1],    # id 5: 0 pixels, min_pixels 0
                  [5, 1, 0, 0, 9],    # no levels (its xform is never looked at)
                  [6, 1, 0, 2, 0],    # id 6: 99 pixels -- one below the fine threshold: the coarse level
                  [7, 0, 6, 1, 0]], np.uint32)  # id_count == 0: 0 pixels, below 7
COUNTS = np.array([60, 40, 9, 25, 35, 0, 99, 1000], np.uint32)


def test_selectref_on_a_hand_worked_table():
    pp = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint32)
    px = S.pixels_of(ITEMS, pix_prefix=pp)
    assert px.tolist() == [100, 9, 60, 0, 0, 99, 0]
    sel = S.choose(ITEMS, LEVELS, px, dst_first_tri=5)
    assert sel.chosen.tolist() == [0, -1, 0, 0, -1, 1, -1]
    assert sel.n.tolist() == [8, 0, 4, 3, 0, 2, 0]
    assert sel.out_first.tolist() == [5, 13, 13, 17, 20, 20, 22, 22] and sel.total == 17
    # the same numbers given as item_pixels: first_id / id_count are not looked at
    blind = ITEMS.copy()
    blind[:, :2] = 0xFFFFFFFF
    again = S.choose(blind, LEVELS, S.pixels_of(blind, item_pixels=px), dst_first_tri=5)
    assert again.chosen.tolist() == sel.chosen.tolist() and again.out_first.tolist() == sel.out_first.tolist()
    assert S.runs_of(ITEMS, LEVELS, sel).tolist() == [[0, 8, 5, 0], [10, 4, 13, 0], [21, 3, 17, 1], [8, 2, 20, 0]]
    assert S.check(ITEMS, LEVELS, 2, 29, 5, frame_ids=8) == 8 + 8 + 6 + 3 + 0 + 8 + 5
    # the thresholds on their own: equal passes, one below does not, 0 always does
    for count, want in ((100, 0), (99, 1), (10, 1), (9, -1), (0, -1)):
        assert S.choose(ITEMS[:1], LEVELS, [count]).chosen.tolist() == [want]
    assert S.choose(ITEMS[3:4], LEVELS, [0]).chosen.tolist() == [0]


def test_selectref_emit_and_errors():
    rng = np.random.default_rng(1)
    src = X.random_arrays(rng, 29)
    xf = X.random_values(rng, (2, 3, 4))
    pp = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint32)
    sel = S.choose(ITEMS, LEVELS, S.pixels_of(ITEMS, pix_prefix=pp), dst_first_tri=5)
    out = S.emit(ITEMS, LEVELS, xf, src, (None,) * 4, sel)
    assert out[0].shape == (3 * 22, 3) and not out[0][:15].any()
    assert np.array_equal(out[0][15:39].view(np.uint32), X.positions(xf[0], src[0][0:24]).view(np.uint32))
    assert np.array_equal(out[2][51:60].view(np.uint32), X.normals(xf[1], src[2][63:72]).view(np.uint32))
    assert np.array_equal(out[1][60:66].view(np.uint32), src[1][24:30].view(np.uint32))
    words = S.emit_selftest(ITEMS, LEVELS, xf, src, 30, sel)
    assert (words[0][:15] == S.GUARD_WORD).all() and (words[3][66:] == S.GUARD_WORD).all()
    assert np.array_equal(words[3][15:66], out[3][15:66].view(np.uint32))
    nothing = S.choose(ITEMS, LEVELS, np.zeros(7, np.int64) + 5)  # below every threshold but the 0s
    assert nothing.chosen.tolist() == [-1, -1, 0, 0, -1, -1, -1]
    none = S.choose(ITEMS[:2], LEVELS, [0, 0], dst_first_tri=3)
    assert none.total == 0 and none.out_first.tolist() == [3, 3, 3]
    assert S.emit(ITEMS[:2], LEVELS, xf, src, (None,) * 4, none) == (None,) * 4
    for kw, status in ((dict(xform_count=1), "ARG"), (dict(src_tris=28), "ARG"), (dict(frame_ids=6), "ARG"),
                       (dict(have_levels=False), "ARG"), (dict(dst_first_tri=S.VERTEX_LIMIT // 3 - 37), "ARG")):
        args = dict(xform_count=2, src_tris=29, dst_first_tri=5, frame_ids=8)
        args.update(kw)
        with pytest.raises(S.Refused) as e:
            S.check(ITEMS, LEVELS, **args)
        assert e.value.status == status, kw
    assert S.check(ITEMS, LEVELS, 2, 29, S.VERTEX_LIMIT // 3 - 38, frame_ids=8) == 38
    many = np.tile(np.array([[0, 0, 0, 1, 0]], np.uint32), (32769, 1))
    with pytest.raises(S.Refused) as e:
        S.check(many, np.array([[0, 0, 65536]], np.uint32), 1, 65536, 0)
    assert e.value.status == "LIMIT"
    with pytest.raises(S.Refused) as e:  # exactly 2^31 is within the limit, and past the vertex limit all the same
        S.check(many[:32768], np.array([[0, 0, 65536]], np.uint32), 1, 65536, 0)
    assert e.value.status == "ARG"
