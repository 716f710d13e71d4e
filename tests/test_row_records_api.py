"""CPU tests of prk_row_records' / prk_draw_rows' C-ABI boundary (no GPU
compute) and of the checker the GPU tests compare the device with:
tests/rowref.py, the restatement of DrawModelOptimizedLines' row loop, is held
here to tests/spanref.py (which test_span_records_api.py holds to the oracle):
its pairs, de-interleaved, are spanref's spans word for word, its EdgeCounts
the spans' per-row counts, and its rows the closed form of prk.h -- a row of
[YMin[0], min(max YMax, height)) is queued if and only if some edge of the
list has YMin <= row < YMax.  The records the device returns are checked on
the GPU (tests/test_gpu_row_records.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import prk
import rowref
import spanref
from prk import abi
from test_gpu_span_records import HAND_HEIGHT, LIGHTS, _soup, _sphere_scene, hand_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YMAX, YMIN = 0, 7


def closed_form_rows(words, counts, height):
    """Per list, the rows prk.h says are emitted."""
    i = np.ascontiguousarray(words, np.uint32).reshape(-1, 27).view(np.int32)
    out, e0 = [], 0
    for n in np.asarray(counts, np.int64).tolist():
        ymin, ymax = i[e0:e0 + n, YMIN], i[e0:e0 + n, YMAX]
        rows = []
        if n:
            for row in range(int(ymin[0]), min(int(ymax.max()), height)):
                if ((ymin <= row) & (row < ymax)).any():
                    rows.append(row)
        out.append(rows)
        e0 += n
    return out


def held_to_spanref(words, counts, height, label):
    rows, pairs, rc = rowref.walk_batch(words, counts, height)
    spans, sc, _, _ = spanref.walk_batch(words, counts, height)
    assert rows.dtype == np.int32 and pairs.dtype == np.uint32 and rc.dtype == np.uint32
    assert np.array_equal(rowref.as_spans(rows, pairs), spans), label  # every word, NaN payloads included
    want = closed_form_rows(words, counts, height)
    assert rc.tolist() == [len(w) for w in want], label
    assert rows[:, 0].tolist() == [r for w in want for r in w], label
    # EdgeCount: the list's spans on that row
    r0 = s0 = 0
    for o, w in enumerate(want):
        r1, s1 = r0 + len(w), s0 + int(sc[o])
        per_row = np.bincount(spans[s0:s1, 24].view(np.int32), minlength=height + 1)
        assert rows[r0:r1, 1].tolist() == per_row[w].tolist(), (label, o)
        assert int(rows[r0:r1, 1].sum()) == int(sc[o]), (label, o)
        r0, s0 = r1, s1
    return rows, pairs, rc


def test_checker_is_spanref_regrouped_hand_made():
    words, counts = hand_batch()
    rows, pairs, rc = held_to_spanref(words, counts, HAND_HEIGHT, "hand")
    assert pairs.shape[0] > 0 and (rows[:, 1] == 0).any() and (rows[:, 1] == 2).any()
    for height in (0, 7, 25):
        held_to_spanref(words, counts, height, "hand height %d" % height)


def test_checker_is_spanref_regrouped_soup():
    s = _soup()
    s.lights, s.ambient = LIGHTS[1]
    per = 60
    ws = [O.fill_edge_table_words(s, t, min(per, s.tri_count - t), setup=3) for t in range(0, s.tri_count, per)]
    words, counts = np.concatenate(ws), np.array([w.shape[0] for w in ws], np.uint32)
    for height in (192, 96, 0):
        rows, pairs, _ = held_to_spanref(words, counts, height, "soup height %d" % height)
        assert (height == 0) == (rows.shape[0] == 0)


def test_checker_is_spanref_regrouped_sphere():
    s = _sphere_scene()
    words = O.fill_edge_table_words(s, 0, s.tri_count, setup=3)
    assert words.shape[0] == 2072
    rows, pairs, rc = held_to_spanref(words, [words.shape[0]], 256, "sphere")
    assert rc.tolist() == [rows.shape[0]] and rows[:, 1].max() > 8 and pairs.shape[0] > 1000


def test_checker_refuses_a_row_over_the_reference_array():
    from test_gpu_span_records import edge
    crowd = np.array([edge(3, 4, float(2002 - i), 0.0, i & 1) for i in range(2002)], np.uint32)
    rows, pairs, rc = rowref.walk_batch(crowd[:2000], [2000], 64)
    assert rows.tolist() == [[3, 1000]] and pairs.shape[0] == 1000 and rc.tolist() == [1]
    with pytest.raises(OverflowError):
        rowref.walk_batch(crowd, [2002], 64)


def test_pair_word_order_matches_the_binding():
    assert [12 * h + k for h, k in rowref.PAIR_WORDS] == abi.ROW_PAIR_SPAN_WORD
    assert sorted(abi.ROW_PAIR_SPAN_WORD) == list(range(24))


def test_row_struct_layouts_match_header():
    assert C.sizeof(abi.PrkRowPair) == 96 and C.sizeof(abi.PrkRow) == 8
    assert (abi.PrkRow.RowIndex.offset, abi.PrkRow.EdgeCount.offset) == (0, 4)
    names = ["LeftXMin", "RightXMin", "LeftZMin", "RightZMin", "LeftOneOverZMin", "RightOneOverZMin", "LeftUMin",
             "RightUMin", "LeftVMin", "RightVMin"]
    for k, n in enumerate(names):
        assert getattr(abi.PrkRowPair, n).offset == 4 * k, n
    assert abi.PrkRowPair.LeftMinColor.offset == 40 and abi.PrkRowPair.RightMinColor.offset == 56
    assert abi.PrkRowPair.LeftMinNormal.offset == 72 and abi.PrkRowPair.RightMinNormal.offset == 84
    # the header's own text: field order, and a compiler's view of sizes and offsets
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        src = f.read()
    m = re.search(r"typedef struct prk_row_pair \{(.*?)\} prk_row_pair;", src, re.S)
    fields = re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", m.group(1))
    assert fields == names + ["LeftMinColor", "RightMinColor", "LeftMinNormal", "RightMinNormal"]
    assert re.search(r"typedef struct prk_row \{ int32_t RowIndex; uint32_t EdgeCount; \} prk_row;", src)


def test_row_struct_sizes_by_the_compiler(tmp_path):
    c = tmp_path / "sz.c"
    c.write_text('#include <stddef.h>\n#include "prk.h"\n'
                 "_Static_assert(sizeof(prk_row_pair) == 96, \"pair\");\n"
                 "_Static_assert(sizeof(prk_row) == 8, \"row\");\n"
                 "_Static_assert(offsetof(prk_row_pair, LeftMinColor) == 40, \"lc\");\n"
                 "_Static_assert(offsetof(prk_row_pair, RightMinNormal) == 84, \"rn\");\n"
                 "_Static_assert(offsetof(prk_row, EdgeCount) == 4, \"ec\");\n")
    run = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_symbols_declared_exported_bound():
    assert {"prk_row_records", "prk_draw_rows"} <= set(prk.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    for n in ("prk_row_records", "prk_draw_rows"):
        assert hasattr(prk.lib(), n) and re.search(r"\bT %s$" % n, out, re.M), n
    assert hasattr(prk.Renderer, "row_records") and hasattr(prk.Renderer, "draw_rows")


def test_argument_errors_without_device():
    L = prk.lib()
    rec = np.zeros((2, 27), np.uint32)
    cnt = np.array([2], np.uint32)
    rows = np.full((4, 2), 0x5A5A5A5A, np.int32)
    pairs = np.full((4, 24), 0xA5A5A5A5, np.uint32)
    rc = np.full(1, 77, np.uint32)
    nr, npair = C.c_uint64(99), C.c_uint64(98)
    assert L.prk_row_records(None, None, None, 0, 64, None, 0, None, 0, None, None, None) == abi.PRK_ERR_ARG
    assert L.prk_row_records(None, rec.ctypes.data, cnt.ctypes.data, 1, 64, rows.ctypes.data, 4, pairs.ctypes.data, 4,
                             rc.ctypes.data, C.byref(nr), C.byref(npair)) == abi.PRK_ERR_ARG
    assert L.prk_draw_rows(None, rows.ctypes.data, 4, pairs.ctypes.data, 4, abi.PRK_SEM_AVX, 1, 0) == abi.PRK_ERR_ARG
    assert (rows == 0x5A5A5A5A).all() and (pairs == 0xA5A5A5A5).all() and (rc == 77).all()
    assert (nr.value, npair.value) == (99, 98)  # nothing written


@pytest.mark.skipif(os.environ.get("PRK_EXPECT_GPU") == "1", reason="GPU box")
def test_row_records_fail_loudly_without_gpu():
    """As the other compute calls: no CPU fallback, the binding raises
    PRK_ERR_DEVICE."""
    if prk.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(prk.PrkError) as e:
        prk.Renderer().row_records(hand_batch()[0], hand_batch()[1], 64)
    assert e.value.code == abi.PRK_ERR_DEVICE
