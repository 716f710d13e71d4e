"""CPU tests of prk_span_records' C-ABI boundary (no GPU compute) and of the
checker the GPU tests compare it with: tests/spanref.py, the Python
restatement of the reference's list walk, is held here to the oracle's own
walk (the list it leaves, word for word and link for link) and to the
oracle's frames (its spans drawn are the list drawn).  The spans the device
returns are checked on the GPU (tests/test_gpu_span_records.py).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import prk
import spanref
from prk import abi, scenes
from test_gpu_span_records import (HAND_HEIGHT, LIGHTS, NAN_WORDS, _soup, _sphere_scene, hand_batch, is_nan,
                                   same_spans)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_span_records_symbol_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        assert re.search(r"\bint prk_span_records\(prk_context \*ctx, const prk_edge \*records, "
                         r"const uint32_t \*counts,\s+uint32_t list_count, int32_t height,\s+"
                         r"prk_span \*spans, uint64_t capacity,\s+uint32_t \*span_counts, uint64_t \*total_out\);",
                         f.read())
    assert "prk_span_records" in prk.exported_symbols()
    assert hasattr(prk.lib(), "prk_span_records")
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT prk_span_records$", out, re.M)
    assert hasattr(prk.Renderer, "span_records")


def test_span_records_null_context():
    import ctypes as C
    L = prk.lib()
    rec = np.zeros((2, 27), np.uint32)
    spans = np.full((4, 25), 0xA5A5A5A5, np.uint32)
    sc = np.full(1, 77, np.uint32)
    cnt = np.array([2], np.uint32)
    total = C.c_uint64(99)
    assert L.prk_span_records(None, None, None, 0, 64, None, 0, None, None) == abi.PRK_ERR_ARG
    assert L.prk_span_records(None, rec.ctypes.data, cnt.ctypes.data, 1, 64, spans.ctypes.data, 4, sc.ctypes.data,
                              C.byref(total)) == abi.PRK_ERR_ARG
    assert (spans == 0xA5A5A5A5).all() and (sc == 77).all() and total.value == 99  # nothing written


def test_nan_rule_of_the_gpu_tests():
    """same_spans: a NaN passes for an expected NaN in the MinColor /
    MinNormal words only; every other word must be equal."""
    a = np.zeros((2, 25), np.uint32)
    b = a.copy()
    a[1, 9], b[1, 9] = 0xFFC00000, 0x7FC00001  # Left.MinNormal[0], both NaNs: allowed
    a[0, 17], b[0, 17] = 0xFFC00000, 0x7FC00000  # Right.MinColor[0]
    same_spans(b, a, "nan for nan")
    b[0, 10] = 0x7FC00000  # a NaN the reference does not have
    with pytest.raises(AssertionError):
        same_spans(b, a, "nan for number")
    b[0, 10], b[1, 9] = 0, 0x3F800000  # a number for the reference's NaN
    with pytest.raises(AssertionError):
        same_spans(b, a, "number for nan")
    b[1, 9], b[1, 13] = 0x7FC00000, 1  # an unequal number
    with pytest.raises(AssertionError):
        same_spans(b, a, "unequal")
    for word in (3, 12, 24):  # Left.UMin, Right.XMin, Row: NaNs there must be the same NaN
        b[1, 13] = 0
        a2, b2 = a.copy(), b.copy()
        a2[0, word], b2[0, word] = 0xFFC00000, 0x7FC00000
        with pytest.raises(AssertionError):
            same_spans(b2, a2, "no allowance")
    assert sorted(NAN_WORDS) == list(range(5, 12)) + list(range(17, 24))


def _held_to_the_oracle(words, height, label):
    spans, adv, nxt = spanref.walk(words, height)
    ow, on = O.advance_edges(words, height)
    assert np.array_equal(adv, ow), (label, np.nonzero((adv != ow).any(1))[0][:5])
    assert np.array_equal(nxt, on), (label, np.nonzero(nxt != on)[0][:5])
    return spans


def test_checker_leaves_the_oracles_lists_hand_made():
    words, counts = hand_batch()
    total, o = 0, 0
    for n in counts.tolist():
        if n:
            spans = _held_to_the_oracle(words[o:o + n], HAND_HEIGHT, "hand list at %d" % o)
            assert not is_nan(spans).any()
            total += spans.shape[0]
        o += n
    bs, bc, _, _ = spanref.walk_batch(words, counts, HAND_HEIGHT)
    assert bs.shape[0] == total == int(bc.sum()) and total > 0


def test_checker_spans_draw_the_soup_object():
    """A 24-triangle object: the list spanref leaves is the oracle's, and its
    spans drawn (FillLineOptimized on each) are the list drawn."""
    s = scenes.random_soup(24, 96, 64, radius=30, seed=41, textured=True)
    words = O.fill_edge_table_words(s, 0, 24, setup=3)
    assert words.shape[0] > 30
    spans = _held_to_the_oracle(words, s.height, "soup object")
    assert spans.shape[0] > 100 and not is_nan(spans).any()
    a = O.render_spans(s, spans, semantics=abi.PRK_SEM_AVX)
    b = O.render_edges(s, words, semantics=abi.PRK_SEM_AVX)
    assert (b[0] != scenes.CLEAR_COLOR).any()
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[0], b[0])


@pytest.mark.parametrize("height", [256, 128])
def test_checker_leaves_the_oracles_list_sphere(height):
    s = _sphere_scene()
    words = O.fill_edge_table_words(s, 0, s.tri_count, setup=3)
    assert words.shape[0] == 2072
    spans = _held_to_the_oracle(words, height, "sphere")
    assert spans.shape[0] > 1000 and not is_nan(spans).any()


def test_soup_seed_leaves_a_part_filled_last_piece():
    """The GPU soup batches: their span totals, by the oracle's records and
    spanref alone, are no multiple of 4 (the packed output's last 16-byte
    piece is part filled), and the Phong + Bitmap setup leaves no NaN in the
    words the allowance covers."""
    s = _soup()
    s.lights, s.ambient = LIGHTS[1]
    for per in (1, 5, 60):
        ws = [O.fill_edge_table_words(s, t, min(per, s.tri_count - t), setup=3) for t in range(0, s.tri_count, per)]
        words, counts = np.concatenate(ws), np.array([w.shape[0] for w in ws], np.uint32)
        for height in (192, 96):
            spans, sc, _, _ = spanref.walk_batch(words, counts, height)
            assert spans.shape[0] % 4 != 0 and spans.shape[0] == int(sc.sum()), (per, height, spans.shape[0])
            assert not is_nan(spans[:, NAN_WORDS]).any()
        assert spanref.walk_batch(words, counts, 0)[0].shape[0] == 0


@pytest.mark.skipif(os.environ.get("PRK_EXPECT_GPU") == "1", reason="GPU box")
def test_span_records_fail_loudly_without_gpu():
    """As the other compute calls (test_abi.py): no CPU fallback, the binding
    raises PRK_ERR_DEVICE."""
    if prk.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(prk.PrkError) as e:
        prk.Renderer().span_records(hand_batch()[0], hand_batch()[1], 64)
    assert e.value.code == abi.PRK_ERR_DEVICE
