"""CPU tests of the target-layer calls' boundary (no GPU compute): the ctypes
mirror against include/prk.h, the exported symbols, NULL contexts, and the
numpy restatement of the definition (tests/layerref.py) against the oracle:
two frames drawn from the same clear, one of a frame's first draws and one of
the rest, merge per pixel into exactly the frame of all the draws -- under the
semantics' own tie rule, and not under the other one.  What the device pass
computes is checked on the GPU (tests/test_gpu_target_layers.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import layerref
import oracle as O
import prk
from prk import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prk_layer_alloc", "prk_layer_wrap_device", "prk_layer_from_target", "prk_target_from_layer",
         "prk_layer_download", "prk_layer_info", "prk_layer_destroy")
METHODS = ("layer_alloc", "layer_wrap", "layer_from_target", "target_from_layer", "layer_download", "layer_info",
           "layer_destroy")

CTYPES = {"prk_context *": C.c_void_p, "int32_t": C.c_int32, "const void *": C.c_void_p, "const float *": C.c_void_p,
          "uint32_t *": C.c_void_p, "float *": C.c_void_p, "int32_t *": C.POINTER(C.c_int32)}

SPLIT = 147  # the first frame draws triangles [0, 147), the second the rest
# (semantics, phong, the rule that reproduces the whole frame)
PAIRS = [(abi.PRK_SEM_AVX, True, layerref.GREATER), (abi.PRK_SEM_SCALAR, True, layerref.GREATER),
         (abi.PRK_SEM_SCALAR, False, layerref.GREATER), (abi.PRK_SEM_AVX_ST, True, layerref.GREATER_EQUAL)]
CONTROL = (abi.PRK_SEM_AVX_ST, True, layerref.GREATER)  # the other tie rule: must differ


def split_scene():
    return scenes.with_ties(scenes.random_soup(300, 72, 40, radius=14, seed=5), 0.5, 3)


def header():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_seven_names_are_exported():
    assert sorted(abi.TARGET_LAYER_SIGS) == sorted(NAMES)
    for name in NAMES:
        assert name in prk.exported_symbols(), name
    m = re.search(r"enum prk_merge \{([^}]*)\}", header())
    assert m
    values = dict(re.findall(r"(PRK_MERGE_\w+) = (\d+)", m.group(1)))
    assert values == {"PRK_MERGE_COPY": "0", "PRK_MERGE_GREATER": "1", "PRK_MERGE_GREATER_EQUAL": "2"}
    for k, v in values.items():
        assert getattr(abi, k) == int(v)
    assert (layerref.COPY, layerref.GREATER, layerref.GREATER_EQUAL) == (0, 1, 2)


@pytest.mark.parametrize("name", NAMES)
def test_signature_declared_exported_bound(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header(), re.M | re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    types = [re.match(r"(.*?[ *])\w+$", p).group(1).strip() for p in params]
    assert [CTYPES[t] for t in types] == abi.TARGET_LAYER_SIGS[name], (name, types)
    f = getattr(prk.lib(), name)
    assert f.restype is C.c_int and list(f.argtypes) == abi.TARGET_LAYER_SIGS[name]
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT %s$" % name, out, re.M)


def test_python_surface_and_null_context():
    for m in METHODS:
        assert hasattr(prk.Renderer, m), m
    L = prk.lib()
    h = C.c_int32(5)
    buf = np.full((4, 4), 9, np.uint32)
    zbuf = np.full((4, 4), 9, np.float32)
    assert L.prk_layer_alloc(None, 4, 4, C.byref(h)) == abi.PRK_ERR_ARG and h.value == 5
    assert L.prk_layer_wrap_device(None, buf.ctypes.data, 16, zbuf.ctypes.data, 4, 4, C.byref(h)) == abi.PRK_ERR_ARG
    assert h.value == 5
    assert L.prk_layer_from_target(None, 0, 0, 0, 4, 4, 0, 0) == abi.PRK_ERR_ARG
    for rule in (abi.PRK_MERGE_COPY, abi.PRK_MERGE_GREATER, abi.PRK_MERGE_GREATER_EQUAL):
        assert L.prk_target_from_layer(None, 0, 0, 0, 4, 4, 0, 0, rule) == abi.PRK_ERR_ARG
    assert L.prk_layer_download(None, 0, buf.ctypes.data, 16, zbuf.ctypes.data) == abi.PRK_ERR_ARG
    assert (buf == 9).all() and (zbuf == 9).all()
    assert L.prk_layer_info(None, 0, C.byref(h), None, None, None) == abi.PRK_ERR_ARG and h.value == 5
    assert L.prk_layer_destroy(None, 0) == abi.PRK_ERR_ARG


# ---- layerref itself ---------------------------------------------------------------------------------------------------
def f32_words(*values):
    return np.array(values, np.float32).view(np.uint32)


def test_layerref_comparison_is_ieee_on_the_words():
    nan, nan_neg, nan_payload = np.uint32(0x7FC00000), np.uint32(0xFFC00000), np.uint32(0x7F800001)
    one, = f32_words(1.0)
    for n in (nan, nan_neg, nan_payload):
        for rule in (layerref.GREATER, layerref.GREATER_EQUAL):
            assert not layerref.wins(np.array([n]), np.array([one]), rule)[0]
            assert not layerref.wins(np.array([one]), np.array([n]), rule)[0]
            assert not layerref.wins(np.array([n]), np.array([n]), rule)[0]
        assert layerref.wins(np.array([n]), np.array([one]), layerref.COPY)[0]
    pz, nz = f32_words(0.0, -0.0)
    assert pz != nz
    assert not layerref.wins(np.array([pz]), np.array([nz]), layerref.GREATER)[0]
    assert layerref.wins(np.array([pz]), np.array([nz]), layerref.GREATER_EQUAL)[0]
    assert layerref.wins(np.array([nz]), np.array([pz]), layerref.GREATER_EQUAL)[0]
    den, = np.array([1], np.uint32)  # the smallest denormal: above zero by value
    assert layerref.wins(np.array([den]), np.array([pz]), layerref.GREATER)[0]
    assert not layerref.wins(np.array([pz]), np.array([den]), layerref.GREATER_EQUAL)[0]


def test_layerref_rectangles():
    rng = np.random.default_rng(2)
    rnd = lambda shape: rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    band_c, band_z = rnd((8, 16)), f32_words(*rng.integers(-2, 3, 128)).reshape(8, 16)
    lay_c, lay_z = rnd((7, 9)), f32_words(*rng.integers(-2, 3, 63)).reshape(7, 9)
    # save: band rows 18..20 (row0 16), columns 3..6, to the layer at (5, 1)
    sc, sz = layerref.save(band_c, band_z, 16, (3, 18, 4, 3), lay_c, lay_z, (5, 1))
    assert np.array_equal(sc[1:4, 5:9], band_c[2:5, 3:7]) and np.array_equal(sz[1:4, 5:9], band_z[2:5, 3:7])
    keep = np.ones(lay_c.shape, bool)
    keep[1:4, 5:9] = False
    assert np.array_equal(sc[keep], lay_c[keep]) and np.array_equal(sz[keep], lay_z[keep]) and sc is not lay_c
    # merge: the layer's (2, 1, 5, 4) to the band at frame pixel (10, 19)
    for rule in (layerref.COPY, layerref.GREATER, layerref.GREATER_EQUAL):
        mc, mz = layerref.merge(band_c, band_z, 16, lay_c, lay_z, (2, 1, 5, 4), (10, 19), rule)
        keep = np.ones(band_c.shape, bool)
        keep[3:7, 10:15] = False
        assert np.array_equal(mc[keep], band_c[keep]) and np.array_equal(mz[keep], band_z[keep])
        s, d = lay_z[1:5, 2:7].view(np.float32), band_z[3:7, 10:15].view(np.float32)
        win = {layerref.COPY: np.ones(s.shape, bool), layerref.GREATER: s > d, layerref.GREATER_EQUAL: s >= d}[rule]
        assert win.any() and (rule == layerref.COPY or not win.all())
        assert np.array_equal(mc[3:7, 10:15], np.where(win, lay_c[1:5, 2:7], band_c[3:7, 10:15]))
        assert np.array_equal(mz[3:7, 10:15], np.where(win, lay_z[1:5, 2:7], band_z[3:7, 10:15]))
    for bad in ((3, 15, 4, 2), (3, 22, 4, 4), (14, 18, 4, 2)):  # a row above the band, one below, a column past W
        with pytest.raises(AssertionError):
            layerref.save(band_c, band_z, 16, bad, lay_c, lay_z)
    with pytest.raises(AssertionError):
        layerref.merge(band_c, band_z, 16, lay_c, lay_z, (6, 0, 4, 4), (0, 16), layerref.COPY)  # past the layer


# ---- the split-frame property, in the oracle -----------------------------------------------------------------------------
def halves(s, sem, phong, per):
    kw = dict(semantics=sem, phong=phong, tris_per_object=per, winners=False)
    whole = O.render(s, **kw)[:2]
    first = O.render(s.subset(0, SPLIT), **kw)[:2]
    second = O.render(s.subset(SPLIT, s.tri_count), **kw)[:2]
    return whole, first, second


def tie_pixels(first, second):
    """Pixels that both halves cover with the same z."""
    covered = layerref.words(first[1]) != layerref.words(np.float32(O.CLEAR_Z))
    return int((covered & (first[1] == second[1])).sum())


@pytest.mark.parametrize("per", [1, 7])
@pytest.mark.parametrize("sem,phong,rule", PAIRS)
def test_split_frame_merges_to_the_whole_frame(sem, phong, rule, per):
    assert SPLIT % per == 0  # (the split falls between objects)
    whole, first, second = halves(split_scene(), sem, phong, per)
    assert tie_pixels(first, second) >= 100
    mc, mz = layerref.merge_frames(first, second, rule)
    assert int((mc != whole[0]).sum()) == 0 and int((mz != layerref.words(whole[1])).sum()) == 0


@pytest.mark.parametrize("per", [1, 7])
def test_the_other_tie_rule_does_not(per):
    sem, phong, rule = CONTROL
    whole, first, second = halves(split_scene(), sem, phong, per)
    ties = tie_pixels(first, second)
    assert ties >= 100
    mc, mz = layerref.merge_frames(first, second, rule)
    differ = int((mc != whole[0]).sum())
    assert 0 < differ <= ties                               # colour: the later draw's, only where the halves tie
    assert int((mz != layerref.words(whole[1])).sum()) == 0  # (a tie's two z words are equal)
