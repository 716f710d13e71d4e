"""CPU tests: every restatement against frames drawn by the reference itself.

tests/golden/ref/*.npz hold what the reference's own FillEdgeTable, DrawModel*
and ConstructSphere produced (tools/make_ref_golden.py, built by
oracle/ref/build_ref.py; MANIFEST.json records the reference's hashes, the
compiler and flags, the pins of the absent headers, the one patch and, per
case, the entry point called).  oracle/prk_oracle.c, tests/pyref.py, the AVX2
baseline and the host edge-record code of libprk_hip.so must reproduce them bit
for bit: z as uint32, winners and colours equal, no tolerance.

Where this machine has the reference and build() made the driver under
oracle/_ref/, fresh scenes are drawn live and one fixture is regenerated;
without it only those two kinds of check cannot run.
"""
import json
import os
import sys

import numpy as np
import pytest

import oracle as O
import prk
import pyref
from prk import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle", "ref")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden  # noqa: E402
import make_ref_golden  # noqa: E402
import ref_run  # noqa: E402

REF = os.path.join(ROOT, "tests", "golden", "ref")
with open(os.path.join(REF, "MANIFEST.json")) as _f:
    MANIFEST = json.load(_f)
CASES = sorted(MANIFEST["cases"])
HAVE_DRIVER = ref_run.driver() is not None and ref_run.driver(patches=("P3",)) is not None
needs_driver = pytest.mark.skipif(not HAVE_DRIVER, reason="no reference on this machine: oracle/_ref/ holds no driver")


def load(name):
    s, sem, phong, d = make_golden.load(os.path.join(REF, name + ".npz"))
    return s, sem, phong, int(d["tris_per_object"]), d


def assert_same(got, d, what):
    col, z, win = got[:3]
    nz = int((z.view(np.uint32) != d["z"].view(np.uint32)).sum())
    nw = int((win != d["winners"]).sum())
    nc = int((col != d["color"]).sum())
    assert (nz, nw, nc) == (0, 0, 0), "%s differs from the reference: z %d, winners %d, colours %d pixels" % (
        what, nz, nw, nc)


def test_manifest_records_the_recipe():
    import build_ref
    assert MANIFEST["reference"]["sha256"] == build_ref.HASHES
    assert MANIFEST["flags"] == build_ref.FLAGS and "-ffp-contract=off" in MANIFEST["flags"]
    assert MANIFEST["pins"] == build_ref.PINS
    assert set(MANIFEST["patches"]) == set(build_ref.PATCHES) == {"P3"}
    assert len(CASES) >= 40
    for name in CASES:
        c = MANIFEST["cases"][name]
        assert os.path.exists(os.path.join(REF, name + ".npz")), name
        assert c["undefined_pixels"] == 0 and c["covered"] > 0, name
        assert set(c["patches"]) <= {"P3"} and c["entry_point"].startswith("FillEdgeTable + "), name
        assert c["unpatched_reference"] in ("same", "crashes", "differs"), name
        assert (c["patches"] == []) == (c["unpatched_reference"] == "same"), name
        assert os.path.getsize(os.path.join(REF, name + ".npz")) <= 128 * 1024, name
    # every committed fixture is in the manifest
    on_disk = {f[:-4] for f in os.listdir(REF) if f.endswith(".npz")}
    assert on_disk == set(CASES) | {"construct_sphere"}
    # every way of drawing, per triangle and as whole objects
    ways = {(c["entry_point"], c["triangles_per_object"] > 1) for c in MANIFEST["cases"].values()}
    for entry in ("DrawModelOptimized(RenderQueue)", "DrawModelOptimized(single thread)", "DrawModel"):
        assert ("FillEdgeTable + " + entry, False) in ways and ("FillEdgeTable + " + entry, True) in ways
    scalar = {(c["phong"], c["textured"]) for c in MANIFEST["cases"].values() if c["entry_point"].endswith("+ DrawModel")}
    assert scalar == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("name", CASES)
def test_oracle_draws_the_reference_frame(name):
    s, sem, phong, tpo, d = load(name)
    assert_same(O.render(s, semantics=sem, phong=phong, tris_per_object=tpo), d, "oracle")


# pyref draws one triangle per object, a pixel at a time: the per-triangle
# fixtures of a few hundred small triangles (what tests/test_oracle.py runs
# through it), not the two 256x256 triangles and the 2208-triangle sphere.
PYREF = [n for n in CASES if MANIFEST["cases"][n]["triangles_per_object"] == 1
         and MANIFEST["cases"][n]["triangles"] <= 450 and MANIFEST["cases"][n]["frame"][0] <= 128]


@pytest.mark.parametrize("name", PYREF)
def test_pyref_draws_the_reference_frame(name):
    s, sem, phong, _, d = load(name)
    assert_same(pyref.render(s, sem, phong), d, "pyref")


def test_pyref_covers_every_way_of_drawing():
    ways = {MANIFEST["cases"][n]["entry_point"] for n in PYREF}
    assert len(ways) == 4 and len(PYREF) >= 20


AVX = [n for n in CASES if MANIFEST["cases"][n]["entry_point"].endswith(("(RenderQueue)", "Lines"))]


@pytest.mark.parametrize("name", AVX)
def test_avx2_baseline_draws_the_reference_frame(name):
    if O.cpu_lib() is None:
        pytest.skip("host has no AVX2")
    s, sem, phong, tpo, d = load(name)
    # (the two work-queue schedules on one thread: with more, which of two
    # equal-z fragments runs first is a race, as in the reference's own queue;
    # oracle/prk_cpu_avx.c says so)
    for cpu, threads in (("banded", 3), ("rows", 1), ("queue", 1)):
        assert_same(O.render(s, semantics=sem, phong=phong, tris_per_object=tpo, threads=threads, cpu=cpu), d,
                    "AVX2 baseline (%s)" % cpu)


EDGE_CASES = [n for n in CASES if MANIFEST["cases"][n]["edge_info"]]


def test_edge_info_fixtures_present():
    sizes = sorted(MANIFEST["cases"][n]["triangles_per_object"] for n in EDGE_CASES)
    assert sizes == [1, 5, 40]


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_tables_equal_the_reference_edge_info(name):
    """FillEdgeTable's records of the fixture's first object, every non-pointer
    field as the reference wrote it (fresh, zeroed EdgeMemory) and Next null:
    the oracle's edge table and prk_fill_edge_records (csrc/prk_edge_records.cpp)."""
    s, sem, phong, tpo, d = load(name)
    want = d["edges"]
    assert want.shape[0] >= 3 and want.shape[1] == 27 and (d["edges_next"] == -1).all()
    setup = (abi.PRK_SETUP_PHONG if phong else 0) | (abi.PRK_SETUP_BITMAP if s.texture is not None else 0)
    got = O.fill_edge_table_words(s, 0, tpo, phong=phong, semantics=sem)
    assert got.shape == want.shape and (got == want).all(), "oracle edge table"
    o = s.subset(0, tpo)
    mem, n = prk.fill_edge_records(o.vertices, o.colors, o.normals, o.uvs, o.P, o.prk_transform(), o.prk_lights(), setup)
    words, nxt = prk.edge_record_words(mem, n)
    assert n == want.shape[0] and (words == want).all() and (nxt == -1).all(), "prk_fill_edge_records"


def test_construct_sphere_equals_the_reference():
    d = np.load(os.path.join(REF, "construct_sphere.npz"))
    got = prk.construct_sphere()
    for a, key in zip(got, ("vertices", "colors", "normals", "uvs")):
        assert a.shape == d[key].shape and (a.view(np.uint32) == d[key].view(np.uint32)).all(), key


OLD = sorted(f[:-4] for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.endswith(".npz"))


@pytest.mark.parametrize("name", OLD)
def test_old_goldens_equal_their_redrawn_copies(name):
    """tests/golden/*.npz (drawn by the oracle) against the same scene drawn by
    the reference, array for array: inputs and frame."""
    if name in MANIFEST["left_out"]:
        assert not os.path.exists(os.path.join(REF, name + ".npz"))
        return  # the manifest says why the reference cannot draw this scene defined
    old = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    new = np.load(os.path.join(REF, name + ".npz"))
    for key in ("width", "height", "vertices", "colors", "normals", "uvs", "P", "transform", "light_p", "light_i",
                "ambient", "texels", "tex_wh", "semantics", "phong", "winners", "color"):
        assert np.array_equal(old[key], new[key]), key
    assert (old["z"].view(np.uint32) == new["z"].view(np.uint32)).all()


def test_old_goldens_redrawn_or_accounted_for():
    assert len(OLD) == 8 and set(MANIFEST["left_out"]) == {"soup_phongtex_128x96"}
    assert all((n in CASES) != (n in MANIFEST["left_out"]) for n in OLD)


# ---- with the reference at hand ------------------------------------------------
LIVE = [("DrawModelOptimized(RenderQueue)", True, True), ("DrawModelOptimized(single thread)", True, True),
        ("DrawModel", False, False), ("DrawModel", True, False)]


@needs_driver
@pytest.mark.parametrize("seed", [901, 902, 903])
@pytest.mark.parametrize("entry,phong,textured", LIVE)
def test_live_reference_equals_oracle_per_triangle(entry, phong, textured, seed):
    s = scenes.random_soup(300, 128, 96, radius=12, seed=seed, textured=textured, tex_size=32,
                           lights=scenes.LIGHTS_TWO, ambient=scenes.AMBIENT_TWO)
    col, z, win, info = ref_run.render(s, entry, phong, patches=("P3",))
    assert info["undefined_pixels"] == 0
    sem = ref_run.ENTRY_POINTS[entry][1]
    assert_same(O.render(s, semantics=sem, phong=phong), dict(color=col, z=z, winners=win), "oracle")


@needs_driver
@pytest.mark.parametrize("seed", [912, 913, 916])
@pytest.mark.parametrize("entry,phong,textured", LIVE)
def test_live_reference_equals_oracle_five_triangle_objects(entry, phong, textured, seed):
    """300 triangles as 60 objects of 5 whose triangles share rows (the
    reference dereferences a list that empties between two triangles: of the
    seeds from 911 on, these are the first three it survives)."""
    s = make_ref_golden.clustered_objects(60, 5, 128, 96, seed, radius=12.0, spread=2.0, textured=textured)
    try:
        col, z, win, info = ref_run.render(s, entry, phong, 5, patches=("P3",))
    except ref_run.ReferenceFailed as e:
        pytest.fail("the reference does not survive this scene (%s): pick another seed" % e)
    assert info["undefined_pixels"] == 0
    sem = ref_run.ENTRY_POINTS[entry][1]
    assert_same(O.render(s, semantics=sem, phong=phong, tris_per_object=5), dict(color=col, z=z, winners=win), "oracle")


@needs_driver
@pytest.mark.parametrize("name", ["queue_objects5", "scalar_clipped"])
def test_regenerating_a_fixture_reproduces_it(name):
    """The committed arrays are what the recipe draws today: one fixture the P3
    build drew (with its edge_info) and one the unpatched reference drew."""
    got, doc = make_ref_golden.generate(name, make_ref_golden.cases()[name])
    d = np.load(os.path.join(REF, name + ".npz"))
    assert set(got) == set(d.files)
    for key in d.files:
        a, b = np.asarray(got[key]), d[key]
        assert a.shape == b.shape and a.tobytes() == np.asarray(b, a.dtype).tobytes(), key
    assert doc == MANIFEST["cases"][name]
