"""GPU tests: the HIP path against frames drawn by the reference itself.

Reads only tests/golden/ref/ (tools/make_ref_golden.py; MANIFEST.json says how
each frame was made): never the reference, its driver or the oracle.
prk.render_scene on every fixture scene must give the reference's z (as
uint32), winners and colours exactly, per triangle and as whole objects; the
whole-object fixtures also under each forced object walk.  Record mode's edge
words are host code (prk_fill_edge_records) and are checked against the
reference's edge_info in tests/test_ref_parity.py.
"""
import json
import os
import sys

import numpy as np
import pytest

import prk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import load  # noqa: E402

pytestmark = pytest.mark.gpu

REF = os.path.join(ROOT, "tests", "golden", "ref")
with open(os.path.join(REF, "MANIFEST.json")) as _f:
    CASES = json.load(_f)["cases"]
OBJECTS = sorted(n for n in CASES if CASES[n]["triangles_per_object"] > 1)


def check(name):
    s, sem, phong, d = load(os.path.join(REF, name + ".npz"))
    tpo = int(d["tris_per_object"])
    col, z, win, _ = prk.render_scene(s, semantics=sem, phong=phong, tris_per_object=tpo)
    nz = int((z.view(np.uint32) != d["z"].view(np.uint32)).sum())
    nw = int((win != d["winners"]).sum())
    nc = int((col != d["color"]).sum())
    assert (nz, nw, nc) == (0, 0, 0), "%s (%s) differs from the reference: z %d, winners %d, colours %d pixels" % (
        name, CASES[name]["entry_point"], nz, nw, nc)


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_draws_the_reference_frame(gpu, name):
    check(name)


def test_whole_object_fixtures_cover_every_semantics():
    ways = {CASES[n]["entry_point"].split(" + ")[1] for n in OBJECTS}
    assert {"DrawModelOptimized(RenderQueue)", "DrawModelOptimized(single thread)", "DrawModel"} <= ways
    assert {CASES[n]["triangles_per_object"] for n in OBJECTS} >= {5, 16, 40, 2208}


@pytest.mark.parametrize("path", ["big", "bigmem", "wave"])
@pytest.mark.parametrize("name", OBJECTS)
def test_gpu_draws_the_reference_frame_every_walk(gpu, name, path, monkeypatch):
    """The whole-object fixtures through the huge-object walk (forced, list in
    LDS and in memory) and the one-wave walk (forced), as
    test_degenerate_geometry_every_walk switches between them; the default
    walks are test_gpu_draws_the_reference_frame."""
    if path in ("big", "bigmem"):
        monkeypatch.setenv("PRK_OBJ_BIG_MIN", "0")
        monkeypatch.setenv("PRK_OBJ_ROWS", "0")
        monkeypatch.setenv("PRK_OBJ_HUGE_EDGES", "100")
        monkeypatch.setenv("PRK_OBJ_LDSWALK", "1" if path == "big" else "0")
    else:
        monkeypatch.setenv("PRK_OBJ_BIG_MIN", "0")
        monkeypatch.setenv("PRK_OBJ_ROWS", "0")
        monkeypatch.setenv("PRK_OBJ_BIG", "0")
    check(name)
