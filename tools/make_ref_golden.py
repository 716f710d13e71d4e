"""Generate tests/golden/ref/*.npz — frames drawn by the reference itself.

Unlike tests/golden/*.npz (drawn by oracle/prk_oracle.c, tools/make_golden.py)
these come out of the reference's own code, built by oracle/ref/build_ref.py
into oracle/_ref/ and called by oracle/ref/ref_driver.cpp: FillEdgeTable and
one of DrawModelOptimized(RenderQueue, ...), the single-thread
DrawModelOptimized overload, DrawModelOptimizedLines and DrawModel.  They pin
the oracle, pyref, the AVX2 baseline and the HIP path to the reference
(tests/test_ref_parity.py, tests/test_gpu_ref_parity.py).  Same layout as
tools/make_golden.py (make_golden.load reads them), plus `entry`, `tris_per_object`
and, for some, `edges` / `edges_next` (edge_info after FillEdgeTable).

Every case is drawn by the unpatched reference and by the P3 build
(oracle/ref/build_ref.py PATCHES).  Where the unpatched one survives and both
agree the fixture is the unpatched frame; where it crashes, or survives with an
edge dropped from its list, the fixture is the P3 frame, and the manifest says
which (P3 is part of what is pinned).  A case with a pixel that depends on
memory the reference does not own (two arena fills differ) is refused: its
scene is changed or it is left out (LEFT_OUT, recorded in MANIFEST.json).
Bilinear filtering is this project's extension and has no reference.

usage: python tools/make_ref_golden.py [case ...]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cpu-renderer_amd", "oracle", os.path.join("oracle", "ref"), "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

from prk import scenes  # noqa: E402
import build_ref  # noqa: E402
import ref_run  # noqa: E402
import make_golden  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref")
QUEUE = "DrawModelOptimized(RenderQueue)"
SINGLE = "DrawModelOptimized(single thread)"
LINES = "DrawModelOptimizedLines"
SCALAR = "DrawModel"

# Cases that cannot be fixtures, and why (goes into the manifest).
LEFT_OUT = {
    "soup_phongtex_128x96": "the redrawn golden of that name: DrawModel reads texels at unmasked uv outside [0, 1] "
                            "(one pixel past each span's right end), i.e. memory around the texture; "
                            "scalar_phongtex_soup draws the same kind of scene with uvs kept inside the texture",
}


def inner_uvs(s, lo=0.45, hi=0.55):
    """The scene with its uvs squeezed into [lo, hi]: DrawModel samples without
    a uv mask, and what it extrapolates past a span's end must stay inside the
    texture for the frame to be defined."""
    s.uvs = (lo + (hi - lo) * s.uvs).astype(np.float32)
    return s


def clustered_objects(n_obj, k, W, H, seed, radius=18.0, spread=3.0, textured=True, tex_size=32):
    """n_obj objects of k triangles each whose triangles overlap in rows: the
    reference dereferences an empty active edge list, so an object it can draw
    has no row without an edge between its first and last.  Otherwise as
    scenes.random_soup."""
    s = scenes.random_soup(n_obj * k, W, H, radius=radius, seed=seed, textured=textured, tex_size=tex_size,
                           lights=scenes.LIGHTS_TWO, ambient=scenes.AMBIENT_TWO)
    rng = np.random.default_rng(seed + 1000)
    cam = s.transform
    centre = np.stack([rng.uniform(radius, W - radius, n_obj), rng.uniform(radius, H - radius, n_obj)], 1)
    c = np.repeat(centre, k, 0) + rng.uniform(-spread, spread, (n_obj * k, 2))
    off = rng.uniform(-radius, radius, (n_obj * k, 3, 2))
    p = c[:, None, :] + off
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    flip = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0
    p[flip, 1], p[flip, 2] = p[flip, 2].copy(), p[flip, 1].copy()
    z = s.vertices[:, 2].reshape(-1, 3).astype(np.float64)
    x, y = scenes._unproject(p[..., 0], p[..., 1], z, cam)
    s.vertices = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    s.name = "objects%dx%d_s%d" % (n_obj, k, seed)
    return s


def half_pixel_soup(n, W, H, seed):
    """Projected vertices exactly on .5 in x and y: screen points k + 0.5 at
    z = 0 under the default camera (D = 4, F = 1, M2P = W/2 a power of two)
    unproject and project back without rounding, so RoundR32ToS32 decides every
    row and span end on a tie."""
    rng = np.random.default_rng(seed)
    cam = scenes.default_camera(W, H)
    c = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    p = (c[:, None, :] + rng.integers(-14, 15, (n, 3, 2))).astype(np.float64) + 0.5
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    p = p[cz != 0]
    cz = cz[cz != 0]
    flip = cz > 0
    p[flip, 1], p[flip, 2] = p[flip, 2].copy(), p[flip, 1].copy()
    n = len(p)
    z = np.zeros((n, 3))
    x, y = scenes._unproject(p[..., 0], p[..., 1], z, cam)
    base = scenes.random_soup(n, W, H, seed=seed, tex_size=32)
    V = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    # the z-test needs depth: one constant per triangle keeps the projection exact only at z = 0, so
    # depth order comes from submission order here (equal z everywhere: the tie rules decide)
    return scenes.Scene(W, H, V, base.colors, base.normals, base.uvs, cam, scenes.LIGHTS_ONE, scenes.AMBIENT_ONE,
                        base.texture, name="half_pixel%d_s%d" % (n, seed))


def hostile_soup(seed, W=128, H=96, n=200):
    """tests/test_gpu_parity.py's _degenerate_soup in small: vertices on the
    camera plane, behind the camera and inside the near plane, zero-area and
    collinear triangles, with duplicates (equal z)."""
    s = scenes.with_ties(scenes.random_soup(n, W, H, radius=24, seed=seed, centroid_margin=20, tex_size=32), seed=seed)
    D = s.transform[0]
    v = s.vertices.reshape(-1, 3, 3).copy()
    rng = np.random.default_rng(seed)
    idx = rng.choice(len(v), 50, replace=False)
    v[idx[:10], 0, 2] = D
    v[idx[10:20], 1, 2] = D + 0.5
    v[idx[20:30], 2, 2] = D - 0.1
    v[idx[30:40], 1] = v[idx[30:40], 0]
    v[idx[40:50], 2] = v[idx[40:50], 0] + (v[idx[40:50], 1] - v[idx[40:50], 0]) * 0.5
    s.vertices = v.reshape(-1, 3).astype(np.float32)
    return s


def one_comb(n=40, W=128, H=96, seed=5):
    """One object of n tall slivers whose apexes share a row: 2n edges enter
    the active edge list on one row (the insertion order and its ties)."""
    return scenes.comb([(n, 6, 60, 90)], W, H, seed=seed, kink=0.0)


def soup(seed, textured=True, **kw):
    return scenes.random_soup(300, 128, 96, radius=12, seed=seed, textured=textured, tex_size=32,
                              lights=scenes.LIGHTS_TWO, ambient=scenes.AMBIENT_TWO, **kw)


def cases():
    """name -> (scene, entry point, phong, triangles per object, store edge_info)."""
    c = {}
    # the present goldens (tools/make_golden.py), scene for scene
    for name, s, sem, phong in make_golden.cases():
        c[name] = (s, SCALAR if sem == make_golden.abi.PRK_SEM_SCALAR else QUEUE, phong, 1, name == "c1_triangle_avx")
    # each way of drawing, per triangle
    for tag, entry in (("queue", QUEUE), ("single", SINGLE), ("lines", LINES)):
        c["%s_soup" % tag] = (soup(51), entry, True, 1, False)
    c["scalar_gouraud_soup"] = (soup(52, textured=False), SCALAR, False, 1, False)
    c["scalar_phong_soup"] = (soup(53, textured=False), SCALAR, True, 1, False)
    # (seeds 54, 57-59 leave 1 to 4 pixels that read outside the texture: refused, see generate())
    c["scalar_gouraudtex_soup"] = (inner_uvs(soup(56)), SCALAR, False, 1, False)
    c["scalar_phongtex_soup"] = (inner_uvs(soup(55)), SCALAR, True, 1, False)
    # whole objects: the sphere as ONE object, objects of 5 and 16 triangles
    sph = make_golden.sphere_scene(128, 128, True)
    for tag, entry in (("queue", QUEUE), ("single", SINGLE)):
        c["%s_sphere_one_object" % tag] = (sph, entry, True, sph.tri_count, False)
        c["%s_objects5" % tag] = (clustered_objects(12, 5, 128, 96, 61), entry, True, 5, tag == "queue")
        c["%s_objects16" % tag] = (clustered_objects(6, 16, 128, 96, 62), entry, True, 16, False)
    c["scalar_sphere_one_object"] = (make_golden.sphere_scene(128, 128, False), SCALAR, False, sph.tri_count, False)
    # (seed 63 has an object whose list empties between two of its triangles: the reference, P3 or not,
    # dereferences the empty list)
    c["scalar_objects5"] = (clustered_objects(12, 5, 128, 96, 65, textured=False), SCALAR, False, 5, False)
    c["scalar_objects16"] = (clustered_objects(6, 16, 128, 96, 64, textured=False), SCALAR, True, 16, False)
    # the pinned quirks
    for tag, entry in (("queue", QUEUE), ("single", SINGLE)):
        c["%s_slivers" % tag] = (scenes.slivers(120, 128, 96, seed=7), entry, True, 1, False)
        c["%s_ties" % tag] = (scenes.with_ties(soup(71, centroid_margin=-10), seed=3), entry, True, 1, False)
        c["%s_half_pixel" % tag] = (half_pixel_soup(150, 128, 96, 8), entry, True, 1, False)
        c["%s_clipped" % tag] = (scenes.random_soup(80, 96, 64, radius=60, seed=72, tex_size=32, centroid_margin=45,
                                                    z_range=(-3.5, 3.0)), entry, True, 1, False)
        c["%s_hostile" % tag] = (hostile_soup(73), entry, True, 1, False)
        c["%s_comb_one_object" % tag] = (one_comb(), entry, True, 40, tag == "queue")
    c["scalar_slivers"] = (scenes.slivers(120, 128, 96, seed=7, textured=False), SCALAR, False, 1, False)
    c["scalar_ties"] = (scenes.with_ties(soup(74, textured=False), seed=4), SCALAR, False, 1, False)
    c["scalar_half_pixel"] = (_untextured(half_pixel_soup(150, 128, 96, 9)), SCALAR, True, 1, False)
    c["scalar_clipped"] = (scenes.random_soup(80, 96, 64, radius=60, seed=75, textured=False, centroid_margin=45,
                                              z_range=(-3.5, 3.0)), SCALAR, False, 1, False)
    c["scalar_comb_one_object"] = (_untextured(one_comb()), SCALAR, False, 40, False)
    # zero lights (two lights: every soup above)
    nolight = scenes.random_soup(150, 128, 96, radius=14, seed=76, tex_size=32, lights=[], ambient=scenes.AMBIENT_TWO)
    c["queue_no_lights"] = (nolight, QUEUE, True, 1, False)
    c["scalar_no_lights"] = (_untextured(scenes.random_soup(150, 128, 96, radius=14, seed=77, lights=[],
                                                            ambient=scenes.AMBIENT_TWO)), SCALAR, False, 1, False)
    # texture shapes (every texture above is square): Width != Height, 24 x 40, through each entry point, and
    # for the queue path uv of exactly 0 and 1 over whole triangles (its mask keeps u == 1 and v == 1: the next
    # row's first texel and the guard row).  The scene of tests/texcases.py's case of that name (edges01 there
    # has pad columns; the driver's Pitch is 4 * Width).  DrawModel masks nothing, so its uvs stay inside the
    # texture as in scalar_phongtex_soup.
    def tex(recipe, seed):
        s = scenes.random_soup(200, 128, 96, radius=12.0, seed=seed, tex_size=8, lights=scenes.LIGHTS_TWO,
                               ambient=scenes.AMBIENT_TWO)
        return scenes.retexture(s, 24, 40, 24, recipe, seed)
    for tag, entry in (("queue", QUEUE), ("single", SINGLE)):
        c["%s_nonsquare" % tag] = (tex(("uniform", 0.0, 1.0), 81), entry, True, 1, False)
    # (of the seeds 82 to 99 with uvs in [0.35, 0.65], 93 is the one with no pixel read outside the texture)
    c["scalar_nonsquare"] = (inner_uvs(tex(("uniform", 0.0, 1.0), 93), 0.35, 0.65), SCALAR, True, 1, False)
    # (without pad columns the (1, 1) corner lies one texel past the guard row: those vertices go to (1, 0))
    e01 = tex(("edges01",), 85)
    e01.uvs[(e01.uvs[:, 0] == 1) & (e01.uvs[:, 1] == 1), 1] = 0
    c["queue_edges01"] = (e01, QUEUE, True, 1, False)
    return c


def _untextured(s):
    s.texture = None
    return s


def draw(s, entry, phong, tpo, edges):
    """(colour, z, winners, info, patches used, what the unpatched reference
    did).  The unpatched reference's frame where it survives the scene and the
    P3 build draws the same ("same"); else the P3 build's: the unpatched one
    "crashes", or it "differs" (it survives, having dropped an edge from its
    list at a first-pair swap; info["unpatched_differs"] counts the pixels)."""
    p3 = ref_run.render(s, entry, phong, tpo, dump_edges=edges, patches=("P3",))
    try:
        plain = ref_run.render(s, entry, phong, tpo, dump_edges=edges)
    except ref_run.ReferenceFailed:
        return p3 + (["P3"], "crashes")
    differs = sum(int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(plain[:2], p3[:2]))
    if differs:
        p3[3]["unpatched_differs"] = differs
        return p3 + (["P3"], "differs")
    return plain + ([], "same")


def arrays(s, entry, phong, tpo, col, z, win, info):
    tex = s.texture
    d = dict(
        width=s.width, height=s.height, vertices=s.vertices, colors=s.colors, normals=s.normals, uvs=s.uvs,
        P=np.array(s.P, np.float32), transform=np.array(s.transform, np.float32),
        light_p=np.array([l[0] for l in s.lights], np.float32).reshape(-1, 3),
        light_i=np.array([l[1] for l in s.lights], np.float32).reshape(-1, 4),
        ambient=np.array(s.ambient, np.float32),
        texels=tex.texels if tex is not None else np.zeros((0, 0), np.uint32),
        tex_wh=np.array([tex.width, tex.height] if tex is not None else [0, 0], np.int32),
        semantics=ref_run.ENTRY_POINTS[entry][1], phong=int(phong), color=col, z=z, winners=win,
        entry=entry, tris_per_object=tpo)
    if "edges" in info:
        d["edges"] = info["edges"]
        d["edges_next"] = info["next"]
    return d


def generate(name, case):
    """The fixture's arrays and its manifest entry."""
    s, entry, phong, tpo, edges = case
    col, z, win, info, patches, unpatched = draw(s, entry, phong, tpo, edges)
    if info["undefined_pixels"]:
        raise ValueError("%s: %d pixels depend on memory the reference does not own" % (name, info["undefined_pixels"]))
    entry_doc = dict(entry_point="FillEdgeTable + " + entry, phong=bool(phong), textured=s.texture is not None,
                     triangles=s.tri_count, triangles_per_object=tpo, frame=[s.width, s.height], patches=patches,
                     unpatched_reference=unpatched, unpatched_differing_values=info.get("unpatched_differs", 0),
                     objects_without_edges=info["objects_without_edges"], undefined_pixels=0,
                     covered=int((win >= 0).sum()), edge_info="edges" in info)
    return arrays(s, entry, phong, tpo, col, z, win, info), entry_doc


def sphere_arrays():
    V, C, N, UV = ref_run.construct_sphere()
    return dict(vertices=V, colors=C, normals=N, uvs=UV)


def main(argv):
    if not build_ref.build_all()[0]:
        raise SystemExit("no reference: nothing to draw")
    os.makedirs(OUT, exist_ok=True)
    all_cases = cases()
    names = argv or list(all_cases)
    path = os.path.join(OUT, "MANIFEST.json")
    manifest = json.load(open(path)) if argv and os.path.exists(path) else {}
    manifest.update(reference=dict(repository="MacSpain/cpu-renderer", sha256=build_ref.HASHES),
                    compiler=build_ref.compiler_version(), flags=build_ref.FLAGS, pins=build_ref.PINS,
                    lane_rewrite=dict(regex=build_ref.LANE.pattern, sites=build_ref.LANE_SITES),
                    patches={k: dict(lines=v["lines"], appended=v["append"], what=v["what"])
                             for k, v in build_ref.PATCHES.items()},
                    undefined_memory_guard="every case drawn twice, the arena around the texture filled with 0x5A and "
                                           "0xA5 (guard row zero in both); fixtures have no pixel that differs",
                    winners="per submission: pixels whose z or colour changed (Appendix C.6)",
                    left_out=LEFT_OUT)
    manifest.setdefault("cases", {})
    for name in names:
        if name in LEFT_OUT:
            try:
                generate(name, all_cases[name])
                raise SystemExit("%s is listed as left out but is drawable" % name)
            except ValueError as e:
                print("left out: %s" % e)
            continue
        d, doc = generate(name, all_cases[name])
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
        manifest["cases"][name] = doc
        print("%-28s %-34s tpo=%-5d covered=%-6d patches=%s no_edges=%d %d KB" % (
            name, doc["entry_point"][16:], doc["triangles_per_object"], doc["covered"], doc["patches"],
            doc["objects_without_edges"], os.path.getsize(os.path.join(OUT, name + ".npz")) // 1024))
    if not argv:
        np.savez_compressed(os.path.join(OUT, "construct_sphere.npz"), **sphere_arrays())
        manifest["construct_sphere"] = dict(entry_point="ConstructSphere", patches=[])
    manifest["cases"] = dict(sorted(manifest["cases"].items()))
    with open(path, "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
