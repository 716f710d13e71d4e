"""Time frames drawn from edge_info records that stay on the device: one
prk_draw_records call of a handle's lists, one prk_draw_edge_lists call of the
same records from host memory, and the prk_draw_objects draw the records came
from -- all three in the same run -- and the making of the records:
prk_records_from_geometry against prk_edge_records.

Two scenes: ConstructSphere as one object (one list of its 2072 edges,
256x256) and C3b's geometry (1 M triangles, 4096x4096) as 16-triangle objects
(62,500 lists).

usage: python tools/time_record_handles.py [--tris N] [--reps K] [--case all|sphere|c3b] [--json OUT]
Per way and scene: `record_ms`, the host time of the recording call, and
`frame_ms`, prk_flush to the end of prk_synchronize; `stage_bytes`, the
pass's staging upload.  `make_ms`: the whole call that makes the records
(the handle is destroyed outside the timed part).  Medians of K repeats after
one warm-up, the ways taken in turn within every repeat.  Every way's frame is
compared with the object draw's (colour and z, bit for bit) once, before the
timing, and the handle's records with prk_edge_records'."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpu-renderer_amd"))
import numpy as np  # noqa: E402
import prk  # noqa: E402
from prk import abi, scenes  # noqa: E402


def sphere_scene():
    V, Cc, N, UV = prk.construct_sphere()
    base = scenes.random_soup(1, 256, 256, seed=0)
    return scenes.Scene(256, 256, V.copy(), Cc.copy(), N.copy(), UV.copy(), base.transform, scenes.LIGHTS_ONE,
                        scenes.AMBIENT_ONE, base.texture, P=(0.0, 0.0, 2.0), name="ConstructSphere_256x256")


def ms(v):
    return round(float(np.median(v)) * 1e3, 3)


def measure(s, per, reps):
    r = prk.Renderer(0)
    try:
        r.target_alloc(s.width, s.height)
        r.set_camera(s.prk_transform(), s.prk_lights())
        tex = r.texture(s.texture)
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
        rec = r.records_from_geometry(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
        assert np.array_equal(rec.counts(), counts) and np.array_equal(rec.download(), words)

        def rec_handle():
            r.draw_records(rec, bitmap=tex)

        def rec_lists():
            r.draw_edge_lists(words, counts, bitmap=tex)

        def rec_objects():
            r.draw(abi.PRK_SEM_AVX, g, s.tri_count, P=s.P, bitmap=tex, phong=True, tris_per_object=per)

        ways = [("draw_records", rec_handle), ("draw_edge_lists", rec_lists), ("draw_objects", rec_objects)]
        frames = {}
        for name, fn in ways:  # the frames agree (and a first warm-up)
            r.clear()
            fn()
            r.complete_all_work()
            frames[name] = r.download()
        for name, _ in ways[:2]:
            assert np.array_equal(frames[name][0], frames["draw_objects"][0]), name
            assert np.array_equal(frames[name][1].view(np.uint32), frames["draw_objects"][1].view(np.uint32)), name
        t = {name: ([], []) for name, _ in ways}
        staged = {}
        for i in range(reps + 1):
            for name, fn in ways:
                r.clear()
                r.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                r.complete_all_work()
                r.synchronize()
                t2 = time.perf_counter()
                if i:
                    t[name][0].append(t1 - t0)
                    t[name][1].append(t2 - t1)
                staged[name] = r.stage_bytes()
        make = {"records_from_geometry": [], "edge_records": []}
        for i in range(reps + 1):
            r.synchronize()
            t0 = time.perf_counter()
            h = r.records_from_geometry(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
            t1 = time.perf_counter()
            h.close()
            r.synchronize()
            t2 = time.perf_counter()
            r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
            t3 = time.perf_counter()
            if i:
                make["records_from_geometry"].append(t1 - t0)
                make["edge_records"].append(t3 - t2)
        out = {"scene": s.name, "tris_per_object": per, "lists": int(counts.size), "records": int(words.shape[0]),
               "record_bytes": int(words.nbytes), "ways": {}, "make_ms": {k: ms(v) for k, v in make.items()}}
        for name, _ in ways:
            out["ways"][name] = {
                "record_ms": ms(t[name][0]), "frame_ms": ms(t[name][1]),
                "frame_ms_min_max": [round(min(t[name][1]) * 1e3, 3), round(max(t[name][1]) * 1e3, 3)],
                "stage_bytes": int(staged[name])}
        return out
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("all", "sphere", "c3b"), default="all")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"command": "python tools/time_record_handles.py --tris %d --reps %d --case %s" % (a.tris, a.reps, a.case),
           "cases": {}}
    if a.case in ("all", "sphere"):
        sp = sphere_scene()
        out["cases"]["sphere_one_list"] = measure(sp, sp.tri_count, a.reps)
        print(json.dumps(out["cases"]["sphere_one_list"]), flush=True)
    if a.case in ("all", "c3b"):
        c3b = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024)  # C3b
        out["cases"]["c3b_16_triangle_objects"] = measure(c3b, 16, a.reps)
        print(json.dumps(out["cases"]["c3b_16_triangle_objects"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
