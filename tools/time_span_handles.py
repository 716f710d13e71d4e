"""Time span handles (prk_spans_from_records, prk_draw_span_records) beside the
routes through host memory they replace, on the same lists, in the same run:

  make    prk_spans_from_records (the spans stay on the device) against
          prk_records_spans into a host array (the filling call, at the
          capacity a sizing call returned);
  frame   record + prk_flush + prk_synchronize of one draw of all the spans:
          prk_draw_span_records from the handle, against prk_draw_spans of the
          host array, with prk_draw_records of the same lists beside them.

Two scenes: ConstructSphere as one list at 256x256 and C3b's geometry (1 M
triangles, 4096x4096) as 16-triangle objects (62,500 lists).

usage: python tools/time_span_handles.py [--tris N] [--reps K] [--case all|sphere|c3b] [--lists N] [--json OUT]
Every figure is the host time of the whole call or frame.  Medians of K
repeats after one warm-up, the ways taken in turn within every repeat.
Before the timing the handle's words are compared with the host array's and
the two span frames with each other, by checksum.  --lists N takes the first
N lists only (for a pass that would not fit the build's 31-bit slot limit)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

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


def ok(name, rc):
    if rc != abi.PRK_OK:
        raise prk.PrkError(name, rc)


def stat(v):
    return {"median": round(float(np.median(v)) * 1e3, 3), "min_max": [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]}


def measure(s, per, reps, lists=None):
    r = prk.Renderer(0)
    try:
        L, ctx = r._L, r._h
        r.target_alloc(s.width, s.height)
        r.set_camera(s.prk_transform(), s.prk_lights())
        tex = r.texture(s.texture)
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        rec = r.records_from_geometry(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
        nl = rec.list_count if lists is None else min(lists, rec.list_count)
        h, H = rec.handle, s.height
        total = C.c_uint64(0)
        sc = np.zeros(nl, np.uint32)
        ok("size", L.prk_records_spans(ctx, h, 0, nl, H, None, 0, sc.ctypes.data, C.byref(total)))
        ns = total.value
        spans = np.empty((ns, 25), np.uint32)
        made = []

        def make_host():
            ok("records_spans", L.prk_records_spans(ctx, h, 0, nl, H, spans.ctypes.data, ns, sc.ctypes.data,
                                                    C.byref(total)))

        def make_handle():
            hh = C.c_int32(-1)
            ok("spans_from_records", L.prk_spans_from_records(ctx, h, 0, nl, H, C.byref(hh), None, None))
            made.append(hh.value)

        make_host()
        sp = rec.spans(H, 0, nl, keep=True)
        assert sp.total == ns and np.array_equal(sp.counts(), sc)
        assert zlib.crc32(sp.download()) == zlib.crc32(spans), "the handle's words differ from prk_records_spans'"

        def frame(draw):
            r.clear()
            r.synchronize()
            t0 = time.perf_counter()
            draw()
            r.complete_all_work()
            r.synchronize()
            return time.perf_counter() - t0

        frames = [
            ("span_handle", lambda: ok("d", L.prk_draw_span_records(ctx, sp.handle, 0, ns, abi.PRK_SEM_AVX, 1, tex))),
            ("draw_spans_host", lambda: ok("d", L.prk_draw_spans(ctx, spans.ctypes.data, ns, abi.PRK_SEM_AVX, 1, tex))),
            ("draw_records", lambda: ok("d", L.prk_draw_records(ctx, h, 0, nl, abi.PRK_SEM_AVX, 1, tex))),
        ]
        sums, staged = {}, {}
        for name, draw in frames:  # the frames agree (the record draw's too: the composition)
            frame(draw)
            c, z = r.download()
            sums[name] = (zlib.crc32(c), zlib.crc32(z))
            staged[name] = r.stage_bytes()
        assert sums["span_handle"] == sums["draw_spans_host"] == sums["draw_records"], sums
        t = {k: [] for k in ("make_handle", "make_host") + tuple("frame_" + n for n, _ in frames)}
        for i in range(reps + 1):
            for name, fn in (("make_handle", make_handle), ("make_host", make_host)):
                r.synchronize()
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                while made:  # (outside the timed part)
                    ok("destroy", L.prk_spans_destroy(ctx, made.pop()))
                if i:
                    t[name].append(dt)
            for name, draw in frames:
                dt = frame(draw)
                if i:
                    t["frame_" + name].append(dt)
        return {"scene": s.name, "tris_per_object": per, "lists": nl, "lists_of": rec.list_count, "records": rec.total,
                "height": H, "spans": ns, "span_bytes": int(spans.nbytes), "stage_bytes": staged,
                "ms": {k: stat(v) for k, v in t.items()}}
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("all", "sphere", "c3b"), default="all")
    ap.add_argument("--lists", type=int)
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {"command": "python tools/time_span_handles.py --tris %d --reps %d --case %s%s" % (
        a.tris, a.reps, a.case, "" if a.lists is None else " --lists %d" % a.lists), "cases": {}}
    if a.case in ("all", "sphere"):
        sp = sphere_scene()
        res["cases"]["sphere_one_list"] = measure(sp, sp.tri_count, a.reps)
        print(json.dumps(res["cases"]["sphere_one_list"]), flush=True)
    if a.case in ("all", "c3b"):
        c3b = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024)  # C3b
        res["cases"]["c3b_16_triangle_objects"] = measure(c3b, 16, a.reps, a.lists)
        print(json.dumps(res["cases"]["c3b_16_triangle_objects"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
