"""Time prk_visibility_bounds on the C3b-sized frame beside the
yardstick of a streaming pass and beside the host route it replaces.

The frame is the headline soup: 1M random triangles (radius 16) at 4096 x 4096,
drawn once; everything below tests boxes against the z it leaves.  The items
are select_bench's: 62 500 items of 16 consecutive triangles, their boxes the
numpy AABB of their vertices.

  (a) k_ztile_min      the library's events around the tile-map kernel
                       (prk_debug_bounds_ms), as GB/s of z read (4 bytes a
                       pixel), beside a whole-target prk_target_from_layer
                       PRK_MERGE_COPY (k_layer, 16 bytes moved a pixel) timed
                       with events in the same process;
  (b) k_bounds_test    the same events around the test kernel for the 62 500
                       boxes;
  (c) ... and for those plus 256 boxes that fill the screen (4096 trips of one
                       wave each: what a coarser second min level would cut);
  (d) the call         host clock around prk_visibility_bounds (tables uploaded,
                       both kernels, the answer copied back), beside the host
                       route: prk_target_download of z and the definition in
                       numpy (tests/boundsref.py).
Before anything is timed the answer is compared with boundsref's word for word.

usage: python tools/bounds_bench.py [--reps K] [--tris T] [--json OUT]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpu-renderer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import boundsref as B  # noqa: E402
import prk  # noqa: E402
import xform_ref as X  # noqa: E402
from prk import scenes  # noqa: E402
from xform_bench import Hip, stat  # noqa: E402

PER = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--json")
    a = ap.parse_args()
    if prk.device_count() <= 0:
        raise SystemExit("bounds_bench: no HIP device")
    T = a.tris - a.tris % PER
    n = T // PER
    s = scenes.random_soup(T, 4096, 4096, radius=16, seed=2024)  # the headline geometry (C3b)
    ident = X.translation((0.0, 0.0, 0.0))[None]
    lo, hi = B.aabb(s.vertices, 3 * PER, 0.0)
    # a box over the whole view volume of the frame: every corner in front of the camera, the rectangle the band
    D, F, M2P, cx, cy = s.transform
    far = float(s.vertices[:, 2].min())
    ext = 1.2 * max(cx, cy) * (D - far) / (M2P * F)
    big_lo, big_hi = [-ext, -ext, far], [ext, ext, float(s.vertices[:, 2].max())]
    small = prk.pack_bounds(lo, hi, 0)
    mixed = np.concatenate([small, prk.pack_bounds([big_lo] * 256, [big_hi] * 256, 0)])
    hip = Hip()
    r = prk.Renderer(0)
    try:
        r.target_alloc(s.width, s.height)
        r.set_camera(s.prk_transform(), s.prk_lights())
        g, tex = r.geometry(s.vertices, s.colors, s.normals, s.uvs), r.texture(s.texture)
        r.clear()
        r.draw_model_optimized(g, T, P=s.P, bitmap=tex, phong=True)
        r.complete_all_work()
        r.synchronize()
        z = r.download()[1]
        want = B.pixels(mixed[:, 0:3], mixed[:, 3:6], np.zeros(len(mixed), int), ident, s.P, s.transform, z, 0)
        got = r.visibility_bounds(mixed, ident, P=s.P)
        assert np.array_equal(got, want), "the answer differs from tests/boundsref.py"
        zt = r.ztiles()[0]
        assert np.array_equal(zt, B.ztiles(z, 0))
        npx = s.width * s.height
        res = {"target": [s.width, s.height], "triangles": T, "items": n, "items_hidden": int((want[:n] == 0).sum()),
               "screen_filling_boxes": 256, "screen_filling_pixels_each": int(want[n]), "z_bytes": 4 * npx}
        ztile_ms, small_ms, mixed_ms, call_ms, dl_ms, ref_ms = ([] for _ in range(6))
        for i in range(a.reps + 2):
            r.synchronize()
            t0 = time.perf_counter()
            r.visibility_bounds(small, ident, P=s.P)
            t1 = time.perf_counter()
            ms = r.bounds_ms()
            r.visibility_bounds(mixed, ident, P=s.P)
            ms2 = r.bounds_ms()
            if i >= 2:  # (the first rounds size the buffers and warm the code)
                ztile_ms.append(ms[0])
                small_ms.append(ms[1])
                mixed_ms.append(ms2[1])
                call_ms.append((t1 - t0) * 1e3)
            if i >= a.reps - 1:  # the host route, seconds a round: three rounds
                t2 = time.perf_counter()
                zz = r.download()[1]
                t3 = time.perf_counter()
                B.pixels(small[:, 0:3], small[:, 3:6], np.zeros(n, int), ident, s.P, s.transform, zz, 0)
                t4 = time.perf_counter()
                dl_ms.append((t3 - t2) * 1e3)
                ref_ms.append((t4 - t3) * 1e3)
        res["ztile_min_events"] = stat(ztile_ms)
        res["ztile_min_GBps_read"] = round(4 * npx / res["ztile_min_events"]["median_ms"] / 1e6, 1)
        res["bounds_test_62500_items_events"] = stat(small_ms)
        res["bounds_test_plus_256_screen_filling_events"] = stat(mixed_ms)
        res["call_62500_items_host_clock"] = stat(call_ms)
        res["host_route_download_host_clock"] = stat(dl_ms)
        res["host_route_numpy_host_clock"] = stat(ref_ms)
        # the yardstick: a whole-target COPY restore (k_layer) on this target
        layer = r.layer_alloc(s.width, s.height)
        r.layer_from_target(layer)
        lstream = C.c_void_p()
        assert r._L.prk_debug_geometry_stream(r._h, C.byref(lstream)) == 0

        def restore():
            assert r._L.prk_target_from_layer(r._h, layer, 0, 0, s.width, s.height, 0, 0, prk.abi.PRK_MERGE_COPY) == 0

        for _ in range(3):
            restore()
        r.synchronize()
        res["layer_copy_events"] = stat(hip.timed(lstream, max(a.reps, 5), restore))
        r.synchronize()
        res["layer_copy_GBps_moved"] = round(16 * npx / res["layer_copy_events"]["median_ms"] / 1e6, 1)
        out = {"command": "python tools/bounds_bench.py --reps %d --tris %d" % (a.reps, T), "c3b": res,
               "notes": ["One MI355X, warm, one process: medians of %d repetitions after two that size the buffers.  "
                         "The events are the library's own around its two kernels (prk_debug_bounds_ms); the host "
                         "clock is around the whole call, which waits for its answer.  The host route (three "
                         "rounds) is prk_target_download of z plus tests/boundsref.py's numpy (a Python loop over the items)."
                         % a.reps]}
        print(json.dumps(out), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        r.close()


if __name__ == "__main__":
    main()
