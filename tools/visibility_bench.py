"""Time the first prk_visibility_info call after a frame -- the reduction of
the frame's winner map to per-id pixel counts on the device
-- beside what a caller had before it, prk_download_winners plus
numpy.bincount on the host, for two frames:

  c3b         1M random triangles (radius 16) at 4096 x 4096: 1M ids, short runs;
  contention  a few hundred screen-filling triangles at 8192 x 8192: nearly all
              pixels on a few counters, runs of thousands of words.

Each frame is flushed in debug mode and waited for; then HIP events on the
context's stream around the one call (the memset of the counters, the
histogram, the flags, two scans, the compaction, two 4-byte copies, with the
host's launch gaps between them), and the host clock around it.  The reduction
reads the map's 4n bytes once; 4n / the events' time is reported as GB/s, a
lower bound of the histogram's own rate, beside the rate of a whole-target
prk_target_from_layer PRK_MERGE_COPY (k_layer, the yardstick for a streaming
pass: 8 bytes read and 8 written a pixel) measured in the same run.  The
counts are compared with numpy.bincount's before anything is timed.

usage: python tools/visibility_bench.py [--reps K] [--tris T] [--big-tris B] [--json OUT]"""
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
import prk  # noqa: E402
import visref  # noqa: E402
from prk import scenes  # noqa: E402
from xform_bench import Hip, stat  # noqa: E402


def run_case(hip, name, s, reps):
    r = prk.Renderer(0)
    try:
        N = s.width
        r.target_alloc(s.width, s.height)
        r.set_debug(True)
        r.set_camera(s.prk_transform(), s.prk_lights())
        g, t = r.geometry(s.vertices, s.colors, s.normals, s.uvs), r.texture(s.texture)
        stream = C.c_void_p(r.device_stream()[1])

        def frame():
            r.clear()
            r.draw_model_optimized(g, s.tri_count, P=s.P, bitmap=t, phong=True)
            r.complete_all_work()
            r.synchronize()

        frame()
        win = r.winners()
        want = visref.reduce(win, s.tri_count)
        assert r.visibility() == (s.tri_count, want.covered, want.visible)
        assert np.array_equal(r.visibility_counts(), want.counts) and np.array_equal(r.visibility_ids(), want.ids)
        n = win.size
        res = {"target": [s.width, s.height], "ids": s.tri_count, "covered": want.covered, "visible_ids": want.visible,
               "largest_count": int(want.counts.max()), "runs_of_65_or_more": visref.runs_of(win, 65),
               "map_bytes": 4 * n}
        del win
        ev_ms, wall_ms, host_ms, frame_ms = [], [], [], []
        ev = hip.events(2)
        for i in range(reps + 1):
            t0 = time.perf_counter()
            frame()
            t1 = time.perf_counter()
            hip.ok(hip.L.hipEventRecord(ev[0], stream))
            info = r.visibility()
            hip.ok(hip.L.hipEventRecord(ev[1], stream))
            t2 = time.perf_counter()
            hip.ok(hip.L.hipEventSynchronize(ev[1]))
            assert info == (s.tri_count, want.covered, want.visible)
            ms = C.c_float(0)
            hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
            # the caller's route at the parent commit, same frame, same box
            t3 = time.perf_counter()
            w = r.winners().reshape(-1)
            counts = np.bincount(w[w >= 0], minlength=s.tri_count)
            t4 = time.perf_counter()
            assert int(counts.sum()) == want.covered
            if i:  # (the first round sizes the buffers)
                frame_ms.append((t1 - t0) * 1e3)
                ev_ms.append(ms.value)
                wall_ms.append((t2 - t1) * 1e3)
                host_ms.append((t4 - t3) * 1e3)
        for e in ev:
            hip.L.hipEventDestroy(e)
        res["first_info_call_events"] = stat(ev_ms)
        res["first_info_call_host_clock"] = stat(wall_ms)
        res["download_winners_plus_bincount_host_clock"] = stat(host_ms)
        res["frame_with_clear_and_wait_host_clock"] = stat(frame_ms)
        res["map_GBps_over_events"] = round(4 * n / res["first_info_call_events"]["median_ms"] / 1e6, 1)
        res["ns_per_pixel_over_events"] = round(res["first_info_call_events"]["median_ms"] * 1e6 / n, 5)
        res["host_route_over_device_route"] = round(
            res["download_winners_plus_bincount_host_clock"]["median_ms"] /
            res["first_info_call_host_clock"]["median_ms"], 1)
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
        res["layer_copy_events"] = stat(hip.timed(lstream, max(reps, 5), restore))
        r.synchronize()
        res["layer_copy_GBps_moved"] = round(16 * N * s.height / res["layer_copy_events"]["median_ms"] / 1e6, 1)
        print(name, json.dumps(res), flush=True)
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--big-tris", type=int, default=300)
    ap.add_argument("--json")
    a = ap.parse_args()
    if prk.device_count() <= 0:
        raise SystemExit("visibility_bench: no HIP device")
    hip = Hip()
    out = {"command": "python tools/visibility_bench.py --reps %d --tris %d --big-tris %d" % (a.reps, a.tris, a.big_tris),
           "cases": {}}
    out["cases"]["c3b"] = run_case(hip, "c3b", scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024), a.reps)
    out["cases"]["contention"] = run_case(
        hip, "contention", scenes.random_soup(a.big_tris, 8192, 8192, radius=8192, seed=7, centroid_margin=0), a.reps)
    c, k = out["cases"]["c3b"], out["cases"]["contention"]
    out["contention_over_c3b_per_pixel"] = round(k["ns_per_pixel_over_events"] / c["ns_per_pixel_over_events"], 2)
    out["notes"] = [
        "Events on the context's stream around one prk_visibility_info call after a waited-for debug-mode frame: the "
        "whole reduction with the host's launch gaps, median of %d frames after one that sizes the buffers; "
        "map_GBps_over_events = 4 bytes a pixel / that time, a lower bound of the histogram's own rate.  "
        "layer_copy: prk_target_from_layer PRK_MERGE_COPY of the whole target, 16 bytes moved a pixel, same "
        "process.  The host route is prk_download_winners + numpy.bincount on the same frame, host clock." % a.reps]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
