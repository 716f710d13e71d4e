"""Time prk_geometry_select on a C3b-sized scene beside the
host route it replaces and beside prk_geometry_transform writing the same
triangles.

The scene is the headline soup: 1M random triangles (radius 16) at 4096 x 4096,
taken as 62 500 items of 16 consecutive triangles.  An item has two levels: all
16 triangles from `--fine` pixels up (default: the median item's count, so
about half the visible items take it), its first 4 triangles from 1 pixel up;
an item without a pixel is dropped.  The frame is drawn once in debug mode and
reduced once (prk_visibility_info); everything below runs on that frame.

  the call      prk_geometry_select from the frame's counts: the host clock
                around the call (tables copied, choice, scan, the wait for the
                total, the emit pass queued, chosen and out_first copied back),
                and the library's own events (prk_debug_select_ms): uploads +
                choice + scan, and the emit pass alone;
  host route    prk_visibility_groups, the runs built on the host (numpy, no
                Python loop), prk_geometry_transform: host clock of each;
  yardstick     prk_debug_transform_ms of that prk_geometry_transform: the same
                output triangles through k_xform.
Both passes move 288 bytes a triangle (three vertices of 12 + 16 + 12 + 8
bytes, read and written); the rates are 288 * total / the pass's time.  Before
anything is timed the two destinations are compared word for word.

usage: python tools/select_bench.py [--reps K] [--tris T] [--fine PIXELS] [--json OUT]"""
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
import selectref as S  # noqa: E402
import xform_ref as X  # noqa: E402
from prk import scenes  # noqa: E402
from xform_bench import stat  # noqa: E402

PER, COARSE = 16, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--fine", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    if prk.device_count() <= 0:
        raise SystemExit("select_bench: no HIP device")
    T = a.tris - a.tris % PER
    n = T // PER
    s = scenes.random_soup(T, 4096, 4096, radius=16, seed=2024)  # the headline geometry (C3b)
    xf = np.stack([X.rotation_yx(0.01 * k, 0.0, (0.0, 0.0, 0.0)) for k in range(64)])
    r = prk.Renderer(0)
    try:
        r.target_alloc(s.width, s.height)
        r.set_debug(True)
        r.set_camera(s.prk_transform(), s.prk_lights())
        g, tex = r.geometry(s.vertices, s.colors, s.normals, s.uvs), r.texture(s.texture)
        r.clear()
        r.draw_model_optimized(g, T, P=s.P, bitmap=tex, phong=True)
        r.complete_all_work()
        r.synchronize()
        assert r.visibility()[0] == T
        starts = (PER * np.arange(n + 1)).astype(np.uint32)
        px = r.visibility_groups(starts)[0]
        fine = a.fine or max(2, int(np.median(px[px > 0])))
        first = PER * np.arange(n)
        items = np.stack([first, np.full(n, PER), 2 * np.arange(n), np.full(n, 2), np.arange(n) % 64], 1).astype(np.uint32)
        levels = np.stack([np.tile([fine, 1], n), np.repeat(first, 2), np.tile([PER, COARSE], n)], 1).astype(np.uint32)

        def host_runs(pixels):
            """The runs a caller builds on the host from the items' pixel counts."""
            cnt = np.where(pixels >= fine, PER, np.where(pixels >= 1, COARSE, 0))
            at = np.concatenate([[0], np.cumsum(cnt)])
            keep = np.flatnonzero(cnt)
            return np.stack([first[keep], cnt[keep], at[keep], items[keep, 4]], 1).astype(np.uint32), at

        runs, at = host_runs(px)
        d_sel, d_host = r.geometry_alloc(), r.geometry_alloc()
        total, chosen, out_first = r.geometry_select(g, d_sel, items, levels, xf)
        r.geometry_transform(g, d_host, runs, xf)
        want = S.choose(items, levels, px)
        assert total == want.total == int(at[-1]) and np.array_equal(chosen, want.chosen)
        assert np.array_equal(out_first, want.out_first) and np.array_equal(out_first, at.astype(np.uint32))
        for got, ref in zip(r.geometry_download(d_sel), r.geometry_download(d_host)):
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        res = {"triangles": T, "items": n, "levels": 2 * n, "fine_min_pixels": fine,
               "items_fine": int((want.chosen == 0).sum()), "items_coarse": int((want.chosen == 1).sum()),
               "items_dropped": int((want.chosen < 0).sum()), "output_triangles": total, "bytes_moved": 288 * total}
        call_ms, choose_ms, emit_ms, groups_ms, build_ms, xform_call_ms, xform_kernel_ms = ([] for _ in range(7))
        rp_t, xp_t = prk.abi.PrkXformRun, prk.abi.PrkXform
        for i in range(a.reps + 2):
            r.synchronize()
            t0 = time.perf_counter()
            tot = r.geometry_select(g, d_sel, items, levels, xf)[0]
            t1 = time.perf_counter()
            ms = r.select_ms()
            r.synchronize()
            t2 = time.perf_counter()
            gp = r.visibility_groups(starts)[0]
            t3 = time.perf_counter()
            rr, _ = host_runs(gp)
            t4 = time.perf_counter()
            rc = r._L.prk_geometry_transform(r._h, g, d_host, C.cast(rr.ctypes.data, C.POINTER(rp_t)), rr.shape[0],
                                             C.cast(xf.ctypes.data, C.POINTER(xp_t)), xf.shape[0])
            t5 = time.perf_counter()
            k = C.c_float(0)
            assert rc == 0 and tot == total and r._L.prk_debug_transform_ms(r._h, C.byref(k)) == 0
            if i >= 2:  # (the first rounds size the buffers and warm the code)
                call_ms.append((t1 - t0) * 1e3)
                choose_ms.append(ms[0])
                emit_ms.append(ms[1])
                groups_ms.append((t3 - t2) * 1e3)
                build_ms.append((t4 - t3) * 1e3)
                xform_call_ms.append((t5 - t4) * 1e3)
                xform_kernel_ms.append(k.value)
        res["select_call_host_clock"] = stat(call_ms)
        res["select_uploads_choice_scan_events"] = stat(choose_ms)
        res["select_emit_pass_events"] = stat(emit_ms)
        res["host_route_visibility_groups_host_clock"] = stat(groups_ms)
        res["host_route_build_runs_numpy_host_clock"] = stat(build_ms)
        res["host_route_transform_call_host_clock"] = stat(xform_call_ms)
        res["host_route_total_host_clock_median_ms"] = round(
            float(np.median(np.array(groups_ms) + np.array(build_ms) + np.array(xform_call_ms))), 4)
        res["transform_kernel_same_triangles_events"] = stat(xform_kernel_ms)
        res["emit_pass_GBps"] = round(288 * total / res["select_emit_pass_events"]["median_ms"] / 1e6, 1)
        res["transform_kernel_GBps"] = round(288 * total / res["transform_kernel_same_triangles_events"]["median_ms"] / 1e6, 1)
        out = {"command": "python tools/select_bench.py --reps %d --tris %d --fine %d" % (a.reps, T, a.fine), "c3b": res,
               "notes": ["One MI355X, warm: medians of %d repetitions after two that size the buffers.  Host clocks are "
                         "around calls that return when their work is queued (the select call also waits for its "
                         "total); the events are the library's own on the geometry stream "
                         "(prk_debug_select_ms, prk_debug_transform_ms).  The frame's reduction "
                         "(prk_visibility_info, profiles/visibility.json) is outside every figure here." % a.reps]}
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
