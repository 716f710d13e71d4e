"""Time FillEdgeTable's edge_info records of C3b's geometry (1 M triangles)
both ways: prk_edge_records (one batched call, set up / sorted / packed on
the GPU, downloaded) and a loop of the host producer prk_fill_edge_records
over the same objects, as objects of one triangle and of 16.

usage: python tools/time_edge_records.py [--tris N] [--reps K] [--json OUT]
GPU: host wall time of the whole call (median of K after one warm-up), the
download of the records included.  Host: one pass of the loop through ctypes,
and the same loop with vertex_count = 0 (the call overhead alone), which the
per-triangle case is dominated by; `host_ms` is their difference."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpu-renderer_amd"))
import numpy as np  # noqa: E402
import prk  # noqa: E402
from prk import scenes  # noqa: E402


def time_gpu(r, g, s, per, setup, reps):
    dts = []
    for i in range(reps + 1):
        r.synchronize()
        t0 = time.perf_counter()
        words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=setup, tris_per_object=per)
        if i:
            dts.append(time.perf_counter() - t0)
    return float(np.median(dts)) * 1e3, int(words.shape[0])


def time_host(s, per, setup, real):
    L = prk.lib()
    tr, li = s.prk_transform(), s.prk_lights()
    mem = np.zeros((3 * per + 1, prk.EDGE_INFO_STRIDE), np.uint8)
    Pc = (C.c_float * 3)(*s.P)
    n = C.c_uint32(0)
    V, Cc, N, UV = (a.ctypes.data for a in (s.vertices, s.colors, s.normals, s.uvs))
    f, T = L.prk_fill_edge_records, s.tri_count
    ptr, memp, trp, lip, np_ = C.c_void_p, C.c_void_p(mem.ctypes.data), C.byref(tr), C.byref(li), C.byref(n)
    total = 0
    t0 = time.perf_counter()
    for t in range(0, T, per):
        nv = 3 * min(per, T - t) if real else 0
        f(ptr(V + 36 * t), ptr(Cc + 48 * t), ptr(N + 36 * t), ptr(UV + 24 * t), nv, Pc, trp, lip, setup, memp,
          prk.EDGE_INFO_STRIDE, prk.EDGE_INFO_NEXT, None, np_)
        total += n.value
    return (time.perf_counter() - t0) * 1e3, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--setup", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    s = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024)  # C3b
    out = {"command": "python tools/time_edge_records.py --tris %d --reps %d --setup %d" % (a.tris, a.reps, a.setup),
           "scene": s.name, "setup": a.setup, "cases": {}}
    r = prk.Renderer(0)
    try:
        r.set_camera(s.prk_transform(), s.prk_lights())
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        for per in (1, 16):
            gpu_ms, total = time_gpu(r, g, s, per, a.setup, a.reps)
            loop_ms, htotal = time_host(s, per, a.setup, True)
            call_ms, _ = time_host(s, per, a.setup, False)
            assert htotal == total, (htotal, total)
            out["cases"]["tris_per_object_%d" % per] = {
                "objects": (s.tri_count + per - 1) // per, "records": total,
                "gpu_ms": round(gpu_ms, 2), "host_loop_ms": round(loop_ms, 1), "host_call_overhead_ms": round(call_ms, 1),
                "host_ms": round(loop_ms - call_ms, 1)}
            print(json.dumps({per: out["cases"]["tris_per_object_%d" % per]}), flush=True)
    finally:
        r.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
