"""Time the lists DrawModel* leaves (every edge stepped, the links as the walk
left them) both ways: prk_advance_edge_lists (one batched call: upload,
import, one GPU thread's walk per list, export, download) and a loop of the
host call prk_advance_edge_records over the same lists -- on C3b's geometry
(1 M triangles) as one-triangle and as 16-triangle lists, and on
ConstructSphere as one list.  Then the thread walk's own rate on two
synthetic lists, which prk_advance_edge_lists' edge-row cap rests on.

usage: python tools/time_advance_lists.py [--tris N] [--reps K] [--gpu-only] [--json OUT]
GPU: host wall time of the whole call (median of K after one warm-up),
transfers included, at the frame's height and at height 0 (the same call
without any row walked: transfers, import and export alone; the difference
is the walk).  Host: one pass of the loop through ctypes over edge_info
memory prepared beforehand, and the same loop with count = 0 (the call
overhead alone); `host_ms` is their difference."""
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


def time_gpu(r, words, counts, height, reps):
    dts = []
    for i in range(reps + 1):
        r.synchronize()
        t0 = time.perf_counter()
        r.advance_edge_lists(words, counts, height)
        if i:
            dts.append(time.perf_counter() - t0)
    return float(np.median(dts)) * 1e3


def time_host(words, counts, height, real):
    mem = np.zeros((max(1, words.shape[0]), prk.EDGE_INFO_STRIDE), np.uint8)  # Next = NULL
    mem[:words.shape[0], :108] = words.view(np.uint8).reshape(-1, 108)
    f, base, ptr = prk.lib().prk_advance_edge_records, mem.ctypes.data, C.c_void_p
    offs = np.concatenate([[0], np.cumsum(counts.astype(np.int64))]).tolist()
    cnts = counts.tolist()
    t0 = time.perf_counter()
    for o, n in zip(offs, cnts):
        f(ptr(base + prk.EDGE_INFO_STRIDE * o), n if real else 0, prk.EDGE_INFO_STRIDE, prk.EDGE_INFO_NEXT, height)
    return (time.perf_counter() - t0) * 1e3


def edge_rows(words, height):
    w = words.view(np.int32)
    return int(np.maximum(0, np.minimum(w[:, 0], height).astype(np.int64) - w[:, 7]).sum())


def case(r, words, counts, height, reps, host):
    gpu = time_gpu(r, words, counts, height, reps)
    gpu0 = time_gpu(r, words, counts, 0, reps)
    loop = time_host(words, counts, height, True) if host else 0.0
    call = time_host(words, counts, height, False) if host else 0.0
    return {"lists": int(counts.shape[0]), "records": int(words.shape[0]), "height": height,
            "edge_rows": edge_rows(words, height), "gpu_ms": round(gpu, 2), "gpu_height0_ms": round(gpu0, 2),
            "gpu_walk_ms": round(gpu - gpu0, 2), "host_loop_ms": round(loop, 1),
            "host_call_overhead_ms": round(call, 1), "host_ms": round(loop - call, 1)}


def rate_list(nedge, rows):
    """One list of nedge edges alive on rows [0, rows): nedge / 2 pairs a row,
    no swaps, every field stepped."""
    f = np.zeros((nedge, 27), np.float32)
    f[:, 1] = np.arange(nedge) * 4.0       # XMin (Gradient 0: the order holds)
    f[:, 2], f[:, 5] = 1.0, 1e-4           # ZMin, ZGradient
    f[:, 3], f[:, 6] = 0.25, 1e-6          # OneOverZMin, OneOverZGradient
    f[:, 13:17], f[:, 17:21] = 0.5, 1e-6   # MinColor, ColorGradient
    f[:, 21:24], f[:, 24:27] = (0.0, 0.6, 0.8), (1e-4, -1e-4, 2e-4)  # MinNormal, NormalGradient
    w = f.view(np.uint32).copy()
    w[:, 0], w[:, 7], w[:, 12] = rows, 0, (np.arange(nedge) + 1) & 1
    return w, np.array([nedge], np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="skip the host loops (A/B runs of library variants)")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"command": "python tools/time_advance_lists.py --tris %d --reps %d" % (a.tris, a.reps), "cases": {},
           "thread_walk": {}}
    s = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024)  # C3b
    r = prk.Renderer(0)
    try:
        r.set_camera(s.prk_transform(), s.prk_lights())
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        for per in (1, 16):
            words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
            k = "c3b_tris_per_list_%d" % per
            out["cases"][k] = case(r, words, counts, s.height, a.reps, not a.gpu_only)
            print(json.dumps({k: out["cases"][k]}), flush=True)
        V, Cc, N, UV = prk.construct_sphere()
        base = scenes.random_soup(1, 256, 256, seed=0)
        r.set_camera(base.prk_transform(), base.prk_lights())
        g = r.geometry(V, Cc, N, UV)
        words, counts = r.edge_records(g, V.shape[0] // 3, P=(0.0, 0.0, 2.0), setup=3)
        out["cases"]["sphere_one_list"] = case(r, words, counts, 256, a.reps, not a.gpu_only)
        print(json.dumps({"sphere_one_list": out["cases"]["sphere_one_list"]}), flush=True)
        # the thread walk alone: one pair a row, and 128 pairs a row
        for nedge, rows in ((2, 65536), (256, 1024)):
            words, counts = rate_list(nedge, rows)
            gpu = time_gpu(r, words, counts, rows, a.reps)
            gpu0 = time_gpu(r, words, counts, 0, a.reps)
            er = nedge * rows
            k = "%d_edges_%d_rows" % (nedge, rows)
            out["thread_walk"][k] = {"edge_rows": er, "gpu_ms": round(gpu, 2), "gpu_height0_ms": round(gpu0, 2),
                                     "edge_rows_per_s": round(er / max(1e-9, (gpu - gpu0) * 1e-3))}
            print(json.dumps({k: out["thread_walk"][k]}), flush=True)
    finally:
        r.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
