"""Time the lists DrawModel* leaves (every edge stepped, the links as the walk
left them) both ways: prk_advance_edge_lists (one batched call: upload,
import, one GPU thread's walk per list, export, download) and a loop of the
host call prk_advance_edge_records over the same lists -- on C3b's geometry
(1 M triangles) as one-triangle and as 16-triangle lists, and on
ConstructSphere as one list.  Then the thread walk's own rate on two
synthetic lists, which prk_advance_edge_lists' edge-row cap rests on (with
the workgroup route off: PRK_ADV_WG_MIN_STEPS is set for those two runs).
--wg-sweep adds the routing measurement kAdvWgMinSteps comes from: one list,
and a batch of 1024 equal lists, at a handful of lengths and shapes (tall and
thin, short and wide, square, the sphere), each walked with the workgroup
route forced on (PRK_ADV_WG_MIN_STEPS=0) and forced off, with the list's
thread-walk cost in list steps (the host's list_walk_steps) beside the times;
and the largest such cost among the C3b lists, which must stay below the
constant.

usage: python tools/time_advance_lists.py [--tris N] [--reps K] [--gpu-only] [--wg-sweep] [--json OUT]
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


def routes_of(r):
    """[thread, the five slot classes] of the last call (None: a library before the route)."""
    try:
        lr = r.list_routes()
    except AttributeError:
        return None
    return [lr["thread"]] + list(lr["slots"])


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
    routes = routes_of(r)  # under the routing the run was started with (default: the library's constants)
    gpu0 = time_gpu(r, words, counts, 0, reps)
    loop = time_host(words, counts, height, True) if host else 0.0
    call = time_host(words, counts, height, False) if host else 0.0
    return {"lists": int(counts.shape[0]), "records": int(words.shape[0]), "height": height,
            "edge_rows": edge_rows(words, height), "gpu_ms": round(gpu, 2), "gpu_height0_ms": round(gpu0, 2),
            "gpu_walk_ms": round(gpu - gpu0, 2), "host_loop_ms": round(loop, 1),
            "host_call_overhead_ms": round(call, 1), "host_ms": round(loop - call, 1), "routes": routes}


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


WG_ENV = "PRK_ADV_WG_MIN_STEPS"  # read by the library on every call
WG_OFF = str(1 << 62)


def thread_cost(words, counts, height):
    """The largest list_walk_steps (prk_record_api.hip) among the lists: edge-rows
    plus the insertion scans' bound n (n - 1) / 2 (the exact sweep, where that
    bound would pass the 2^21 cap, only lowers it)."""
    w = words.view(np.int32)
    er = np.maximum(0, np.minimum(w[:, 0], height).astype(np.int64) - w[:, 7])
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    per = np.add.reduceat(np.concatenate([er, [0]]), np.minimum(off[:-1], er.shape[0]))
    per = np.where(counts > 0, per, 0)
    n = counts.astype(np.int64)
    return int((per + n * (n - 1) // 2).max())


def restore_env(saved):
    if saved is None:
        os.environ.pop(WG_ENV, None)
    else:
        os.environ[WG_ENV] = saved


def sweep_case(r, words, counts, height, reps):
    saved = os.environ.get(WG_ENV)
    try:
        return _sweep_case(r, words, counts, height, reps)
    finally:
        restore_env(saved)


def _sweep_case(r, words, counts, height, reps):
    out = {"lists": int(counts.shape[0]), "records": int(words.shape[0]),
           "thread_cost_steps": thread_cost(words, counts, height)}
    for key, env in (("wg", "0"), ("thread", WG_OFF)):
        os.environ[WG_ENV] = env
        gpu = time_gpu(r, words, counts, height, reps)
        routes = routes_of(r)  # of the call at full height
        gpu0 = time_gpu(r, words, counts, 0, reps)
        out[key + "_ms"], out[key + "_walk_ms"] = round(gpu, 3), round(gpu - gpu0, 3)
        out[key + "_routes"] = routes
    return out


def wg_sweep(r, reps, sphere, c3b):
    shapes = [("tall_2x256", 2, 256), ("tall_2x4096", 2, 4096), ("tall_8x1024", 8, 1024),
              ("square_16x16", 16, 16), ("square_32x32", 32, 32), ("square_48x48", 48, 48),
              ("square_64x64", 64, 64), ("square_128x128", 128, 128),
              ("wide_16x4", 16, 4), ("wide_64x4", 64, 4), ("wide_256x4", 256, 4), ("wide_1000x4", 1000, 4)]
    # the lists just above kAdvWgMinSteps in larger and larger batches: threads
    # run side by side, workgroups queue for the CUs
    many = {"square_48x48": (4096, 16384, 61440), "square_64x64": (4096, 16384, 61440)}
    out = {}
    for name, nedge, rows in shapes:
        words, counts = rate_list(nedge, rows)
        out[name] = sweep_case(r, words, counts, rows, reps)
        print(json.dumps({name: out[name]}), flush=True)
        if nedge * rows <= 4096:  # the same list 1024 times: the thread walk's lanes and CUs fill up
            bw, bc = np.tile(words, (1024, 1)), np.full(1024, nedge, np.uint32)
            out[name + "_x1024"] = sweep_case(r, bw, bc, rows, reps)
            print(json.dumps({name + "_x1024": out[name + "_x1024"]}), flush=True)
        for k in many.get(name, ()):
            key = "%s_x%d" % (name, k)
            out[key] = sweep_case(r, np.tile(words, (k, 1)), np.full(k, nedge, np.uint32), rows, reps)
            print(json.dumps({key: out[key]}), flush=True)
    for k, (words, counts, height) in c3b.items():  # the whole batches, every list a workgroup's or a thread's
        out[k] = sweep_case(r, words, counts, height, reps)
        print(json.dumps({k: out[k]}), flush=True)
    out["sphere_one_list"] = sweep_case(r, sphere[0], sphere[1], 256, reps)
    print(json.dumps({"sphere_one_list": out["sphere_one_list"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="skip the host loops (A/B runs of library variants)")
    ap.add_argument("--wg-sweep", action="store_true", help="the routing sweep (workgroup route forced on / off)")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"command": "python tools/time_advance_lists.py --tris %d --reps %d" % (a.tris, a.reps), "cases": {},
           "thread_walk": {}}
    s = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024)  # C3b
    r = prk.Renderer(0)
    try:
        r.set_camera(s.prk_transform(), s.prk_lights())
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        c3b = {}
        for per in (1, 16):
            words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
            k = "c3b_tris_per_list_%d" % per
            out["cases"][k] = case(r, words, counts, s.height, a.reps, not a.gpu_only)
            out["cases"][k]["max_thread_cost_steps"] = thread_cost(words, counts, s.height)
            if a.wg_sweep:
                c3b[k] = (words, counts, s.height)
            print(json.dumps({k: out["cases"][k]}), flush=True)
        V, Cc, N, UV = prk.construct_sphere()
        base = scenes.random_soup(1, 256, 256, seed=0)
        r.set_camera(base.prk_transform(), base.prk_lights())
        g = r.geometry(V, Cc, N, UV)
        words, counts = r.edge_records(g, V.shape[0] // 3, P=(0.0, 0.0, 2.0), setup=3)
        out["cases"]["sphere_one_list"] = case(r, words, counts, 256, a.reps, not a.gpu_only)
        print(json.dumps({"sphere_one_list": out["cases"]["sphere_one_list"]}), flush=True)
        if a.wg_sweep:
            out["wg_sweep"] = wg_sweep(r, a.reps, (words, counts), c3b)
        # the thread walk alone: one pair a row, and 128 pairs a row
        saved = os.environ.get(WG_ENV)
        os.environ[WG_ENV] = WG_OFF
        for nedge, rows in ((2, 65536), (256, 1024)):
            words, counts = rate_list(nedge, rows)
            gpu = time_gpu(r, words, counts, rows, a.reps)
            gpu0 = time_gpu(r, words, counts, 0, a.reps)
            er = nedge * rows
            k = "%d_edges_%d_rows" % (nedge, rows)
            out["thread_walk"][k] = {"edge_rows": er, "gpu_ms": round(gpu, 2), "gpu_height0_ms": round(gpu0, 2),
                                     "edge_rows_per_s": round(er / max(1e-9, (gpu - gpu0) * 1e-3))}
            print(json.dumps({k: out["thread_walk"][k]}), flush=True)
        restore_env(saved)
    finally:
        r.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
