"""Time prk_geometry_transform on the headline geometry (1 M triangles, all
four arrays: 144 B read and 144 B written a triangle) for three run layouts --
62,500 runs of 16 triangles, one run of 1 M, 1 M runs of 1 -- beside two other
ways of getting moved vertices into a resident geometry, in one process:

  (a) transform   the call, HIP events on its own stream around each of K warm
                  calls (table upload + kernel), median;
  (b) d2d_copy    hipMemcpyAsync device to device of the same four arrays:
                  the same bytes moved, no arithmetic, no run lookup: the floor;
  (c) host        what a caller does without the pass: the numpy transform of
                  every vertex on the host plus prk_geometry_update (host
                  clock, to the end of prk_synchronize), and the update alone.

usage: python tools/xform_bench.py [--tris N] [--calls K] [--host-reps R] [--json OUT]
Every layout's output is compared with tests/xform_ref.py's on a sample of
triangles before it is timed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpu-renderer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import prk  # noqa: E402
import xform_ref as X  # noqa: E402
from prk import scenes  # noqa: E402


class Hip:
    """The few runtime calls the timing needs, from the runtime the library uses."""

    def __init__(self):
        prk.lib()
        self.L = L = C.CDLL("libamdhip64.so")
        L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        L.hipEventSynchronize.argtypes = [C.c_void_p]
        L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        L.hipEventDestroy.argtypes = [C.c_void_p]
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]

    def ok(self, e):
        if e:
            raise RuntimeError("HIP error %d" % e)

    def events(self, n):
        out = []
        for _ in range(n):
            e = C.c_void_p()
            self.ok(self.L.hipEventCreate(C.byref(e)))
            out.append(e)
        return out

    def timed(self, stream, calls, fn):
        """fn() queued `calls` times on `stream`, an event before and after each: ms per call."""
        ev = self.events(2 * calls)
        for i in range(calls):
            self.ok(self.L.hipEventRecord(ev[2 * i], stream))
            fn()
            self.ok(self.L.hipEventRecord(ev[2 * i + 1], stream))
        self.ok(self.L.hipEventSynchronize(ev[-1]))
        out = []
        for i in range(calls):
            t = C.c_float(0)
            self.ok(self.L.hipEventElapsedTime(C.byref(t), ev[2 * i], ev[2 * i + 1]))
            out.append(t.value)
        for e in ev:
            self.L.hipEventDestroy(e)
        return out


def stat(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4),
            "max_ms": round(float(max(v)), 4)}


def layouts(T):
    def runs(per):
        n = T // per
        first = np.arange(n, dtype=np.uint32) * per
        return np.stack([first, np.full(n, per, np.uint32), first, np.arange(n, dtype=np.uint32) % 64], 1)
    return [("62500_runs_of_16" if T == 1_000_000 else "runs_of_16", runs(16)),
            ("one_run", np.array([[0, T, 0, 0]], np.uint32)),
            ("runs_of_1", runs(1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    T = a.tris - a.tris % 16
    if prk.device_count() <= 0:
        raise SystemExit("xform_bench: no HIP device")
    hip = Hip()
    s = scenes.random_soup(T, 4096, 4096, radius=16, seed=2024)  # the headline geometry (C3b)
    src = (s.vertices, s.colors, s.normals, s.uvs)
    xf = np.stack([X.rotation_yx(3.0 * k, 2.0 * k, (0.01 * k, 0.0, 0.0)) for k in range(64)])
    out = {"command": "python tools/xform_bench.py --tris %d --calls %d --host-reps %d" % (T, a.calls, a.host_reps),
           "triangles": T, "bytes_moved": 288 * T, "layouts": {}}
    r = prk.Renderer(0)
    try:
        g, d = r.geometry(*src), r.geometry_alloc()
        stream = C.c_void_p()
        assert r._L.prk_debug_geometry_stream(r._h, C.byref(stream)) == 0
        for name, runs in layouts(T):
            r.geometry_transform(g, d, runs, xf)  # (the first call grows dst: not timed)
            for t0 in (0, T // 2, T - 40):  # the output, on a sample of triangles
                got = r.geometry_download(d, first_tri=t0, tri_count=40)
                sub = runs[(runs[:, 2] < t0 + 40) & (runs[:, 2] + runs[:, 1] > t0)].astype(np.int64)
                for s0, n, d0, x in sub.tolist():
                    lo, hi = max(d0, t0), min(d0 + n, t0 + 40)
                    want = X.apply(xf[x], tuple(b[3 * (lo - d0 + s0):3 * (hi - d0 + s0)] for b in src))
                    for k in range(4):
                        assert np.array_equal(got[k][3 * (lo - t0):3 * (hi - t0)].view(np.uint32),
                                              want[k].view(np.uint32)), (name, t0, k)
            rp = C.cast(runs.ctypes.data, C.POINTER(prk.abi.PrkXformRun))
            xp = C.cast(xf.ctypes.data, C.POINTER(prk.abi.PrkXform))

            def call():
                rc = r._L.prk_geometry_transform(r._h, g, d, rp, runs.shape[0], xp, xf.shape[0])
                assert rc == 0, rc
            for _ in range(5):
                call()
            r.synchronize()
            ms = hip.timed(stream, a.calls, call)
            r.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            r.synchronize()
            wall = (time.perf_counter() - t0) * 1e3 / a.calls
            kern = []  # the kernel alone (the library's own events: after the table upload, after the kernel)
            for _ in range(a.calls):
                call()
                k = C.c_float(0)
                assert r._L.prk_debug_transform_ms(r._h, C.byref(k)) == 0
                kern.append(k.value)
            out["layouts"][name] = {"runs": int(runs.shape[0]), "transform": stat(ms),
                                    "transform_kernel_alone": stat(kern),
                                    "kernel_GBps": round(288 * T / np.median(kern) / 1e6, 1),
                                    "transform_host_clock_ms_per_call": round(wall, 4)}
            print(name, json.dumps(out["layouts"][name]), flush=True)
        # (b) the same bytes, device to device
        bufs = []
        for arr in src:
            p, q = C.c_void_p(), C.c_void_p()
            hip.ok(hip.L.hipMalloc(C.byref(p), arr.nbytes))
            hip.ok(hip.L.hipMalloc(C.byref(q), arr.nbytes))
            hip.ok(hip.L.hipMemset(p, 0, arr.nbytes))
            hip.ok(hip.L.hipMemset(q, 0, arr.nbytes))
            bufs.append((p, q, arr.nbytes))

        def copy():
            for p, q, n in bufs:
                hip.ok(hip.L.hipMemcpyAsync(q, p, n, 3, stream))  # hipMemcpyDeviceToDevice
        for _ in range(5):
            copy()
        r.synchronize()
        ms = hip.timed(stream, a.calls, copy)
        r.synchronize()
        out["d2d_copy"] = dict(stat(ms), GBps=round(288 * T / np.median(ms) / 1e6, 1))
        print("d2d_copy", json.dumps(out["d2d_copy"]), flush=True)
        for p, q, _ in bufs:
            hip.L.hipFree(p)
            hip.L.hipFree(q)
        # (c) the host way: numpy transform + prk_geometry_update, and the update alone
        M = xf[1]
        t_all, t_up = [], []
        for i in range(a.host_reps + 1):
            r.synchronize()
            t0 = time.perf_counter()
            moved = X.apply(M, src)
            t1 = time.perf_counter()
            r.geometry_update(g, *moved)
            r.synchronize()
            t2 = time.perf_counter()
            if i:
                t_all.append((t2 - t0) * 1e3)
                t_up.append((t2 - t1) * 1e3)
        out["host_numpy_plus_update"] = stat(t_all)
        out["host_update_alone"] = stat(t_up)
        print("host", json.dumps(out["host_numpy_plus_update"]), json.dumps(out["host_update_alone"]), flush=True)
        floor = out["d2d_copy"]["median_ms"]
        for name in out["layouts"]:
            lay = out["layouts"][name]
            lay["transform_over_d2d_copy"] = round(lay["transform"]["median_ms"] / floor, 3)
            lay["kernel_over_d2d_copy"] = round(lay["transform_kernel_alone"]["median_ms"] / floor, 3)
            lay["call_within_1.5x_of_copy"] = bool(lay["transform_over_d2d_copy"] <= 1.5)
        out["notes"] = [
            "transform: events around the whole call on its stream: the host's table preparation while the stream "
            "runs dry, the upload of the tables (4 + 16 bytes a run, 48 a matrix) and the kernel; "
            "transform_kernel_alone: the kernel only.",
            "Where a layout's call is outside 1.5x of the copy while its kernel is inside, the difference is the "
            "per-call table (prepared on the host and uploaded before the kernel), not an access pattern of the "
            "arrays; the kernel's own distance from the one-run layout is the run lookup: a dependent binary search "
            "over the scan (log2(runs) loads by one wave of a workgroup's three) before the workgroup streams."]
    finally:
        r.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
