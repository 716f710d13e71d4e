"""Time prk_layer_from_target and prk_target_from_layer on a 4096 x 4096
target, from / into a library-owned target (16-byte aligned rows) and a
caller-bound one 4 bytes past a 16-byte boundary with a pitch of 4 * W + 4 and
z 4 bytes past one (rows at every word of a 16-byte line), beside the
yardstick of this pass in the same process:

  save             prk_layer_from_target of the whole target;
  copy             prk_target_from_layer, PRK_MERGE_COPY;
  greater_none     PRK_MERGE_GREATER where no pixel of the layer wins;
  greater_all      PRK_MERGE_GREATER where every pixel wins;
  d2d_copy         hipMemcpy2DAsync device to device of the same rectangle's
                   colour bytes, then of its z bytes, on the same stream: the
                   bytes save and copy move (the merge rules read the target's
                   z as well).

HIP events on the calls' stream around each of K warm calls, median.  Then one
PRK_MERGE_COPY restore beside one C3b frame (1M random triangles, Phong +
texture, FillLineOptimized semantics) on that target: what a caller saves by
restoring a static frame instead of drawing it.

usage: python tools/layer_bench.py [--size N] [--calls K] [--tris T] [--json OUT]
Every case's output is compared with tests/layerref.py's on three strips of
rows before it is timed."""
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
import layerref  # noqa: E402
import prk  # noqa: E402
from prk import abi, scenes  # noqa: E402
from xform_bench import Hip, stat  # noqa: E402


def strips(n):
    return [slice(d0, d0 + 8) for d0 in (0, n // 2, n - 8)]


def check(got, want, label):
    for s in strips(got[0].shape[0]):
        for g, w in zip(got, want):
            assert np.array_equal(layerref.words(g)[s], layerref.words(w)[s]), (label, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--json")
    a = ap.parse_args()
    N = a.size - a.size % 32
    if prk.device_count() <= 0:
        raise SystemExit("layer_bench: no HIP device")
    hip = Hip()
    hip.L.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                       C.c_void_p]
    rng = np.random.default_rng(2025)
    frame = rng.integers(0, 2**32, (N, N), dtype=np.uint64).astype(np.uint32)
    other = rng.integers(0, 2**32, (N, N), dtype=np.uint64).astype(np.uint32)
    z_mid = rng.uniform(-1, 1, (N, N)).astype(np.float32)
    out = {"command": "python tools/layer_bench.py --size %d --calls %d --tris %d" % (N, a.calls, a.tris),
           "target": [N, N], "cases": {}}
    r = prk.Renderer(0)
    mem = []
    try:
        stream = C.c_void_p()
        assert r._L.prk_debug_geometry_stream(r._h, C.byref(stream)) == 0
        upitch = 4 * N + 4
        ucol, uz, scratch_c, scratch_z = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p, n in ((ucol, 16 + N * upitch), (uz, 16 + 4 * N * N), (scratch_c, 4 * N * N), (scratch_z, 4 * N * N)):
            hip.ok(hip.L.hipMalloc(C.byref(p), n))
            hip.ok(hip.L.hipMemset(p, 0, n))
            mem.append(p)
        for layout in ("aligned", "unaligned"):
            if layout == "aligned":
                r.target_alloc(N, N)
            else:
                r.target_bind(ucol.value + 4, upitch, uz.value + 4, N, N)
            color, pitch, zbuf = r.target()[:3]
            # three layers through the target: the frame itself at z_mid, and another frame below / above it
            layers = {}
            for name, c, z in (("mid", frame, z_mid), ("below", other, z_mid - 4), ("above", other, z_mid + 4)):
                r.upload(c, z)
                layers[name] = r.layer_alloc(N, N)
                r.layer_from_target(layers[name])
                check(r.layer_download(layers[name]), (c, z), (layout, "save", name))
            dst = r.layer_alloc(N, N)
            r.upload(frame, z_mid)
            whole = (0, 0, N, N)
            for name, layer, rule in (("copy", "mid", abi.PRK_MERGE_COPY), ("greater_none", "below", abi.PRK_MERGE_GREATER),
                                      ("greater_all", "above", abi.PRK_MERGE_GREATER)):
                r.upload(frame, z_mid)
                r.target_from_layer(layers[layer], rule=rule)
                lay = (frame, z_mid) if layer == "mid" else (other, z_mid + (4 if layer == "above" else -4))
                want = layerref.merge(frame, z_mid, 0, lay[0], lay[1], whole, (0, 0), rule)
                assert np.array_equal(want[0], other if name == "greater_all" else frame)
                check(r.download(), want, (layout, name))
            r.upload(frame, z_mid)

            def save():
                assert r._L.prk_layer_from_target(r._h, dst, 0, 0, N, N, 0, 0) == 0

            def merge(layer, rule):
                def call():
                    assert r._L.prk_target_from_layer(r._h, layers[layer], 0, 0, N, N, 0, 0, rule) == 0
                return call

            def d2d():
                hip.ok(hip.L.hipMemcpy2DAsync(scratch_c, 4 * N, C.c_void_p(color), pitch, 4 * N, N, 3, stream))
                hip.ok(hip.L.hipMemcpy2DAsync(scratch_z, 4 * N, C.c_void_p(zbuf), 4 * N, 4 * N, N, 3, stream))

            # greater_all last: its first call replaces the target's pixels by the layer's, later ones tie and lose,
            # so each timed call gets the target back first (a copy, outside the events)
            res = {}
            for name, fn in (("d2d_copy", d2d), ("save", save), ("copy", merge("mid", abi.PRK_MERGE_COPY)),
                             ("greater_none", merge("below", abi.PRK_MERGE_GREATER))):
                for _ in range(5):
                    fn()
                r.synchronize()
                res[name] = stat(hip.timed(stream, a.calls, fn))
                r.synchronize()
            restore, win = merge("mid", abi.PRK_MERGE_COPY), merge("above", abi.PRK_MERGE_GREATER)
            ev = hip.events(2 * a.calls)
            for i in range(5 + a.calls):
                restore()
                k = max(i - 5, 0)
                hip.ok(hip.L.hipEventRecord(ev[2 * k], stream))
                win()
                hip.ok(hip.L.hipEventRecord(ev[2 * k + 1], stream))
            r.synchronize()
            ms = []
            for k in range(a.calls):
                t = C.c_float(0)
                hip.ok(hip.L.hipEventElapsedTime(C.byref(t), ev[2 * k], ev[2 * k + 1]))
                ms.append(t.value)
            for e in ev:
                hip.L.hipEventDestroy(e)
            res["greater_all"] = stat(ms)
            res["copy_bytes"] = nbytes = 8 * N * N  # colour + z, read once and written once
            base = res["d2d_copy"]["median_ms"]
            for name in ("d2d_copy", "save", "copy", "greater_none", "greater_all"):
                res[name]["GBps_moved"] = round(nbytes / res[name]["median_ms"] / 1e6, 1)
                if name != "d2d_copy":
                    res[name]["over_d2d_copy"] = round(res[name]["median_ms"] / base, 3)
            for name in ("save", "copy"):  # they move exactly the copy's bytes: the 1.5x margin of §2.1 / §2.2
                res[name]["within_1.5x_of_copy"] = bool(res[name]["over_d2d_copy"] <= 1.5)
            out["cases"][layout] = res
            print(layout, json.dumps(res), flush=True)
            if layout == "aligned":
                # one restore beside one C3b frame on this target, this process
                s = scenes.random_soup(a.tris, N, N, radius=16, seed=2024)
                r.set_camera(s.prk_transform(), s.prk_lights())
                g, t = r.geometry(s.vertices, s.colors, s.normals, s.uvs), r.texture(s.texture)

                def frame_c3b():
                    r.clear_on_flush()
                    r.draw_model_optimized(g, s.tri_count, P=s.P, bitmap=t, phong=True)
                    r.complete_all_work()

                walls = {}
                for name, fn in (("c3b_frame", frame_c3b), ("copy_restore", restore)):
                    for _ in range(5):
                        fn()
                    r.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn()
                    r.synchronize()
                    walls[name + "_ms"] = round((time.perf_counter() - t0) * 1e3 / a.calls, 4)
                walls["frame_over_restore"] = round(walls["c3b_frame_ms"] / walls["copy_restore_ms"], 2)
                out["restore_vs_c3b_frame"] = walls
                print("restore_vs_c3b_frame", json.dumps(walls), flush=True)
            for name in layers.values():
                r.layer_destroy(name)
            r.layer_destroy(dst)
        r.synchronize()
        out["notes"] = [
            "Events around the whole call on its stream (the mark on the context's stream, the wait for it, the "
            "kernel); d2d_copy: two hipMemcpy2DAsync device to device, the rectangle's colour bytes and its z bytes, "
            "on the same stream; medians of %d warm calls, one process.  greater_all: each timed call follows a "
            "PRK_MERGE_COPY restore outside its events, so every pixel wins every time.  save and copy move the "
            "copy's bytes and are held to 1.5x of it; the merge rules read the target's z as well and are reported "
            "as a ratio only.  Planes that fit the 256 MiB Infinity Cache give warm-cache times." % a.calls,
            "restore_vs_c3b_frame: host clock over %d queued calls ending in a synchronize, per call; the frame is "
            "clear_on_flush + one draw of %d triangles + flush." % (a.calls, a.tris)]
    finally:
        r.close()
        for p in mem:
            hip.L.hipFree(p)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
