"""Time prk_texture_from_target on a 4096 x 4096 source for factor 1, 2 and 4,
each from a library-owned target (16-byte aligned rows) and from a
caller-bound target 4 bytes past a 16-byte boundary with a pitch of 4 * W + 4
and x0 = 1 (rows at every word of a 16-byte line), beside the yardstick of
this pass in the same process:

  (a) from_target  the call, HIP events on its own stream around each of K
                   warm calls, median;
  (b) d2d_copy     hipMemcpy2DAsync device to device of the source rectangle's
                   bytes on the same stream: the pass reads S bytes and writes
                   S / factor^2, the copy reads and writes S.

usage: python tools/texture_bench.py [--size N] [--calls K] [--json OUT]
Every case's output is compared with tests/texref.py's on three strips of rows
before it is timed."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpu-renderer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import prk  # noqa: E402
import texref  # noqa: E402
from xform_bench import Hip, stat  # noqa: E402


def check(r, tex, frame, rect, factor):
    got = r.texture_download(tex)
    x0, y0, w, h = rect
    dh = h // factor
    for d0 in (0, dh // 2, dh - 8):
        want = texref.resolve(frame[y0 + factor * d0:y0 + factor * (d0 + 8), x0:x0 + w], factor)
        assert np.array_equal(got[d0:d0 + 8, :w // factor], want), (rect, factor, d0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--json")
    a = ap.parse_args()
    N = a.size - a.size % 32
    if prk.device_count() <= 0:
        raise SystemExit("texture_bench: no HIP device")
    hip = Hip()
    hip.L.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                       C.c_void_p]
    rng = np.random.default_rng(2025)
    frame = rng.integers(0, 2**32, (N, N), dtype=np.uint64).astype(np.uint32)
    z = np.zeros((N, N), np.float32)
    out = {"command": "python tools/texture_bench.py --size %d --calls %d" % (N, a.calls), "source": [N, N], "cases": {}}
    r = prk.Renderer(0)
    mem = []
    try:
        stream = C.c_void_p()
        assert r._L.prk_debug_geometry_stream(r._h, C.byref(stream)) == 0
        upitch = 4 * N + 4
        ucol, uz, scratch = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p, n in ((ucol, 16 + N * upitch), (uz, 4 * N * N), (scratch, 4 * N * N)):
            hip.ok(hip.L.hipMalloc(C.byref(p), n))
            hip.ok(hip.L.hipMemset(p, 0, n))
            mem.append(p)
        for layout in ("aligned", "unaligned"):
            if layout == "aligned":
                r.target_alloc(N, N)
            else:
                r.target_bind(ucol.value + 4, upitch, uz.value, N, N)
            r.upload(frame, z)
            color, pitch = r.target()[:2]
            for factor in (1, 2, 4):
                x0 = 0 if layout == "aligned" else 1
                w = N if layout == "aligned" else (N - 1) - (N - 1) % factor
                rect = (x0, 0, w, N)
                tex = r.texture_alloc(w // factor, N // factor)
                r.texture_from_target(tex, rect, factor)
                check(r, tex, frame, rect, factor)

                def call():
                    rc = r._L.prk_texture_from_target(r._h, tex, x0, 0, w, N, factor, 0, 0)
                    assert rc == 0, rc

                def copy():
                    hip.ok(hip.L.hipMemcpy2DAsync(scratch, 4 * w, C.c_void_p(color + 4 * x0), pitch, 4 * w, N, 3,
                                                  stream))  # hipMemcpyDeviceToDevice
                res = {}
                for name, fn in (("from_target", call), ("d2d_copy", copy)):
                    for _ in range(5):
                        fn()
                    r.synchronize()
                    res[name] = stat(hip.timed(stream, a.calls, fn))
                    r.synchronize()
                src_bytes = 4 * w * N
                res["source_bytes"] = src_bytes
                res["from_target_GBps_read"] = round(src_bytes / res["from_target"]["median_ms"] / 1e6, 1)
                res["d2d_copy_GBps_read"] = round(src_bytes / res["d2d_copy"]["median_ms"] / 1e6, 1)
                res["from_target_over_d2d_copy"] = round(res["from_target"]["median_ms"] / res["d2d_copy"]["median_ms"], 3)
                res["within_1.5x_of_copy"] = bool(res["from_target_over_d2d_copy"] <= 1.5)
                out["cases"]["%s_factor_%d" % (layout, factor)] = res
                print(layout, factor, json.dumps(res), flush=True)
        r.synchronize()
        out["notes"] = [
            "from_target: events around the whole call on its stream (the mark on the context's stream, the wait for "
            "it, the kernel); d2d_copy: hipMemcpy2DAsync device to device of the source rectangle's bytes on the same "
            "stream; medians of %d warm calls, one process.  A source and destinations that fit the 256 MiB Infinity "
            "Cache give warm-cache times." % a.calls]
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
