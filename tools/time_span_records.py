"""Time prk_span_records (the spans DrawModelOptimized(RenderQueue) queues for
every list of a batch: upload, import, one GPU thread's walk per list with
the emission, count scan, pack, download) on the cases of
tools/time_advance_lists.py: C3b's geometry as one-triangle and as
16-triangle lists, and ConstructSphere as one list.  The triangle count is
scaled down from C3b's 1 M (--tris) so that the packed spans stay within a
few hundred MB; the sizes used are in the output.

usage: python tools/time_span_records.py [--tris N] [--reps K] [--advance-only] [--json OUT]
Per case, host wall time (median of K after one warm-up), transfers included:
  span_ms        the filling call (spans != NULL, capacity = the total)
  count_ms       the counting call (spans == NULL)
  advance_ms     prk_advance_edge_lists on the same batch (the same walk
                 without the emission, plus its export and download)
--advance-only times the last alone: it runs on a tree without
prk_span_records, which gives the figure of the commit before it.
  span_fresh_array_ms  the filling call into a new numpy array every time
These calls but the last write into arrays made and touched beforehand and
used again: a fresh output array adds its page faults to the copy that fills
it, which is the caller's choice and not the call's cost.  Compare figures of
one run on one machine only."""
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


def median_ms(r, fn, reps):
    dts = []
    for i in range(reps + 1):
        r.synchronize()
        t0 = time.perf_counter()
        fn()
        if i:
            dts.append(time.perf_counter() - t0)
    return round(float(np.median(dts)) * 1e3, 2)


def edge_rows(words, counts, height):
    """The batch's edge-rows and span slots (half of each list's, prk.h)."""
    w = words.view(np.int32)
    rows = np.maximum(0, np.minimum(w[:, 0], height).astype(np.int64) - w[:, 7])
    ids = np.repeat(np.arange(counts.shape[0]), counts)
    per_list = np.bincount(ids, weights=rows, minlength=counts.shape[0]).astype(np.int64)
    return int(rows.sum()), int((per_list // 2).sum())


def case(r, words, counts, height, reps, advance_only):
    er, slots = edge_rows(words, counts.astype(np.int64), height)
    out = {"lists": int(counts.shape[0]), "records": int(words.shape[0]), "height": height, "edge_rows": er,
           "span_slots": slots}
    L, h = r._L, r._h
    wp, cp, n = words.ctypes.data, counts.ctypes.data, counts.shape[0]
    rec_out, nxt = np.zeros_like(words), np.zeros(words.shape[0], np.int32)

    def advance():
        assert L.prk_advance_edge_lists(h, wp, cp, n, height, rec_out.ctypes.data, nxt.ctypes.data) == 0

    out["advance_ms"] = median_ms(r, advance, reps)
    if advance_only:
        return out
    sc = np.zeros(counts.shape[0], np.uint32)
    total = C.c_uint64(0)

    def count():
        assert L.prk_span_records(h, wp, cp, n, height, None, 0, sc.ctypes.data, C.byref(total)) == 0

    out["count_ms"] = median_ms(r, count, reps)
    spans = np.zeros((total.value, 25), np.uint32)

    def fill():
        assert L.prk_span_records(h, wp, cp, n, height, spans.ctypes.data, spans.shape[0], sc.ctypes.data,
                                  C.byref(total)) == 0

    out["span_ms"] = median_ms(r, fill, reps)

    def fill_fresh():  # as Renderer.span_records fills: a new array, its page faults inside the copy
        sp = np.empty((total.value, 25), np.uint32)
        assert L.prk_span_records(h, wp, cp, n, height, sp.ctypes.data, sp.shape[0], sc.ctypes.data,
                                  C.byref(total)) == 0

    out["span_fresh_array_ms"] = median_ms(r, fill_fresh, reps)
    out["spans"] = int(total.value)
    out["span_bytes"] = int(spans.nbytes)
    out["span_over_advance"] = round(out["span_ms"] / max(1e-9, out["advance_ms"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--advance-only", action="store_true", help="prk_advance_edge_lists alone (a tree before this call)")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"command": "python tools/time_span_records.py --tris %d --reps %d%s" % (
        a.tris, a.reps, " --advance-only" if a.advance_only else ""), "cases": {}}
    s = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024)  # C3b, fewer triangles
    r = prk.Renderer(0)
    try:
        r.set_camera(s.prk_transform(), s.prk_lights())
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        for per in (1, 16):
            words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
            k = "c3b_tris_per_list_%d" % per
            out["cases"][k] = case(r, words, counts, s.height, a.reps, a.advance_only)
            print(json.dumps({k: out["cases"][k]}), flush=True)
        V, Cc, N, UV = prk.construct_sphere()
        base = scenes.random_soup(1, 256, 256, seed=0)
        r.set_camera(base.prk_transform(), base.prk_lights())
        g = r.geometry(V, Cc, N, UV)
        words, counts = r.edge_records(g, V.shape[0] // 3, P=(0.0, 0.0, 2.0), setup=3)
        out["cases"]["sphere_one_list"] = case(r, words, counts, 256, a.reps, a.advance_only)
        print(json.dumps({"sphere_one_list": out["cases"]["sphere_one_list"]}), flush=True)
    finally:
        r.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
