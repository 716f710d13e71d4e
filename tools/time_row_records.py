"""Time prk_row_records (the row work DrawModelOptimizedLines queues for every
list of a batch: upload, import, one GPU thread's walk per list with the pair
and row emission, two count scans, pack, download) and prk_draw_rows on the
cases of tools/time_span_records.py: C3b's geometry as one-triangle and as
16-triangle lists, and ConstructSphere as one list.  The triangle count is
scaled down from C3b's 1 M (--tris) as there; the sizes used are in the output.

usage: python tools/time_row_records.py [--tris N] [--reps K] [--baselines-only] [--json OUT]
Per case, host wall time (median of K after one warm-up), transfers included:
  row_ms          the filling call (both arrays, capacities = the totals)
  row_count_ms    the counting call (rows == pairs == NULL)
  span_ms         prk_span_records' filling call on the same batch (the same
                  walk, one dword a record more, no row records)
  span_count_ms   its counting call
  advance_ms      prk_advance_edge_lists on the same batch
  draw_rows_ms    prk_draw_rows of the row records (upload, regroup on the
                  GPU, spans back into the pending frame), then prk_reset_draws
  draw_spans_ms   prk_draw_spans of the same pairs as spans (a host copy), then
                  prk_reset_draws
--baselines-only times span_ms, span_count_ms, advance_ms and draw_spans_ms
alone: with PRK_LIB set to the library of the commit before these calls it
gives that commit's figures.  All calls write into arrays made and touched
beforehand.  Compare figures of one run on one machine only."""
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
from prk import abi, scenes  # noqa: E402


def median_ms(r, fn, reps):
    dts = []
    for i in range(reps + 1):
        r.synchronize()
        t0 = time.perf_counter()
        fn()
        if i:
            dts.append(time.perf_counter() - t0)
    return round(float(np.median(dts)) * 1e3, 2)


def case(r, tex, words, counts, height, reps, baselines_only):
    out = {"lists": int(counts.shape[0]), "records": int(words.shape[0]), "height": height}
    L, h = r._L, r._h
    wp, cp, n = words.ctypes.data, counts.ctypes.data, counts.shape[0]
    rec_out, nxt = np.zeros_like(words), np.zeros(words.shape[0], np.int32)

    def advance():
        assert L.prk_advance_edge_lists(h, wp, cp, n, height, rec_out.ctypes.data, nxt.ctypes.data) == 0

    out["advance_ms"] = median_ms(r, advance, reps)
    sc = np.zeros(counts.shape[0], np.uint32)
    total = C.c_uint64(0)

    def span_count():
        assert L.prk_span_records(h, wp, cp, n, height, None, 0, sc.ctypes.data, C.byref(total)) == 0

    out["span_count_ms"] = median_ms(r, span_count, reps)
    spans = np.zeros((total.value, 25), np.uint32)

    def span_fill():
        assert L.prk_span_records(h, wp, cp, n, height, spans.ctypes.data, spans.shape[0], sc.ctypes.data,
                                  C.byref(total)) == 0

    out["span_ms"] = median_ms(r, span_fill, reps)
    out["spans"] = int(total.value)

    def draw_spans():
        assert L.prk_draw_spans(h, spans.ctypes.data, spans.shape[0], abi.PRK_SEM_AVX, 1, tex) == 0
        assert L.prk_reset_draws(h) == 0

    out["draw_spans_ms"] = median_ms(r, draw_spans, reps)
    if baselines_only:
        return out
    rc = np.zeros(counts.shape[0], np.uint32)
    nrow, npair = C.c_uint64(0), C.c_uint64(0)

    def row_count():
        assert L.prk_row_records(h, wp, cp, n, height, None, 0, None, 0, rc.ctypes.data, C.byref(nrow),
                                 C.byref(npair)) == 0

    out["row_count_ms"] = median_ms(r, row_count, reps)
    rows, pairs = np.zeros((nrow.value, 2), np.int32), np.zeros((npair.value, 24), np.uint32)

    def row_fill():
        assert L.prk_row_records(h, wp, cp, n, height, rows.ctypes.data, rows.shape[0], pairs.ctypes.data,
                                 pairs.shape[0], rc.ctypes.data, C.byref(nrow), C.byref(npair)) == 0

    out["row_ms"] = median_ms(r, row_fill, reps)
    assert npair.value == total.value
    out["rows"], out["pairs"] = int(nrow.value), int(npair.value)
    out["row_bytes"] = int(rows.nbytes + pairs.nbytes)
    out["span_bytes"] = int(spans.nbytes)

    def draw_rows():
        assert L.prk_draw_rows(h, rows.ctypes.data, rows.shape[0], pairs.ctypes.data, pairs.shape[0],
                               abi.PRK_SEM_AVX, 1, tex) == 0
        assert L.prk_reset_draws(h) == 0

    out["draw_rows_ms"] = median_ms(r, draw_rows, reps)
    out["row_over_span"] = round(out["row_ms"] / max(1e-9, out["span_ms"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baselines-only", action="store_true", help="the existing calls alone (a library before these)")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"command": "python tools/time_row_records.py --tris %d --reps %d%s" % (
        a.tris, a.reps, " --baselines-only" if a.baselines_only else ""), "cases": {}}
    s = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024, textured=True)  # C3b, fewer triangles
    r = prk.Renderer(0)
    try:
        r.set_camera(s.prk_transform(), s.prk_lights())
        tex = r.texture(s.texture)
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        for per in (1, 16):
            words, counts = r.edge_records(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
            k = "c3b_tris_per_list_%d" % per
            out["cases"][k] = case(r, tex, words, counts, s.height, a.reps, a.baselines_only)
            print(json.dumps({k: out["cases"][k]}), flush=True)
        V, Cc, N, UV = prk.construct_sphere()
        base = scenes.random_soup(1, 256, 256, seed=0)
        r.set_camera(base.prk_transform(), base.prk_lights())
        g = r.geometry(V, Cc, N, UV)
        words, counts = r.edge_records(g, V.shape[0] // 3, P=(0.0, 0.0, 2.0), setup=3)
        out["cases"]["sphere_one_list"] = case(r, tex, words, counts, 256, a.reps, a.baselines_only)
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
