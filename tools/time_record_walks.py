"""Time the record walks of a handle (prk_records_advance / _spans / _rows)
beside their host-input calls (prk_advance_edge_lists, prk_span_records,
prk_row_records) on the same lists, in the same run; prk_records_advance into
a new handle with no host output; and the statistics pass alone
(prk_debug_list_stats: k_list_stats, k_list_most and their download).

Two scenes: ConstructSphere as one list (2072 records, 256 rows) and C3b's
geometry (1 M triangles, 4096 rows) as 16-triangle objects (62,500 lists).

usage: python tools/time_record_walks.py [--tris N] [--reps K] [--case all|sphere|c3b] [--json OUT]
Every figure is the host time of the whole call (the calls are synchronous),
into arrays made once outside the timed part; the span and row calls are the
filling calls at the capacities a sizing call returned.  Medians of K repeats
after one warm-up, the ways taken in turn within every repeat.  Before the
timing every handle call's outputs are compared with its host-input call's,
word for word."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpu-renderer_amd"))
import numpy as np  # noqa: E402
import prk  # noqa: E402
from prk import abi, scenes  # noqa: E402


def sphere_scene():
    V, Cc, N, UV = prk.construct_sphere()
    base = scenes.random_soup(1, 256, 256, seed=0)
    return scenes.Scene(256, 256, V.copy(), Cc.copy(), N.copy(), UV.copy(), base.transform, scenes.LIGHTS_ONE,
                        scenes.AMBIENT_ONE, base.texture, P=(0.0, 0.0, 2.0), name="ConstructSphere_256x256")


def ms(v):
    return round(float(np.median(v)) * 1e3, 3)


def ok(name, rc):
    if rc != abi.PRK_OK:
        raise prk.PrkError(name, rc)


def measure(s, per, reps):
    r = prk.Renderer(0)
    try:
        L, ctx = r._L, r._h
        r.set_camera(s.prk_transform(), s.prk_lights())
        g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        rec = r.records_from_geometry(g, s.tri_count, P=s.P, setup=3, tris_per_object=per)
        words, counts = rec.download(), rec.counts()
        nl, n, h, H = int(counts.size), int(words.shape[0]), rec.handle, s.height
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        u64 = lambda: C.c_uint64(0)  # noqa: E731
        # sizes, and the outputs of either way (made once)
        total, nrow, npair = u64(), u64(), u64()
        sc, rc_ = np.zeros(nl, np.uint32), np.zeros(nl, np.uint32)
        ok("size", L.prk_records_spans(ctx, h, 0, nl, H, None, 0, p(sc), C.byref(total)))
        ok("size", L.prk_records_rows(ctx, h, 0, nl, H, None, 0, None, 0, p(rc_), C.byref(nrow), C.byref(npair)))
        ns, nr, npr = total.value, nrow.value, npair.value
        out, nxt = np.empty((n, 27), np.uint32), np.empty(n, np.int32)
        spans, scs = np.empty((ns, 25), np.uint32), np.zeros(nl, np.uint32)
        rows, pairs, rcs = np.empty((nr, 2), np.int32), np.empty((npr, 24), np.uint32), np.zeros(nl, np.uint32)
        outputs = {"advance": (out, nxt), "spans": (spans, scs), "rows": (rows, pairs, rcs)}
        stats = np.zeros((nl, 5), np.uint64)
        made = []

        def keep_only():
            hh = C.c_int32(-1)
            ok("keep", L.prk_records_advance(ctx, h, 0, nl, H, C.byref(hh), None, None))
            made.append(hh.value)

        ways = [
            ("advance", "host", lambda: ok("a", L.prk_advance_edge_lists(ctx, p(words), p(counts), nl, H, p(out),
                                                                         p(nxt)))),
            ("advance", "handle", lambda: ok("a", L.prk_records_advance(ctx, h, 0, nl, H, None, p(out), p(nxt)))),
            ("advance", "handle_keep_no_host", keep_only),
            ("spans", "host", lambda: ok("s", L.prk_span_records(ctx, p(words), p(counts), nl, H, p(spans), ns,
                                                                 p(scs), C.byref(total)))),
            ("spans", "handle", lambda: ok("s", L.prk_records_spans(ctx, h, 0, nl, H, p(spans), ns, p(scs),
                                                                    C.byref(total)))),
            ("rows", "host", lambda: ok("r", L.prk_row_records(ctx, p(words), p(counts), nl, H, p(rows), nr,
                                                               p(pairs), npr, p(rcs), C.byref(nrow),
                                                               C.byref(npair)))),
            ("rows", "handle", lambda: ok("r", L.prk_records_rows(ctx, h, 0, nl, H, p(rows), nr, p(pairs), npr,
                                                                  p(rcs), C.byref(nrow), C.byref(npair)))),
            ("statistics", "handle", lambda: ok("t", L.prk_debug_list_stats(ctx, h, 0, nl, H, p(stats)))),
        ]
        t = {(a, b): [] for a, b, _ in ways}
        sums = {}
        for i in range(reps + 1):
            for a, b, fn in ways:
                r.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if i:
                    t[(a, b)].append(t1 - t0)
                while made:  # (outside the timed part)
                    ok("destroy", L.prk_records_destroy(ctx, made.pop()))
                if i == 0 and b in ("host", "handle") and a in outputs:  # the two ways agree, word for word
                    sums[(a, b)] = [zlib.crc32(x) for x in outputs[a]]
                    for x in outputs[a]:
                        x.fill(0)
            if i == 0:
                for a in outputs:
                    assert sums[(a, "host")] == sums[(a, "handle")], a
        res = {"scene": s.name, "tris_per_object": per, "lists": nl, "records": n, "record_bytes": int(words.nbytes),
               "height": H, "spans": ns, "rows": nr, "pairs": npr, "routes": r.list_routes(),
               "candidates": int((stats[:, 2] > 0).sum()), "ms": {}}
        for (a, b), v in t.items():
            res["ms"].setdefault(a, {})[b] = {"median": ms(v), "min_max": [round(min(v) * 1e3, 3),
                                                                            round(max(v) * 1e3, 3)]}
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("all", "sphere", "c3b"), default="all")
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {"command": "python tools/time_record_walks.py --tris %d --reps %d --case %s" % (a.tris, a.reps, a.case),
           "cases": {}}
    if a.case in ("all", "sphere"):
        sp = sphere_scene()
        res["cases"]["sphere_one_list"] = measure(sp, sp.tri_count, a.reps)
        print(json.dumps(res["cases"]["sphere_one_list"]), flush=True)
    if a.case in ("all", "c3b"):
        c3b = scenes.random_soup(a.tris, 4096, 4096, radius=16, seed=2024)  # C3b
        res["cases"]["c3b_16_triangle_objects"] = measure(c3b, 16, a.reps)
        print(json.dumps(res["cases"]["c3b_16_triangle_objects"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
