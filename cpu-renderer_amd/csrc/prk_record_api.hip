// prk_record_api.hip — the record API of include/prk.h: FillEdgeTable's
// records from the GPU (prk_edge_records), the record handles that keep them
// on the device (prk_records_*), the walks of such lists -- advance, spans,
// rows -- from the caller's memory or a handle, routed list by list
// (ListRouter, WalkPlan), and the span handles (prk_spans_*).  The kernels
// are prk_records.hip's and prk_spans.hip's, through prk_launch.h; the
// scratch is the span pass's (prk_context::SpanScratch), taken while the
// device is idle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "prk_ctx.h"

#include "../../include/prk_edge_count.h"
using prk::ObjDesc;
using prk::ObjEdge;
using prk::ObjRun;
using prk::PairRaw;
using prk::kAdvWgCaps;
using prk::packed_edge_bytes;
using prk::packed_span_bytes;

extern "C" {

// FillEdgeTable's return value (projekt.cpp:3882-4121), computed on the host
// at the call so the drop-in can return it there: the number of edge_info
// records the reference writes for one object, i.e. over its triangles that
// pass the back-face test (3926-3943) the edges with MaxY > 0 (3968) and
// MinY != MaxY (4066).  The same float operations as the device setup
// (ProjectVertex 74-93, Normalize(a) = (1/sqrt(a.a))*a); the library is built
// with -ffp-contract=off, so host and device round alike.  The setup itself
// (edges, gradients, lighting, MergeSort) runs on the GPU at the flush.
// Per triangle: include/prk_edge_count.h (the drop-in header inlines it).
int prk_fill_edge_count(const float *V, uint32_t vertex_count, const float P[3], const prk_transform *T,
                        uint32_t *count_out) {
    if (!count_out || !T || (!V && vertex_count >= 3)) return PRK_ERR_ARG;
    const float p0 = P ? P[0] : 0.0f, p1 = P ? P[1] : 0.0f, p2 = P ? P[2] : 0.0f;
    uint32_t n = 0;
    for (uint32_t t = 0; t < vertex_count / 3; ++t) n += prk_tri_edge_count(V + 9 * (size_t)t, p0, p1, p2, T);
    *count_out = n;
    return PRK_OK;
}

// FillEdgeTable's records of a batch of objects, set up on the GPU: the span
// path's own chain (k_objtri_count -> scan -> emit -> sort, prk_spans.hip)
// with the record setup (k_rec_emit: all 27 fields, the sort key on the true
// YMin) in place of the frame's, then k_rec_export packs the sorted edges as
// prk_edge.  The scratch is the span path's (c->spans), taken only once the
// device is idle, as prk_geometry_update takes the geometry; nothing the
// next flush reads is kept in it from one pass to the next.  The call needs
// no target (the frame parameters' rows only bound the span slots, which are
// not used here), records no draw and leaves c->draws, the pending edge /
// span input and c->stats as they are.
// keep (prk_records_from_geometry): k_rec_export writes into a buffer of the
// call's own, handed over in *keep, instead of the scratch -- nothing is
// downloaded (records, capacity, counts: null; the objects' counts stay in
// d_reccnt, *nobj_out of them).
static int edge_records_run(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                            uint32_t tris_per_object, const float P[3], int32_t setup, prk_edge *records,
                            uint64_t capacity, uint32_t *counts, uint64_t *total_out, void **keep,
                            uint32_t *nobj_out) {
    if (!c || !total_out) return PRK_ERR_ARG;
    *total_out = 0;
    if (geometry < 0 || geometry >= (int32_t)c->geoms.size() || tris_per_object == 0) return PRK_ERR_ARG;
    if (setup < 0 || setup > (PRK_SETUP_PHONG | PRK_SETUP_BITMAP)) return PRK_ERR_ARG;
    const Geometry &g = c->geoms[geometry];
    if ((uint64_t)first_tri + tri_count > g.vertex_count / 3) return PRK_ERR_ARG;
    if (!c->have_camera) return PRK_ERR_ARG;
    if (nobj_out) *nobj_out = 0;
    if (tri_count == 0) return PRK_OK;
    const uint32_t nt = tri_count, per = std::min(tris_per_object, tri_count);
    const uint32_t nobj = (uint32_t)(((uint64_t)nt + per - 1) / per);
    if (3ull * nt >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;  // 31-bit edge slots
    if (nobj_out) *nobj_out = nobj;
    // MergeSort key: (object, true YMin: 31 bits, recursion path)
    auto bitlen = [](uint64_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b; };
    const uint32_t maxn = 3 * per;  // the most edges FillEdgeTable writes for one object
    const uint32_t pbits = bitlen(maxn) + 1, ybits = 31, obits = std::max(1u, bitlen(nobj - 1));
    if (obits + ybits + pbits > 64) return PRK_ERR_LIMIT;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // frames in flight use the scratch below and read the geometry
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    prk::FrameParams fp;
    frame_params(c, fp);
    fp.tri_count = nt;
    fp.ndraws = 1;
    prk::DrawRec d{};
    d.V = g.V; d.C = g.C; d.N = g.N; d.UV = g.UV;
    d.geom = geometry;
    d.geom_tri0 = first_tri;
    d.tri_count = nt;
    d.mode = prk::MODE_AVX;
    d.tex = -1;
    d.P[0] = P ? P[0] : 0.0f;
    d.P[1] = P ? P[1] : 0.0f;
    d.P[2] = P ? P[2] : 0.0f;
    d.obj_tris = per;
    const ObjRun run{0u, 0u, 0u, nobj, per, nt, 0u, 0u, 0u, 0u, 0u, 0u};
    // the draw and the run of objects (one small upload), expanded on the device
    constexpr size_t kRunOff = (sizeof(prk::DrawRec) + 255) & ~(size_t)255;
    char tab[kRunOff + sizeof(ObjRun)] = {};
    std::memcpy(tab, &d, sizeof d);
    std::memcpy(tab + kRunOff, &run, sizeof run);
    PRK_TRY(S.d_rectab.ensure(sizeof tab));
    PRK_TRY(hipMemcpyAsync(S.d_rectab.p, tab, sizeof tab, hipMemcpyHostToDevice, s));
    PRK_TRY(hipStreamSynchronize(s));  // (tab is on this stack)
    fp.draws = (const prk::DrawRec *)S.d_rectab.p;
    fp.draw0 = d;
    PRK_TRY(S.d_objtab.ensure_n<ObjDesc>(nobj));
    PRK_TRY(S.d_k0tab.ensure((size_t)nobj * 8));
    ObjDesc *d_objs = S.d_objtab.as<ObjDesc>();
    uint32_t *k0tab = (uint32_t *)S.d_k0tab.p;
    const uint32_t *d_k0obj = k0tab, *d_k0tri0 = k0tab + nobj;
    PRK_TRY(prk_obj_tables(reinterpret_cast<const ObjRun *>(S.d_rectab.as<char>() + kRunOff), 1, nobj, kObjWaveTris,
                           d_objs, k0tab, k0tab + nobj, nullptr, nullptr, nullptr, 0u, nullptr, s));
    const size_t es = 3 * (size_t)nt;
    PRK_TRY(S.d_ecnt.ensure(((size_t)nt + 1) * 4));
    PRK_TRY(S.d_escan.ensure(((size_t)nt + 1) * 4));
    PRK_TRY(S.d_rcnt.ensure(((size_t)nt + 1) * 8));
    PRK_TRY(S.d_reccnt.ensure((size_t)nobj * 4));
    PRK_TRY(S.d_err.ensure(16));
    PRK_TRY(hipMemsetAsync(S.d_err.p, 0, 16, s));
    uint32_t *escan = (uint32_t *)S.d_escan.p;
    PRK_TRY(prk_objtri_count(&fp, d_objs, d_k0obj, d_k0tri0, nobj, nt, (uint32_t *)S.d_ecnt.p,
                             (unsigned long long *)S.d_rcnt.p, s));
    PRK_TRY(scan_u32(S.d_temp, (const uint32_t *)S.d_ecnt.p, escan, nt + 1, s));
    PRK_TRY(prk_rec_counts(d_objs, d_k0obj, nobj, escan, (uint32_t *)S.d_reccnt.p, s));
    // the total sizes the records (and decides whether the caller's buffer holds them)
    uint32_t total = 0;
    PRK_TRY(hipMemcpyAsync(&total, escan + nt, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    *total_out = total;
    const bool fill = keep || (records != nullptr && capacity >= total);
    if (fill && total) {
        PRK_TRY(S.d_edges.ensure_n<ObjEdge>(es));
        PRK_TRY(S.d_ekeys.ensure(es * 8));
        PRK_TRY(S.d_evals.ensure(es * 4));
        const size_t out_bytes = packed_edge_bytes(total);
        void *d_out = nullptr;
        if (keep) {
            PRK_TRY(hipMalloc(&d_out, out_bytes));
            *keep = d_out;  // (the caller's from here on, whatever follows)
        } else {
            PRK_TRY(S.d_recout.ensure(out_bytes));
            d_out = S.d_recout.p;
        }
        // MergeSort per object: at most 64 edges by one wave each
        // (k_obj_sort_local, into the working copy), else one radix sort
        const bool local_sort = maxn <= 64;
        unsigned long long *ekeys = S.d_ekeys.as<unsigned long long>();
        PRK_TRY(prk_rec_emit(&fp, d_objs, d_k0obj, d_k0tri0, nobj, nt, escan, setup, pbits, S.d_edges.as<ObjEdge>(),
                             ekeys, (uint32_t *)S.d_evals.p, local_sort ? 0 : 1, s));
        if (local_sort) {
            PRK_TRY(S.d_work.ensure_n<ObjEdge>(es));
            PRK_TRY(prk_obj_sort_local(d_objs, d_k0obj, nobj, escan, ekeys, S.d_edges.as<ObjEdge>(),
                                       S.d_work.as<ObjEdge>(), nullptr, (uint32_t *)S.d_err.p, s));
            PRK_TRY(prk_rec_export(S.d_work.as<ObjEdge>(), nullptr, total, d_out, s));
        } else {
            PRK_TRY(S.d_ekeys2.ensure(es * 8));
            PRK_TRY(S.d_ord.ensure(es * 4));
            PRK_TRY(obj_sort(S.d_temp, ekeys, (uint32_t *)S.d_evals.p, S.d_ekeys2.p, (uint32_t *)S.d_ord.p, 3 * nt,
                             obits + ybits + pbits, s));
            PRK_TRY(prk_rec_export(S.d_edges.as<ObjEdge>(), (const uint32_t *)S.d_ord.p, total, d_out, s));
        }
        uint32_t err = 0;
        PRK_TRY(hipMemcpyAsync(&err, S.d_err.p, 4, hipMemcpyDeviceToHost, s));
        if (!keep)
            PRK_TRY(hipMemcpyAsync(records, d_out, (size_t)total * sizeof(prk_edge), hipMemcpyDeviceToHost, s));
        if (counts) PRK_TRY(hipMemcpyAsync(counts, S.d_reccnt.p, (size_t)nobj * 4, hipMemcpyDeviceToHost, s));
        PRK_TRY(hipStreamSynchronize(s));
        if (err) return PRK_ERR_DEVICE;
        return PRK_OK;
    }
    if (counts) PRK_TRY(hipMemcpy(counts, S.d_reccnt.p, (size_t)nobj * 4, hipMemcpyDeviceToHost));
    return records && capacity < total ? PRK_ERR_ARG : PRK_OK;
}

int prk_edge_records(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                     uint32_t tris_per_object, const float P[3], int32_t setup, prk_edge *records,
                     uint64_t capacity, uint32_t *counts, uint64_t *total_out) {
    return edge_records_run(c, geometry, first_tri, tri_count, tris_per_object, P, setup, records, capacity, counts,
                            total_out, nullptr, nullptr);
}

// ---- record handles (prk.h) -------------------------------
static Records *records_of(prk_context *c, int32_t handle) {
    if (!c || handle < 0 || (size_t)handle >= c->recs.size() || !c->recs[handle].live) return nullptr;
    return &c->recs[handle];
}
static void records_free(Records &R) {
    (void)hipFree(R.rec);
    (void)hipFree(R.tab);
    R = Records{};
}
// The rest of a handle whose records (R.rec, `total` of them) and counts
// (R.tab[0 .. nlist)) are on the device: the sorted rule of every list
// (k_list_rule over the scan of the counts), and the host's copies of the
// counts and flags -- the one readback of the handle's life.  The device is
// idle (the scratch is the span path's).
static int records_finish(prk_context *c, Records &R, uint32_t nlist, uint64_t total) {
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    R.total = total;
    R.cnt.assign(nlist, 0u);
    R.flag.assign(nlist, 0u);
    if (nlist) {
        uint32_t *d_cnt = R.tab, *d_flag = R.tab + nlist + 1;
        PRK_TRY(hipMemsetAsync(d_cnt + nlist, 0, 4, s));  // (the scan's total)
        PRK_TRY(S.d_lscan.ensure(((size_t)nlist + 1) * 4));
        uint32_t *lscan = (uint32_t *)S.d_lscan.p;
        PRK_TRY(scan_u32(S.d_temp, d_cnt, lscan, nlist + 1, s));
        PRK_TRY(prk_list_rule(R.rec, (uint32_t)total, lscan, nlist, d_flag, s));
        PRK_TRY(hipMemcpyAsync(R.cnt.data(), d_cnt, (size_t)nlist * 4, hipMemcpyDeviceToHost, s));
        PRK_TRY(hipMemcpyAsync(R.flag.data(), d_flag, (size_t)nlist * 4, hipMemcpyDeviceToHost, s));
        PRK_TRY(hipStreamSynchronize(s));
    }
    R.live = true;
    return PRK_OK;
}
static int records_tab_alloc(Records &R, uint32_t nlist) {
    PRK_TRY(hipMalloc((void **)&R.tab, (2 * (size_t)nlist + 1) * 4));
    return PRK_OK;
}

int prk_records_from_geometry(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                              uint32_t tris_per_object, const float P[3], int32_t setup, int32_t *handle_out,
                              uint32_t *list_count_out, uint64_t *total_out) {
    if (!c || !handle_out) return PRK_ERR_ARG;
    *handle_out = -1;
    if (list_count_out) *list_count_out = 0;
    uint64_t total = 0;
    if (total_out) *total_out = 0;
    if (c->recs.size() >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    Records R;
    uint32_t nlist = 0;
    int rc = edge_records_run(c, geometry, first_tri, tri_count, tris_per_object, P, setup, nullptr, 0, nullptr,
                              &total, &R.rec, &nlist);
    if (rc == PRK_OK) rc = status_of(hipSetDevice(c->device));
    if (rc == PRK_OK) rc = records_tab_alloc(R, nlist);
    if (rc == PRK_OK && nlist)
        rc = status_of(hipMemcpyAsync(R.tab, c->spans.d_reccnt.p, (size_t)nlist * 4, hipMemcpyDeviceToDevice,
                                      c->own_stream));
    if (rc == PRK_OK) rc = records_finish(c, R, nlist, total);
    if (rc != PRK_OK) {
        records_free(R);
        return rc;
    }
    *handle_out = (int32_t)c->recs.size();
    c->recs.push_back(std::move(R));
    if (list_count_out) *list_count_out = nlist;
    if (total_out) *total_out = total;
    return PRK_OK;
}

int prk_records_upload(prk_context *c, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                       int32_t *handle_out) {
    if (!c || !handle_out || (!counts && list_count)) return PRK_ERR_ARG;
    *handle_out = -1;
    uint64_t total = 0;
    for (uint32_t o = 0; o < list_count; ++o) total += counts[o];
    if (!records && total) return PRK_ERR_ARG;
    // a handle's records and lists are indexed by 31 bits, as a pass's
    if (total >= 0x7FFFFFFFull || list_count >= 0x7FFFFFFFu || c->recs.size() >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // frames in flight use the scratch records_finish takes
    Records R;
    int rc = records_tab_alloc(R, list_count);
    if (rc == PRK_OK && total) {
        rc = status_of(hipMalloc(&R.rec, packed_edge_bytes(total)));
        if (rc == PRK_OK)  // the one copy of the caller's records
            rc = status_of(hipMemcpy(R.rec, records, (size_t)total * sizeof(prk_edge), hipMemcpyHostToDevice));
    }
    if (rc == PRK_OK && list_count)
        rc = status_of(hipMemcpy(R.tab, counts, (size_t)list_count * 4, hipMemcpyHostToDevice));
    if (rc == PRK_OK) rc = records_finish(c, R, list_count, total);
    if (rc != PRK_OK) {
        records_free(R);
        return rc;
    }
    *handle_out = (int32_t)c->recs.size();
    c->recs.push_back(std::move(R));
    return PRK_OK;
}

int prk_records_info(prk_context *c, int32_t handle, uint32_t *list_count_out, uint64_t *total_out) {
    const Records *R = records_of(c, handle);
    if (!R) return PRK_ERR_ARG;
    if (list_count_out) *list_count_out = (uint32_t)R->cnt.size();
    if (total_out) *total_out = R->total;
    return PRK_OK;
}

int prk_records_lists(prk_context *c, int32_t handle, uint32_t *counts, uint32_t *sorted_flags) {
    const Records *R = records_of(c, handle);
    if (!R) return PRK_ERR_ARG;
    if (counts && !R->cnt.empty()) std::memcpy(counts, R->cnt.data(), R->cnt.size() * 4);
    if (sorted_flags && !R->flag.empty()) std::memcpy(sorted_flags, R->flag.data(), R->flag.size() * 4);
    return PRK_OK;
}

int prk_records_download(prk_context *c, int32_t handle, prk_edge *records, uint64_t capacity) {
    const Records *R = records_of(c, handle);
    if (!R || capacity < R->total || (!records && R->total)) return PRK_ERR_ARG;
    if (!R->total) return PRK_OK;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipMemcpy(records, R->rec, (size_t)R->total * sizeof(prk_edge), hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_records_destroy(prk_context *c, int32_t handle) {
    Records *R = records_of(c, handle);
    if (!R) return PRK_ERR_ARG;
    for (const prk::DrawRec &d : c->draws)  // a recorded draw reads it at the flush (prk_reset_draws releases it)
        if (d.src_kind == 4 && d.geom == handle) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // frames in flight read it
    records_free(*R);
    return PRK_OK;
}

// One draw of lists [first_list, first_list + list_count) of a handle: what
// prk_draw_edge_lists records for the same lists, minus the copies -- the
// flush reads the records where they are (flush_spans, src_kind 4).
int prk_draw_records(prk_context *c, int32_t handle, uint32_t first_list, uint32_t list_count, int32_t semantics,
                     int32_t phong, int32_t texture) {
    const Records *R = records_of(c, handle);
    if (!R || (uint64_t)first_list + list_count > R->cnt.size()) return PRK_ERR_ARG;
    if (list_count == 0) return PRK_OK;
    uint64_t r0 = 0, n = 0;
    for (uint32_t o = 0; o < first_list; ++o) r0 += R->cnt[o];
    for (uint32_t o = 0; o < list_count; ++o) n += R->cnt[first_list + o];
    const int rc = draw_src(c, 4, (uint32_t)r0, (uint32_t)n, list_count, semantics, phong, texture);
    if (rc != PRK_OK) return rc;
    c->draws.back().geom_tri0 = first_list;
    c->draws.back().geom = handle;
    return PRK_OK;
}

// The lists DrawModel* leaves (prk_advance_edge_records' result) for a batch
// of sorted lists, walked on the GPU: k_adv_import -> k_adv_walk (one thread
// per list) and k_adv_walk_wg (one workgroup per long list, ListRouter below)
// -> k_rec_export + k_adv_next (prk_records.hip, prk_spans.hip).  Every refusal is decided on
// the host, in the one pass over the records that checks the sorted rule
// (list_walks_sorted), sizes each list's walk and routes it -- a list over
// kAdvMaxSteps is refused before anything is launched.  The scratch is the
// span path's, taken as prk_edge_records takes it; the packed records go in
// and come out through one buffer (the import has read it before the export
// writes it).
//
// kAdvMaxSteps: one thread walks 1.6 M edge-rows a second (DESIGN §4.4.3,
// one pair a row and 128 pairs a row alike), so the 2^24 edge-rows first
// meant would hold the GPU for 10 s; halved until a list at the cap stays
// under two seconds: 2^21, 1.3 s.
constexpr uint64_t kAdvMaxSteps = 1ull << 21;
// A list's walk in list steps: its edge-rows, the sum over its edges of
// max(0, min(YMax, height) - YMin) (k_list_prep's lrows; the removal scan and
// the pairing visit every listed edge once a row), plus its insertion scans:
// an inserted edge is compared with at most every edge still linked, those
// inserted before it whose YMax is not below its YMin (an edge leaves the
// list on row YMax, after that row's insertions).  The count of all earlier
// edges bounds that for short lists; a list that bound would refuse is swept
// with a heap of the linked edges' YMax.  Returns at once past `cap`.
// (edge_rows: the first term alone, which bounds the list's pairs --
// prk_span_records' slots -- at half of it.)
static uint64_t list_walk_steps(const prk_edge *e, uint32_t n, int32_t height, uint64_t cap,
                                std::vector<int32_t> &heap, uint64_t *edge_rows = nullptr) {
    uint64_t steps = 0;
    for (uint32_t i = 0; i < n; ++i) steps += (uint64_t)std::max(0, std::min(e[i].YMax, height) - e[i].YMin);
    if (edge_rows) *edge_rows = steps;
    const uint64_t all = (uint64_t)n * (n ? n - 1 : 0) / 2;
    if (steps > cap || steps + all <= cap) return steps + all;
    heap.clear();
    for (uint32_t i = 0; i < n && e[i].YMin < height && steps <= cap; ++i) {  // (the walk ends at `height`)
        while (!heap.empty() && heap.front() < e[i].YMin) {
            std::pop_heap(heap.begin(), heap.end(), std::greater<int32_t>());
            heap.pop_back();
        }
        steps += heap.size();
        heap.push_back(e[i].YMax);
        std::push_heap(heap.begin(), heap.end(), std::greater<int32_t>());
    }
    return steps;
}
// The most edges of a sorted list linked at once: list_walk_steps' sweep (the
// edges in YMin order, a heap of the linked edges' YMax), an edge counted from
// its YMin row through its YMax row -- it is still linked while that row's
// insertions happen.  Only edges with YMin < height are ever inserted.
// Returns at once past `stop`.
static uint32_t list_most_listed(const prk_edge *e, uint32_t n, int32_t height, uint32_t stop,
                                 std::vector<int32_t> &heap) {
    size_t most = 0;
    heap.clear();
    for (uint32_t i = 0; i < n && e[i].YMin < height && most <= stop; ++i) {
        while (!heap.empty() && heap.front() < e[i].YMin) {
            std::pop_heap(heap.begin(), heap.end(), std::greater<int32_t>());
            heap.pop_back();
        }
        heap.push_back(e[i].YMax);
        std::push_heap(heap.begin(), heap.end(), std::greater<int32_t>());
        most = std::max(most, heap.size());
    }
    return (uint32_t)std::min<size_t>(most, 0xFFFFFFFFu);
}
// Which walk each list of a record call takes.  A thread
// (k_adv_walk, k_span_walk, k_row_walk) walks a list unless its thread-walk
// cost, list_walk_steps, reaches kAdvWgMinSteps and its most linked edges fit
// the workgroup walk's largest slot class: then a workgroup walks it
// (k_*_walk_wg), in the smallest class that holds them.  A routed list has no
// insertion scan -- a row's new edges are inserted as one batch -- so only the
// edge-row term of kAdvMaxSteps applies to it; that term applies to every
// list.  The route does not depend on how many lists take it: 61,440 equal
// lists at the threshold are still faster as workgroups.
// kAdvWgMinSteps: the sweep of tools/time_advance_lists.py
// (profiles/advance_edge_lists.json, "wg_sweep"; DESIGN §4.4.6 names the
// rows).  PRK_ADV_WG_MIN_STEPS=n in the environment, read per call, replaces
// it: 0 routes every list that fits, a huge value none.
// A call without a candidate does what it did before there was a route: the
// device is not asked for its slot classes, no route word is made or
// uploaded, and the thread kernels get a null route.
constexpr uint64_t kAdvWgMinSteps = 3432;  // (the sweep's square_48x48: 48 * 48 + 48 * 47 / 2)
// (kAdvWgCaps, prk_launch.h: the workgroup walks' five slot classes)
struct ListRouter {
    struct Cand {
        uint32_t o, cls;
    };
    int device;
    uint64_t min_steps = kAdvWgMinSteps;
    bool asked = false;
    uint32_t lcap = 0;  // the largest class the device grants
    std::vector<int32_t> heap;
    std::vector<Cand> cand;
    std::vector<uint32_t> words;  // finish(): a route word per list (+ 1), then the routed lists by class
    uint32_t ncls[5] = {};
    explicit ListRouter(int dev) : device(dev) {
        if (const char *env = std::getenv("PRK_ADV_WG_MIN_STEPS")) {
            char *end = nullptr;
            const unsigned long long v = std::strtoull(env, &end, 10);
            if (end != env) min_steps = v;
        }
    }
    // The decisions about one list of n edges, from three numbers: its
    // thread-walk cost and edge-rows (list_walk_steps) and, where candidate()
    // says it is wanted, its most linked edges (list_most_listed, exact up
    // to lcap).  The host-input calls take them from the caller's records
    // (take), the handle calls from k_list_stats and k_list_most.
    bool candidate(uint32_t n, uint64_t cost, uint64_t edge_rows) {
        if (!(n && cost >= min_steps && edge_rows <= kAdvMaxSteps)) return false;
        if (!asked) {  // (the first list past the threshold: the device's slot classes)
            asked = true;
            if (hipSetDevice(device) == hipSuccess) lcap = std::min(prk_adv_wg_lcap(), kAdvWgCaps[4]);
        }
        return lcap != 0;
    }
    // false: over the cap.
    bool route(uint32_t n, uint64_t cost, uint64_t edge_rows, uint32_t most, uint32_t o) {
        if (candidate(n, cost, edge_rows))
            for (uint32_t ci = 0; ci < 5; ++ci)
                if (most <= kAdvWgCaps[ci] && kAdvWgCaps[ci] <= lcap) {
                    cand.push_back(Cand{o, ci});
                    return true;
                }
        return cost <= kAdvMaxSteps;
    }
    // One list of a host pass; false: over the cap.
    bool take(const prk_edge *e, uint32_t n, int32_t height, uint32_t o, uint64_t *edge_rows_out) {
        uint64_t edge_rows = 0;
        const uint64_t cost = list_walk_steps(e, n, height, kAdvMaxSteps, heap, &edge_rows);
        if (edge_rows_out) *edge_rows_out = edge_rows;
        const uint32_t most = candidate(n, cost, edge_rows) ? list_most_listed(e, n, height, lcap, heap) : 0u;
        return route(n, cost, edge_rows, most, o);
    }
    // After the pass: the routed lists' words.
    void finish(uint32_t list_count) {
        if (cand.empty()) return;
        const size_t nl1 = (size_t)list_count + 1;
        words.assign(nl1 + cand.size(), 0u);
        for (const Cand &k : cand) {
            words[k.o] = k.cls + 1;
            ++ncls[k.cls];
        }
        uint32_t at[5], sum = 0;
        for (int ci = 0; ci < 5; sum += ncls[ci], ++ci) at[ci] = sum;
        for (const Cand &k : cand) words[nl1 + at[k.cls]++] = k.o;
    }
    size_t routed() const { return cand.size(); }
    void note(prk_context *c, uint32_t list_count) const {
        c->spans.list_routes[0] = list_count - (uint32_t)cand.size();
        for (int ci = 0; ci < 5; ++ci) c->spans.list_routes[1 + ci] = ncls[ci];
    }
};
// The host side of a record call's pass over its lists: each list's first
// edge (lscan), its first pair slot (sbase: prk_span_records, prk_row_records)
// and first row slot (rbase: prk_row_records) -- `tables` of them, nl1 words
// each -- its route, and whether anything is over a limit.  The host-input
// calls fill it from the caller's records, the handle calls from the device's
// statistics (records_plan); the rest of a call (advance_run, spans_run,
// rows_run) does not know which.
struct WalkPlan {
    const uint32_t list_count;
    const size_t nl1;
    const int tables;
    std::vector<uint32_t> tab;
    ListRouter router;
    uint64_t nslot = 0, nrslot = 0;
    uint32_t n = 0;  // the lists' edges
    bool too_long = false;
    WalkPlan(int device, uint32_t lists, int ntab)
        : list_count(lists), nl1((size_t)lists + 1), tables(ntab), tab((size_t)ntab * nl1), router(device) {}
    // list o (or the end of the last: o == list_count) begins at edge `at`
    void open(uint32_t o, uint32_t at) {
        tab[o] = at;
        if (tables > 1) tab[nl1 + o] = (uint32_t)nslot;
        if (tables > 2) tab[2 * nl1 + o] = (uint32_t)nrslot;
        if (o == list_count) n = at;
    }
    // ... was routed (fits: not over the cap) and takes floor(edge-rows / 2)
    // pair slots and a row slot for each of the `rows` rows of its walk
    void close(bool fits, uint64_t edge_rows, uint64_t rows) {
        too_long = !fits || too_long;
        if (tables > 1) nslot += edge_rows / 2;
        if (tables > 2) nrslot += rows;
        too_long = too_long || nslot >= 0x7FFFFFFFull || nrslot >= 0x7FFFFFFFull;
    }
};
// The host-input calls' pass over the caller's lists (counts: list_count of
// them); PRK_ERR_UNSUPPORTED: a list breaks the sorted rule.  The walk's rows,
// [YMin[0], min(max YMax, height)), are found for a plan with row slots only:
// the pass is on the timed path of large batches.
static int plan_lists(WalkPlan &plan, const prk_edge *e, const uint32_t *counts, int32_t height) {
    uint32_t at = 0;
    for (uint32_t o = 0; o < plan.list_count; e += counts[o], at += counts[o], ++o) {
        plan.open(o, at);
        if (!list_walks_sorted(e, counts[o])) return PRK_ERR_UNSUPPORTED;
        uint64_t edge_rows = 0, walk_rows = 0;
        const bool fits = plan.router.take(e, counts[o], height, o, &edge_rows);
        if (plan.tables > 2 && counts[o]) {
            int32_t ymax = e[0].YMax;
            for (uint32_t i = 1; i < counts[o]; ++i) ymax = std::max(ymax, e[i].YMax);
            walk_rows = (uint64_t)std::max(0, std::min(ymax, height) - e[0].YMin);
        }
        plan.close(fits, edge_rows, walk_rows);
    }
    plan.open(plan.list_count, at);
    return PRK_OK;
}
// What the host-input record calls check first, in this order: the counts and
// the height (PRK_ERR_ARG), the buffers a batch with records needs (have_bufs;
// PRK_ERR_ARG), the limits (PRK_ERR_LIMIT).  *total_out == 0: an empty batch.
static int lists_check(const uint32_t *counts, uint32_t list_count, int32_t height, bool have_bufs,
                       uint64_t *total_out) {
    if ((!counts && list_count) || height < 0) return PRK_ERR_ARG;
    uint64_t total = 0;
    for (uint32_t o = 0; o < list_count; ++o) total += counts[o];
    if (!have_bufs && total) return PRK_ERR_ARG;
    if (total >= 0x7FFFFFFFull || list_count >= 0x7FFFFFFFu || height > 65536) return PRK_ERR_LIMIT;
    *total_out = total;
    return PRK_OK;
}
// An empty batch's per-list counts.
static void zero_counts(uint32_t *counts_out, uint32_t list_count) {
    if (counts_out) std::fill(counts_out, counts_out + list_count, 0u);
}
// What advance_run, spans_run and rows_run begin with: a too-long plan
// refused, the router finished, the device idle, the walk's scratch sized --
// for plan.tables - 1, the walk's kind, and with slots to fill or not --, the
// records (host or device memory: kind), the plan's tables and the route words
// uploaded, the counts and the error word cleared, all of it waited for.
// *a: the walk's arguments; *d_lists: the routed lists by class (null: none).
// A plan of one table without a routed list is prk_advance_edge_lists as it
// was before there was a route: no error word is sized or cleared.
static int walk_begin(prk_context *c, WalkPlan &plan, const void *records, hipMemcpyKind kind, int32_t height,
                      bool fill, prk::ListWalkArgs *a, const uint32_t **d_lists) {
    if (plan.too_long) return PRK_ERR_LIMIT;
    ListRouter &router = plan.router;
    const std::vector<uint32_t> &tab = plan.tab;
    const size_t nl1 = plan.nl1;
    const int tables = plan.tables;
    router.finish(plan.list_count);
    const bool wg = router.routed() != 0, use_err = wg || tables > 1;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // frames in flight use the scratch below
    router.note(c, plan.list_count);
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    const uint32_t n = plan.n;
    PRK_TRY(S.d_recout.ensure(packed_edge_bytes(n)));
    PRK_TRY(S.d_work.ensure_n<ObjEdge>(n));
    PRK_TRY(S.d_escan.ensure((tab.size() + router.words.size()) * 4));
    if (tables > 1) {
        PRK_TRY(S.d_scnt.ensure(nl1 * 4));
        PRK_TRY(S.d_soff.ensure(nl1 * 4));
    }
    if (tables > 2) {
        PRK_TRY(S.d_rowcnt.ensure(nl1 * 4));
        PRK_TRY(S.d_rowscan.ensure(nl1 * 4));
    }
    if (use_err) PRK_TRY(S.d_err.ensure(16));
    if (fill) {
        PRK_TRY(S.d_raw.ensure(std::max<size_t>(plan.nslot * sizeof(PairRaw), 16)));
        if (tables == 2) PRK_TRY(S.d_pos.ensure(std::max<size_t>((size_t)plan.nslot * 4, 16)));      // the slots' rows
        if (tables == 3) PRK_TRY(S.d_rowslot.ensure(std::max<size_t>(plan.nrslot * sizeof(prk::RowRec), 16)));
    }
    PRK_TRY(hipMemcpyAsync(S.d_recout.p, records, (size_t)n * sizeof(prk_edge), kind, s));
    PRK_TRY(hipMemcpyAsync(S.d_escan.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    if (wg)
        PRK_TRY(hipMemcpyAsync((uint32_t *)S.d_escan.p + tab.size(), router.words.data(), router.words.size() * 4,
                               hipMemcpyHostToDevice, s));
    if (tables > 1) PRK_TRY(hipMemsetAsync(S.d_scnt.p, 0, nl1 * 4, s));  // (the scans read list_count + 1 counts)
    if (tables > 2) PRK_TRY(hipMemsetAsync(S.d_rowcnt.p, 0, nl1 * 4, s));
    if (use_err) PRK_TRY(hipMemsetAsync(S.d_err.p, 0, 16, s));
    PRK_TRY(hipStreamSynchronize(s));  // (tab is this call's; records may be an output)
    const uint32_t *d_lscan = (const uint32_t *)S.d_escan.p, *d_route = wg ? d_lscan + tab.size() : nullptr;
    *d_lists = wg ? d_route + nl1 : nullptr;
    a->work = S.d_work.as<ObjEdge>();
    a->lscan = d_lscan;
    a->nlist = plan.list_count;
    a->route = d_route;
    a->height = height;
    a->sbase = tables > 1 ? d_lscan + nl1 : nullptr;
    a->rbase = tables > 2 ? d_lscan + 2 * nl1 : nullptr;
    a->raw = fill ? S.d_raw.as<PairRaw>() : nullptr;
    a->prow = fill && tables == 2 ? (int32_t *)S.d_pos.p : nullptr;
    a->rows = fill && tables == 3 ? S.d_rowslot.as<prk::RowRec>() : nullptr;
    a->cnt = tables > 1 ? (uint32_t *)S.d_scnt.p : nullptr;
    a->rcnt = tables > 2 ? (uint32_t *)S.d_rowcnt.p : nullptr;
    a->err = (uint32_t *)S.d_err.p;
    return PRK_OK;
}
// ... and the walk itself: the import and the thread kernel, then the
// workgroup kernels, a launch per occupied slot class.
static hipError_t walk_launch(prk_context *c, const WalkPlan &plan, const prk::ListWalkArgs &a,
                              const uint32_t *d_lists) {
    const int kind = plan.tables - 1;
    const uint32_t *ncls = plan.router.ncls;
    hipError_t e = prk_list_walk(kind, c->spans.d_recout.p, plan.n, &a, c->own_stream);
    for (int ci = 0; ci < 5 && d_lists && e == hipSuccess; d_lists += ncls[ci], ++ci)
        e = prk_list_walk_wg(kind, kAdvWgCaps[ci], d_lists, ncls[ci], &a, c->own_stream);
    return e;
}
// prk_advance_edge_lists after its pass, for records in host memory or on the
// device (kind).  records_out, next_out: null, or host memory.  keep: null,
// or a handle in the making, which gets a buffer of its own that k_rec_export
// writes the advanced records into (prk_records_advance); the host outputs
// are then left to the caller, which copies them once the handle stands.
static int advance_run(prk_context *c, WalkPlan &plan, const void *records, hipMemcpyKind kind, int32_t height,
                       prk_edge *records_out, int32_t *next_out, Records *keep) {
    prk::ListWalkArgs a;
    const uint32_t *d_lists = nullptr;
    const int rb = walk_begin(c, plan, records, kind, height, false, &a, &d_lists);
    if (rb != PRK_OK) return rb;
    const bool wg = plan.router.routed() != 0;  // (else: the call as it was before there was a route)
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    const uint32_t n = plan.n;
    const size_t rec_bytes = (size_t)n * sizeof(prk_edge);
    if (next_out) PRK_TRY(S.d_evals.ensure((size_t)n * 4));
    void *d_out = S.d_recout.p;
    if (keep) {
        PRK_TRY(hipMalloc(&keep->rec, packed_edge_bytes(n)));  // (the caller frees it, whatever follows)
        d_out = keep->rec;
    }
    PRK_TRY(walk_launch(c, plan, a, d_lists));
    if (records_out || keep) PRK_TRY(prk_rec_export(S.d_work.as<ObjEdge>(), nullptr, n, d_out, s));
    if (next_out) PRK_TRY(prk_adv_next(S.d_work.as<ObjEdge>(), n, (int32_t *)S.d_evals.p, s));
    uint32_t err = 0;
    if (wg) PRK_TRY(hipMemcpyAsync(&err, S.d_err.p, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));  // nothing is written to the outputs unless the kernels ran
    if (err) return PRK_ERR_DEVICE;    // a workgroup walk ran out of slots
    if (keep) return PRK_OK;           // (the caller copies, from keep->rec and d_evals, once the handle stands)
    if (records_out) PRK_TRY(hipMemcpyAsync(records_out, d_out, rec_bytes, hipMemcpyDeviceToHost, s));
    if (next_out) PRK_TRY(hipMemcpyAsync(next_out, S.d_evals.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    return PRK_OK;
}
int prk_advance_edge_lists(prk_context *c, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                           int32_t height, prk_edge *records_out, int32_t *next_out) {
    if (!c) return PRK_ERR_ARG;
    uint64_t total = 0;
    const int rc = lists_check(counts, list_count, height, records && records_out, &total);
    if (rc != PRK_OK) return rc;
    if (list_count == 0 || total == 0) return PRK_OK;
    WalkPlan plan(c->device, list_count, 1);
    const int rp = plan_lists(plan, records, counts, height);
    if (rp != PRK_OK) return rp;
    return advance_run(c, plan, records, hipMemcpyHostToDevice, height, records_out, next_out, nullptr);
}

// The work records DrawModelOptimized(RenderQueue) queues for every list of
// such a batch (3756-3809: both edges of every pair as they stand on the row,
// and the row), from prk_advance_edge_lists' walk with the emission hook:
// k_adv_import -> k_span_walk (one thread per list: pairs into the list's
// slots, its count) and k_span_walk_wg (a workgroup per routed list, the same
// slots and count) -> scan of the counts -> k_span_pack (prk_records.hip).
// The refusals and the one host pass are prk_advance_edge_lists'; the pass
// also sizes each list's slots, floor(edge-rows / 2): a pair uses up one row
// of each of two listed edges (each listed on rows [YMin, min(YMax, height))
// at most, and in one pair a row), so no walk passes that.  spans == NULL:
// the counting walk, no slots.
// prk_span_records after its pass, for records in host memory or on the
// device (kind).  keep (prk_spans_from_records; `spans` is then NULL and no
// capacity applies): k_span_pack writes into a buffer of the batch's own and
// nothing is copied to the host but the counts -- keep->sp, keep->cnt and
// keep->total are set on PRK_OK only (sp stays NULL for no spans).
static int spans_run(prk_context *c, WalkPlan &plan, const void *records, hipMemcpyKind kind, int32_t height,
                     prk_span *spans, uint64_t capacity, uint32_t *span_counts, uint64_t *total_out,
                     SpanBatch *keep = nullptr) {
    prk::ListWalkArgs a;
    const uint32_t *d_lists = nullptr;
    const int rb = walk_begin(c, plan, records, kind, height, spans || keep, &a, &d_lists);
    if (rb != PRK_OK) return rb;
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    const uint32_t list_count = plan.list_count;
    const uint32_t *d_sbase = a.sbase;
    uint32_t *d_cnt = a.cnt, *d_cscan = (uint32_t *)S.d_soff.p;
    PRK_TRY(walk_launch(c, plan, a, d_lists));
    PRK_TRY(scan_u32(S.d_temp, d_cnt, d_cscan, list_count + 1, s));
    uint32_t nspan = 0, err = 0;
    PRK_TRY(hipMemcpyAsync(&nspan, d_cscan + list_count, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipMemcpyAsync(&err, S.d_err.p, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    if (err) return PRK_ERR_DEVICE;  // a walk passed its slot bound
    *total_out = nspan;
    if (span_counts) PRK_TRY(hipMemcpy(span_counts, d_cnt, (size_t)list_count * 4, hipMemcpyDeviceToHost));
    if (keep) {  // the packed spans into the batch's own buffer; they stay there
        std::vector<uint32_t> cnt(list_count);
        PRK_TRY(hipMemcpy(cnt.data(), d_cnt, (size_t)list_count * 4, hipMemcpyDeviceToHost));
        void *buf = nullptr;
        if (nspan) {
            PRK_TRY(hipMalloc(&buf, packed_span_bytes(nspan)));
            hipError_t e = prk_span_pack(S.d_raw.as<PairRaw>(), (const int32_t *)S.d_pos.p, d_sbase, d_cscan,
                                         list_count, nspan, buf, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                (void)hipFree(buf);
                return status_of(e);
            }
        }
        keep->sp = buf;
        keep->cnt = std::move(cnt);
        keep->total = nspan;
        return PRK_OK;
    }
    if (!spans) return PRK_OK;
    if (capacity < nspan) return PRK_ERR_ARG;
    if (nspan == 0) return PRK_OK;
    PRK_TRY(S.d_spanout.ensure(packed_span_bytes(nspan)));
    PRK_TRY(prk_span_pack(S.d_raw.as<PairRaw>(), (const int32_t *)S.d_pos.p, d_sbase, d_cscan, list_count, nspan,
                          S.d_spanout.p, s));
    PRK_TRY(hipStreamSynchronize(s));  // nothing is written to `spans` unless the kernel ran
    PRK_TRY(hipMemcpyAsync(spans, S.d_spanout.p, (size_t)nspan * sizeof(prk_span), hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    return PRK_OK;
}
int prk_span_records(prk_context *c, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                     int32_t height, prk_span *spans, uint64_t capacity, uint32_t *span_counts,
                     uint64_t *total_out) {
    if (!c || !total_out) return PRK_ERR_ARG;
    *total_out = 0;
    uint64_t total = 0;
    const int rc = lists_check(counts, list_count, height, records != nullptr, &total);
    if (rc != PRK_OK) return rc;
    if (list_count == 0 || total == 0) {
        zero_counts(span_counts, list_count);
        return PRK_OK;
    }
    // lscan, then sbase: each list's first edge and first slot
    WalkPlan plan(c->device, list_count, 2);
    const int rp = plan_lists(plan, records, counts, height);
    if (rp != PRK_OK) return rp;
    return spans_run(c, plan, records, hipMemcpyHostToDevice, height, spans, capacity, span_counts, total_out);
}

// The row work records DrawModelOptimizedLines queues for every list of such
// a batch (3509-3609: one buffer_line_render_work a row the walk reaches,
// RowIndex, EdgeCount and that many thread_edge_info pairs), from the same
// walk with the row hook: k_adv_import -> k_row_walk (one thread per list:
// pairs into the list's pair slots, a row record a row into its row slots, its
// two counts) and k_row_walk_wg (a workgroup per routed list) -> two scans ->
// k_row_pack (prk_records.hip).  The refusals and the one host pass are
// prk_span_records'; the pass also sizes each list's row slots, the rows of
// its walk.  What the pass cannot know -- a row with more
// than 1000 pairs, the reference's ThreadEdges[1000] -- the walk flags, and
// the flag is read before anything is written.  rows == pairs == NULL: the
// counting walk, no slots.
// prk_row_records after its pass, for records in host memory or on the
// device (kind).
static int rows_run(prk_context *c, WalkPlan &plan, const void *records, hipMemcpyKind kind, int32_t height,
                    prk_row *rows, uint64_t row_capacity, prk_row_pair *pairs, uint64_t pair_capacity,
                    uint32_t *row_counts, uint64_t *row_total_out, uint64_t *pair_total_out) {
    const bool fill = rows != nullptr;
    prk::ListWalkArgs a;
    const uint32_t *d_lists = nullptr;
    const int rb = walk_begin(c, plan, records, kind, height, fill, &a, &d_lists);
    if (rb != PRK_OK) return rb;
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    const uint32_t list_count = plan.list_count;
    const uint32_t *d_sbase = a.sbase, *d_rbase = a.rbase;
    uint32_t *d_pcnt = a.cnt, *d_pscan = (uint32_t *)S.d_soff.p;
    uint32_t *d_rcnt = a.rcnt, *d_rscan = (uint32_t *)S.d_rowscan.p;
    PRK_TRY(walk_launch(c, plan, a, d_lists));
    // (two scans of one length: the second finds the buffer the first ensured)
    PRK_TRY(scan_u32(S.d_temp, d_pcnt, d_pscan, list_count + 1, s));
    PRK_TRY(scan_u32(S.d_temp, d_rcnt, d_rscan, list_count + 1, s));
    uint32_t npair = 0, nrow = 0, err = 0;
    PRK_TRY(hipMemcpyAsync(&npair, d_pscan + list_count, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipMemcpyAsync(&nrow, d_rscan + list_count, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipMemcpyAsync(&err, S.d_err.p, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    if (err & 1u) return PRK_ERR_DEVICE;       // a walk passed a slot bound
    if (err & 2u) return PRK_ERR_UNSUPPORTED;  // a row of more than 1000 pairs
    const bool is_short = fill && (row_capacity < nrow || pair_capacity < npair);
    if (fill && !is_short && (npair || nrow)) {
        PRK_TRY(S.d_spanout.ensure(std::max<size_t>((size_t)npair * sizeof(prk_row_pair), 16)));
        PRK_TRY(S.d_rowout.ensure(std::max<size_t>((size_t)nrow * sizeof(prk_row), 16)));
        PRK_TRY(prk_row_pack(S.d_raw.as<PairRaw>(), S.d_rowslot.as<prk::RowRec>(), d_sbase, d_rbase, d_pscan, d_rscan,
                             list_count, npair, nrow, S.d_spanout.p, S.d_rowout.as<prk::RowRec>(), s));
        PRK_TRY(hipStreamSynchronize(s));  // nothing is written to the outputs unless the kernel ran
    }
    *row_total_out = nrow;
    *pair_total_out = npair;
    if (row_counts) PRK_TRY(hipMemcpy(row_counts, d_rcnt, (size_t)list_count * 4, hipMemcpyDeviceToHost));
    if (!fill) return PRK_OK;
    if (is_short) return PRK_ERR_ARG;
    if (nrow) PRK_TRY(hipMemcpyAsync(rows, S.d_rowout.p, (size_t)nrow * sizeof(prk_row), hipMemcpyDeviceToHost, s));
    if (npair)
        PRK_TRY(hipMemcpyAsync(pairs, S.d_spanout.p, (size_t)npair * sizeof(prk_row_pair), hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    return PRK_OK;
}
int prk_row_records(prk_context *c, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                    int32_t height, prk_row *rows, uint64_t row_capacity, prk_row_pair *pairs,
                    uint64_t pair_capacity, uint32_t *row_counts, uint64_t *row_total_out, uint64_t *pair_total_out) {
    if (!c || !row_total_out || !pair_total_out) return PRK_ERR_ARG;
    if ((rows == nullptr) != (pairs == nullptr)) return PRK_ERR_ARG;
    uint64_t total = 0;
    const int rc = lists_check(counts, list_count, height, records != nullptr, &total);
    if (rc != PRK_OK) return rc;
    if (list_count == 0 || total == 0) {
        *row_total_out = *pair_total_out = 0;
        zero_counts(row_counts, list_count);
        return PRK_OK;
    }
    // lscan, sbase, rbase: each list's first edge, first pair slot and first row slot
    WalkPlan plan(c->device, list_count, 3);
    const int rp = plan_lists(plan, records, counts, height);
    if (rp != PRK_OK) return rp;
    return rows_run(c, plan, records, hipMemcpyHostToDevice, height, rows, row_capacity, pairs, pair_capacity,
                    row_counts, row_total_out, pair_total_out);
}

// ---- the record walks of a handle (prk.h) ----------------
// What the device tells the host about one list (k_list_stats, k_list_most).
struct ListStats {
    uint64_t edge_rows = 0, scans = 0;
    uint32_t most = 0;  // (of a route candidate; else 0)
    int32_t ymin0 = 0, ymax_max = 0;
};
// list_walk_steps' value from the exact insertion scans: all earlier edges
// bound the scans where that settles the matter, as there.  (The sweep there
// stops adding once past the cap, the device's sum does not: the two differ
// only in values above kAdvMaxSteps.)
static uint64_t list_cost(uint64_t edge_rows, uint64_t scans, uint32_t n) {
    const uint64_t all = (uint64_t)n * (n ? n - 1 : 0) / 2;
    if (edge_rows > kAdvMaxSteps || edge_rows + all <= kAdvMaxSteps) return edge_rows + all;
    return edge_rows + scans;
}
// The pass of a handle call over lists [first_list, first_list + list_count)
// of R at `height` (not empty: `n` records from record r0, every list's flag
// 1): the statistics kernels, their download -- a few words a list, no
// records -- and ListRouter's decisions from them.  The device is idle.
// stats_out: null, or list_count of them.
static int records_plan(prk_context *c, const Records &R, uint32_t first_list, uint64_t r0, int32_t height,
                        WalkPlan &plan, ListStats *stats_out) {
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    const uint32_t nlist = plan.list_count;
    const uint32_t *cnt = R.cnt.data() + first_list;
    std::vector<uint32_t> lscan(plan.nl1);
    uint32_t at = 0;
    for (uint32_t o = 0; o < nlist; at += cnt[o], ++o) lscan[o] = at;
    lscan[nlist] = at;
    const void *rec = R.at(r0);
    // device: lscan | the statistics (ListStatsLayout) | the candidates | their most linked
    const prk::ListStatsLayout lay{nlist};
    const size_t stat_off = (plan.nl1 * 4 + 7) & ~(size_t)7, cand_off = stat_off + lay.bytes();
    PRK_TRY(S.d_lstat.ensure(cand_off + (size_t)nlist * 8));
    char *base = static_cast<char *>(S.d_lstat.p);
    const uint32_t *d_lscan = reinterpret_cast<const uint32_t *>(base);
    uint32_t *d_cand = reinterpret_cast<uint32_t *>(base + cand_off), *d_most = d_cand + nlist;
    PRK_TRY(hipMemcpyAsync(base, lscan.data(), plan.nl1 * 4, hipMemcpyHostToDevice, s));
    PRK_TRY(prk_list_stats(rec, at, d_lscan, nlist, height, base + stat_off, s));
    std::vector<unsigned long long> raw(lay.bytes() / 8);
    PRK_TRY(hipMemcpyAsync(raw.data(), base + stat_off, lay.bytes(), hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    const prk::ListStatsView st = lay.view(raw.data());
    const unsigned long long *erows = st.erows, *scans = st.scans;
    const int32_t *ymin0 = st.ymin0, *ymax_max = st.ymaxmax;
    ListRouter &router = plan.router;
    std::vector<uint32_t> cand, most;
    for (uint32_t o = 0; o < nlist; ++o)
        if (router.candidate(cnt[o], list_cost(erows[o], scans[o], cnt[o]), erows[o])) cand.push_back(o);
    if (!cand.empty()) {
        most.resize(cand.size());
        PRK_TRY(hipMemcpyAsync(d_cand, cand.data(), cand.size() * 4, hipMemcpyHostToDevice, s));
        PRK_TRY(prk_list_most(rec, d_lscan, d_cand, (uint32_t)cand.size(), height, d_most, s));
        PRK_TRY(hipMemcpyAsync(most.data(), d_most, cand.size() * 4, hipMemcpyDeviceToHost, s));
        PRK_TRY(hipStreamSynchronize(s));
    }
    size_t k = 0;
    for (uint32_t o = 0; o < nlist; ++o) {
        plan.open(o, lscan[o]);
        const uint32_t m = k < cand.size() && cand[k] == o ? most[k++] : 0u;
        const bool fits = router.route(cnt[o], list_cost(erows[o], scans[o], cnt[o]), erows[o], m, o);
        plan.close(fits, erows[o], (uint64_t)std::max(0, std::min(ymax_max[o], height) - ymin0[o]));
        if (stats_out) {
            ListStats &t = stats_out[o];
            t.edge_rows = erows[o];
            t.scans = scans[o];
            t.most = m;
            t.ymin0 = ymin0[o];
            t.ymax_max = ymax_max[o];
        }
    }
    plan.open(nlist, at);
    return PRK_OK;
}
// What every handle call checks first, in the order of the host-input calls'
// refusals: the handle and the range (PRK_ERR_ARG), the height
// (PRK_ERR_LIMIT), the sorted flags of the range (PRK_ERR_UNSUPPORTED).
// *n_out == 0: nothing to walk.
static int records_range(prk_context *c, int32_t handle, uint32_t first_list, uint32_t list_count, int32_t height,
                         const Records **R_out, uint64_t *r0_out, uint64_t *n_out) {
    const Records *R = records_of(c, handle);
    if (!R || (uint64_t)first_list + list_count > R->cnt.size() || height < 0) return PRK_ERR_ARG;
    if (height > 65536) return PRK_ERR_LIMIT;
    uint64_t r0 = 0, n = 0;
    for (uint32_t o = 0; o < first_list; ++o) r0 += R->cnt[o];
    for (uint32_t o = 0; o < list_count; ++o) {
        if (!R->flag[first_list + o]) return PRK_ERR_UNSUPPORTED;
        n += R->cnt[first_list + o];
    }
    *R_out = R;
    *r0_out = r0;
    *n_out = n;
    return PRK_OK;
}
// ... and what follows for a range with records: the device idle (frames in
// flight read the scratch), then the pass.
static int records_begin(prk_context *c, const Records &R, uint32_t first_list, uint64_t r0, int32_t height,
                         WalkPlan &plan, ListStats *stats_out) {
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    return records_plan(c, R, first_list, r0, height, plan, stats_out);
}

int prk_debug_list_stats(prk_context *c, int32_t handle, uint32_t first_list, uint32_t list_count, int32_t height,
                         uint64_t *out) {
    const Records *R = nullptr;
    uint64_t r0 = 0, n = 0;
    if (!c || (!out && list_count)) return PRK_ERR_ARG;
    const int rc = records_range(c, handle, first_list, list_count, height, &R, &r0, &n);
    if (rc != PRK_OK) return rc;
    std::vector<ListStats> st(list_count);
    if (n) {
        WalkPlan plan(c->device, list_count, 3);
        const int rp = records_begin(c, *R, first_list, r0, height, plan, st.data());
        if (rp != PRK_OK) return rp;
    }
    for (uint32_t o = 0; o < list_count; ++o) {
        const ListStats &t = st[o];
        uint64_t *w = out + 5 * (size_t)o;
        w[0] = t.edge_rows;
        w[1] = t.scans;
        w[2] = t.most;
        w[3] = (uint64_t)(int64_t)t.ymin0;
        w[4] = (uint64_t)(int64_t)t.ymax_max;
    }
    return PRK_OK;
}

int prk_records_advance(prk_context *c, int32_t handle, uint32_t first_list, uint32_t list_count, int32_t height,
                        int32_t *advanced_out, prk_edge *records_out, int32_t *next_out) {
    if (!c) return PRK_ERR_ARG;
    if (advanced_out) *advanced_out = -1;
    if (!advanced_out && !records_out && !next_out) return PRK_ERR_ARG;
    const Records *R = nullptr;
    uint64_t r0 = 0, n = 0;
    const int rc = records_range(c, handle, first_list, list_count, height, &R, &r0, &n);
    if (rc != PRK_OK) return rc;
    if (advanced_out && c->recs.size() >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    Records A;  // the advanced lists' handle, if asked for
    int ra = PRK_OK;
    if (n) {
        WalkPlan plan(c->device, list_count, 1);
        ra = records_begin(c, *R, first_list, r0, height, plan, nullptr);
        if (ra == PRK_OK)
            ra = advance_run(c, plan, R->at(r0), hipMemcpyDeviceToDevice, height, records_out, next_out,
                             advanced_out ? &A : nullptr);
    } else if (advanced_out) {
        RESOLVE_COUNT(c);
        ra = status_of(hipSetDevice(c->device));
        if (ra == PRK_OK) ra = status_of(hipDeviceSynchronize());  // frames in flight use the scratch records_finish takes
    }
    if (!advanced_out || ra != PRK_OK) {
        records_free(A);
        return ra;
    }
    // the new handle (records_finish: the walk changes no YMin, YMax or Left,
    // so k_list_rule finds every flag 1 again), then the host's outputs --
    // nothing is written, and no handle is made, unless all of it succeeded
    prk_context::SpanScratch &S = c->spans;
    hipStream_t s = c->own_stream;
    R = records_of(c, handle);
    ra = records_tab_alloc(A, list_count);
    if (ra == PRK_OK && list_count)
        ra = status_of(hipMemcpyAsync(A.tab, R->d_cnt() + first_list, (size_t)list_count * 4,
                                      hipMemcpyDeviceToDevice, s));
    if (ra == PRK_OK) ra = records_finish(c, A, list_count, n);
    if (ra == PRK_OK && n && records_out)
        ra = status_of(hipMemcpyAsync(records_out, A.rec, (size_t)n * sizeof(prk_edge), hipMemcpyDeviceToHost, s));
    if (ra == PRK_OK && n && next_out)
        ra = status_of(hipMemcpyAsync(next_out, S.d_evals.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (ra == PRK_OK) ra = status_of(hipStreamSynchronize(s));
    if (ra != PRK_OK) {
        records_free(A);
        return ra;
    }
    *advanced_out = (int32_t)c->recs.size();
    c->recs.push_back(std::move(A));
    return PRK_OK;
}

int prk_records_spans(prk_context *c, int32_t handle, uint32_t first_list, uint32_t list_count, int32_t height,
                      prk_span *spans, uint64_t capacity, uint32_t *span_counts, uint64_t *total_out) {
    if (!c || !total_out) return PRK_ERR_ARG;
    *total_out = 0;
    const Records *R = nullptr;
    uint64_t r0 = 0, n = 0;
    const int rc = records_range(c, handle, first_list, list_count, height, &R, &r0, &n);
    if (rc != PRK_OK) return rc;
    if (n == 0) {
        zero_counts(span_counts, list_count);
        return PRK_OK;
    }
    WalkPlan plan(c->device, list_count, 2);
    const int rp = records_begin(c, *R, first_list, r0, height, plan, nullptr);
    if (rp != PRK_OK) return rp;
    return spans_run(c, plan, R->at(r0), hipMemcpyDeviceToDevice, height, spans, capacity, span_counts, total_out);
}

int prk_records_rows(prk_context *c, int32_t handle, uint32_t first_list, uint32_t list_count, int32_t height,
                     prk_row *rows, uint64_t row_capacity, prk_row_pair *pairs, uint64_t pair_capacity,
                     uint32_t *row_counts, uint64_t *row_total_out, uint64_t *pair_total_out) {
    if (!c || !row_total_out || !pair_total_out) return PRK_ERR_ARG;
    if ((rows == nullptr) != (pairs == nullptr)) return PRK_ERR_ARG;
    const Records *R = nullptr;
    uint64_t r0 = 0, n = 0;
    const int rc = records_range(c, handle, first_list, list_count, height, &R, &r0, &n);
    if (rc != PRK_OK) return rc;
    if (n == 0) {
        *row_total_out = *pair_total_out = 0;
        zero_counts(row_counts, list_count);
        return PRK_OK;
    }
    WalkPlan plan(c->device, list_count, 3);
    const int rp = records_begin(c, *R, first_list, r0, height, plan, nullptr);
    if (rp != PRK_OK) return rp;
    return rows_run(c, plan, R->at(r0), hipMemcpyDeviceToDevice, height, rows, row_capacity, pairs, pair_capacity,
                    row_counts, row_total_out, pair_total_out);
}

// ---- span handles (prk.h) ---------------------------------
// Packed prk_span records that stay on the device: made by the span walk of a
// record handle (spans_run with `keep`), uploaded once, or regrouped from row
// work records (rows_to_spans with `keep`); drawn where they are
// (flush_spans, src_kind 5 -> k_span_handle_walk).
static SpanBatch *sbatch_of(prk_context *c, int32_t handle) {
    if (!c || handle < 0 || (size_t)handle >= c->sbatches.size() || !c->sbatches[handle].live) return nullptr;
    return &c->sbatches[handle];
}
static int sbatch_add(prk_context *c, SpanBatch &&B, int32_t *spans_out) {
    B.live = true;
    *spans_out = (int32_t)c->sbatches.size();
    c->sbatches.push_back(std::move(B));
    return PRK_OK;
}

int prk_spans_from_records(prk_context *c, int32_t records_handle, uint32_t first_list, uint32_t list_count,
                           int32_t height, int32_t *spans_out, uint32_t *span_counts, uint64_t *total_out) {
    if (!c || !spans_out) return PRK_ERR_ARG;
    *spans_out = -1;
    if (total_out) *total_out = 0;
    const Records *R = nullptr;
    uint64_t r0 = 0, n = 0;
    const int rc = records_range(c, records_handle, first_list, list_count, height, &R, &r0, &n);
    if (rc != PRK_OK) return rc;
    if (c->sbatches.size() >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    SpanBatch B;
    uint64_t total = 0;
    if (n == 0) {
        B.cnt.assign(list_count, 0u);
        zero_counts(span_counts, list_count);
    } else {
        WalkPlan plan(c->device, list_count, 2);
        const int rp = records_begin(c, *R, first_list, r0, height, plan, nullptr);
        if (rp != PRK_OK) return rp;
        const int rs = spans_run(c, plan, R->at(r0), hipMemcpyDeviceToDevice, height, nullptr, 0, span_counts, &total,
                                 &B);
        if (rs != PRK_OK) return rs;
    }
    if (total_out) *total_out = total;
    return sbatch_add(c, std::move(B), spans_out);
}

int prk_spans_upload(prk_context *c, const prk_span *spans, uint32_t count, int32_t *spans_out) {
    if (!c || !spans_out) return PRK_ERR_ARG;
    *spans_out = -1;
    if (!spans && count) return PRK_ERR_ARG;
    // a handle's spans are indexed by 31 bits, as a frame's span input
    if (count >= 0x7FFFFFFFu || c->sbatches.size() >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    SpanBatch B;
    B.cnt.assign(1, count);
    B.total = count;
    if (count) {
        PRK_TRY(hipSetDevice(c->device));
        const size_t bytes = packed_span_bytes(count), used = (size_t)count * sizeof(prk_span);
        PRK_TRY(hipMalloc(&B.sp, bytes));
        hipError_t e = hipMemset(static_cast<char *>(B.sp) + bytes - 16, 0, 16);  // (the last piece's spare dwords)
        if (e == hipSuccess) e = hipMemcpy(B.sp, spans, used, hipMemcpyHostToDevice);  // the one copy of the caller's spans
        if (e != hipSuccess) {
            (void)hipFree(B.sp);
            return status_of(e);
        }
    }
    return sbatch_add(c, std::move(B), spans_out);
}

int prk_spans_upload_rows(prk_context *c, const prk_row *rows, uint64_t row_count, const prk_row_pair *pairs,
                          uint64_t pair_count, int32_t *spans_out) {
    if (!c || !spans_out) return PRK_ERR_ARG;
    *spans_out = -1;
    if ((!rows && row_count) || (!pairs && pair_count)) return PRK_ERR_ARG;
    uint64_t sum = 0;
    for (uint64_t r = 0; r < row_count; ++r) {  // (prk_draw_rows' checks)
        if (rows[r].RowIndex < 0) return PRK_ERR_ARG;
        sum += rows[r].EdgeCount;
    }
    if (sum != pair_count) return PRK_ERR_ARG;
    if (row_count >= 0x7FFFFFFFull || pair_count >= 0x7FFFFFFFull || c->sbatches.size() >= 0x7FFFFFFFull)
        return PRK_ERR_LIMIT;
    SpanBatch B;
    const uint32_t n = row_count ? (uint32_t)pair_count : 0u;
    B.cnt.assign(1, n);
    B.total = n;
    if (n) {
        PRK_TRY(hipSetDevice(c->device));
        PRK_TRY(hipMalloc(&B.sp, packed_span_bytes(n)));
        const int rc = rows_to_spans(c, rows, (uint32_t)row_count, pairs, n, nullptr, B.sp);
        if (rc != PRK_OK) {
            (void)hipFree(B.sp);
            return rc;
        }
    }
    return sbatch_add(c, std::move(B), spans_out);
}

int prk_spans_info(prk_context *c, int32_t handle, uint32_t *list_count_out, uint64_t *total_out) {
    const SpanBatch *B = sbatch_of(c, handle);
    if (!B) return PRK_ERR_ARG;
    if (list_count_out) *list_count_out = (uint32_t)B->cnt.size();
    if (total_out) *total_out = B->total;
    return PRK_OK;
}

int prk_spans_lists(prk_context *c, int32_t handle, uint32_t *span_counts) {
    const SpanBatch *B = sbatch_of(c, handle);
    if (!B) return PRK_ERR_ARG;
    if (span_counts && !B->cnt.empty()) std::memcpy(span_counts, B->cnt.data(), B->cnt.size() * 4);
    return PRK_OK;
}

int prk_spans_download(prk_context *c, int32_t handle, prk_span *spans, uint64_t capacity) {
    const SpanBatch *B = sbatch_of(c, handle);
    if (!B || capacity < B->total || (!spans && B->total)) return PRK_ERR_ARG;
    if (!B->total) return PRK_OK;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipMemcpy(spans, B->sp, (size_t)B->total * sizeof(prk_span), hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_spans_destroy(prk_context *c, int32_t handle) {
    SpanBatch *B = sbatch_of(c, handle);
    if (!B) return PRK_ERR_ARG;
    for (const prk::DrawRec &d : c->draws)  // a recorded draw reads it at the flush (prk_reset_draws releases it)
        if (d.src_kind == 5 && d.geom == handle) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // frames in flight read it
    (void)hipFree(B->sp);
    *B = SpanBatch{};
    return PRK_OK;
}

// One draw of spans [first_span, first_span + span_count) of a handle: what
// prk_draw_spans records for the same spans, minus the copies.
int prk_draw_span_records(prk_context *c, int32_t handle, uint32_t first_span, uint32_t span_count,
                          int32_t semantics, int32_t phong, int32_t texture) {
    const SpanBatch *B = sbatch_of(c, handle);
    if (!B || (uint64_t)first_span + span_count > B->total) return PRK_ERR_ARG;
    if (span_count == 0) return PRK_OK;
    const int rc = draw_src(c, 5, first_span, span_count, span_count, semantics, phong, texture);
    if (rc != PRK_OK) return rc;
    c->draws.back().geom = handle;
    return PRK_OK;
}

int prk_debug_list_routes(prk_context *c, uint32_t *out, int32_t n) {
    if (!c || !out || n < 0 || n > 6) return PRK_ERR_ARG;
    for (int i = 0; i < n; ++i) out[i] = c->spans.list_routes[i];
    return PRK_OK;
}

}  // extern "C"
