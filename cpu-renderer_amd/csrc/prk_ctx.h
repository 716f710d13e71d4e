// prk_ctx.h — the host runtime's own header: struct prk_context (opaque in
// include/prk.h) with the resources and scratch it owns, the state a pass is
// queued with, the ordering of the side passes between frames (side_begin),
// and the few host functions that cross the host files (prk_api.hip,
// prk_target_api.hip, prk_geometry_api.hip, prk_selftest.hip, prk_flush.hip,
// prk_span_pass.hip, prk_record_api.hip, prk_visibility_api.hip,
// prk_select_api.hip, prk_bounds_api.hip).  Host only; prk_launch.h stays the
// seam to the kernel files (prk_types.h: the records the buffers here hold),
// and prk_dist.hip keeps the context opaque.
//
// Nothing here reaches the library's dynamic symbol table: the helper types
// and inline functions sit in a hidden-visibility region (one definition for
// the host files, none exported), the cross-file functions are declared
// hidden one by one.  Only prk_context itself keeps default visibility.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/prk.h"
#include "prk_device.h"
#include "prk_launch.h"  // the kernel files' launchers, and what the host shares with them

constexpr uint32_t kObjWaveTris = 48;        // objects of this many triangles or more
// ... and sorted edge lists (prk_draw_edge_lists) of this many edges or more
// are large objects: the most edges the smallest large triangle object has
constexpr uint32_t kObjWaveEdges = 3 * kObjWaveTris;
constexpr uint64_t kPrMaxEntries = 1ull << 23;  // the chunked walk's list entries per pass (~3 GB of scratch)

// Per-frame scratch sets in flight: a frame whose target band has at most
// kSmallBandPx pixels (64 Mpx) cycles PRK_FRAME_SETS sets, larger ones 2 (the set
// count nsets; consecutive frames take consecutive sets): with three, frame k+1's binning need not wait for
// frame k-1's raster (round 2, band of 512 x 4096 px, one rank of 8: 0.284 ->
// 0.247 ms; 1024 rows: 0.405 -> 0.378; the whole 4096^2 frame then 1-3 %
// slower, with the host waiting for every frame's count).
#ifndef PRK_FRAME_SETS
#define PRK_FRAME_SETS 3
#endif
// Round 3 (lazy bin count): three sets for every target up to 64 Mpx (C5
// included) — the whole C3b frame 1.049-1.053 -> 1.041-1.044 ms (interleaved
// A/B, three rounds); round 2 measured three sets 1-3 % slower there when the
// host waited for every frame's count.
#ifndef PRK_SMALL_BAND_LOG2
#define PRK_SMALL_BAND_LOG2 26
#endif
constexpr size_t kSmallBandPx = (size_t)1 << PRK_SMALL_BAND_LOG2;

#pragma GCC visibility push(hidden)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // The buffer as n records of T (prk_types.h): sized by the type, read through it.
    template <class T> hipError_t ensure_n(size_t n) { return ensure(n * sizeof(T)); }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct Geometry {
    const float *V = nullptr, *C = nullptr, *N = nullptr, *UV = nullptr;
    uint32_t vertex_count = 0;
    uint32_t cap[4] = {0, 0, 0, 0};  // owned V / C / N / UV buffers hold this many vertices
    bool owned = false;
};
constexpr size_t kGeomComp[4] = {3, 4, 3, 2};  // floats a vertex in V / C / N / UV

struct Texture {
    uint8_t *mem = nullptr;
    int32_t w = 0, h = 0, pitch = 0;
    int32_t filter = 0;  // PRK_FILTER_*
};

// A target layer (prk_layer_*): a rectangle of (colour, z) pixels in device
// memory, the library's (prk_layer_alloc) or the caller's (wrapped: read-only).
struct Layer {
    uint8_t *color = nullptr;
    float *z = nullptr;  // rows of w floats
    int32_t w = 0, h = 0, pitch = 0;
    bool wrapped = false, live = false;
};

// A record batch (prk_records_*): lists in prk_edge_records' packed layout,
// kept in device memory.  The host keeps each list's edge count and whether
// it takes the sorted walks (flush_spans routes by them) -- no records.
struct Records {
    void *rec = nullptr;      // the packed records, readable up to a multiple of 16 bytes
    uint32_t *tab = nullptr;  // device: the counts (lists + 1 words, the last 0), then the sorted flags
    std::vector<uint32_t> cnt, flag;
    uint64_t total = 0;
    bool live = false;
    const uint32_t *d_cnt() const { return tab; }
    const uint32_t *d_flag() const { return tab + cnt.size() + 1; }
    const void *at(uint64_t r) const { return static_cast<const char *>(rec) + r * sizeof(prk_edge); }  // record r
};

// A span batch (prk_spans_*): packed prk_span records kept in device memory.
// The host keeps each list's span count and the total -- no spans.
struct SpanBatch {
    void *sp = nullptr;  // the packed spans, readable up to a multiple of 16 bytes (the spare dwords zero)
    std::vector<uint32_t> cnt;
    uint64_t total = 0;
    bool live = false;
};

inline int status_of(hipError_t e) {
    if (e == hipSuccess) return PRK_OK;
    static const bool trace = std::getenv("PRK_TRACE_HIP") != nullptr;  // diagnostics: name the HIP error
    if (trace) std::fprintf(stderr, "prk: HIP error %d (%s)\n", (int)e, hipGetErrorName(e));
    if (e == hipErrorOutOfMemory) return PRK_ERR_NOMEM;
    return PRK_ERR_DEVICE;
}

// An exclusive scan, or the objects' radix sort, with its temporary storage
// in `temp`: the size query, the buffer, the run.
inline hipError_t scan_u32(DevBuf &temp, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t s) {
    size_t tb = 0;
    hipError_t e = prk_scan_u32(in, out, n, nullptr, &tb, s);
    if (e == hipSuccess) e = temp.ensure(std::max<size_t>(tb, 16));
    if (e == hipSuccess) e = prk_scan_u32(in, out, n, temp.p, &tb, s);
    return e;
}
inline hipError_t scan_u64(DevBuf &temp, const unsigned long long *in, unsigned long long *out, uint32_t n, hipStream_t s) {
    size_t tb = 0;
    hipError_t e = prk_scan_u64(in, out, n, nullptr, &tb, s);
    if (e == hipSuccess) e = temp.ensure(std::max<size_t>(tb, 16));
    if (e == hipSuccess) e = prk_scan_u64(in, out, n, temp.p, &tb, s);
    return e;
}
inline hipError_t obj_sort(DevBuf &temp, void *keys_in, uint32_t *vals_in, void *keys_out, uint32_t *vals_out, uint32_t n,
                    uint32_t end_bit, hipStream_t s) {
    size_t tb = 0;
    hipError_t e = prk_obj_sort(keys_in, vals_in, keys_out, vals_out, n, end_bit, nullptr, &tb, s);
    if (e == hipSuccess) e = temp.ensure(std::max<size_t>(tb, 16));
    if (e == hipSuccess) e = prk_obj_sort(keys_in, vals_in, keys_out, vals_out, n, end_bit, temp.p, &tb, s);
    return e;
}

// Visibility feedback (prk_visibility_*, prk_visibility_api.hip): the winner
// map of the last flush reduced to per-id pixel counts.  prk_flush says
// whether its frame has an answer (draws, and the winner map of debug mode)
// and how many ids it handed out; the first query reduces the map, later ones
// of the same frame reuse the arrays.  The buffers grow with ensure and are
// reused frame to frame.
struct VisState {
    DevBuf d_counts, d_flags, d_pix, d_vis, d_ids, d_temp;  // id_count + 1 words each (d_ids: id_count)
    DevBuf d_starts, d_gout;                                // prk_visibility_groups: its ranges, its two outputs
    bool frame = false;  // the last prk_flush drew, with the winner map on
    bool done = false;   // ... and has been reduced
    uint32_t id_count = 0, visible = 0;
    uint64_t covered = 0;
};

// prk_geometry_transform (prk_geometry_api.hip): its tables (scan, runs, matrices),
// staged in pinned memory and copied on copy_stream ahead of the kernel.
struct XformState {
    DevBuf d_tab;
    void *h_tab = nullptr;
    size_t h_cap = 0;
    hipEvent_t copied_ev = nullptr;  // the staging has been copied (the next call refills it)
    hipEvent_t end_ev = nullptr;     // after the kernel (timed from copied_ev: prk_debug_transform_ms)
    bool busy = false;
};

// prk_geometry_select (prk_select_api.hip): the call's tables as uploaded, what
// the device builds from them (chosen, n, start, the runs) and the scan's
// scratch, all reused call to call; the emit pass of one call reads them
// until the next call's uploads, which the geometry stream orders behind it.
struct SelState {
    DevBuf d_tab, d_out, d_temp;
    hipEvent_t ev[4] = {};  // (timed: prk_debug_select_ms) before the uploads, after the total's copy; around the emit pass
    bool timed = false, emitted = false;
};

// prk_visibility_bounds (prk_bounds_api.hip): the target's min-z tile map,
// rebuilt at every call (it belongs to the target, not to a frame's winner
// map), the call's tables as uploaded, and the answer -- `count` words that
// stay valid until the next call or until the target is replaced.
struct BoundsState {
    DevBuf d_zmin, d_tab, d_pixels;
    hipEvent_t ev[3] = {};  // (timed: prk_debug_bounds_ms) before k_ztile_min, between the kernels, after k_bounds_test
    bool answered = false, timed = false, tested = false;  // tested: the timed call ran k_bounds_test (count > 0)
    uint32_t count = 0;
    int32_t tiles_x = 0, tiles_y = 0, first_tile_row = 0;  // the map of the last call (prk_debug_ztiles)
};

// The state a pass is queued with and an overflow re-run (resolve_count)
// runs with again: the target, the tile, the cameras and lights, the clear.
// The context holds its own as its base (prk_context), so this is the one
// list of these fields: pass_state() copies them out, apply_pass_state() in.
struct PassState {
    // target
    void *color = nullptr;
    int32_t pitch = 0;
    float *zbuf = nullptr;
    int32_t W = 0, H = 0, row0 = 0, row1 = 0;
    int32_t tile_w = 256, tile_h = 8;  // measured best for C3b
    // camera + lights: transform / lights set the draws up (FillEdgeTable's
    // ProjectVertex and Gouraud lighting), shade_* shade their spans (Phong and
    // UnprojectVertex, read when DrawModel* runs); prk_set_camera sets both
    prk_transform transform{};
    prk_light_data lights{};
    prk_transform shade_transform{};
    prk_light_data shade_lights{};
    bool clear_pending = false;  // prk_target_clear_on_flush
    uint32_t clear_color = 0;
    float clear_z = 0.0f;
    bool debug = false;
};

#pragma GCC visibility pop

struct prk_context : PassState {  // (the target, tile, cameras, lights, clear and debug flag: PassState)
    int device = 0;
    hipStream_t own_stream = nullptr;
    // Side passes: work queued between frames, without waiting, on what frames
    // read or write.  It runs on copy_stream between side_begin() and side_end().
    //   Geometry form (prk_geometry_write, prk_geometry_transform, the emit pass
    //   of prk_geometry_select): the pass waits for read_ev, which prk_flush (and
    //   a re-run, resolve_count) records on the flush stream at the frame's end;
    //   read_rec: there is such a record (geometry_grow drops it once the device
    //   is idle).  prk_resolve_pending's gather stream waits for it too.
    //   Target form (prk_target_upload_async, prk_texture_from_target, the layer
    //   passes, prk_visibility_bounds): the pass touches the target, so it also
    //   waits for s_mark, recorded on own_stream then: the clears and uploads
    //   queued so far.  (s_mark is a scratch event; flush_tris' vis stream waits
    //   on it the same way for the flush stream's work so far.)
    // side_end() records in_ev after the work and sets in_wait; side_wait() is
    // the wait for it: the three streams of the next prk_flush, which then
    // clears in_wait, and prk_target_clear (prk_target_upload joins it on the
    // host).  prk_visibility_bounds only reads and waits itself: no side_end().
    hipStream_t copy_stream = nullptr;
    hipEvent_t read_ev = nullptr, in_ev = nullptr, s_mark = nullptr;
    bool read_rec = false, in_wait = false;
    bool owns_target = false;
    bool have_camera = false;
    // resources
    std::vector<Geometry> geoms;
    std::vector<Texture> texs;
    // record batches by handle (a destroyed one keeps its slot, dead).  A
    // prk_draw_records DrawRec: src_kind 4, geom the handle, geom_tri0 /
    // tri_count its lists, src_off / src_n their records within the handle.
    std::vector<Records> recs;
    // span batches by handle, their own number space (a destroyed one keeps
    // its slot, dead).  A prk_draw_span_records DrawRec: src_kind 5, geom the
    // handle, src_off / src_n its spans within the handle.
    std::vector<SpanBatch> sbatches;
    // target layers by handle, their own number space (a destroyed one keeps
    // its slot, dead)
    std::vector<Layer> layers;
    std::vector<prk::DrawRec> draws;
    uint32_t pending_tris = 0;
    std::vector<prk_edge> pend_edges;  // prk_draw_edges input of the pending frame
    std::vector<prk_span> pend_spans;  // prk_draw_spans input of the pending frame
    // prk_draw_edge_lists input of the pending frame: the batches' records back
    // to back, and per list its edge count and whether it takes the sorted
    // walks (list_walks_sorted).  A batch's DrawRec: src_kind 3, src_off /
    // src_n its records, geom_tri0 its first list, tri_count its lists.
    std::vector<prk_edge> pend_ledges;
    std::vector<uint32_t> pend_lcnt, pend_lflag;
    // Per-frame scratch, nsets of them in use (2, or PRK_FRAME_SETS for small
    // bands): frame k bins (and, on span-record frames, runs k_vis) into the
    // set after frame k-1's on bin_stream while frame k-1 shades on the
    // flush's stream.
    struct BinSet {
        DevBuf d_draws, d_texs, d_tri_draw, d_ranges, d_tri_n, d_tri_off, d_pair_tri, d_bins, d_offs, d_won, d_list,
            d_nwin, d_wtag, d_recs, d_trwon, d_wlist, d_seltemp, d_trec, d_ghist, d_tile_tot, d_chunk, d_info,
            d_runlist, d_run_n;
        uint32_t *h_info = nullptr;       // pinned: [entry count, overflow] of the set's last binning
        hipEvent_t counted_ev = nullptr;  // h_info of this set's binning has landed
        hipEvent_t listed_ev = nullptr;   // a band frame's run lists are written (k_band_rec may start)
        // bytes last uploaded into d_draws / d_texs and the buffer they went
        // to: an unchanged table (every frame of a static scene) is not sent again
        std::vector<uint8_t> h_draws, h_texs;
        const void *h_draws_at = nullptr, *h_texs_at = nullptr;
        hipEvent_t free_ev = nullptr;    // the raster that read this set is done
        hipEvent_t binned_ev = nullptr;  // this set's binning is done
        bool used = false;
    };
    static constexpr int kSets = PRK_FRAME_SETS;
    BinSet bset[kSets];
    hipStream_t bin_stream = nullptr;
    hipStream_t vis_stream = nullptr;  // k_vis of span-record frames
    DevBuf d_winners, d_anomaly, d_prof;
    // z early: the last flush was a span-record pass, whose k_vis writes the
    // final z (k_pix only the colour): a download takes z from the event after
    // k_vis (ev[z_slot][3]) while the frame shades.  d_negz counts the -0.0
    // z k_pix wrote over k_vis's +0.0 since the last download.
    DevBuf d_negz;
    bool early_z = false;  // prk_set_early_z
    bool z_early = false;
    int z_slot = -1;
    uint32_t *h_total = nullptr;  // pinned
    uint32_t pair_hint = 0;       // entry count of the last frame (counting-sort capacity)
    // Automatic tile (until prk_set_tile): 256x8, or narrower tiles for frames
    // with few bin entries per tile (under one wave's 64-entry chunk per
    // tile: 32x8, C2; under 8: 64x8, C1 — the binning's per-tile passes then
    // cost more than the extra parallelism gains), decided from a frame's
    // count at 256x8 and kept while the triangle count and the band stay
    // within 2x of that frame's (measured, profiles/r02b/small_config_tiles.log).
    bool tile_auto = true;
    int32_t auto_small = 0;  // 0: 256x8; else the small tile width (64: under 8 entries per tile, 32: under 64)
    // Wide tiles: an all-AVX frame whose triangles make >= 4.5 bin entries
    // each at 256x8 (large triangles: C5's radius-32 soup makes 5.6) draws
    // faster at 512x8 (C5 3.24 -> 2.97 ms, its band of 8 0.474 -> 0.426 ms;
    // C3b, 3.2 entries a triangle, is fastest at 256x8: 1.021 vs 1.029 ms;
    // scalar C3a is slower at 512x8), decided and kept like auto_small.
    int32_t auto_wide = 0;
    uint32_t auto_T = 0;
    int32_t auto_px = 0;
    // all-AVX frames: per-triangle setup records; the AVX k_vis / k_walk read
    // them instead of running FillEdgeTable, so they are not optional
    bool setup_rec = true;
    bool winners_valid = false;
    VisState vis;
    XformState xf;
    SelState sel;
    BoundsState bnd;
    prk_stats stats{};
    // Timing ring: 6 events per flush.
    static constexpr int kRing = 32;
    // bin start, bin end (bin_stream); raster end, k_vis end, k_walk end,
    // raster start (flush stream)
    hipEvent_t ev[kRing][6] = {};
    bool pending[kRing] = {};
    bool split_span[kRing] = {};  // the slot's flush ran k_walk + k_pix
    uint32_t frame = 0;
    int last_slot = -1;
    int last_set = -1;  // scratch set of the last per-triangle pass
    // The last per-triangle pass, whose bin entry count the host has not read
    // yet (flush_tris with `defer`): prk_flush returns once the frame is
    // queued, and the count is read at the next call that needs it
    // (resolve_count) — by then the binning has long finished, so the host
    // no longer waits for every frame's binning before queueing the next
    // frame.  A pass whose entries overflowed the scratch is re-run there,
    // before anything else is queued or read, with the state it was queued
    // with (target, camera, tile, clear).
    struct PendingCount {
        bool active = false;
        int set = 0;
        hipStream_t s = nullptr;
        std::vector<prk::DrawRec> draws;
        uint32_t T = 0, win_base = 0, ntiles = 0;
        bool fuse = false;  // the pass folded a pending clear in: the re-run's clear_pending
        PassState state;
    } pcount;
    // Span path (whole-object AETs) scratch, reused frame to frame.
    struct SpanScratch {
        DevBuf d_stage, d_edges, d_ord, d_temp, d_recs, d_pos, d_span_tri, d_scnt, d_soff, d_vals_b,
            d_offs, d_nwin, d_wtag, d_srecs, d_work, d_ekeys, d_ekeys2, d_evals, d_ecnt, d_escan,
            d_rcnt, d_rscan, d_bound, d_oslot, d_pool, d_err, d_raw, d_most, d_cls, d_prrow, d_prcnt, d_preoff,
            d_prfge, d_prccur, d_prkey, d_prest, d_prsst, d_preend, d_preendm, d_prmatch, d_prsidx, d_prsm, d_prstat,
            d_segcnt, d_segoff, d_segs, d_wy, d_mhuge, d_objtab, d_k0tab, d_lscan, d_lobj, d_lrows,
            d_ltab,  // a pass with handle draws: its lists' counts and flags (k_list_tables)
            d_rectab, d_reccnt, d_recout,  // prk_edge_records: its tables, counts and packed records
            d_spanout,                     // prk_span_records: its packed spans
            d_rowslot, d_rowcnt, d_rowscan, d_rowout,  // prk_row_records: its row slots, counts, scan, packed rows
            d_lstat;  // the record walks of a handle: its lists' statistics, the candidates and their most linked
        // prk_draw_rows' own buffers (frames in flight use the ones above): the
        // caller's rows and pairs, the EdgeCounts and their scan, the spans
        DevBuf d_dr_rows, d_dr_pairs, d_dr_cnt, d_dr_scan, d_dr_temp, d_dr_out;
        // the pass's host tables, packed into pinned memory for one upload
        // (stage_ev: that upload, before the staging is rewritten)
        char *h_stage = nullptr;
        size_t stage_cap = 0;
        hipEvent_t stage_ev = nullptr;
        bool stage_busy = false;
        // host tables of the pass, kept until their asynchronous uploads ran
        std::vector<prk::ObjRun> h_runs;
        std::vector<uint32_t> h_big_gl, h_k1src, h_lcnt;
        std::vector<prk::PrepSeg> h_segs;     // a pass with handle draws: its batch edges' segments
        std::vector<prk::ListSrc> h_lsrc;     // ... and the handles its runs take their list tables from
        size_t last_stage_bytes = 0;     // debug (prk_debug_stage_bytes): the last pass's staging upload
        std::vector<prk::DrawRec> h_draws;
        std::vector<prk::TexRec> h_texs;
        uint32_t *h_rb = nullptr;  // pinned readback words
        char *h_cls = nullptr;     // pinned: the large objects' most active entries, then their walk groups
        size_t cls_cap = 0;
        // debug (prk_debug_walk_routes): the last pass with large objects --
        // objects per walk class, objects sized by k_maxact_huge_*, and the
        // first large object's (most, rows, entries) as read back
        uint32_t walk_routes[9] = {};
        int32_t walk_sizes[3] = {};
        // debug (prk_debug_list_routes): the most recent record call's lists
        // on the thread walk, then in each slot class of the workgroup walk
        uint32_t list_routes[6] = {};
    } spans;
    // debug (prk_debug_bins): the last per-triangle pass of the most recent
    // flush, if it was queued with the debug flag on -- its scratch set and
    // the frame sizes its binning ran with
    struct BinsDebug {
        bool valid = false, rerun = false;
        int set = 0;
        uint32_t T = 0, per = 0;
        int32_t tile_w = 0, tile_h = 0, tiles_x = 0, tiles_y = 0, row0 = 0, row1 = 0;
    } bdbg;
};

#define PRK_HIDDEN __attribute__((visibility("hidden")))

PRK_HIDDEN inline PassState pass_state(const prk_context *c) { return *c; }
PRK_HIDDEN inline void apply_pass_state(prk_context *c, const PassState &p) { static_cast<PassState &>(*c) = p; }

// The side passes' ordering (the rule: prk_context::copy_stream); after_own_stream is the target form.
PRK_HIDDEN inline hipError_t side_begin(prk_context *c, bool after_own_stream) {
    hipError_t e = c->read_rec ? hipStreamWaitEvent(c->copy_stream, c->read_ev, 0) : hipSuccess;
    if (e == hipSuccess && after_own_stream) e = hipEventRecord(c->s_mark, c->own_stream);
    if (e == hipSuccess && after_own_stream) e = hipStreamWaitEvent(c->copy_stream, c->s_mark, 0);
    return e;
}
PRK_HIDDEN inline hipError_t side_end(prk_context *c) {
    const hipError_t e = hipEventRecord(c->in_ev, c->copy_stream);
    if (e == hipSuccess) c->in_wait = true;
    return e;
}
PRK_HIDDEN inline hipError_t side_wait(const prk_context *c, hipStream_t s) {
    return c->in_wait ? hipStreamWaitEvent(s, c->in_ev, 0) : hipSuccess;
}

// `device` among the devices there are: PRK_ERR_DEVICE without any,
// PRK_ERR_ARG outside them; it is then made current (unless `set` is off).
PRK_HIDDEN inline int use_device(int device, bool set = true) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device < 0 || device >= ndev) return PRK_ERR_ARG;
    return set ? status_of(hipSetDevice(device)) : PRK_OK;
}

// The texture table as the kernels read it (FrameParams texs), from the
// context's textures: one entry a handle.
PRK_HIDDEN inline void tex_table(const prk_context *c, std::vector<prk::TexRec> &out) {
    out.resize(c->texs.size());
    for (size_t i = 0; i < out.size(); ++i)
        out[i] = prk::TexRec{c->texs[i].mem, c->texs[i].w, c->texs[i].h, c->texs[i].pitch, c->texs[i].filter};
}

// ---- host functions that cross the host files (each defined once; C linkage
// and hidden, as prk_resolve_pending in prk_launch.h) -------------------------
extern "C" {
// prk_flush.hip
PRK_HIDDEN int resolve_count(prk_context *c);
PRK_HIDDEN void frame_params(const prk_context *c, prk::FrameParams &fp);
PRK_HIDDEN hipError_t launch_fill_target(void *color, int32_t pitch, float *z, int32_t W, int32_t rows,
                                         uint32_t cval, float zval, hipStream_t s);
// prk_span_pass.hip
PRK_HIDDEN int flush_spans(prk_context *c, hipStream_t s, const std::vector<prk::DrawRec> &draws, uint32_t T,
                           uint32_t win_base);
// prk_api.hip: the draw recorders' and the timing ring's
PRK_HIDDEN void harvest(prk_context *c, int slot);
PRK_HIDDEN int draw_src(prk_context *c, uint32_t kind, uint32_t off, uint32_t n, uint32_t ids, int32_t semantics,
                        int32_t phong, int32_t texture);
PRK_HIDDEN bool list_walks_sorted(const prk_edge *e, uint32_t n);
PRK_HIDDEN int rows_to_spans(prk_context *c, const prk_row *rows, uint32_t nrow, const prk_row_pair *pairs,
                             uint32_t npair, prk_span *out, void *keep = nullptr);
// prk_geometry_api.hip: room for `end` vertices in a library-owned geometry's arrays that exist or are wanted now.
PRK_HIDDEN int geometry_grow(prk_context *c, int32_t handle, const bool want[4], uint32_t end);
// prk_visibility_api.hip: the frame's answer, reduced if this is the first query since its flush.
PRK_HIDDEN int vis_ready(prk_context *c);
// prk_select_api.hip: prk_geometry_select's table checks (prk_selftest.hip runs them too).
PRK_HIDDEN int select_check(const prk_select_item *items, uint32_t item_count, const prk_select_level *levels,
                            uint32_t level_count, const prk_xform *xforms, uint32_t xform_count, uint32_t src_tris,
                            const uint32_t *frame_ids, uint64_t *worst);
// prk_bounds_api.hip: prk_visibility_bounds' band and camera record (false: a band of 2^32 pixels or more;
// prk_selftest.hip builds its own with it).
PRK_HIDDEN bool bounds_frame(int32_t W, int32_t row0, int32_t row1, const prk_transform &t, const float P[3],
                             prk::BoundsFrame *out);
}  // extern "C"

// A status passed on unless it is PRK_OK.
#define PRK_CHECK(expr)                \
    do {                               \
        const int _rc = (expr);        \
        if (_rc != PRK_OK) return _rc; \
    } while (0)

// Calls that read or replace the target, or change what a re-run of the
// pending pass would read, first resolve its count (PendingCount).
#define RESOLVE_COUNT(c) PRK_CHECK(resolve_count(c))

#define PRK_TRY(expr)                              \
    do {                                           \
        hipError_t _e = (expr);                    \
        if (_e != hipSuccess) return status_of(_e); \
    } while (0)
