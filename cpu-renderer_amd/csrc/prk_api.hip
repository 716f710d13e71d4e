// prk_api.cpp — host side of libprk_hip.so: the C-ABI declared in include/prk.h.
//
// Owns device resources (geometry, textures, scratch for binning) and turns the
// reference's draw calls into one GPU frame per prk_flush:
//   FillEdgeTable + DrawModelOptimized / DrawModel (projekt.cpp:3882, 3615, 162)
//   -> prk_draw records {geometry range, P, semantics, Phong, Bitmap}
//   Platform.CompleteAllWork -> prk_flush runs bin + raster kernels.
// There is no CPU fallback: every entry point that computes pixels needs the
// HIP device and fails with PRK_ERR_DEVICE without one.
#include <hip/hip_runtime.h>
#include <link.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <functional>
#include <atomic>
#include <string>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/prk.h"
#include "../../include/prk_edge_count.h"
#include "prk_device.h"
#include "prk_launch.h"  // the kernel files' launchers, and what the host shares with them

#ifndef PRK_REC_AFTER_CS
#define PRK_REC_AFTER_CS 1  // a band's k_band_rec queued after the counting sort's launches
#endif
#ifndef PRK_BINNED_EARLY
#define PRK_BINNED_EARLY 0  // 1: binned_ev before the entry count's copy to the host (serial band binning
                            // 0.084 -> 0.075 ms, but C3b N = 8 pipelined 0.186 -> 0.21-0.22 ms: the copy,
                            // which the host waits for, then queues behind k_vis)
#endif

using prk::ListSrc;
using prk::ObjDesc;
using prk::ObjRun;
using prk::PrepSeg;
using prk::kAdvWgCaps;
using prk::kObjEdgeBytes;
using prk::kPairRawBytes;
using prk::kPrepEdges;
using prk::kScSpanRecBytes;
using prk::kWaveListArrays;
using prk::packed_edge_bytes;
using prk::packed_span_bytes;
constexpr uint32_t kObjWaveTris = 48;        // objects of this many triangles or more
// ... and sorted edge lists (prk_draw_edge_lists) of this many edges or more
// are large objects: the most edges the smallest large triangle object has
constexpr uint32_t kObjWaveEdges = 3 * kObjWaveTris;
constexpr uint64_t kPrMaxEntries = 1ull << 23;  // the chunked walk's list entries per pass (~3 GB of scratch)

// AVX frames shade through span records (k_walk + k_pix); must match
// PRK_SPAN_RECORDS of prk_kernels.hip.
#define PRK_SPAN_RECORDS_HOST 1
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

namespace {

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
};

struct Geometry {
    const float *V = nullptr, *C = nullptr, *N = nullptr, *UV = nullptr;
    uint32_t vertex_count = 0;
    uint32_t cap[4] = {0, 0, 0, 0};  // owned V / C / N / UV buffers hold this many vertices
    bool owned = false;
};

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

int status_of(hipError_t e) {
    if (e == hipSuccess) return PRK_OK;
    static const bool trace = std::getenv("PRK_TRACE_HIP") != nullptr;  // diagnostics: name the HIP error
    if (trace) std::fprintf(stderr, "prk: HIP error %d (%s)\n", (int)e, hipGetErrorName(e));
    if (e == hipErrorOutOfMemory) return PRK_ERR_NOMEM;
    return PRK_ERR_DEVICE;
}

// An exclusive scan, or the objects' radix sort, with its temporary storage
// in `temp`: the size query, the buffer, the run.
hipError_t scan_u32(DevBuf &temp, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t s) {
    size_t tb = 0;
    hipError_t e = prk_scan_u32(in, out, n, nullptr, &tb, s);
    if (e == hipSuccess) e = temp.ensure(std::max<size_t>(tb, 16));
    if (e == hipSuccess) e = prk_scan_u32(in, out, n, temp.p, &tb, s);
    return e;
}
hipError_t scan_u64(DevBuf &temp, const unsigned long long *in, unsigned long long *out, uint32_t n, hipStream_t s) {
    size_t tb = 0;
    hipError_t e = prk_scan_u64(in, out, n, nullptr, &tb, s);
    if (e == hipSuccess) e = temp.ensure(std::max<size_t>(tb, 16));
    if (e == hipSuccess) e = prk_scan_u64(in, out, n, temp.p, &tb, s);
    return e;
}
hipError_t obj_sort(DevBuf &temp, void *keys_in, uint32_t *vals_in, void *keys_out, uint32_t *vals_out, uint32_t n,
                    uint32_t end_bit, hipStream_t s) {
    size_t tb = 0;
    hipError_t e = prk_obj_sort(keys_in, vals_in, keys_out, vals_out, n, end_bit, nullptr, &tb, s);
    if (e == hipSuccess) e = temp.ensure(std::max<size_t>(tb, 16));
    if (e == hipSuccess) e = prk_obj_sort(keys_in, vals_in, keys_out, vals_out, n, end_bit, temp.p, &tb, s);
    return e;
}

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

// The switches a span pass (flush_spans) obeys, read from the environment at
// the start of every pass: tests set and unset them between the flushes of
// one process.
struct SpanSwitches {
    // PRK_OBJ_LOCAL_SORT=0: one radix sort of the padded keys even when no
    // object has more than 64 edges (else per object, k_obj_sort_local)
    bool local_sort = !off("PRK_OBJ_LOCAL_SORT");
    // PRK_OBJ_SEGMENTS=0: the small objects a thread per object, not a thread
    // per stretch of rows with a non-empty list (k_obj_seg)
    bool segments = !off("PRK_OBJ_SEGMENTS");
    // PRK_OBJ_HUGE_EDGES=n (tests): objects of n edges or more, not of 2^18,
    // are sized by many workgroups each (k_maxact_huge_*)
    uint32_t huge_edges = 1u << 18;
    // PRK_OBJ_BIG=0: an object past the slot classes is always walked by one
    // wave (k_obj_walk_wave), never by the huge-object walk
    bool big = !off("PRK_OBJ_BIG");
    // PRK_OBJ_LDSWALK=0: the huge-object walk never in its LDS form (k_obj_walk_lds)
    bool ldswalk = !off("PRK_OBJ_LDSWALK");
    // PRK_OBJ_BIG_MIN=n (tests): objects of more than n active edges skip the
    // walk groups' slot classes (the chunked walk's groups do not look at it)
    int64_t big_min = INT64_MAX;
    // PRK_OBJ_ROWS=0: no chunked walk; every large object takes the workgroup walk alone
    bool rows = !off("PRK_OBJ_ROWS");
    // PRK_OBJ_CHUNK_WARMUP=0 (tests: every fix-up path): the chunked walk without its warm-up
    bool chunk_warmup = !off("PRK_OBJ_CHUNK_WARMUP");
    // PRK_POS_MEMSET=1: the span slots are marked unused by a memset even in a
    // pass without large objects (whose walks mark their own)
    bool pos_memset = false;
    // PRK_PR_DEBUG: a line about the pass's chunked walk on stderr
    bool pr_debug = std::getenv("PRK_PR_DEBUG") != nullptr;
    SpanSwitches() {
        if (const char *env = std::getenv("PRK_OBJ_HUGE_EDGES")) huge_edges = (uint32_t)std::max(1l, std::atol(env));
        if (const char *env = std::getenv("PRK_OBJ_BIG_MIN")) big_min = std::atoll(env);
        const char *env = std::getenv("PRK_POS_MEMSET");
        pos_memset = env && env[0] == '1';
    }
    static bool off(const char *name) {
        const char *env = std::getenv(name);
        return env && env[0] == '0';
    }
};

// The slot class of a large object whose list holds `most` entries at the
// most: the smallest of the slot walk's LDS capacities (kAdvWgCaps) that holds
// them and that the device grants (lcap), or 0 for none.
uint32_t slot_class(int32_t most, uint32_t lcap) {
    if (most < 0) return 0;
    for (const uint32_t cap : kAdvWgCaps)
        if (cap <= lcap && (uint32_t)most <= cap) return cap;
    return 0;
}

// The classification block of a pass with n large objects (SpanScratch
// h_cls, d_cls), one layout for the host's pinned copy and the device's:
// (most, rows, entries) as k_obj_maxact writes them (12 n bytes), then the
// walk groups' objects, pool offsets and list capacities, the chunked walk's
// table (prk_spans.hip PrObj, 8 words an object) and its objects by group,
// and the huge walk's (rows, entries) per object in walk-group order.
struct ClsView {
    int32_t *most, *rows, *ents;
    uint32_t *big;
    unsigned long long *off;
    uint32_t *cap, *pr, *grp, *meta;
};
struct ClsLayout {
    size_t n, big, off, cap, pr, grp, meta, end;
    explicit ClsLayout(uint32_t nbig = 0) : n(nbig) {
        big = 12 * n;
        off = (big + 4 * n + 7) & ~(size_t)7;
        cap = off + 8 * n;
        pr = cap + 4 * n;
        grp = pr + 32 * n;
        meta = grp + 4 * n;
        end = meta + 8 * n;
    }
    size_t alloc_bytes() const { return end + 64; }  // (never empty)
    // what the host uploads after the readback: [big, end)
    size_t upload_bytes() const { return end - big; }
    ClsView view(void *base) const {
        char *b = static_cast<char *>(base);
        int32_t *m = reinterpret_cast<int32_t *>(b);
        return ClsView{m,
                       m + n,
                       m + 2 * n,
                       reinterpret_cast<uint32_t *>(b + big),
                       reinterpret_cast<unsigned long long *>(b + off),
                       reinterpret_cast<uint32_t *>(b + cap),
                       reinterpret_cast<uint32_t *>(b + pr),
                       reinterpret_cast<uint32_t *>(b + grp),
                       reinterpret_cast<uint32_t *>(b + meta)};
    }
};

}  // namespace

struct prk_context : PassState {  // (the target, tile, cameras, lights, clear and debug flag: PassState)
    int device = 0;
    hipStream_t own_stream = nullptr;
    // prk_geometry_write: copies on copy_stream after read_ev (the end of the
    // last flush); the next flush's streams wait for in_ev
    hipStream_t copy_stream = nullptr;
    hipEvent_t in_ev = nullptr, read_ev = nullptr;
    bool in_wait = false, read_rec = false;
    // prk_geometry_transform's tables (scan, runs, matrices): staged in pinned
    // memory, copied on copy_stream ahead of the kernel; xf_ev: that copy is
    // done (the next call refills the staging)
    DevBuf d_xform;
    void *h_xform = nullptr;
    size_t h_xform_cap = 0;
    hipEvent_t xf_ev = nullptr, xf_end_ev = nullptr;  // (timed: prk_debug_transform_ms)
    bool xf_busy = false;
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
        DevBuf d_draws, d_texs, d_tri_draw, d_ranges, d_tri_n, d_tri_off, d_pair_tri, d_keys_a, d_vals_a, d_keys_b,
            d_bins, d_offs, d_temp, d_won, d_list, d_nwin, d_wtag, d_recs, d_trwon, d_wlist, d_seltemp, d_trec,
            d_ghist, d_tile_tot, d_chunk, d_info, d_runlist, d_run_n;
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
    hipEvent_t s_mark = nullptr;  // flush-stream point the bin stream waits for (prior target contents)
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
    // them (prk_kernels.hip PRK_SETUP_REC), so they are not optional
    bool setup_rec = true;
    bool winners_valid = false;
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
        std::vector<ObjRun> h_runs;
        std::vector<uint32_t> h_big_gl, h_k1src, h_lcnt;
        std::vector<PrepSeg> h_segs;     // a pass with handle draws: its batch edges' segments
        std::vector<ListSrc> h_lsrc;     // ... and the handles its runs take their list tables from
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

static PassState pass_state(const prk_context *c) { return *c; }
static void apply_pass_state(prk_context *c, const PassState &p) { static_cast<PassState &>(*c) = p; }

static int resolve_count(prk_context *c);
// Calls that read or replace the target, or change what a re-run of the
// pending pass would read, first resolve its count (PendingCount).
#define RESOLVE_COUNT(c)                             \
    do {                                             \
        const int _rc = resolve_count(c);            \
        if (_rc != PRK_OK) return _rc;               \
    } while (0)

#define PRK_TRY(expr)                              \
    do {                                           \
        hipError_t _e = (expr);                    \
        if (_e != hipSuccess) return status_of(_e); \
    } while (0)

// ---- one ROCm runtime per process (prk.h prk_create) ------
namespace {
struct MapScan {
    std::vector<std::string> hip, smi;  // distinct mapped files of each library
};
int scan_object(struct dl_phdr_info *info, size_t, void *data) {
    MapScan &m = *static_cast<MapScan *>(data);
    const char *path = info->dlpi_name;
    if (!path || !*path) return 0;
    const char *base = std::strrchr(path, '/');
    base = base ? base + 1 : path;
    std::vector<std::string> *v = nullptr;
    if (std::strncmp(base, "libamdhip64", 11) == 0) v = &m.hip;
    else if (std::strncmp(base, "librocm_smi64", 13) == 0) v = &m.smi;
    if (!v) return 0;
    char real[4096];
    const std::string key = realpath(path, real) ? std::string(real) : std::string(path);
    if (std::find(v->begin(), v->end(), key) == v->end()) v->push_back(key);
    return 0;
}
// Runs before the destructors of every library loaded earlier (exit handlers
// run last-registered first): ends the process with its own exit status
// before the duplicated librocm_smi64 destructors free one map twice.
void exit_guard(int status, void *) {
    std::fflush(nullptr);
    _exit(status);
}
std::atomic<bool> g_guarded{false};

// prk_selftest_sort / _scan: a device buffer of `bytes` payload bytes and
// kGuardBytes of kGuardByte after them, filled and read with copies only.
constexpr size_t kGuardBytes = 4096;
constexpr unsigned char kGuardByte = 0xA5;
struct GuardedBuf {
    char *p = nullptr;
    size_t bytes = 0;
    std::vector<unsigned char> host;  // what the buffer was last filled with, then what it holds
    ~GuardedBuf() {
        if (p) (void)hipFree(p);
    }
    // the pattern everywhere, then `src` (may be null) over the payload
    hipError_t fill(size_t payload, const void *src) {
        if (!p) {
            bytes = payload;
            const hipError_t e = hipMalloc(&p, bytes + kGuardBytes);
            if (e != hipSuccess) return e;
        }
        host.assign(bytes + kGuardBytes, kGuardByte);
        if (src && bytes) std::memcpy(host.data(), src, bytes);
        return hipMemcpy(p, host.data(), host.size(), hipMemcpyHostToDevice);
    }
    hipError_t read() { return hipMemcpy(host.data(), p, host.size(), hipMemcpyDeviceToHost); }
    bool guard_intact() const {
        for (size_t i = bytes; i < host.size(); ++i)
            if (host[i] != kGuardByte) return false;
        return true;
    }
    bool holds(const void *src) const { return bytes == 0 || std::memcmp(host.data(), src, bytes) == 0; }
};
}  // namespace

extern "C" {

int prk_runtime_check(void) {
    MapScan m;
    dl_iterate_phdr(scan_object, &m);
    if (m.hip.size() <= 1 && m.smi.size() <= 1) return PRK_OK;
    if (!g_guarded.exchange(true)) {
        std::fprintf(stderr,
                     "prk: %zu copies of libamdhip64 and %zu of librocm_smi64 are mapped in this process (e.g. "
                     "/opt/rocm's, loaded with libprk_hip.so, and torch's own): load torch (or the framework that "
                     "ships its own ROCm) BEFORE libprk_hip.so (INTEGRATION.md, 'One ROCm stack per process'); "
                     "the process will end at exit before their destructors run\n",
                     m.hip.size(), m.smi.size());
        // The guard ends the process before every exit handler registered
        // earlier (profiler flushes, LSan, earlier libraries' static
        // destructors): without it the duplicated librocm_smi64 destructors
        // abort the process there anyway (SIGABRT, the same handlers lost).
        // PRK_EXIT_GUARD=0 leaves the exit path alone (the host takes the abort).
        const char *g = std::getenv("PRK_EXIT_GUARD");
        if (!(g && g[0] == '0')) on_exit(exit_guard, nullptr);
    }
    return PRK_ERR_RUNTIME_MIX;
}

const char *prk_version(void) { return "prk 0.1 (gfx950)"; }

int prk_device_count(int *out) {
    if (!out) return PRK_ERR_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *out = n;
    return PRK_OK;
}

// Self-test of the shared-divisor quotients against the compiler's division
// (prk.h).  Runs on `device`, synchronously.
int prk_selftest_div_paths(int32_t device, uint32_t n, uint64_t seed, uint64_t *mismatches, uint32_t fast_waves[2]) {
    if (!mismatches || device < 0) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    unsigned long long *d = nullptr;
    PRK_TRY(hipMalloc(&d, 3 * sizeof(unsigned long long)));
    hipError_t e = hipMemset(d, 0, 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = prk_selftest_div_launch(n, seed, d, nullptr);
    unsigned long long h[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return status_of(e);
    *mismatches = h[0];
    if (fast_waves) {
        fast_waves[0] = (uint32_t)h[1];
        fast_waves[1] = (uint32_t)h[2];
    }
    return PRK_OK;
}
int prk_selftest_div(int32_t device, uint32_t n, uint64_t seed, uint64_t *mismatches) {
    return prk_selftest_div_paths(device, n, seed, mismatches, nullptr);
}

// One device primitive on the caller's words (prk.h).  Runs on `device`,
// synchronously; the kernel reads and writes whole 4 x n buffers, so an input
// the op does not read is zeros.
int prk_selftest_ops(int32_t device, int32_t op, uint32_t n, const uint32_t *a, const uint32_t *b,
                     const uint32_t *c, const uint32_t *d, uint32_t *out0, uint32_t *out1, uint32_t *out2,
                     uint32_t *fast) {
    static const uint8_t kInputs[PRK_OP_COUNT] = {2, 2, 4, 4, 4, 4, 4, 2, 1, 1, 3, 3, 1,
                                                  1, 1, 1, 2, 2, 1, 2, 1, 1, 2, 1, 3, 3};
    if (device < 0 || op < 0 || op >= PRK_OP_COUNT || n > (1u << 24) || !out0) return PRK_ERR_ARG;
    const uint32_t *in[4] = {a, b, c, d};
    for (int k = 0; k < kInputs[op]; ++k)
        if (!in[k]) return PRK_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    if (n == 0) return PRK_OK;
    PRK_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    uint32_t *din = nullptr, *dout = nullptr;
    PRK_TRY(hipMalloc(&din, 4 * bytes));
    hipError_t e = hipMalloc(&dout, 4 * bytes);
    if (e == hipSuccess) e = hipMemset(din, 0, 4 * bytes);
    for (int k = 0; k < kInputs[op] && e == hipSuccess; ++k)
        e = hipMemcpy(din + (size_t)k * n, in[k], bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = prk_selftest_ops_launch(op, n, din, dout, nullptr);
    uint32_t *outs[4] = {out0, out1, out2, fast};
    for (int k = 0; k < 4 && e == hipSuccess; ++k)
        if (outs[k]) e = hipMemcpy(outs[k], dout + (size_t)k * n, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return status_of(e);
}

// The radix sort on the caller's pairs (prk.h): guarded buffers, the temp
// buffer at exactly the queried size and left as it is between the repeats.
int prk_selftest_sort(int32_t device, uint32_t n, uint32_t end_bit, const uint64_t *keys, const uint32_t *vals,
                      uint32_t repeats, uint64_t *keys_out, uint32_t *vals_out, uint32_t *damage) {
    if (device < 0 || !keys || !vals || !keys_out || !vals_out || !damage || repeats == 0) return PRK_ERR_ARG;
    size_t tb = 0;
    PRK_TRY(prk_obj_sort(nullptr, nullptr, nullptr, nullptr, n, end_bit, nullptr, &tb, nullptr));  // (host only)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    const size_t kb = (size_t)n * 8, vb = (size_t)n * 4;
    GuardedBuf kin, vin, kout, vout, temp;
    PRK_TRY(kin.fill(kb, keys));
    PRK_TRY(vin.fill(vb, vals));
    PRK_TRY(temp.fill(tb, nullptr));
    for (uint32_t r = 0; r < repeats; ++r) {
        PRK_TRY(kout.fill(kb, nullptr));
        PRK_TRY(vout.fill(vb, nullptr));
        PRK_TRY(prk_obj_sort(kin.p, (uint32_t *)vin.p, kout.p, (uint32_t *)vout.p, n, end_bit, temp.p, &tb, nullptr));
        PRK_TRY(hipDeviceSynchronize());
    }
    PRK_TRY(kin.read());
    PRK_TRY(vin.read());
    PRK_TRY(kout.read());
    PRK_TRY(vout.read());
    PRK_TRY(temp.read());
    *damage = (kin.holds(keys) && vin.holds(vals) && kin.guard_intact() && vin.guard_intact() ? 0u : PRK_DAMAGE_INPUT) |
              (kout.guard_intact() && vout.guard_intact() ? 0u : PRK_DAMAGE_OUTPUT_GUARD) |
              (temp.guard_intact() ? 0u : PRK_DAMAGE_TEMP_GUARD);
    if (n) {
        std::memcpy(keys_out, kout.host.data(), kb);
        std::memcpy(vals_out, vout.host.data(), vb);
    }
    return PRK_OK;
}

// An exclusive scan on the caller's words (prk.h), in and out distinct.
int prk_selftest_scan(int32_t device, int32_t width, uint32_t n, const void *in, void *out, uint32_t *damage) {
    if (device < 0 || (width != 32 && width != 64) || !in || !out || !damage) return PRK_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * (size_t)(width / 8);
    size_t tb = 0;
    GuardedBuf din, dout, temp;
    PRK_TRY(din.fill(bytes, in));
    PRK_TRY(dout.fill(bytes, nullptr));
    if (width == 32) {
        PRK_TRY(prk_scan_u32(nullptr, nullptr, n, nullptr, &tb, nullptr));
        PRK_TRY(temp.fill(tb, nullptr));
        PRK_TRY(prk_scan_u32((const uint32_t *)din.p, (uint32_t *)dout.p, n, temp.p, &tb, nullptr));
    } else {
        PRK_TRY(prk_scan_u64(nullptr, nullptr, n, nullptr, &tb, nullptr));
        PRK_TRY(temp.fill(tb, nullptr));
        PRK_TRY(prk_scan_u64((const unsigned long long *)din.p, (unsigned long long *)dout.p, n, temp.p, &tb,
                             nullptr));
    }
    PRK_TRY(hipDeviceSynchronize());
    PRK_TRY(din.read());
    PRK_TRY(dout.read());
    PRK_TRY(temp.read());
    *damage = (din.holds(in) && din.guard_intact() ? 0u : PRK_DAMAGE_INPUT) |
              (dout.guard_intact() ? 0u : PRK_DAMAGE_OUTPUT_GUARD) | (temp.guard_intact() ? 0u : PRK_DAMAGE_TEMP_GUARD);
    if (bytes) std::memcpy(out, dout.host.data(), bytes);
    return PRK_OK;
}

int prk_create(int device, prk_context **out) {
    if (!out) return PRK_ERR_ARG;
    *out = nullptr;
    {
        const int rc = prk_runtime_check();
        if (rc != PRK_OK) return rc;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PRK_ERR_DEVICE;
    if (device < 0 || device >= n) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    prk_context *c = new (std::nothrow) prk_context();
    if (!c) return PRK_ERR_NOMEM;
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->bin_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->vis_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->s_mark, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->in_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->read_ev, hipEventDisableTiming);
    for (int i = 0; i < prk_context::kSets && e == hipSuccess; ++i) {
        e = hipEventCreateWithFlags(&c->bset[i].free_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bset[i].binned_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bset[i].counted_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bset[i].listed_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipHostMalloc((void **)&c->bset[i].h_info, 2 * sizeof(uint32_t), hipHostMallocDefault);
    }
    for (int i = 0; i < prk_context::kRing && e == hipSuccess; ++i)
        for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipEventCreate(&c->ev[i][k]);
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_total, sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) {
        prk_destroy(c);
        return status_of(e);
    }
    *out = c;
    return PRK_OK;
}

int prk_destroy(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    (void)prk_runtime_check();  // (a runtime loaded since prk_create: guard the exit)
    // Destroy never queues GPU work: a frame whose bin count was never read
    // (PendingCount) is dropped, not re-run — its target may already belong
    // to someone else (a torch tensor freed at interpreter exit, a peer
    // context), and a re-run there is exactly what a caller tearing down does
    // not expect.  Only waits and frees follow.
    c->pcount.active = false;
    c->pcount.draws.clear();
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    (void)hipDeviceSynchronize();
    for (auto &g : c->geoms)
        if (g.owned) {
            (void)hipFree((void *)g.V);
            (void)hipFree((void *)g.C);
            (void)hipFree((void *)g.N);
            (void)hipFree((void *)g.UV);
        }
    for (auto &t : c->texs) (void)hipFree(t.mem);
    for (auto &r : c->recs) {
        (void)hipFree(r.rec);
        (void)hipFree(r.tab);
    }
    for (auto &b : c->sbatches) (void)hipFree(b.sp);
    for (auto &l : c->layers)
        if (l.live && !l.wrapped) {
            (void)hipFree(l.color);
            (void)hipFree(l.z);
        }
    if (c->owns_target) {
        (void)hipFree(c->color);
        (void)hipFree(c->zbuf);
    }
    for (auto &B : c->bset) {
        DevBuf *bb[] = {&B.d_draws, &B.d_texs, &B.d_tri_draw, &B.d_ranges, &B.d_tri_n, &B.d_tri_off, &B.d_pair_tri,
                        &B.d_keys_a, &B.d_vals_a, &B.d_keys_b, &B.d_bins, &B.d_offs, &B.d_temp, &B.d_won,
                        &B.d_list, &B.d_nwin, &B.d_wtag, &B.d_recs, &B.d_trwon, &B.d_wlist, &B.d_seltemp,
                        &B.d_trec, &B.d_ghist, &B.d_tile_tot, &B.d_chunk, &B.d_info, &B.d_runlist, &B.d_run_n};
        for (DevBuf *b : bb) b->release();
        if (B.free_ev) (void)hipEventDestroy(B.free_ev);
        if (B.binned_ev) (void)hipEventDestroy(B.binned_ev);
        if (B.counted_ev) (void)hipEventDestroy(B.counted_ev);
        if (B.listed_ev) (void)hipEventDestroy(B.listed_ev);
        if (B.h_info) (void)hipHostFree(B.h_info);
    }
    DevBuf *bufs[] = {&c->d_winners, &c->d_anomaly, &c->d_prof, &c->d_negz, &c->d_xform};
    for (DevBuf *b : bufs) b->release();
    if (c->h_xform) (void)hipHostFree(c->h_xform);
    if (c->xf_ev) (void)hipEventDestroy(c->xf_ev);
    if (c->xf_end_ev) (void)hipEventDestroy(c->xf_end_ev);
    {
        auto &S = c->spans;
        DevBuf *sb[] = {&S.d_stage, &S.d_edges, &S.d_ord, &S.d_temp, &S.d_recs, &S.d_pos, &S.d_span_tri, &S.d_scnt,
                        &S.d_soff, &S.d_vals_b, &S.d_offs, &S.d_nwin,
                        &S.d_wtag, &S.d_srecs, &S.d_work, &S.d_ekeys, &S.d_ekeys2, &S.d_evals, &S.d_ecnt,
                        &S.d_escan, &S.d_rcnt, &S.d_rscan, &S.d_bound, &S.d_oslot, &S.d_pool, &S.d_err,
                        &S.d_raw, &S.d_most, &S.d_cls, &S.d_prrow, &S.d_prcnt, &S.d_preoff, &S.d_prfge,
                        &S.d_prccur, &S.d_prkey, &S.d_prest, &S.d_prsst, &S.d_preend, &S.d_preendm,
                        &S.d_prmatch, &S.d_prsidx, &S.d_prsm, &S.d_prstat, &S.d_segcnt, &S.d_segoff,
                        &S.d_segs, &S.d_wy, &S.d_mhuge, &S.d_objtab, &S.d_k0tab, &S.d_lscan, &S.d_lobj, &S.d_lrows,
                        &S.d_ltab, &S.d_rectab, &S.d_reccnt,
                        &S.d_recout, &S.d_spanout, &S.d_rowslot, &S.d_rowcnt, &S.d_rowscan, &S.d_rowout,
                        &S.d_lstat, &S.d_dr_rows, &S.d_dr_pairs, &S.d_dr_cnt, &S.d_dr_scan, &S.d_dr_temp, &S.d_dr_out};
        for (DevBuf *b : sb) b->release();
        if (S.h_rb) (void)hipHostFree(S.h_rb);
        if (S.stage_ev) {
            if (S.stage_busy) (void)hipEventSynchronize(S.stage_ev);
            (void)hipEventDestroy(S.stage_ev);
        }
        if (S.h_stage) (void)hipHostFree(S.h_stage);
        if (S.h_cls) (void)hipHostFree(S.h_cls);
    }
    if (c->s_mark) (void)hipEventDestroy(c->s_mark);
    if (c->in_ev) (void)hipEventDestroy(c->in_ev);
    if (c->read_ev) (void)hipEventDestroy(c->read_ev);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->h_total) (void)hipHostFree(c->h_total);
    for (auto &slot : c->ev)
        for (auto &e : slot)
            if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->bin_stream) (void)hipStreamDestroy(c->bin_stream);
    if (c->vis_stream) (void)hipStreamDestroy(c->vis_stream);
    delete c;
    return PRK_OK;
}

static void drop_target(prk_context *c) {
    c->z_early = false;
    if (c->owns_target) {
        (void)hipFree(c->color);
        (void)hipFree(c->zbuf);
    }
    c->color = nullptr;
    c->zbuf = nullptr;
    c->owns_target = false;
    c->W = c->H = c->row0 = c->row1 = 0;
}

int prk_target_bind(prk_context *c, void *color, int32_t pitch_bytes, float *zbuf, int32_t width,
                    int32_t height, int32_t row0, int32_t row1) {
    if (!c || !color || !zbuf || width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 >= row1 ||
        pitch_bytes < width * 4 || (pitch_bytes & 3))
        return PRK_ERR_ARG;
    // the pending frame's count first, whoever owns its target: an overflowed
    // frame is re-run into the target it was queued with before a caller
    // hands that memory to anything else (a gather, the next frame)
    RESOLVE_COUNT(c);
    drop_target(c);
    c->color = color;
    c->pitch = pitch_bytes;
    c->zbuf = zbuf;
    c->W = width;
    c->H = height;
    c->row0 = row0;
    c->row1 = row1;
    c->winners_valid = false;
    return PRK_OK;
}

int prk_target_alloc(prk_context *c, int32_t width, int32_t height, int32_t row0, int32_t row1,
                     void **color_out, float **zbuf_out) {
    if (!c || width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 >= row1) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    drop_target(c);
    size_t px = (size_t)width * (row1 - row0);
    void *col = nullptr;
    float *z = nullptr;
    hipError_t e = hipMalloc(&col, px * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&z, px * 4);
    if (e != hipSuccess) {
        (void)hipFree(col);
        (void)hipFree(z);
        return status_of(e);
    }
    c->color = col;
    c->zbuf = z;
    c->pitch = width * 4;
    c->W = width;
    c->H = height;
    c->row0 = row0;
    c->row1 = row1;
    c->owns_target = true;
    c->winners_valid = false;
    if (color_out) *color_out = col;
    if (zbuf_out) *zbuf_out = z;
    return PRK_OK;
}

__global__ void k_fill_target(uint32_t *color, int32_t pitch, float *z, int32_t W, int32_t rows,
                              uint32_t cval, float zval) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = (size_t)W * rows;
    if (i >= n) return;
    size_t r = i / W, x = i % W;
    reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(color) + r * pitch)[x] = cval;
    z[i] = zval;
}

int prk_target_clear(prk_context *c, uint32_t color, float z) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    c->z_early = false;  // (z written outside a frame)
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    // after a prk_target_upload_async still in flight (it would land on top)
    if (c->in_wait) PRK_TRY(hipStreamWaitEvent(c->own_stream, c->in_ev, 0));
    size_t n = (size_t)c->W * (c->row1 - c->row0);
    hipLaunchKernelGGL(k_fill_target, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->own_stream,
                       (uint32_t *)c->color, c->pitch, c->zbuf, c->W, c->row1 - c->row0, color, z);
    PRK_TRY(hipGetLastError());
    return PRK_OK;
}

int prk_target_clear_on_flush(prk_context *c, uint32_t color, float z) {
    if (!c) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    c->clear_pending = true;
    c->clear_color = color;
    c->clear_z = z;
    return PRK_OK;
}

int prk_target_download(prk_context *c, uint32_t *color_host, int32_t host_pitch, float *z_host) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    int rows = c->row1 - c->row0;
    const size_t zbytes = (size_t)c->W * rows * 4;
    // A span-record frame's z is final after its k_vis: it goes down while
    // the frame shades (the copy engine holds the link while k_walk / k_pix
    // run), the colour after the frame.
    const bool early = z_host && c->z_early && c->z_slot >= 0 && c->d_negz.p;
    if (early) {
        PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->ev[c->z_slot][3], 0));
        PRK_TRY(hipMemcpyAsync(z_host, c->zbuf, zbytes, hipMemcpyDeviceToHost, c->copy_stream));
    }
    PRK_TRY(hipStreamSynchronize(c->own_stream));
    PRK_TRY(hipDeviceSynchronize());
    if (color_host)
        PRK_TRY(hipMemcpy2D(color_host, host_pitch, c->color, c->pitch, (size_t)c->W * 4, rows,
                            hipMemcpyDeviceToHost));
    if (early) {  // a -0.0 z written by k_pix after k_vis's +0.0: take z again
        uint32_t negz = 0;
        PRK_TRY(hipMemcpy(&negz, c->d_negz.p, 4, hipMemcpyDeviceToHost));
        if (negz) {
            PRK_TRY(hipMemcpy(z_host, c->zbuf, zbytes, hipMemcpyDeviceToHost));
            PRK_TRY(hipMemset(c->d_negz.p, 0, 4));
        }
    } else if (z_host) {
        PRK_TRY(hipMemcpy(z_host, c->zbuf, zbytes, hipMemcpyDeviceToHost));
    }
    return PRK_OK;
}

int prk_target_upload(prk_context *c, const uint32_t *color_host, int32_t host_pitch, const float *z_host) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    c->z_early = false;  // (z written outside a frame)
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->own_stream));
    if (c->in_wait) PRK_TRY(hipEventSynchronize(c->in_ev));  // an earlier asynchronous upload lands first
    int rows = c->row1 - c->row0;
    if (color_host)
        PRK_TRY(hipMemcpy2D(c->color, c->pitch, color_host, host_pitch, (size_t)c->W * 4, rows,
                            hipMemcpyHostToDevice));
    if (z_host) PRK_TRY(hipMemcpy(c->zbuf, z_host, (size_t)c->W * rows * 4, hipMemcpyHostToDevice));
    return PRK_OK;
}

int prk_target_upload_async(prk_context *c, const uint32_t *color_host, int32_t host_pitch, const float *z_host) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    c->z_early = false;  // (z written outside a frame)
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    // after the frames already flushed (they read and write the target) and
    // whatever the context's stream holds (a clear, an earlier upload)
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipEventRecord(c->s_mark, c->own_stream));
    PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->s_mark, 0));
    const int rows = c->row1 - c->row0;
    if (color_host)
        PRK_TRY(hipMemcpy2DAsync(c->color, c->pitch, color_host, host_pitch, (size_t)c->W * 4, rows,
                                 hipMemcpyHostToDevice, c->copy_stream));
    if (z_host)
        PRK_TRY(hipMemcpyAsync(c->zbuf, z_host, (size_t)c->W * rows * 4, hipMemcpyHostToDevice, c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
    return PRK_OK;
}

int prk_set_camera(prk_context *c, const prk_transform *t, const prk_light_data *l) {
    if (!c || !t || !l || l->LightCount > PRK_MAX_LIGHTS) return PRK_ERR_ARG;
    c->transform = *t;
    c->lights = *l;
    c->shade_transform = *t;
    c->shade_lights = *l;
    c->have_camera = true;
    return PRK_OK;
}

int prk_set_shade_camera(prk_context *c, const prk_transform *t, const prk_light_data *l) {
    if (!c || !t || !l || l->LightCount > PRK_MAX_LIGHTS) return PRK_ERR_ARG;
    if (!c->have_camera) return PRK_ERR_ARG;  // the setup camera first (prk_set_camera)
    c->shade_transform = *t;
    c->shade_lights = *l;
    return PRK_OK;
}

static bool bitmap_ok(const prk_bitmap *b) {
    return b && b->Memory && b->Width > 0 && b->Height > 0 && b->Pitch >= 4 * b->Width && !(b->Pitch & 3);
}

// Copy the caller's Height rows (Pitch bytes each) into a texture holding
// Height + 1 rows, the last one the zeroed guard row that the u == 1 / v == 1
// over-read lands on: the caller's loaded_bitmap is read
// exactly as the reference reads it (Memory, Width, Height, Pitch,
// projekt.cpp:1506, 1881-1935) and never past its last row.
static hipError_t texture_fill(const Texture &t, const prk_bitmap *b) {
    hipError_t e = hipMemcpy(t.mem, b->Memory, (size_t)b->Pitch * b->Height, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t.mem + (size_t)b->Pitch * b->Height, 0, (size_t)b->Pitch);
    return e;
}

int prk_texture_create(prk_context *c, const prk_bitmap *b, int32_t *handle_out) {
    if (!c || !bitmap_ok(b) || !handle_out) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Texture t;
    t.w = b->Width;
    t.h = b->Height;
    t.pitch = b->Pitch;
    PRK_TRY(hipMalloc((void **)&t.mem, (size_t)b->Pitch * (b->Height + 1)));
    hipError_t e = texture_fill(t, b);
    if (e != hipSuccess) {
        (void)hipFree(t.mem);
        return status_of(e);
    }
    *handle_out = (int32_t)c->texs.size();
    c->texs.push_back(t);
    return PRK_OK;
}

int prk_texture_update(prk_context *c, int32_t handle, const prk_bitmap *b) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size() || !bitmap_ok(b)) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    Texture &t = c->texs[handle];
    PRK_TRY(hipDeviceSynchronize());  // frames in flight may still sample it
    if (t.w != b->Width || t.h != b->Height || t.pitch != b->Pitch) {
        uint8_t *m = nullptr;
        PRK_TRY(hipMalloc((void **)&m, (size_t)b->Pitch * (b->Height + 1)));
        (void)hipFree(t.mem);
        t.mem = m;
        t.w = b->Width;
        t.h = b->Height;
        t.pitch = b->Pitch;
    }
    PRK_TRY(texture_fill(t, b));
    return PRK_OK;
}

int prk_texture_alloc(prk_context *c, int32_t width, int32_t height, int32_t *handle_out) {
    if (!c || width <= 0 || height <= 0 || width > INT32_MAX / 4 || !handle_out) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Texture t;
    t.w = width;
    t.h = height;
    t.pitch = 4 * width;
    const size_t bytes = (size_t)t.pitch * ((size_t)height + 1);  // (the guard row with them)
    PRK_TRY(hipMalloc((void **)&t.mem, bytes));
    hipError_t e = hipMemset(t.mem, 0, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the context's streams do not wait for that stream)
    if (e != hipSuccess) {
        (void)hipFree(t.mem);
        return status_of(e);
    }
    *handle_out = (int32_t)c->texs.size();
    c->texs.push_back(t);
    return PRK_OK;
}

// A rectangle of the target's colour into a rectangle of a texture (prk.h;
// kernel: prk_tex.hip).  Ordered as prk_target_upload_async orders its copies:
// on copy_stream after read_ev (the frames already flushed wrote the target
// and sampled the texture) and after what own_stream holds (clears, uploads);
// the next flush waits for in_ev.
int prk_texture_from_target(prk_context *c, int32_t texture, int32_t x0, int32_t y0, int32_t width, int32_t height,
                            int32_t factor, int32_t dst_x, int32_t dst_y) {
    if (!c || texture < 0 || (size_t)texture >= c->texs.size()) return PRK_ERR_ARG;
    if (factor != 1 && factor != 2 && factor != 4) return PRK_ERR_ARG;
    if (width <= 0 || height <= 0 || width % factor || height % factor) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    const Texture &t = c->texs[texture];
    const int32_t dw = width / factor, dh = height / factor;
    if (x0 < 0 || (int64_t)x0 + width > c->W || y0 < c->row0 || (int64_t)y0 + height > c->row1) return PRK_ERR_ARG;
    if (dst_x < 0 || (int64_t)dst_x + dw > t.w || dst_y < 0 || (int64_t)dst_y + dh > t.h) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    const uint8_t *src = static_cast<const uint8_t *>(c->color) + (size_t)(y0 - c->row0) * c->pitch + (size_t)x0 * 4;
    uint8_t *dst = t.mem + (size_t)dst_y * t.pitch + (size_t)dst_x * 4;
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipEventRecord(c->s_mark, c->own_stream));
    PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->s_mark, 0));
    PRK_TRY(prk_tex_from_target_launch(src, (size_t)c->pitch, dst, (size_t)t.pitch, (uint32_t)dw, (uint32_t)dh, factor,
                                       c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
    return PRK_OK;
}

int prk_texture_download(prk_context *c, int32_t handle, void *memory, int32_t pitch_bytes) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size() || !memory) return PRK_ERR_ARG;
    const Texture &t = c->texs[handle];
    if (pitch_bytes < 4 * t.w || (pitch_bytes & 3)) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->copy_stream));  // every queued prk_texture_from_target runs there
    PRK_TRY(hipMemcpy2D(memory, pitch_bytes, t.mem, t.pitch, (size_t)t.w * 4, t.h, hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_texture_info(prk_context *c, int32_t handle, int32_t *width, int32_t *height, int32_t *pitch_bytes) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size()) return PRK_ERR_ARG;
    const Texture &t = c->texs[handle];
    if (width) *width = t.w;
    if (height) *height = t.h;
    if (pitch_bytes) *pitch_bytes = t.pitch;
    return PRK_OK;
}

// ---- target layers (prk.h; kernel: prk_layer.hip) -------------------------------
static Layer *layer_of(prk_context *c, int32_t handle) {
    if (!c || handle < 0 || (size_t)handle >= c->layers.size() || !c->layers[handle].live) return nullptr;
    return &c->layers[handle];
}

int prk_layer_alloc(prk_context *c, int32_t width, int32_t height, int32_t *handle_out) {
    if (!c || width <= 0 || height <= 0 || width > INT32_MAX / 4 || !handle_out) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Layer l;
    l.w = width;
    l.h = height;
    l.pitch = 4 * width;
    l.live = true;
    const size_t px = (size_t)width * (size_t)height;
    hipError_t e = hipMalloc((void **)&l.color, px * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&l.z, px * 4);
    if (e == hipSuccess) e = hipMemset(l.color, 0, px * 4);
    if (e == hipSuccess) e = hipMemsetD32((hipDeviceptr_t)l.z, (int)0xFF7FFFFFu, px);  // -FLT_MAX
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the context's streams do not wait for that stream)
    if (e != hipSuccess) {
        (void)hipFree(l.color);
        (void)hipFree(l.z);
        return status_of(e);
    }
    *handle_out = (int32_t)c->layers.size();
    c->layers.push_back(l);
    return PRK_OK;
}

int prk_layer_wrap_device(prk_context *c, const void *color, int32_t pitch_bytes, const float *zbuf, int32_t width,
                          int32_t height, int32_t *handle_out) {
    if (!c || !color || !zbuf || width <= 0 || height <= 0 || width > INT32_MAX / 4 || !handle_out) return PRK_ERR_ARG;
    if (pitch_bytes < 4 * width || (pitch_bytes & 3)) return PRK_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(color) & 3) || (reinterpret_cast<uintptr_t>(zbuf) & 3)) return PRK_ERR_ARG;
    Layer l;
    l.color = static_cast<uint8_t *>(const_cast<void *>(color));  // (never written: no call takes it as destination)
    l.z = const_cast<float *>(zbuf);
    l.w = width;
    l.h = height;
    l.pitch = pitch_bytes;
    l.wrapped = l.live = true;
    *handle_out = (int32_t)c->layers.size();
    c->layers.push_back(l);
    return PRK_OK;
}

// Do a layer's rectangle at (lx, ly) and the target's at frame pixel (x0, y0), both width x height, lie inside?
static bool layer_rects_ok(const prk_context *c, const Layer &l, int32_t lx, int32_t ly, int32_t x0, int32_t y0,
                           int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return false;
    if (x0 < 0 || (int64_t)x0 + width > c->W || y0 < c->row0 || (int64_t)y0 + height > c->row1) return false;
    return lx >= 0 && (int64_t)lx + width <= l.w && ly >= 0 && (int64_t)ly + height <= l.h;
}

// One pass between a layer's rectangle at (lx, ly) and the target's at frame
// pixel (x0, y0): rule < 0 saves target to layer, else the layer goes to the
// target under rule.  Ordered as prk_texture_from_target: on copy_stream
// after read_ev (the frames already flushed) and after what own_stream holds
// (clears, uploads); the next flush, clear, upload or layer call waits for
// in_ev.
static int layer_pass(prk_context *c, const Layer &l, int32_t lx, int32_t ly, int32_t x0, int32_t y0, int32_t width,
                      int32_t height, int32_t rule) {
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    const size_t toff = (size_t)(y0 - c->row0) * c->W + (size_t)x0, loff = (size_t)ly * l.w + (size_t)lx;
    uint8_t *tc = static_cast<uint8_t *>(c->color) + (size_t)(y0 - c->row0) * c->pitch + (size_t)x0 * 4;
    uint8_t *lc = l.color + (size_t)ly * l.pitch + (size_t)lx * 4;
    float *tz = c->zbuf + toff, *lz = l.z + loff;
    const size_t tzp = (size_t)c->W * 4, lzp = (size_t)l.w * 4;
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipEventRecord(c->s_mark, c->own_stream));
    PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->s_mark, 0));
    if (rule < 0)
        PRK_TRY(prk_layer_launch(tc, (size_t)c->pitch, tz, tzp, lc, (size_t)l.pitch, lz, lzp, (uint32_t)width,
                                 (uint32_t)height, PRK_MERGE_COPY, c->copy_stream));
    else
        PRK_TRY(prk_layer_launch(lc, (size_t)l.pitch, lz, lzp, tc, (size_t)c->pitch, tz, tzp, (uint32_t)width,
                                 (uint32_t)height, rule, c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
    return PRK_OK;
}

int prk_layer_from_target(prk_context *c, int32_t layer, int32_t x0, int32_t y0, int32_t width, int32_t height,
                          int32_t dst_x, int32_t dst_y) {
    const Layer *l = layer_of(c, layer);
    if (!l || l->wrapped) return PRK_ERR_ARG;
    if (width <= 0 || height <= 0) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (!layer_rects_ok(c, *l, dst_x, dst_y, x0, y0, width, height)) return PRK_ERR_ARG;
    return layer_pass(c, *l, dst_x, dst_y, x0, y0, width, height, -1);
}

int prk_target_from_layer(prk_context *c, int32_t layer, int32_t src_x, int32_t src_y, int32_t width, int32_t height,
                          int32_t x0, int32_t y0, int32_t rule) {
    const Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    if (rule != PRK_MERGE_COPY && rule != PRK_MERGE_GREATER && rule != PRK_MERGE_GREATER_EQUAL) return PRK_ERR_ARG;
    if (width <= 0 || height <= 0) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (!layer_rects_ok(c, *l, src_x, src_y, x0, y0, width, height)) return PRK_ERR_ARG;
    c->z_early = false;  // (z written outside a frame)
    return layer_pass(c, *l, src_x, src_y, x0, y0, width, height, rule);
}

int prk_layer_download(prk_context *c, int32_t layer, uint32_t *color_host, int32_t host_pitch, float *z_host) {
    const Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    if (color_host && (host_pitch < 4 * l->w || (host_pitch & 3))) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->copy_stream));  // every queued layer call runs there
    if (color_host)
        PRK_TRY(hipMemcpy2D(color_host, host_pitch, l->color, l->pitch, (size_t)l->w * 4, l->h, hipMemcpyDeviceToHost));
    if (z_host) PRK_TRY(hipMemcpy(z_host, l->z, (size_t)l->w * l->h * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_layer_info(prk_context *c, int32_t layer, int32_t *width, int32_t *height, int32_t *pitch_bytes,
                   int32_t *wrapped) {
    const Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    if (width) *width = l->w;
    if (height) *height = l->h;
    if (pitch_bytes) *pitch_bytes = l->pitch;
    if (wrapped) *wrapped = l->wrapped ? 1 : 0;
    return PRK_OK;
}

int prk_layer_destroy(prk_context *c, int32_t layer) {
    Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // frames in flight and queued layer calls first
    if (!l->wrapped) {
        (void)hipFree(l->color);
        (void)hipFree(l->z);
    }
    *l = Layer();  // (the slot stays, dead)
    return PRK_OK;
}

// Allocations of 2 MB and more: heap memory on transparent huge pages,
// page-locked with hipHostRegister, instead of hipHostMalloc's 4-KB pinned
// pages -- the drop-in's staging arena takes ~150 MB of per-call vertex
// snapshots a frame, which the 2-MB pages make cheaper for the CPU (TLB).
// PRK_HOST_ALLOC_THP=0: hipHostMalloc for every size.
static std::mutex g_thp_mu;
static std::map<void *, size_t> g_thp;  // (any context may free)
static bool host_alloc_thp() {
    static const bool on = [] {
        const char *e = std::getenv("PRK_HOST_ALLOC_THP");
        return !(e && e[0] == '0');
    }();
    return on;
}

int prk_host_alloc(prk_context *c, size_t bytes, void **out) {
    if (!c || !out) return PRK_ERR_ARG;
    *out = nullptr;
    PRK_TRY(hipSetDevice(c->device));
    constexpr size_t kHuge = (size_t)2 << 20;
    if (bytes >= kHuge && host_alloc_thp()) {
        const size_t sz = (bytes + kHuge - 1) & ~(kHuge - 1);
        void *p = std::aligned_alloc(kHuge, sz);
        if (!p) return PRK_ERR_NOMEM;
        (void)madvise(p, sz, MADV_HUGEPAGE);  // (best effort)
        memset(p, 0, sz);                      // (faulted in on huge pages before the pinning)
        const hipError_t e = hipHostRegister(p, sz, hipHostRegisterPortable);
        if (e != hipSuccess) {
            std::free(p);
            return status_of(e);
        }
        std::lock_guard<std::mutex> g(g_thp_mu);
        g_thp[p] = sz;
        *out = p;
        return PRK_OK;
    }
    PRK_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return PRK_OK;
}

int prk_host_free(prk_context *c, void *p) {
    if (!c) return PRK_ERR_ARG;
    if (!p) return PRK_OK;
    {
        std::lock_guard<std::mutex> g(g_thp_mu);
        auto it = g_thp.find(p);
        if (it != g_thp.end()) {
            g_thp.erase(it);
            const hipError_t e = hipHostUnregister(p);
            std::free(p);
            return e == hipSuccess ? PRK_OK : status_of(e);
        }
    }
    PRK_TRY(hipHostFree(p));
    return PRK_OK;
}

int prk_host_register(prk_context *c, void *p, size_t bytes) {
    if (!c || !p || !bytes) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return PRK_OK;
}

int prk_host_unregister(prk_context *c, void *p) {
    if (!c || !p) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipHostUnregister(p));
    return PRK_OK;
}

int prk_texture_set_filter(prk_context *c, int32_t handle, int32_t filter) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size()) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (filter != PRK_FILTER_NEAREST && filter != PRK_FILTER_BILINEAR) return PRK_ERR_ARG;
    c->texs[handle].filter = filter;
    return PRK_OK;
}

static int upload_array(const float *src, size_t n, const float **dst) {
    *dst = nullptr;
    if (!src) return PRK_OK;
    float *d = nullptr;
    PRK_TRY(hipMalloc((void **)&d, n * sizeof(float)));
    hipError_t e = hipMemcpy(d, src, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return status_of(e);
    }
    *dst = d;
    return PRK_OK;
}

int prk_geometry_create(prk_context *c, const float *v, const float *col, const float *n, const float *uv,
                        uint32_t vertex_count, int32_t *handle_out) {
    if (!c || !v || !handle_out || vertex_count % 3) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Geometry g;
    g.vertex_count = vertex_count;
    for (int k = 0; k < 4; ++k) g.cap[k] = vertex_count;
    g.owned = true;
    int rc = upload_array(v, (size_t)vertex_count * 3, &g.V);
    if (rc == PRK_OK) rc = upload_array(col, (size_t)vertex_count * 4, &g.C);
    if (rc == PRK_OK) rc = upload_array(n, (size_t)vertex_count * 3, &g.N);
    if (rc == PRK_OK) rc = upload_array(uv, (size_t)vertex_count * 2, &g.UV);
    if (rc != PRK_OK) {
        (void)hipFree((void *)g.V);
        (void)hipFree((void *)g.C);
        (void)hipFree((void *)g.N);
        (void)hipFree((void *)g.UV);
        return rc;
    }
    *handle_out = (int32_t)c->geoms.size();
    c->geoms.push_back(g);
    return PRK_OK;
}

// Replace a library-owned geometry's contents (the reference re-reads
// VertexData at every FillEdgeTable, projekt.cpp:3898-3925).  Buffers are kept
// when large enough; frames in flight finish first.  Draws recorded before
// the update read the new contents.
int prk_geometry_update(prk_context *c, int32_t handle, const float *v, const float *col, const float *n,
                        const float *uv, uint32_t vertex_count) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size() || !v || vertex_count % 3) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    Geometry &g = c->geoms[handle];
    if (!g.owned) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    const float *src[4] = {v, col, n, uv};
    const float **dst[4] = {&g.V, &g.C, &g.N, &g.UV};
    const size_t comp[4] = {3, 4, 3, 2};
    for (int k = 0; k < 4; ++k) {  // an array passed as null keeps its previous contents
        const size_t bytes = (size_t)vertex_count * comp[k] * sizeof(float);
        if (!src[k]) {
            // ... and grows with the vertex count: its first cap[k] vertices
            // kept, the new ones zero, so no draw reads past its allocation.
            if (*dst[k] && vertex_count > g.cap[k]) {
                const size_t old = (size_t)g.cap[k] * comp[k] * sizeof(float);
                float *d = nullptr;
                PRK_TRY(hipMalloc((void **)&d, bytes));
                hipError_t e = hipMemcpy(d, *dst[k], old, hipMemcpyDeviceToDevice);
                if (e == hipSuccess) e = hipMemset((uint8_t *)d + old, 0, bytes - old);
                if (e != hipSuccess) {
                    (void)hipFree(d);
                    return status_of(e);
                }
                (void)hipFree((void *)*dst[k]);
                *dst[k] = d;
                g.cap[k] = vertex_count;
            }
            continue;
        }
        if (!*dst[k] || vertex_count > g.cap[k]) {
            float *d = nullptr;
            PRK_TRY(hipMalloc((void **)&d, bytes ? bytes : 4));
            (void)hipFree((void *)*dst[k]);
            *dst[k] = d;
            g.cap[k] = vertex_count;
        }
        PRK_TRY(hipMemcpy((void *)*dst[k], src[k], bytes, hipMemcpyHostToDevice));
    }
    g.vertex_count = vertex_count;
    // recorded draws carry the geometry's device pointers: refresh them
    for (auto &d : c->draws)
        if (d.src_kind == 0 && d.geom == handle) {
            d.V = g.V; d.C = g.C; d.N = g.N; d.UV = g.UV;
        }
    return PRK_OK;
}

static int geometry_grow(prk_context *c, int32_t handle, const bool want[4], uint32_t end);

int prk_geometry_write(prk_context *c, int32_t handle, uint32_t first_vertex, uint32_t vertex_count,
                       const float *v, const float *col, const float *n, const float *uv) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size() || first_vertex % 3 || vertex_count % 3)
        return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    const uint64_t end64 = (uint64_t)first_vertex + vertex_count;
    if (end64 > 0xFFFFFFF0ull) return PRK_ERR_ARG;
    const uint32_t end = (uint32_t)end64;
    Geometry &g = c->geoms[handle];
    if (!g.owned) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    const float *src[4] = {v, col, n, uv};
    const float **dst[4] = {&g.V, &g.C, &g.N, &g.UV};
    const size_t comp[4] = {3, 4, 3, 2};
    const bool given[4] = {v != nullptr, col != nullptr, n != nullptr, uv != nullptr};
    {
        const int rc = geometry_grow(c, handle, given, end);
        if (rc != PRK_OK) return rc;
    }
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if (!src[k] || !vertex_count) continue;
        const size_t off = (size_t)first_vertex * comp[k];
        PRK_TRY(hipMemcpyAsync((void *)(*dst[k] + off), src[k], (size_t)vertex_count * comp[k] * sizeof(float),
                               hipMemcpyHostToDevice, c->copy_stream));
        any = true;
    }
    if (any) {
        PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
        c->in_wait = true;
    }
    g.vertex_count = end;
    return PRK_OK;
}

// Room for `end` vertices in a library-owned geometry's arrays that exist or
// are wanted now (prk_geometry_write, prk_geometry_transform): buffers that
// must grow do so by half again at least, so a frame streamed in chunks
// reallocates rarely; contents kept, zeros past them (a new array: all zeros),
// recorded draws repointed.  Growing waits for the device.
static int geometry_grow(prk_context *c, int32_t handle, const bool want[4], uint32_t end) {
    Geometry &g = c->geoms[handle];
    const float **dst[4] = {&g.V, &g.C, &g.N, &g.UV};
    const size_t comp[4] = {3, 4, 3, 2};
    bool grow = false;
    for (int k = 0; k < 4; ++k) grow |= (want[k] || *dst[k]) && end > g.cap[k];
    if (grow) {
        PRK_TRY(hipDeviceSynchronize());  // frames in flight and earlier writes read / fill the old buffers
        for (int k = 0; k < 4; ++k) {
            if (!(want[k] || *dst[k]) || end <= g.cap[k]) continue;
            const uint64_t need = std::max<uint64_t>(end, (uint64_t)g.cap[k] + g.cap[k] / 2);
            const uint32_t cap = (uint32_t)std::min<uint64_t>(need, 0xFFFFFFF0ull);
            const size_t bytes = (size_t)cap * comp[k] * sizeof(float);
            const size_t old = *dst[k] ? (size_t)g.cap[k] * comp[k] * sizeof(float) : 0;
            float *d = nullptr;
            PRK_TRY(hipMalloc((void **)&d, bytes));
            hipError_t e = old ? hipMemcpy(d, *dst[k], old, hipMemcpyDeviceToDevice) : hipSuccess;
            if (e == hipSuccess) e = hipMemset((uint8_t *)d + old, 0, bytes - old);
            if (e != hipSuccess) {
                (void)hipFree(d);
                return status_of(e);
            }
            (void)hipFree((void *)*dst[k]);
            *dst[k] = d;
            g.cap[k] = cap;
        }
        for (auto &d : c->draws)
            if (d.src_kind == 0 && d.geom == handle) {
                d.V = g.V; d.C = g.C; d.N = g.N; d.UV = g.UV;
            }
        c->read_rec = false;  // the device is idle
    }
    return PRK_OK;
}

int prk_geometry_wrap_device(prk_context *c, const float *v, const float *col, const float *n,
                             const float *uv, uint32_t vertex_count, int32_t *handle_out) {
    if (!c || !v || !handle_out || vertex_count % 3) return PRK_ERR_ARG;
    Geometry g;
    g.V = v;
    g.C = col;
    g.N = n;
    g.UV = uv;
    g.vertex_count = vertex_count;
    g.owned = false;
    *handle_out = (int32_t)c->geoms.size();
    c->geoms.push_back(g);
    return PRK_OK;
}

int prk_geometry_alloc(prk_context *c, int32_t *handle_out) {
    if (!c || !handle_out) return PRK_ERR_ARG;
    Geometry g;  // no vertices, no arrays: prk_geometry_transform / prk_geometry_write give it both
    g.owned = true;
    *handle_out = (int32_t)c->geoms.size();
    c->geoms.push_back(g);
    return PRK_OK;
}

// Runs of src's triangles through a matrix each into dst (prk.h; kernel and
// table layout: prk_xform.hip).  Ordered as prk_geometry_write orders its
// copies: on copy_stream after read_ev, the next flush waits for in_ev.
int prk_geometry_transform(prk_context *c, int32_t src, int32_t dst, const prk_xform_run *runs, uint32_t run_count,
                           const prk_xform *xforms, uint32_t xform_count) {
    if (!c || src < 0 || (size_t)src >= c->geoms.size() || dst < 0 || (size_t)dst >= c->geoms.size() || src == dst)
        return PRK_ERR_ARG;
    if (!c->geoms[dst].owned) return PRK_ERR_ARG;
    if (run_count && (!runs || !xforms)) return PRK_ERR_ARG;
    const uint32_t src_tris = c->geoms[src].vertex_count / 3;
    uint64_t total = 0, top = 0;  // output triangles; one past the highest triangle written
    uint32_t nruns = 0;
    for (uint32_t i = 0; i < run_count; ++i) {
        const prk_xform_run &r = runs[i];
        if (!r.tri_count) continue;
        if (r.xform >= xform_count) return PRK_ERR_ARG;
        if ((uint64_t)r.src_first_tri + r.tri_count > src_tris) return PRK_ERR_ARG;
        const uint64_t dend = (uint64_t)r.dst_first_tri + r.tri_count;
        if (dend * 3 > 0xFFFFFFF0ull) return PRK_ERR_ARG;
        top = std::max(top, dend);
        total += r.tri_count;
        ++nruns;
    }
    if (!nruns) return PRK_OK;
    if (!c->geoms[src].V) return PRK_ERR_ARG;  // (a geometry written without positions)
    if (total > (1ull << 31)) return PRK_ERR_LIMIT;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    // the tables: scan (nruns + 1 words), runs, matrices (prk_xform.hip)
    const size_t runs_off = ((size_t)(nruns + 1) * 4 + 15) & ~(size_t)15;
    const size_t xf_off = runs_off + (size_t)nruns * 16;
    const size_t bytes = xf_off + (size_t)xform_count * sizeof(prk_xform);
    if (c->xf_busy) {  // the staging's previous contents have been copied
        PRK_TRY(hipEventSynchronize(c->xf_ev));
        c->xf_busy = false;
    }
    if (bytes > c->h_xform_cap) {
        if (c->h_xform) (void)hipHostFree(c->h_xform);
        c->h_xform = nullptr;
        c->h_xform_cap = 0;
        const size_t want = bytes + bytes / 4;
        PRK_TRY(hipHostMalloc(&c->h_xform, want, hipHostMallocDefault));
        c->h_xform_cap = want;
    }
    if (!c->xf_ev) PRK_TRY(hipEventCreate(&c->xf_ev));
    if (!c->xf_end_ev) PRK_TRY(hipEventCreate(&c->xf_end_ev));
    {
        uint8_t *h = static_cast<uint8_t *>(c->h_xform);
        uint32_t *scan = reinterpret_cast<uint32_t *>(h);
        uint32_t *rr = reinterpret_cast<uint32_t *>(h + runs_off);
        uint32_t at = 0, k = 0;
        for (uint32_t i = 0; i < run_count; ++i) {
            const prk_xform_run &r = runs[i];
            if (!r.tri_count) continue;
            scan[k] = at;
            rr[4 * k + 0] = r.src_first_tri;
            rr[4 * k + 1] = r.dst_first_tri;
            rr[4 * k + 2] = r.xform;
            rr[4 * k + 3] = at;
            at += r.tri_count;
            ++k;
        }
        scan[nruns] = at;
        std::memcpy(h + xf_off, xforms, (size_t)xform_count * sizeof(prk_xform));
    }
    // dst takes every array src has; its size covers the highest triangle written
    Geometry &s = c->geoms[src];
    const bool has[4] = {s.V != nullptr, s.C != nullptr, s.N != nullptr, s.UV != nullptr};
    const uint32_t end = std::max<uint32_t>(c->geoms[dst].vertex_count, (uint32_t)(top * 3));
    {
        const int rc = geometry_grow(c, dst, has, end);
        if (rc != PRK_OK) return rc;
    }
    Geometry &d = c->geoms[dst];
    PRK_TRY(c->d_xform.ensure(bytes));  // (a larger buffer: hipFree waits for the kernels that read the old one)
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipMemcpyAsync(c->d_xform.p, c->h_xform, bytes, hipMemcpyHostToDevice, c->copy_stream));
    PRK_TRY(hipEventRecord(c->xf_ev, c->copy_stream));
    c->xf_busy = true;
    PRK_TRY(prk_xform_launch(c->d_xform.p, runs_off, xf_off, nruns, (uint32_t)total, s.V, s.C, s.N, s.UV,
                             (float *)d.V, (float *)d.C, (float *)d.N, (float *)d.UV, c->copy_stream));
    PRK_TRY(hipEventRecord(c->xf_end_ev, c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
    d.vertex_count = end;
    return PRK_OK;
}

int prk_geometry_info(prk_context *c, int32_t handle, uint32_t *vertex_count_out, uint32_t *arrays_out) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size()) return PRK_ERR_ARG;
    const Geometry &g = c->geoms[handle];
    if (vertex_count_out) *vertex_count_out = g.vertex_count;
    if (arrays_out) *arrays_out = (g.V ? 1u : 0u) | (g.C ? 2u : 0u) | (g.N ? 4u : 0u) | (g.UV ? 8u : 0u);
    return PRK_OK;
}

int prk_debug_transform_ms(prk_context *c, float *kernel_ms) {
    if (!c || !kernel_ms || !c->xf_busy) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipEventSynchronize(c->xf_end_ev));
    PRK_TRY(hipEventElapsedTime(kernel_ms, c->xf_ev, c->xf_end_ev));
    return PRK_OK;
}

int prk_debug_geometry_stream(prk_context *c, void **stream) {
    if (!c || !stream) return PRK_ERR_ARG;
    *stream = (void *)c->copy_stream;
    return PRK_OK;
}

int prk_geometry_download(prk_context *c, int32_t handle, uint32_t first_vertex, uint32_t vertex_count,
                          float *v, float *col, float *n, float *uv) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size() || first_vertex % 3 || vertex_count % 3)
        return PRK_ERR_ARG;
    const Geometry &g = c->geoms[handle];
    if ((uint64_t)first_vertex + vertex_count > g.vertex_count) return PRK_ERR_ARG;
    float *dst[4] = {v, col, n, uv};
    const float *src[4] = {g.V, g.C, g.N, g.UV};
    const size_t comp[4] = {3, 4, 3, 2};
    for (int k = 0; k < 4; ++k)
        if (dst[k] && !src[k]) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->copy_stream));  // every queued write of a geometry runs there
    for (int k = 0; k < 4; ++k) {
        if (!dst[k] || !vertex_count) continue;
        PRK_TRY(hipMemcpy(dst[k], src[k] + (size_t)first_vertex * comp[k],
                          (size_t)vertex_count * comp[k] * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PRK_OK;
}

int prk_draw(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count, const float P[3],
             int32_t semantics, int32_t phong, int32_t texture) {
    return prk_draw_objects(c, geometry, first_tri, tri_count, 1, P, semantics, phong, texture);
}

int prk_draw_objects(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                     uint32_t tris_per_object, const float P[3], int32_t semantics, int32_t phong, int32_t texture) {
    return prk_draw_objects_setup(c, geometry, first_tri, tri_count, tris_per_object, P, semantics, phong, texture,
                                  -1);
}

int prk_draw_objects_setup(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                           uint32_t tris_per_object, const float P[3], int32_t semantics, int32_t phong,
                           int32_t texture, int32_t setup) {
    if (!c || geometry < 0 || geometry >= (int32_t)c->geoms.size() || tris_per_object == 0) return PRK_ERR_ARG;
    const Geometry &g = c->geoms[geometry];
    if ((uint64_t)first_tri + tri_count > g.vertex_count / 3) return PRK_ERR_ARG;
    if (texture >= (int32_t)c->texs.size()) return PRK_ERR_ARG;
    if (setup > (PRK_SETUP_PHONG | PRK_SETUP_BITMAP)) return PRK_ERR_ARG;
    const bool tex = texture >= 0;
    // FillEdgeTable's PhongShading and Object->Bitmap (prk.h prk_setup)
    const bool fe_phong = setup < 0 ? phong != 0 : (setup & PRK_SETUP_PHONG) != 0;
    const bool fe_bitmap = setup < 0 ? tex : (setup & PRK_SETUP_BITMAP) != 0;
    int mode;
    uint32_t flags = 0;
    if (semantics == PRK_SEM_AVX || semantics == PRK_SEM_AVX_ST) {
        // FillLineOptimized dereferences Bitmap at entry (projekt.cpp:1506) and
        // its non-Phong branch stores garbage (2285-2316): undefined -> rejected.
        // The single-thread overload (2350-3358) shares both (2494, 3262-3290).
        if (!tex || !phong) return PRK_ERR_UNSUPPORTED;
        mode = prk::MODE_AVX;
        if (semantics == PRK_SEM_AVX_ST) flags = prk::DRAW_ST;
    } else if (semantics == PRK_SEM_SCALAR) {
        mode = phong ? (tex ? prk::MODE_SC_PHONG_TEX : prk::MODE_SC_PHONG)
                     : (tex ? prk::MODE_SC_GOURAUD_TEX : prk::MODE_SC_GOURAUD);
    } else {
        return PRK_ERR_ARG;
    }
    // Edge fields FillEdgeTable never wrote: MinNormal without PhongShading
    // (4012-4064), the U/V/(1/z) gradients without Object->Bitmap (4078-4089).
    if ((phong && !fe_phong) || (tex && !fe_bitmap)) return PRK_ERR_UNSUPPORTED;
    if (mode == prk::MODE_SC_GOURAUD) {
        if (fe_phong) flags |= prk::DRAW_RAWCOL;        // raw colours, unlit (4014-4015)
        else if (fe_bitmap) flags |= prk::DRAW_WHITELIT;  // lighting from white (4034-4054)
    }
    if ((phong || !tex) && !g.N) return PRK_ERR_ARG;  // (the Gouraud setup kernels load them in every case)
    if (tex && !g.UV) return PRK_ERR_ARG;
    if ((mode == prk::MODE_SC_GOURAUD || mode == prk::MODE_SC_PHONG) && !g.C) return PRK_ERR_ARG;
    if (tri_count == 0) return PRK_OK;
    if ((uint64_t)c->pending_tris + tri_count >= 0xFFFFFFF0ull) return PRK_ERR_ARG;
    // A draw that continues the previous one (same geometry, the next
    // triangles, same object offset, semantics, texture and object size, the
    // previous one ending on an object boundary) extends it: per-object AETs
    // in submission order are unchanged, and a caller submitting one object
    // per call (the reference's render_entry_3d_object pattern) yields a few
    // draws per frame instead of one per triangle.
    if (!c->draws.empty()) {
        prk::DrawRec &b = c->draws.back();
        const float p0 = P ? P[0] : 0.0f, p1 = P ? P[1] : 0.0f, p2 = P ? P[2] : 0.0f;
        if (b.src_kind == 0 && b.geom == geometry && b.geom_tri0 + b.tri_count == first_tri && b.mode == mode &&
            b.flags == flags && b.tex == texture && b.obj_tris == tris_per_object &&
            b.tri_count % tris_per_object == 0 && b.P[0] == p0 && b.P[1] == p1 && b.P[2] == p2 &&
            std::signbit(b.P[0]) == std::signbit(p0) && std::signbit(b.P[1]) == std::signbit(p1) &&
            std::signbit(b.P[2]) == std::signbit(p2)) {
            b.tri_count += tri_count;
            c->pending_tris += tri_count;
            return PRK_OK;
        }
    }
    prk::DrawRec d{};
    d.V = g.V;
    d.C = g.C;
    d.N = g.N;
    d.UV = g.UV;
    d.geom = geometry;
    d.geom_tri0 = first_tri;
    d.first_global = c->pending_tris;
    d.tri_count = tri_count;
    d.mode = mode;
    d.tex = texture;
    d.P[0] = P ? P[0] : 0.0f;
    d.P[1] = P ? P[1] : 0.0f;
    d.P[2] = P ? P[2] : 0.0f;
    d.flags = flags;
    d.obj_tris = tris_per_object;
    c->draws.push_back(d);
    c->pending_tris += tri_count;
    return PRK_OK;
}

// A draw of caller edges or spans (span path): semantics / texture checks as
// prk_draw; it takes `ids` triangle ids of the frame's numbering.
static int draw_src(prk_context *c, uint32_t kind, uint32_t off, uint32_t n, uint32_t ids, int32_t semantics,
                    int32_t phong, int32_t texture) {
    if (texture >= (int32_t)c->texs.size()) return PRK_ERR_ARG;
    int mode = prk::MODE_AVX;
    if (semantics == PRK_SEM_SCALAR) {
        // DrawModel on a caller's edge list (projekt.cpp:162-601); work
        // records (kind 2; kind 5: those of a span handle) are FillLineOptimized spans only
        if (kind == 2 || kind == 5) return PRK_ERR_UNSUPPORTED;
        const bool tex = texture >= 0;
        mode = phong ? (tex ? prk::MODE_SC_PHONG_TEX : prk::MODE_SC_PHONG)
                     : (tex ? prk::MODE_SC_GOURAUD_TEX : prk::MODE_SC_GOURAUD);
    } else if (semantics != PRK_SEM_AVX && semantics != PRK_SEM_AVX_ST) {
        return PRK_ERR_ARG;
    } else if (texture < 0 || !phong) {
        return PRK_ERR_UNSUPPORTED;  // projekt.cpp:1506, 2285-2316
    }
    if ((uint64_t)c->pending_tris + ids >= 0xFFFFFFF0ull) return PRK_ERR_ARG;
    prk::DrawRec d{};
    d.first_global = c->pending_tris;
    d.tri_count = ids;
    d.mode = mode;
    d.tex = texture;
    d.flags = semantics == PRK_SEM_AVX_ST ? prk::DRAW_ST : 0u;
    d.obj_tris = 1;
    d.src_kind = kind;
    d.src_off = off;
    d.src_n = n;
    c->draws.push_back(d);
    c->pending_tris += ids;
    return PRK_OK;
}

int prk_draw_edges(prk_context *c, const prk_edge *edges, uint32_t edge_count, int32_t semantics, int32_t phong,
                   int32_t texture) {
    if (!c || (!edges && edge_count)) return PRK_ERR_ARG;
    if (edge_count == 0) return PRK_OK;  // 0 edges: nothing to draw (P1)
    const uint32_t off = (uint32_t)c->pend_edges.size();
    const int rc = draw_src(c, 1, off, edge_count, 1, semantics, phong, texture);
    if (rc == PRK_OK) c->pend_edges.insert(c->pend_edges.end(), edges, edges + edge_count);
    return rc;
}

// Whether a list of a batch takes the walks of a triangle object: sorted by
// YMin (the sorted insertion cursor then inserts exactly what the reference's
// whole-list scan inserts, in the same order), and every edge inside the
// value range FillEdgeTable writes (0 <= YMin <= YMax, Left 0 or 1), which
// those walks' list mirrors are sized for.  Any other list is walked as
// prk_draw_edges walks it.
static bool list_walks_sorted(const prk_edge *e, uint32_t n) {
    int32_t prev = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (e[i].YMin < prev || e[i].YMax < e[i].YMin || (uint32_t)e[i].Left > 1u) return false;
        prev = e[i].YMin;
    }
    return true;
}

int prk_draw_edge_lists(prk_context *c, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                        int32_t semantics, int32_t phong, int32_t texture) {
    if (!c || (!counts && list_count)) return PRK_ERR_ARG;
    uint64_t total = 0;
    for (uint32_t o = 0; o < list_count; ++o) total += counts[o];
    if (!records && total) return PRK_ERR_ARG;
    if (list_count == 0) return PRK_OK;
    // the frame's batch records and lists are indexed by 31 bits (as a pass's edge slots, flush_spans)
    if (c->pend_ledges.size() + total >= 0x7FFFFFFFull || c->pend_lcnt.size() + (uint64_t)list_count >= 0x7FFFFFFFull)
        return PRK_ERR_LIMIT;
    const uint32_t off = (uint32_t)c->pend_ledges.size(), l0 = (uint32_t)c->pend_lcnt.size();
    const int rc = draw_src(c, 3, off, (uint32_t)total, list_count, semantics, phong, texture);
    if (rc != PRK_OK) return rc;
    c->draws.back().geom_tri0 = l0;
    c->pend_ledges.insert(c->pend_ledges.end(), records, records + total);
    c->pend_lcnt.insert(c->pend_lcnt.end(), counts, counts + list_count);
    const prk_edge *e = records;
    for (uint32_t o = 0; o < list_count; e += counts[o], ++o)
        c->pend_lflag.push_back(list_walks_sorted(e, counts[o]) ? 1u : 0u);
    return PRK_OK;
}

int prk_draw_spans(prk_context *c, const prk_span *spans, uint32_t count, int32_t semantics, int32_t phong,
                   int32_t texture) {
    if (!c || (!spans && count)) return PRK_ERR_ARG;
    if (count == 0) return PRK_OK;
    const uint32_t off = (uint32_t)c->pend_spans.size();
    const int rc = draw_src(c, 2, off, count, count, semantics, phong, texture);
    if (rc == PRK_OK) c->pend_spans.insert(c->pend_spans.end(), spans, spans + count);
    return rc;
}

// Row work records (prk_row_records' output, or a caller's own) as a draw of
// their pairs: the rows and pairs go up as they are, k_rows_unpack
// (prk_records.hip) turns every pair into the prk_span of its row on the device
// -- no host loop over the pairs, only the one over the rows that checks the
// arguments -- and the spans come back into the pending frame's span input,
// where the draw is prk_draw_spans' from then on.  The buffers are this
// call's own: frames in flight keep the span scratch.  keep
// (prk_spans_upload_rows; `out` is then NULL): the spans are written into
// that device buffer (25 * npair dwords rounded up to four) and stay there.
static int rows_to_spans(prk_context *c, const prk_row *rows, uint32_t nrow, const prk_row_pair *pairs,
                         uint32_t npair, prk_span *out, void *keep = nullptr) {
    PRK_TRY(hipSetDevice(c->device));
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    const size_t out_bytes = packed_span_bytes(npair);
    PRK_TRY(S.d_dr_rows.ensure((size_t)nrow * sizeof(prk_row)));
    PRK_TRY(S.d_dr_pairs.ensure((size_t)npair * sizeof(prk_row_pair)));
    PRK_TRY(S.d_dr_cnt.ensure(((size_t)nrow + 1) * 4));
    PRK_TRY(S.d_dr_scan.ensure(((size_t)nrow + 1) * 4));
    if (!keep) PRK_TRY(S.d_dr_out.ensure(out_bytes));
    PRK_TRY(hipMemcpyAsync(S.d_dr_rows.p, rows, (size_t)nrow * sizeof(prk_row), hipMemcpyHostToDevice, s));
    PRK_TRY(hipMemcpyAsync(S.d_dr_pairs.p, pairs, (size_t)npair * sizeof(prk_row_pair), hipMemcpyHostToDevice, s));
    PRK_TRY(prk_rows_counts(S.d_dr_rows.p, nrow, (uint32_t *)S.d_dr_cnt.p, s));
    PRK_TRY(scan_u32(S.d_dr_temp, (const uint32_t *)S.d_dr_cnt.p, (uint32_t *)S.d_dr_scan.p, nrow + 1, s));
    PRK_TRY(prk_rows_unpack(S.d_dr_rows.p, (const uint32_t *)S.d_dr_scan.p, nrow, S.d_dr_pairs.p, npair,
                            keep ? keep : S.d_dr_out.p, s));
    if (!keep) PRK_TRY(hipMemcpyAsync(out, S.d_dr_out.p, (size_t)npair * sizeof(prk_span), hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));  // (the caller's arrays are copied at the call)
    return PRK_OK;
}

int prk_draw_rows(prk_context *c, const prk_row *rows, uint64_t row_count, const prk_row_pair *pairs,
                  uint64_t pair_count, int32_t semantics, int32_t phong, int32_t texture) {
    if (!c || (!rows && row_count) || (!pairs && pair_count)) return PRK_ERR_ARG;
    uint64_t sum = 0;
    for (uint64_t r = 0; r < row_count; ++r) {
        if (rows[r].RowIndex < 0) return PRK_ERR_ARG;
        sum += rows[r].EdgeCount;
    }
    if (sum != pair_count) return PRK_ERR_ARG;
    if (row_count == 0 || pair_count == 0) return PRK_OK;
    // the frame's span input is indexed by 31 bits, as the other caller records
    if (row_count >= 0x7FFFFFFFull || c->pend_spans.size() + pair_count >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    const uint32_t off = (uint32_t)c->pend_spans.size(), n = (uint32_t)pair_count;
    int rc = draw_src(c, 2, off, n, n, semantics, phong, texture);
    if (rc != PRK_OK) return rc;
    c->pend_spans.resize((size_t)off + n);
    rc = rows_to_spans(c, rows, (uint32_t)row_count, pairs, n, c->pend_spans.data() + off);
    if (rc != PRK_OK) {  // nothing is recorded
        c->pend_spans.resize(off);
        c->draws.pop_back();
        c->pending_tris -= n;
    }
    return rc;
}

int prk_reset_draws(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    c->draws.clear();
    c->pending_tris = 0;
    c->pend_edges.clear();
    c->pend_spans.clear();
    c->pend_ledges.clear();
    c->pend_lcnt.clear();
    c->pend_lflag.clear();
    return PRK_OK;
}

int prk_set_tile(prk_context *c, int32_t tw, int32_t th) {
    // tile_w: a power of two >= 8 (pixel index <-> (x, y) by shifts)
    if (!c || tw < 8 || th <= 0 || (tw & (tw - 1)) || tw * th > 8192 || tw * th < 64) return PRK_ERR_ARG;
    c->tile_w = tw;
    c->tile_h = th;
    c->tile_auto = false;
    return PRK_OK;
}

int prk_set_early_z(prk_context *c, int on) {
    if (!c) return PRK_ERR_ARG;
    c->early_z = on != 0;
    return PRK_OK;
}

int prk_set_debug(prk_context *c, int32_t enable) {
    if (!c) return PRK_ERR_ARG;
    c->debug = enable != 0;
    return PRK_OK;
}

// Accumulate the kernel times of a timed flush slot (waits for its last event).
static void harvest(prk_context *c, int slot) {
    if (!c->pending[slot]) return;
    c->pending[slot] = false;
    if (hipEventSynchronize(c->ev[slot][2]) != hipSuccess) return;
    float a = 0, b = 0, v = 0, sp = 0;
    if (hipEventElapsedTime(&a, c->ev[slot][0], c->ev[slot][1]) != hipSuccess) a = 0;
    if (hipEventElapsedTime(&b, c->ev[slot][5], c->ev[slot][2]) != hipSuccess) b = 0;
    if (hipEventElapsedTime(&v, c->ev[slot][5], c->ev[slot][3]) != hipSuccess) v = 0;
    if (!c->split_span[slot] || hipEventElapsedTime(&sp, c->ev[slot][3], c->ev[slot][4]) != hipSuccess) sp = 0;
    c->stats.sum_ms_bin += a;
    c->stats.sum_ms_raster += b;
    c->stats.sum_ms_vis += v;
    c->stats.sum_ms_span += sp;
    c->stats.frames_timed += 1;
    if (slot == c->last_slot) {
        c->stats.ms_bin = a;
        c->stats.ms_raster = b;
    }
}

int prk_timing_reset(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    for (int i = 0; i < prk_context::kRing; ++i) c->pending[i] = false;
    c->stats.frames_timed = 0;
    c->stats.sum_ms_bin = c->stats.sum_ms_raster = c->stats.sum_ms_vis = c->stats.sum_ms_span = 0.0;
    if (c->d_prof.p) PRK_TRY(hipMemset(c->d_prof.p, 0, 16 * sizeof(uint64_t)));
    return PRK_OK;
}

int prk_debug_counters(prk_context *c, uint64_t *out, int32_t n) {
    if (!c || !out || n < 0 || n > 16) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    for (int i = 0; i < n; ++i) out[i] = 0;
    if (c->d_prof.p && n) PRK_TRY(hipMemcpy(out, c->d_prof.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_debug_walk_routes(prk_context *c, uint32_t *out, int32_t n) {
    if (!c || !out || n < 0 || n > 12) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    const prk_context::SpanScratch &S = c->spans;
    for (int i = 0; i < n; ++i) out[i] = i < 9 ? S.walk_routes[i] : (uint32_t)S.walk_sizes[i - 9];
    return PRK_OK;
}

int prk_debug_list_routes(prk_context *c, uint32_t *out, int32_t n) {
    if (!c || !out || n < 0 || n > 6) return PRK_ERR_ARG;
    for (int i = 0; i < n; ++i) out[i] = c->spans.list_routes[i];
    return PRK_OK;
}

int prk_debug_bins(prk_context *c, prk_bins_info *info, uint32_t *tri_n, uint16_t *ranges, uint32_t *tri_off,
                   uint8_t *listed, uint64_t tri_capacity, uint32_t *offs, uint64_t tile_capacity, uint32_t *bins,
                   uint32_t *pair_tri, uint64_t entry_capacity) {
    if (!c || !info) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);  // (an overflowed pass is re-run here: bdbg then names the re-run's set)
    const prk_context::BinsDebug &D = c->bdbg;
    if (!D.valid) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    const prk_context::BinSet &B = c->bset[D.set];
    const uint32_t T = D.T, ntiles = (uint32_t)(D.tiles_x * D.tiles_y), total = B.h_info[0];
    *info = prk_bins_info{D.tile_w, D.tile_h, D.tiles_x, D.tiles_y, D.row0, D.row1, T, total, D.rerun ? 1u : 0u,
                          D.per};
    if ((tri_n || ranges || tri_off || listed) && tri_capacity < T) return PRK_ERR_ARG;
    if (offs && tile_capacity < ntiles) return PRK_ERR_ARG;
    if ((bins || pair_tri) && entry_capacity < total) return PRK_ERR_ARG;
    if (tri_n) PRK_TRY(hipMemcpy(tri_n, B.d_tri_n.p, (size_t)T * 4, hipMemcpyDeviceToHost));
    if (ranges) PRK_TRY(hipMemcpy(ranges, B.d_ranges.p, (size_t)T * 16, hipMemcpyDeviceToHost));
    if (tri_off) PRK_TRY(hipMemcpy(tri_off, B.d_tri_off.p, ((size_t)T + 1) * 4, hipMemcpyDeviceToHost));
    if (listed) std::memset(listed, D.per ? 0 : 1, T);
    if (D.per && (tri_n || ranges || tri_off || listed)) {
        // a row band: k_bin_band and k_cs_emit wrote only the triangles of the
        // run lists; the others hold what an earlier frame left
        const uint32_t nruns = prk_bin_runs(T), len = prk_bin_run_len();
        std::vector<uint32_t> run_n(nruns), list((size_t)nruns * len);
        std::vector<uint8_t> in(T, 0);
        PRK_TRY(hipMemcpy(run_n.data(), B.d_run_n.p, (size_t)nruns * 4, hipMemcpyDeviceToHost));
        PRK_TRY(hipMemcpy(list.data(), B.d_runlist.p, list.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t r = 0; r < nruns; ++r)
            for (uint32_t i = 0; i < std::min(run_n[r], len); ++i) {
                const uint32_t g = list[(size_t)r * len + i];
                if (g < T) in[g] = 1;
            }
        static const uint16_t kEmpty[8] = {1, 1, 0, 0, 1, 0, 0, 0};
        for (uint32_t g = 0; g < T; ++g) {
            if (listed) listed[g] = in[g];
            if (in[g]) continue;
            if (tri_n) tri_n[g] = 0;
            if (ranges) std::memcpy(ranges + 8 * (size_t)g, kEmpty, sizeof(kEmpty));
            if (tri_off) tri_off[g] = UINT32_MAX;
        }
    }
    if (offs) PRK_TRY(hipMemcpy(offs, B.d_offs.p, ((size_t)ntiles + 1) * 4, hipMemcpyDeviceToHost));
    if (bins && total) PRK_TRY(hipMemcpy(bins, B.d_bins.p, (size_t)total * 8, hipMemcpyDeviceToHost));
    if (pair_tri && total) PRK_TRY(hipMemcpy(pair_tri, B.d_pair_tri.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

// The frame parameters every pass of a flush shares (camera, lights, target, tiling).
static void frame_params(const prk_context *c, prk::FrameParams &fp) {
    fp = prk::FrameParams{};
    fp.D = c->transform.DistanceAboveTarget;
    fp.F = c->transform.FocalLength;
    fp.M2P = c->transform.MetersToPixels;
    fp.Cx = c->transform.ScreenCenter[0];
    fp.Cy = c->transform.ScreenCenter[1];
    fp.InvM2P = 1.0f / fp.M2P;
    {
        int e = 0;
        const float m = std::frexp(fp.F, &e);  // F = m * 2^e, |m| in [0.5, 1)
        fp.f_pow2 = (std::isfinite(fp.F) && (m == 0.5f || m == -0.5f) && e - 1 >= -125 && e - 1 <= 126) ? 1 : 0;
        fp.InvF = fp.f_pow2 ? 1.0f / fp.F : 0.0f;
    }
    fp.light_count = c->lights.LightCount;
    for (int k = 0; k < 4; ++k) fp.amb[k] = c->lights.AmbientIntensity[k];
    for (uint32_t l = 0; l < PRK_MAX_LIGHTS; ++l) {
        for (int k = 0; k < 3; ++k) fp.lp[l][k] = c->lights.Lights[l].P[k];
        for (int k = 0; k < 4; ++k) fp.li[l][k] = c->lights.Lights[l].Intensity[k];
    }
    // the span shading's camera and lights (prk_set_shade_camera)
    {
        const prk_transform &t = c->shade_transform;
        const prk_light_data &L = c->shade_lights;
        prk::ShadeCam &sh = fp.sh;
        sh.D = t.DistanceAboveTarget;
        sh.F = t.FocalLength;
        sh.Cx = t.ScreenCenter[0];
        sh.Cy = t.ScreenCenter[1];
        sh.InvM2P = 1.0f / t.MetersToPixels;
        int e = 0;
        const float m = std::frexp(sh.F, &e);  // F = m * 2^e, |m| in [0.5, 1)
        sh.f_pow2 = (std::isfinite(sh.F) && (m == 0.5f || m == -0.5f) && e - 1 >= -125 && e - 1 <= 126) ? 1 : 0;
        sh.InvF = sh.f_pow2 ? 1.0f / sh.F : 0.0f;
        sh.light_count = L.LightCount;
        for (int k = 0; k < 4; ++k) sh.amb[k] = L.AmbientIntensity[k];
        for (uint32_t l = 0; l < PRK_MAX_LIGHTS; ++l) {
            for (int k = 0; k < 3; ++k) sh.lp[l][k] = L.Lights[l].P[k];
            for (int k = 0; k < 4; ++k) sh.li[l][k] = L.Lights[l].Intensity[k];
        }
    }
    fp.W = c->W;
    fp.H = c->H;
    fp.row0 = c->row0;
    fp.row1 = c->row1;
    fp.pitch = c->pitch;
    fp.color = (uint32_t *)c->color;
    fp.zbuf = c->zbuf;
    // The context's tile, made taller (then wider) while the frame would have
    // more tiles than the counting-sort binning holds (kCsMaxTiles): results
    // never depend on the tile, and every tile keeps <= 8192 pixels.
    int32_t tw = c->tile_w, th = c->tile_h;
    auto ntl = [&](int32_t w, int32_t h) {
        return (uint64_t)((c->W + w - 1) / w) * (uint64_t)((c->row1 - c->row0 + h - 1) / h);
    };
    while (ntl(tw, th) > prk_cs_max_tiles() && tw * th * 2 <= 8192) {
        if (th < tw / 8) th *= 2;
        else tw *= 2;
    }
    fp.tile_w = tw;
    fp.tile_h = th;
    fp.tile_w_log2 = 0;
    while ((1 << fp.tile_w_log2) < tw) ++fp.tile_w_log2;
    fp.tiles_x = (c->W + tw - 1) / tw;
    fp.tiles_y = (c->row1 - c->row0 + th - 1) / th;
    fp.prof = (unsigned long long *)c->d_prof.p;
    fp.negz = (uint32_t *)c->d_negz.p;
    fp.z_in_vis = c->early_z && c->d_negz.p ? 1 : 0;
    fp.winners = c->debug ? (int32_t *)c->d_winners.p : nullptr;
    fp.clear_color = c->clear_color;
    fp.clear_z = c->clear_z;
}

// A pending clear that the pass cannot fuse into its kernels: fill first.
static int fill_pending_clear(prk_context *c, hipStream_t s) {
    c->z_early = false;
    if (!c->clear_pending) return PRK_OK;
    c->clear_pending = false;
    const size_t n = (size_t)c->W * (c->row1 - c->row0);
    if (n) {
        hipLaunchKernelGGL(k_fill_target, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint32_t *)c->color,
                           c->pitch, c->zbuf, c->W, c->row1 - c->row0, c->clear_color, c->clear_z);
        PRK_TRY(hipGetLastError());
    }
    return PRK_OK;
}

// One pass of per-triangle AETs (draws of one triangle per object): bin +
// raster into the target.  `draws` number their triangles from 0; winner ids
// are win_base + that index.
static int flush_tris(prk_context *c, hipStream_t s, const std::vector<prk::DrawRec> &draws, uint32_t T,
                      uint32_t win_base, bool defer = false) {
    int modeset = -2;
    for (const auto &d : draws) {
        if (modeset == -2) modeset = d.mode;
        else if (modeset != d.mode) modeset = -1;
    }
    if (modeset != prk::MODE_AVX && modeset != prk::MODE_SC_GOURAUD && modeset != prk::MODE_SC_PHONG)
        modeset = -1;
    prk::FrameParams fp;
    frame_params(c, fp);
    fp.tri_count = T;
    fp.ndraws = (uint32_t)draws.size();
    fp.win_base = win_base;
    const uint32_t ntiles = (uint32_t)(fp.tiles_x * fp.tiles_y);

    c->stats.triangles = T;
    c->stats.tiles = ntiles;
    c->stats.bin_entries = 0;
    const int slot = (int)(c->frame % prk_context::kRing);
    harvest(c, slot);  // a flush kRing frames old: long finished
    // A pending fused clear: the span-record kernels (AVX frames) fold it in;
    // every other frame fills the target first, on this stream.
    const bool fuse = c->clear_pending && T > 0 && modeset == prk::MODE_AVX && PRK_SPAN_RECORDS_HOST;
    if (!fuse) {
        const int rc = fill_pending_clear(c, s);
        if (rc != PRK_OK) return rc;
    }
    c->clear_pending = false;
    fp.clear_fused = fuse ? 1 : 0;
    if (T == 0) return PRK_OK;
    // Binning runs on bin_stream into one of the scratch sets, so it overlaps
    // the previous frame's raster on the flush stream; the raster waits for
    // it.  Consecutive frames take consecutive sets (nsets of them), and a
    // set's reuse waits for its own last reader.
    const int nsets = (size_t)c->W * (size_t)(c->row1 - c->row0) <= kSmallBandPx ? prk_context::kSets
                                                                                : std::min(prk_context::kSets, 2);
    const int si = (c->last_set + 1) % nsets;
    c->last_set = si;
    prk_context::BinSet &B = c->bset[si];
    // Any error below leaves the set's table mirrors unknown: forget them.
    struct MirrorGuard {
        prk_context::BinSet &b;
        bool ok = false;
        ~MirrorGuard() {
            if (!ok) b.h_draws_at = b.h_texs_at = nullptr;
        }
    } guard{B};
    hipStream_t bs = c->bin_stream;
    if (B.used) PRK_TRY(hipStreamWaitEvent(bs, B.free_ev, 0));  // the raster of frame k-nsets read this set
    // A set buffer that must grow is freed by the host: wait for its reader.
    auto bset_ensure = [&](DevBuf &d, size_t n) -> hipError_t {
        if (d.cap < n && B.used) {
            hipError_t e = hipEventSynchronize(B.free_ev);
            if (e != hipSuccess) return e;
        }
        return d.ensure(n);
    };
    // Device-side draw + texture tables.
    std::vector<prk::TexRec> texs(c->texs.size());
    for (size_t i = 0; i < texs.size(); ++i) {
        texs[i].mem = c->texs[i].mem;
        texs[i].w = c->texs[i].w;
        texs[i].h = c->texs[i].h;
        texs[i].pitch = c->texs[i].pitch;
        texs[i].filter = c->texs[i].filter;
    }
    // Upload a table into this set unless the set already holds the same
    // bytes (the set's previous reader, frame k-nsets's raster, is waited for above).
    auto upload_table = [&](DevBuf &d, std::vector<uint8_t> &mirror, const void *&at, const void *src,
                            size_t bytes) -> hipError_t {
        hipError_t e = bset_ensure(d, bytes);
        if (e != hipSuccess) return e;
        if (at == d.p && mirror.size() == bytes && std::memcmp(mirror.data(), src, bytes) == 0) return hipSuccess;
        at = nullptr;  // unknown until the copy is queued
        mirror.assign((const uint8_t *)src, (const uint8_t *)src + bytes);
        // from the mirror: it outlives this call (the set's next use waits for
        // this frame's raster, which follows the copy on the bin stream)
        e = hipMemcpyAsync(d.p, mirror.data(), bytes, hipMemcpyHostToDevice, bs);
        if (e == hipSuccess) at = d.p;
        return e;
    };
    PRK_TRY(upload_table(B.d_draws, B.h_draws, B.h_draws_at, draws.data(), draws.size() * sizeof(prk::DrawRec)));
    if (!texs.empty())
        PRK_TRY(upload_table(B.d_texs, B.h_texs, B.h_texs_at, texs.data(), texs.size() * sizeof(prk::TexRec)));
    fp.draws = (const prk::DrawRec *)B.d_draws.p;
    fp.texs = (const prk::TexRec *)B.d_texs.p;
    fp.draw0 = draws[0];
    fp.tex0 = prk::TexRec{};
    if (fp.draw0.tex >= 0 && (size_t)fp.draw0.tex < texs.size()) fp.tex0 = texs[fp.draw0.tex];
    fp.tri_draw = nullptr;
    if (fp.ndraws > 1) {
        PRK_TRY(bset_ensure(B.d_tri_draw, (size_t)T * 4));
        PRK_TRY(prk_launch_tri_draw(fp.draws, fp.ndraws, (uint32_t *)B.d_tri_draw.p, T, bs));
        fp.tri_draw = (const uint32_t *)B.d_tri_draw.p;
    }
    PRK_TRY(bset_ensure(B.d_ranges, (size_t)T * 16));
    PRK_TRY(bset_ensure(B.d_tri_n, (size_t)(T + 1) * 4));
    PRK_TRY(bset_ensure(B.d_tri_off, (size_t)(T + 1) * 4));
    PRK_TRY(bset_ensure(B.d_offs, (size_t)(ntiles + 1) * 4));
    fp.trec = nullptr;
    if (modeset == prk::MODE_AVX && c->setup_rec) {
        PRK_TRY(bset_ensure(B.d_trec, (size_t)T * sizeof(prk::TriRec)));
        fp.trec = (prk::TriRec *)B.d_trec.p;
    }
    const bool span_rec = modeset == prk::MODE_AVX;
    // won flags: per (pair, row in tile) for span-record (AVX) frames, per
    // pair otherwise; the binning clears them (and trwon) for every pair.
    const uint32_t won_stride = span_rec ? (uint32_t)fp.tile_h : 1u;
    size_t sel_bytes = 0;
    if (span_rec) PRK_TRY(prk_walk_select_bytes(T, &sel_bytes));
    // Every per-pair array of the set, for `np` pairs.
    auto ensure_pairs = [&](size_t np) -> hipError_t {
        const size_t ne = std::max<size_t>(np, 1);
        hipError_t e = hipSuccess;
        if (e == hipSuccess) e = bset_ensure(B.d_pair_tri, ne * 4);
        if (e == hipSuccess) e = bset_ensure(B.d_bins, ne * 8);  // (triangle, pair) per bin slot
        if (e == hipSuccess) e = bset_ensure(B.d_list, ne * 4);
        if (e == hipSuccess) e = bset_ensure(B.d_won, ne * won_stride);
        // span records: 64 B per (pair, row in tile); only won ones are written
        if (e == hipSuccess && span_rec) e = bset_ensure(B.d_recs, ne * won_stride * 64);
        return e;
    };
    PRK_TRY(bset_ensure(B.d_nwin, (size_t)ntiles * 4));
    PRK_TRY(bset_ensure(B.d_wtag, (size_t)ntiles * fp.tile_w * fp.tile_h * 4));
    if (span_rec) {
        PRK_TRY(bset_ensure(B.d_trwon, T));
        PRK_TRY(bset_ensure(B.d_wlist, ((size_t)T + 1) * 4));  // won triangles + their count
        PRK_TRY(bset_ensure(B.d_seltemp, std::max<size_t>(sel_bytes, 16)));
    }
    uint8_t *won, *trwon;
    // (frame_params keeps every frame within the counting sort's tile count)
    if (ntiles > prk_cs_max_tiles()) return PRK_ERR_LIMIT;
    if (!prk_cs_ready(ntiles)) return PRK_ERR_DEVICE;
    {
        // Counting-sort binning (prk_bin.hip k_cs_*): all sizes stay on the
        // device.  The per-pair arrays hold `cap` pairs (the last frame's
        // count plus room; a first frame guesses 2.5 per triangle, C3b has
        // 3.2); a frame with more entries leaves its bins empty and is re-run
        // below, once the count is known.
        // a row band's sort walks only its triangles (listed per run by k_bin_band)
        const uint32_t per = prk_cs_band_runs_per_chunk(&fp);
        if (per) {
            PRK_TRY(bset_ensure(B.d_runlist, (size_t)prk_bin_runs(T) * prk_bin_run_len() * 4));
            PRK_TRY(bset_ensure(B.d_run_n, (size_t)prk_bin_runs(T) * 4));
        }
        const uint32_t nch = prk_cs_nchunks(T, per);
        const uint64_t want64 = c->pair_hint ? (uint64_t)c->pair_hint + c->pair_hint / 8 + 4096
                                             : std::max<uint64_t>(5ull * T / 2, 1u << 16);
        const uint32_t want = (uint32_t)std::min<uint64_t>(want64, prk_cs_max_pairs());
        // pairs the set's per-pair arrays hold now (they never shrink)
        auto pairs_held = [&]() -> size_t {
            size_t m = std::min(B.d_pair_tri.cap / 4, B.d_bins.cap / 8);
            m = std::min(m, B.d_list.cap / 4);
            m = std::min(m, B.d_won.cap / won_stride);
            if (span_rec) m = std::min(m, B.d_recs.cap / ((size_t)won_stride * 64));
            return m;
        };
        if (pairs_held() > 4ull * want && pairs_held() > (1u << 20)) {
            // far more room than the frames need (a big frame earlier): give
            // it back once the set's last reader is done
            if (B.used) PRK_TRY(hipEventSynchronize(B.free_ev));
            DevBuf *pb[] = {&B.d_pair_tri, &B.d_bins, &B.d_list, &B.d_won, &B.d_recs};
            for (DevBuf *b : pb) b->release();
        }
        if (pairs_held() < want) PRK_TRY(ensure_pairs(want));
        const uint32_t cap = (uint32_t)std::min<size_t>(pairs_held(), prk_cs_max_pairs());
        PRK_TRY(bset_ensure(B.d_ghist, std::max<size_t>((size_t)nch * ntiles * 4, 4)));
        PRK_TRY(bset_ensure(B.d_tile_tot, (size_t)ntiles * 4));
        PRK_TRY(bset_ensure(B.d_chunk, std::max<size_t>((size_t)nch * 8, 8)));
        PRK_TRY(bset_ensure(B.d_info, 8));
        won = (uint8_t *)B.d_won.p;
        trwon = span_rec ? (uint8_t *)B.d_trwon.p : nullptr;
        PRK_TRY(hipEventRecord(c->ev[slot][0], bs));
        uint32_t *runlist = per ? (uint32_t *)B.d_runlist.p : nullptr, *run_n = per ? (uint32_t *)B.d_run_n.p : nullptr;
        PRK_TRY(prk_bin_count(&fp, (uint32_t *)B.d_tri_n.p, B.d_ranges.p, runlist, run_n, trwon, bs));
        // a row band's setup records (k_band_rec) run on the vis stream beside
        // the counting sort, once k_bin_band has listed the runs; queued after
        // the sort's launches, so a host that is only just ahead of the GPU
        // (a frame after a wait) does not hold the sort back
        const bool band_rec = runlist && fp.trec;
        if (band_rec) PRK_TRY(hipEventRecord(B.listed_ev, bs));
        if (band_rec && !PRK_REC_AFTER_CS) {
            PRK_TRY(hipStreamWaitEvent(c->vis_stream, B.listed_ev, 0));
            PRK_TRY(prk_band_records(&fp, runlist, run_n, c->vis_stream));
        }
        uint32_t *chunk = (uint32_t *)B.d_chunk.p;
        PRK_TRY(prk_bin_cs(&fp, B.d_ranges.p, (const uint32_t *)B.d_tri_n.p, (uint32_t *)B.d_ghist.p,
                           (uint32_t *)B.d_tile_tot.p, chunk, chunk + nch, (uint32_t *)B.d_offs.p, cap,
                           (uint32_t *)B.d_info.p, (uint32_t *)B.d_tri_off.p, B.d_bins.p, (uint32_t *)B.d_pair_tri.p,
                           won, won_stride, trwon, runlist, run_n, per, bs));
        // the bins are ready: the raster may start (after the entry count's
        // copy to the host, PRK_BINNED_EARLY)
        if (PRK_BINNED_EARLY) {
            PRK_TRY(hipEventRecord(c->ev[slot][1], bs));
            PRK_TRY(hipEventRecord(B.binned_ev, bs));
        }
        PRK_TRY(hipMemcpyAsync(B.h_info, B.d_info.p, 8, hipMemcpyDeviceToHost, bs));
        PRK_TRY(hipEventRecord(B.counted_ev, bs));
        if (!PRK_BINNED_EARLY) {
            PRK_TRY(hipEventRecord(c->ev[slot][1], bs));
            PRK_TRY(hipEventRecord(B.binned_ev, bs));
        }
        if (band_rec && PRK_REC_AFTER_CS) {  // (this frame's k_vis follows the records on the vis stream)
            PRK_TRY(hipStreamWaitEvent(c->vis_stream, B.listed_ev, 0));
            PRK_TRY(prk_band_records(&fp, runlist, run_n, c->vis_stream));
        }
    }

    // Raster.  Span-record frames run k_vis on vis_stream once their binning
    // is done (so it overlaps the previous frame's k_walk / k_pix on the
    // flush stream, while the next frame bins on bin_stream) and shade on the
    // flush stream after it; k_vis waits for the flush stream only when it
    // reads the target's prior z (no fused clear), writes the debug winner
    // map, or writes z itself (early z: the flush stream may still hold an
    // earlier frame's z writers -- k_shade, k_pix, k_span_shade, a -0.0
    // fix-up -- that must land before this frame's z).
    // Other frames run on the flush stream.
    if (!c->d_anomaly.p) {
        PRK_TRY(c->d_anomaly.ensure(8));  // [anomalies, slow replays]
        PRK_TRY(hipMemsetAsync(c->d_anomaly.p, 0, 8, s));
        PRK_TRY(hipStreamSynchronize(s));
    }
    hipStream_t sv = s;
    if (span_rec) {
        sv = c->vis_stream;
        PRK_TRY(hipStreamWaitEvent(sv, B.binned_ev, 0));
        if (!fuse || c->debug || fp.z_in_vis) {  // prior z / winner map / early z: after the flush stream's work so far
            PRK_TRY(hipEventRecord(c->s_mark, s));
            PRK_TRY(hipStreamWaitEvent(sv, c->s_mark, 0));
        }
    } else {
        PRK_TRY(hipStreamWaitEvent(s, B.binned_ev, 0));
    }
    PRK_TRY(hipEventRecord(c->ev[slot][5], sv));
    PRK_TRY(prk_launch_raster(&fp, modeset, (const uint32_t *)B.d_offs.p, B.d_bins.p,
                              (const uint32_t *)B.d_pair_tri.p, (const uint32_t *)B.d_tri_off.p, B.d_ranges.p,
                              (uint8_t *)B.d_won.p, (uint8_t *)B.d_trwon.p, (uint32_t *)B.d_wlist.p,
                              B.d_seltemp.p, sel_bytes, (uint32_t *)B.d_list.p,
                              (uint32_t *)B.d_nwin.p, (uint32_t *)B.d_wtag.p, B.d_recs.p,
                              (uint32_t *)c->d_anomaly.p, c->ev[slot][3], span_rec ? c->ev[slot][4] : nullptr, sv,
                              s));
    PRK_TRY(hipEventRecord(c->ev[slot][2], s));
    PRK_TRY(hipEventRecord(B.free_ev, s));
    // a span-record pass's z is final after k_vis (ev[slot][3], on the vis stream)
    c->z_early = span_rec && sv != s && fp.z_in_vis;
    c->z_slot = slot;
    B.used = true;
    c->pending[slot] = true;
    c->split_span[slot] = modeset == prk::MODE_AVX;
    c->last_slot = slot;
    c->frame++;
    guard.ok = true;
    c->bdbg.valid = c->debug;
    if (c->debug) {  // (prk_debug_bins reads this set once the frame is done)
        prk_context::BinsDebug &D = c->bdbg;
        D.rerun = false;
        D.set = si;
        D.T = T;
        D.per = prk_cs_band_runs_per_chunk(&fp);
        D.tile_w = fp.tile_w;
        D.tile_h = fp.tile_h;
        D.tiles_x = fp.tiles_x;
        D.tiles_y = fp.tiles_y;
        D.row0 = fp.row0;
        D.row1 = fp.row1;
    }
    {
        // The whole frame is queued; now the entry count (the binning's first
        // few kernels) decides whether it fitted — read here, or, for the
        // frame's last pass once a previous frame has sized the scratch, by
        // the next call that needs it (resolve_count).
        prk_context::PendingCount &P = c->pcount;
        P.set = si;
        P.s = s;
        P.draws = draws;
        P.T = T;
        P.win_base = win_base;
        P.ntiles = ntiles;
        P.fuse = fuse;
        P.state = pass_state(c);
        P.active = true;
        if (!(defer && c->pair_hint)) return resolve_count(c);
    }
    return PRK_OK;
}

// The entry count of the pending pass (PendingCount): stats, the next
// frame's capacity and tile; an over-capacity pass drew nothing (empty bins;
// with a fused clear its k_pix wrote the clear values, which the re-run
// writes again) and is re-run with room for every entry, with the state it
// was queued with.
static int resolve_count(prk_context *c) {
    prk_context::PendingCount &P = c->pcount;
    if (!P.active) return PRK_OK;
    P.active = false;
    PRK_TRY(hipSetDevice(c->device));
    prk_context::BinSet &B = c->bset[P.set];
    PRK_TRY(hipEventSynchronize(B.counted_ev));
    const uint32_t total = B.h_info[0];
    c->stats.bin_entries = total;
    c->pair_hint = total;
    const PassState &Q = P.state;
    if (c->tile_auto && !c->auto_small && Q.tile_w == 256 && total < 64u * P.ntiles &&
        8u * P.ntiles <= prk_cs_max_tiles()) {  // (32x8 tiles stay within the counting sort)
        c->auto_small = total < 8u * P.ntiles ? 64 : 32;  // (from the next frame on)
        c->auto_T = P.T;
        c->auto_px = Q.W * (Q.row1 - Q.row0);
    }
    // (a row band's entries against its share of the triangles, T * rows / H)
    if (c->tile_auto && !c->auto_small && !c->auto_wide && Q.tile_w == 256 && Q.tile_h == 8 && P.T && Q.H > 0 &&
        2ull * total * (uint64_t)Q.H >= 9ull * P.T * (uint64_t)std::max(1, Q.row1 - Q.row0) &&
        std::all_of(P.draws.begin(), P.draws.end(), [](const prk::DrawRec &d) { return d.mode == prk::MODE_AVX; })) {
        c->auto_wide = 512;  // (from the next frame on)
        c->auto_T = P.T;
        c->auto_px = Q.W * (Q.row1 - Q.row0);
    }
    if (!B.h_info[1]) return PRK_OK;
    if (total > prk_cs_max_pairs()) return PRK_ERR_LIMIT;  // 29-bit pair index in the bins
    // re-run with the pass's own state, then give the caller's back
    const PassState callers = pass_state(c);
    apply_pass_state(c, P.state);
    c->clear_pending = P.fuse;
    const std::vector<prk::DrawRec> draws = std::move(P.draws);
    const int rc = flush_tris(c, P.s, draws, P.T, P.win_base);
    // (the re-run ran with the pass's own debug flag, P.state: a prk_set_debug
    // since the flush does not change what prk_debug_bins answers for)
    if (rc == PRK_OK) c->bdbg.rerun = true;
    else c->bdbg.valid = false;
    c->read_rec = hipEventRecord(c->read_ev, P.s) == hipSuccess;  // (geometry writes wait for the re-run)
    c->z_early = false;  // (a re-run: the download takes z after everything)
    apply_pass_state(c, callers);
    return rc;
}

// ---- the span pass (flush_spans) and its phases ----------------------------
namespace {
struct HandleRun {  // a prk_draw_span_records draw: its launch after the thread walks
    uint32_t draw, g0, obj0, first, n;
    const void *sp;
};
// Walk groups: per mode, the large objects by the workgroup their list needs
// (slot_threads(lcap) >= most + 2, lcap <= the device's), the rest (more than
// lcap, or rows past k_obj_maxact's histogram) the huge-object walk or one
// wave each with the list in a pool slice.
struct WalkGroup {
    int32_t mode;
    uint32_t lcap, start, count;
    bool big;           // the huge-object walk (k_obj_walk_big / k_obj_walk_lds)
    uint32_t max_rows;  // (big: its objects' most rows)
    bool lds;           // (big: the list in LDS, k_obj_walk_lds)
};
// The chunked walk's groups: its objects by (mode, LDS capacity class).
struct PrGroup {
    int32_t mode;
    uint32_t cap, start, count, max_chunks;
};
// What classify() decides about a pass's large objects (with the h_cls tables).
struct ObjWalks {
    std::vector<WalkGroup> groups;
    std::vector<PrGroup> prgroups;
    uint64_t pool = 0;  // the pool slices' ints
    uint32_t npr = 0, pr_rows = 0, pr_chunks = 0, pr_max_edges = 0;  // the chunked walk's objects, rows, chunks
    uint64_t pr_ents = 0;
};
// The large objects of a pass by mode (the object, its edges), and as the
// readback lists them: mode after mode (SpanScratch h_big_gl's order).
struct BigObjs {
    std::vector<uint32_t> obj[prk::MODE_COUNT], edges[prk::MODE_COUNT];
    std::vector<uint32_t> all_edges;
};
// A host table of the pass in the pinned staging, and where the one upload puts it.
struct StagePart {
    const void *src = nullptr;
    size_t bytes = 0, off = 0;
};

// The walk groups of a pass, from what k_obj_maxact read back (h.most, rows,
// ents): the objects of every group into h.big / off / cap / meta, one group
// after the other.  Objects whose lists outgrow the slot walk's LDS classes
// take the huge-object walk (a workgroup of 1024: k_obj_walk_lds with the
// whole list in LDS when it fits prk_big_lds_cap() entries, else
// k_obj_walk_big with it in device memory) when their sizes are known and
// fit, else one wave each (k_obj_walk_wave).
static void classify_walks(const SpanSwitches &sw, uint32_t lcap, const BigObjs &B, const ClsView &h, ObjWalks &out,
                           uint32_t routes[9]) {
    uint32_t k = 0, b = 0;
    for (int mo = 0; mo < prk::MODE_COUNT; ++mo) {
        const std::vector<uint32_t> &objs = B.obj[mo];
        const uint32_t b0 = b;
        for (int ci = 0; ci <= 7; ++ci) {  // ci 5 / 6: the huge-object walk in LDS / device memory, 7: one wave each
            const uint32_t capc = ci < 5 ? kAdvWgCaps[ci] : 0u;
            if (ci < 5 && capc > lcap) continue;
            const uint32_t start = k;
            uint32_t gmax = 0;  // (the huge walk: its objects' most rows)
            for (uint32_t i = 0; i < objs.size(); ++i) {
                const uint32_t bi = b0 + i;
                const int32_t most = h.most[bi];
                // (big_min is a test switch of these groups alone: it sends
                // objects that fit a slot class to the walks past them; the
                // chunked walk's groups keep the plain rule)
                if ((most <= sw.big_min ? slot_class(most, lcap) : 0u) != capc) continue;
                const int32_t rows = h.rows[bi], ents = h.ents[bi];
                const bool huge = ci == 5 || ci == 6;
                if (ci >= 5) {
                    const bool hb = sw.big && most > 0 && (uint32_t)most <= prk_big_max_entries() && rows > 0 &&
                                    rows < INT32_MAX && ents >= 0 && ents < INT32_MAX && objs.size() <= 65535;
                    const bool hl = hb && sw.ldswalk && (uint32_t)most <= prk_big_lds_cap() && rows < 16000;
                    if ((hb ? (hl ? 5 : 6) : 7) != ci) continue;
                }
                const uint32_t cap = huge ? (uint32_t)most : B.edges[mo][i];
                if (huge) out.pool = (out.pool + 3) & ~3ull;  // (16-B aligned slices)
                h.big[k] = objs[i];
                h.off[k] = capc ? 0ull : out.pool;
                h.cap[k] = capc ? 0u : cap;
                h.meta[2 * k] = huge ? (uint32_t)rows : 0u;
                h.meta[2 * k + 1] = huge ? (uint32_t)ents : 0u;
                if (!capc)
                    out.pool += huge ? prk_big_slice_ints(cap, (uint32_t)rows, (uint32_t)ents)
                                     : (uint64_t)kWaveListArrays * (cap + 2);
                if (huge) gmax = std::max(gmax, (uint32_t)rows);
                ++routes[ci];
                ++k;
            }
            if (k > start) out.groups.push_back(WalkGroup{mo, capc, start, k - start, ci == 5 || ci == 6, gmax, ci == 5});
        }
        b += (uint32_t)objs.size();
    }
}

// The chunked walk (prk_spans.hip k_pr_*): the large objects walked with
// their lists in LDS whose rows fit its histogram, by (mode, slot class) as
// the walk groups; its table into h.pr, its objects by group into h.grp.
static void classify_chunked(const SpanSwitches &sw, uint32_t lcap, const BigObjs &B, const std::vector<uint32_t> &big_gl,
                      const ClsView &h, ObjWalks &out) {
    const uint32_t K = prk_pr_chunk_rows();
    uint32_t b = 0;
    for (int mo = 0; sw.rows && mo < prk::MODE_COUNT; ++mo) {
        const uint32_t b0 = b;
        for (const uint32_t capc : kAdvWgCaps) {
            if (capc > lcap) continue;
            PrGroup g{mo, capc, out.npr, 0, 0};
            for (uint32_t i = 0; i < B.obj[mo].size(); ++i) {
                const uint32_t bi = b0 + i;
                const int32_t most = h.most[bi], rows = h.rows[bi];
                if (most <= 0 || most > prk_pr_max_row_entries() || rows <= 0 || rows > prk_pr_max_rows()) continue;
                if (slot_class(most, lcap) != capc) continue;
                const uint32_t nch = ((uint32_t)rows + K - 1) / K;
                const uint64_t ents = (uint64_t)most * nch;
                if (out.pr_ents + ents > kPrMaxEntries || out.npr >= 65535 ||
                    (uint64_t)out.pr_rows + rows + 1 > 0x7FFFFFFFull)
                    continue;
                uint32_t *q = h.pr + 8 * (size_t)out.npr;
                q[0] = big_gl[bi];
                q[1] = out.pr_rows;
                q[2] = (uint32_t)rows;
                q[3] = out.pr_chunks;
                q[4] = (uint32_t)most;
                q[5] = (uint32_t)out.pr_ents;
                q[6] = q[7] = 0;
                h.grp[out.npr] = out.npr;
                out.pr_rows += (uint32_t)rows + 1;
                out.pr_chunks += nch;
                out.pr_ents += ents;
                out.pr_max_edges = std::max(out.pr_max_edges, B.all_edges[bi]);
                g.max_chunks = std::max(g.max_chunks, nch);
                ++g.count;
                ++out.npr;
            }
            if (g.count) out.prgroups.push_back(g);
        }
        b += (uint32_t)B.obj[mo].size();
    }
}

// One span pass: what its phases share.  flush_spans runs them in order.
struct SpanPass {
    prk_context *c;
    prk_context::SpanScratch &S;
    hipStream_t s;
    const std::vector<prk::DrawRec> &draws;
    const SpanSwitches sw;
    prk::FrameParams fp;
    uint32_t ntiles = 0;
    uint32_t lcap = 0;  // LDS list capacity of the wave walk (edges)
    // plan(): objects, kind-0 objects, triangles; the prk_draw_edges edges.
    // The pass's batches (prk_draw_edge_lists) take consecutive records and
    // lists of the frame's: [le0, le0 + nhe) and [ll0, ll0 + nhl).  With the
    // handle draws' (prk_draw_records) the pass has nle batch edges and nll
    // batch lists, in submission order.
    uint32_t nobj = 0, nk0 = 0, nt = 0, nbig = 0, le0 = 0, ll0 = 0, nsegblk = 0;
    uint64_t nk1 = 0, nle = 0, nll = 0, nhe = 0, nhl = 0;
    uint64_t maxn = 1, small_tris = 0, small_ledges = 0;
    uint32_t pbits = 0, ybits = 0, obits = 0;  // MergeSort key: (object, min(YMin, H), recursion path)
    bool handles = false;                      // a pass with handle draws (prk_draw_records)
    bool thread_links = false;  // a thread-walked triangle object small enough for LDS list links
    BigObjs big;
    std::vector<HandleRun> hruns;
    std::vector<uint8_t> seg_staged;  // per h_segs segment: its records are staged ones
    // upload(): the staged tables, in the staging's order
    StagePart st_draws, st_texs, st_runs, st_big, st_k1src, st_edges, st_spans, st_lcnt, st_lflag, st_ledges, st_lseg,
        st_lsrc;
    // edges(): the pass's span kinds (bit per Mode), the sort and the small objects' walk
    uint32_t modes = 0;
    bool scalar = false, local_sort = false, segmented = false;
    uint64_t max_segs = 0;
    void *d_objs = nullptr;
    uint32_t *escan = nullptr;
    const uint32_t *total0p = nullptr;
    unsigned long long *oslot = nullptr;
    // sizes(): the span slots; the classification block
    uint32_t nslot = 0;
    ClsLayout cls;
    ObjWalks walks;
    const uint32_t *d_prstat = nullptr;  // the chunked walk ran: its objects' status

    SpanPass(prk_context *ctx, hipStream_t stream, const std::vector<prk::DrawRec> &d)
        : c(ctx), S(ctx->spans), s(stream), draws(d) {}
    void *dev(const StagePart &p) const { return static_cast<char *>(S.d_stage.p) + p.off; }
    void *srecs() const { return scalar ? S.d_srecs.p : nullptr; }  // DrawModel span records
    void *wy() const { return segmented ? S.d_wy.p : nullptr; }
    int plan();
    int upload();
    int edges();
    int sizes();
    void classify();
    int chunked();
    int walk();
    int bin_shade(uint32_t T);
};

// The loop over the draws, host only.  Objects in submission order (ObjDesc
// kinds: prk_spans.hip): kind 0 objects' triangles numbered 0..ntri-1 in order
// (FillEdgeTable runs per triangle), caller edge lists' edges after the
// triangles' edges.  Objects of kObjWaveTris triangles or more are large.
// (the objects themselves are expanded on the device from runs: a draw of
// kind 0 is a run of ceil(tris / obj_tris) objects, kind 2 one of its spans;
// only the large objects are listed here)
int SpanPass::plan() {
    S.h_runs.clear();
    S.h_big_gl.clear();
    S.h_k1src.clear();
    S.h_segs.clear();
    S.h_lsrc.clear();
    uint64_t ntri = 0, nobj64 = 0, nk064 = 0;
    for (const prk::DrawRec &d : draws) handles = handles || d.src_kind == 4;
    // only a pass with handle draws lists the segments of its batch edges
    // (h_segs; a staged segment's src: its record among the staged ones, until
    // the staging has its address)
    auto add_seg = [&](uint64_t src, bool staged, uint32_t n) {
        if (!handles || !n) return;
        if (!S.h_segs.empty() && seg_staged.back() == (staged ? 1 : 0) &&
            reinterpret_cast<uintptr_t>(S.h_segs.back().src) + sizeof(prk_edge) * (uint64_t)S.h_segs.back().n == src) {
            S.h_segs.back().n += n;  // (the records go on where the previous segment's end)
            return;
        }
        S.h_segs.push_back(PrepSeg{reinterpret_cast<const uint32_t *>(src), (uint32_t)nle, n, 0u, 0u});
        seg_staged.push_back(staged ? 1 : 0);
    };
    for (uint32_t di = 0; di < draws.size(); ++di) {
        const prk::DrawRec &d = draws[di];
        if (d.src_kind == 1) {
            S.h_runs.push_back(ObjRun{1u, di, (uint32_t)nobj64, 1u, 0u, 0u, d.first_global, 0u, 0u, d.src_off, d.src_n,
                                      (uint32_t)nk1});
            for (uint32_t e = 0; e < d.src_n; ++e) S.h_k1src.push_back(d.src_off + e);
            nk1 += d.src_n;
            nobj64 += 1;
        } else if (d.src_kind == 2) {
            if (!d.src_n) continue;
            S.h_runs.push_back(ObjRun{2u, di, (uint32_t)nobj64, d.src_n, 0u, 0u, d.first_global, 0u, 0u, d.src_off, 0u, 0u});
            nobj64 += d.src_n;
        } else if (d.src_kind == 5) {
            // the spans stay where they are: a run of one-slot objects that
            // k_span_handle_walk fills from the handle's buffer
            if (!d.src_n) continue;
            S.h_runs.push_back(ObjRun{4u, di, (uint32_t)nobj64, d.src_n, 0u, 0u, d.first_global, 0u, 0u, d.src_off, 0u, 0u});
            hruns.push_back(HandleRun{di, d.first_global, (uint32_t)nobj64, d.src_off, d.src_n, c->sbatches[d.geom].sp});
            nobj64 += d.src_n;
        } else if (d.src_kind == 3 || d.src_kind == 4) {
            // one run for the batch; its sorted lists are routed like triangle
            // objects of as many edges (k1off: the first batch edge's slot, below).
            // The run's list tables: `per` on in the staged ones (tri0 0), or
            // in those of handle source tri0 - 1 (k_list_tables).
            const uint32_t *lcnt, *lflag;
            uint32_t src = 0, at;
            if (d.src_kind == 3) {
                if (!nhl) {
                    le0 = d.src_off;
                    ll0 = d.geom_tri0;
                }
                lcnt = c->pend_lcnt.data() + d.geom_tri0;
                lflag = c->pend_lflag.data() + d.geom_tri0;
                at = (uint32_t)nhl;
                add_seg(sizeof(prk_edge) * nhe, true, d.src_n);
                nhl += d.tri_count;
                nhe += d.src_n;
            } else {
                const Records &R = c->recs[d.geom];
                lcnt = R.cnt.data() + d.geom_tri0;
                lflag = R.flag.data() + d.geom_tri0;
                at = d.geom_tri0;
                for (src = 0; src < S.h_lsrc.size() && S.h_lsrc[src].cnt != R.d_cnt(); ++src) {}
                if (src == S.h_lsrc.size()) S.h_lsrc.push_back(ListSrc{R.d_cnt(), R.d_flag()});
                ++src;
                add_seg(reinterpret_cast<uintptr_t>(R.rec) + sizeof(prk_edge) * (uint64_t)d.src_off, false, d.src_n);
            }
            S.h_runs.push_back(ObjRun{3u, di, (uint32_t)nobj64, d.tri_count, handles ? at : 0u, 0u, d.first_global,
                                      src, (uint32_t)nll, 0u, 0u, 0u});
            for (uint32_t j = 0; j < d.tri_count; ++j) {
                const uint32_t n = lcnt[j];
                if (!lflag[j]) continue;
                if (n >= kObjWaveEdges) {
                    big.obj[d.mode].push_back((uint32_t)(nobj64 + j));
                    big.edges[d.mode].push_back(n);
                } else {
                    small_ledges += n;
                    thread_links = thread_links || (n && n <= prk_obj_link_cap());
                }
            }
            nobj64 += d.tri_count;
            nll += d.tri_count;
            nle += d.src_n;
        } else {
            const uint32_t per = std::max<uint32_t>(1u, d.obj_tris);
            const uint32_t cnt = (uint32_t)(((uint64_t)d.tri_count + per - 1) / per);
            if (!cnt) continue;
            S.h_runs.push_back(ObjRun{0u, di, (uint32_t)nobj64, cnt, per, d.tri_count, d.first_global, (uint32_t)ntri,
                                      (uint32_t)nk064, 0u, 0u, 0u});
            maxn = std::max<uint64_t>(maxn, 3ull * std::min(per, d.tri_count));  // the most its FillEdgeTable writes
            if (per >= kObjWaveTris) {
                for (uint32_t j = 0; j < cnt; ++j) {
                    const uint32_t n = std::min(per, d.tri_count - j * per);
                    if (n >= kObjWaveTris) {
                        big.obj[d.mode].push_back((uint32_t)(nobj64 + j));
                        big.edges[d.mode].push_back(3u * n);
                    } else {
                        small_tris += n;
                        thread_links = thread_links || 3ull * n <= prk_obj_link_cap();
                    }
                }
            } else {
                const uint32_t rem = d.tri_count % per;
                small_tris += d.tri_count;
                thread_links = thread_links || (d.tri_count >= per && 3ull * per <= prk_obj_link_cap()) ||
                               (rem && 3ull * rem <= prk_obj_link_cap());
            }
            nobj64 += cnt;
            nk064 += cnt;
            ntri += d.tri_count;
        }
        if (nobj64 >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    }
    for (int mo = 0; mo < prk::MODE_COUNT; ++mo)  // the large objects, by mode (their walk groups: after the readback)
        for (size_t i = 0; i < big.obj[mo].size(); ++i) {
            S.h_big_gl.push_back(big.obj[mo][i]);
            big.all_edges.push_back(big.edges[mo][i]);
        }
    // edge slots (3 per triangle + the caller edges) are indexed by 31 bits
    if (3 * ntri + nk1 + nle >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    for (ObjRun &r : S.h_runs)  // the batch edges' slots follow the prk_draw_edges lists'
        if (r.kind == 3) r.k1off = (uint32_t)nk1;
    S.h_lcnt.assign(c->pend_lcnt.begin() + ll0, c->pend_lcnt.begin() + ll0 + nhl);
    S.h_lcnt.push_back(0u);  // (the scan's total)
    for (PrepSeg &sg : S.h_segs) {
        sg.blk0 = nsegblk;
        nsegblk += (sg.n + kPrepEdges - 1) / kPrepEdges;
    }
    nobj = (uint32_t)nobj64;
    nk0 = (uint32_t)nk064;
    nt = (uint32_t)ntri;
    nbig = (uint32_t)S.h_big_gl.size();
    // MergeSort key: (object, min(YMin, H), recursion path) in one radix sort
    auto bitlen = [](uint64_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b; };
    pbits = bitlen(maxn) + 1;
    ybits = std::max(1u, bitlen((uint64_t)c->H));
    obits = std::max(1u, bitlen(nk0 > 0 ? nk0 - 1 : 0));
    if (obits + ybits + pbits > 64) return PRK_ERR_LIMIT;
    S.h_texs.resize(c->texs.size());
    for (size_t i = 0; i < S.h_texs.size(); ++i)
        S.h_texs[i] = prk::TexRec{c->texs[i].mem, c->texs[i].w, c->texs[i].h, c->texs[i].pitch, c->texs[i].filter};
    S.h_draws = draws;
    return PRK_OK;
}

// The pass's host tables go up in one copy from pinned staging (a pageable
// hipMemcpyAsync per table held the host for each).
// (the scratch is reused frame to frame: stream order on s covers it)
int SpanPass::upload() {
    st_draws = {S.h_draws.data(), S.h_draws.size() * sizeof(prk::DrawRec)};
    st_texs = {S.h_texs.data(), S.h_texs.size() * sizeof(prk::TexRec)};
    st_runs = {S.h_runs.data(), S.h_runs.size() * sizeof(ObjRun)};
    st_big = {S.h_big_gl.data(), S.h_big_gl.size() * 4};
    st_k1src = {S.h_k1src.data(), S.h_k1src.size() * 4};
    st_edges = {c->pend_edges.data(), c->pend_edges.size() * sizeof(prk_edge)};
    st_spans = {c->pend_spans.data(), c->pend_spans.size() * sizeof(prk_span)};
    st_lcnt = {S.h_lcnt.data(), nhl ? S.h_lcnt.size() * 4 : 0};
    st_lflag = {c->pend_lflag.data() + ll0, (size_t)nhl * 4};
    st_ledges = {c->pend_ledges.data() + le0, (size_t)nhe * sizeof(prk_edge)};
    st_lseg = {S.h_segs.data(), S.h_segs.size() * sizeof(PrepSeg)};
    st_lsrc = {S.h_lsrc.data(), S.h_lsrc.size() * sizeof(ListSrc)};
    StagePart *parts[] = {&st_draws, &st_texs,  &st_runs,   &st_big,  &st_k1src, &st_edges,
                          &st_spans, &st_lcnt, &st_lflag, &st_ledges, &st_lseg, &st_lsrc};
    size_t stage_bytes = 0;
    for (StagePart *pt : parts) {
        pt->off = stage_bytes;
        stage_bytes = (stage_bytes + pt->bytes + 255) & ~(size_t)255;
    }
    stage_bytes = std::max<size_t>(stage_bytes, 256);
    S.last_stage_bytes = stage_bytes;
    if (!S.stage_ev) PRK_TRY(hipEventCreateWithFlags(&S.stage_ev, hipEventDisableTiming));
    if (S.stage_busy) {  // the previous pass's upload still reads the staging
        PRK_TRY(hipEventSynchronize(S.stage_ev));
        S.stage_busy = false;
    }
    if (stage_bytes > S.stage_cap) {
        if (S.h_stage) (void)hipHostFree(S.h_stage);
        S.h_stage = nullptr;
        S.stage_cap = 0;
        const size_t want = stage_bytes + stage_bytes / 4;
        PRK_TRY(hipHostMalloc((void **)&S.h_stage, want, hipHostMallocDefault));
        S.stage_cap = want;
    }
    PRK_TRY(S.d_stage.ensure(stage_bytes));
    for (size_t i = 0; i < S.h_segs.size(); ++i)  // the staged segments' records, where the staging puts them
        if (seg_staged[i])  // (src held the record's byte offset till now)
            S.h_segs[i].src = reinterpret_cast<const uint32_t *>(static_cast<const char *>(dev(st_ledges)) +
                                                                 reinterpret_cast<uintptr_t>(S.h_segs[i].src));
    for (const StagePart *pt : parts)
        if (pt->bytes && pt->src) std::memcpy(S.h_stage + pt->off, pt->src, pt->bytes);
    PRK_TRY(hipMemcpyAsync(S.d_stage.p, S.h_stage, stage_bytes, hipMemcpyHostToDevice, s));
    PRK_TRY(hipEventRecord(S.stage_ev, s));
    S.stage_busy = true;
    fp.draws = (const prk::DrawRec *)dev(st_draws);
    fp.texs = (const prk::TexRec *)dev(st_texs);
    fp.draw0 = draws[0];
    fp.tex0 = prk::TexRec{};
    if (fp.draw0.tex >= 0 && (size_t)fp.draw0.tex < S.h_texs.size()) fp.tex0 = S.h_texs[fp.draw0.tex];
    return PRK_OK;
}

// The object tables, FillEdgeTable per triangle (counts, scans, edges +
// MergeSort keys), the sort, the walk's working copy, each object's bound
// and its scan into the objects' first span slots.
int SpanPass::edges() {
    // the objects (ObjDesc), the kind-0 objects' indices and first triangles
    PRK_TRY(S.d_objtab.ensure((size_t)std::max<uint32_t>(nobj, 1) * sizeof(ObjDesc)));
    PRK_TRY(S.d_k0tab.ensure((size_t)std::max<uint32_t>(nk0, 1) * 8));
    d_objs = S.d_objtab.p;
    uint32_t *k0tab = (uint32_t *)S.d_k0tab.p;
    const uint32_t *d_k0obj = k0tab, *d_k0tri0 = k0tab + nk0;
    // the batch lists' first edges: the scan of their counts
    const uint32_t nlist = (uint32_t)nll, nledge = (uint32_t)nle;
    uint32_t *lscan = nullptr, *lobj = nullptr;
    const uint32_t *d_lcnt = (const uint32_t *)dev(st_lcnt), *d_lflag = (const uint32_t *)dev(st_lflag);
    if (nlist) {
        PRK_TRY(S.d_lscan.ensure(((size_t)nlist + 1) * 4));
        PRK_TRY(S.d_lobj.ensure((size_t)nlist * 4));
        PRK_TRY(S.d_lrows.ensure((size_t)nlist * 8));
        lscan = (uint32_t *)S.d_lscan.p;
        lobj = (uint32_t *)S.d_lobj.p;
        if (handles) {  // the lists' tables from their sources, on the device
            PRK_TRY(S.d_ltab.ensure((2 * (size_t)nlist + 1) * 4));
            uint32_t *lt = (uint32_t *)S.d_ltab.p;
            PRK_TRY(prk_list_tables(dev(st_runs), (uint32_t)S.h_runs.size(), nobj, d_lcnt, d_lflag, dev(st_lsrc), nlist,
                                    lt, lt + nlist + 1, s));
            d_lcnt = lt;
            d_lflag = lt + nlist + 1;
        }
        PRK_TRY(scan_u32(S.d_temp, d_lcnt, lscan, nlist + 1, s));
    }
    PRK_TRY(prk_obj_tables(dev(st_runs), (uint32_t)S.h_runs.size(), nobj, kObjWaveTris, d_objs, k0tab, k0tab + nk0,
                           d_lcnt, d_lflag, lscan, kObjWaveEdges, lobj, s));
    const uint32_t *d_k1src = (const uint32_t *)dev(st_k1src);
    for (const auto &d : draws) modes |= 1u << d.mode;
    scalar = (modes & ~(1u << prk::MODE_AVX)) != 0;
    // FillEdgeTable per triangle: counts, scans, edges + MergeSort keys.
    const size_t es = std::max<size_t>(3 * (size_t)nt, 1);
    PRK_TRY(S.d_ecnt.ensure(((size_t)nt + 1) * 4));
    PRK_TRY(S.d_escan.ensure(((size_t)nt + 1) * 4));
    PRK_TRY(S.d_rcnt.ensure(((size_t)nt + 1) * 8));
    PRK_TRY(S.d_rscan.ensure(((size_t)nt + 1) * 8));
    PRK_TRY(S.d_edges.ensure(es * kObjEdgeBytes));
    PRK_TRY(S.d_ekeys.ensure(es * 8));
    PRK_TRY(S.d_ekeys2.ensure(es * 8));
    PRK_TRY(S.d_evals.ensure(es * 4));
    PRK_TRY(S.d_ord.ensure(es * 4));
    PRK_TRY(S.d_err.ensure(16));
    PRK_TRY(hipMemsetAsync(S.d_err.p, 0, 16, s));  // (error bits, then the chunked walk's tally)
    escan = (uint32_t *)S.d_escan.p;
    uint32_t *ord = (uint32_t *)S.d_ord.p;
    unsigned long long *rscan = (unsigned long long *)S.d_rscan.p;
    total0p = escan + nt;
    if (nt) {
        PRK_TRY(prk_objtri_count(&fp, d_objs, d_k0obj, d_k0tri0, nk0,
                                 nt, (uint32_t *)S.d_ecnt.p, (unsigned long long *)S.d_rcnt.p, s));
    } else {
        PRK_TRY(hipMemsetAsync(S.d_ecnt.p, 0, 4, s));
        PRK_TRY(hipMemsetAsync(S.d_rcnt.p, 0, 8, s));
    }
    PRK_TRY(scan_u32(S.d_temp, (const uint32_t *)S.d_ecnt.p, escan, nt + 1, s));
    PRK_TRY(scan_u64(S.d_temp, (const unsigned long long *)S.d_rcnt.p, rscan, nt + 1, s));
    // MergeSort of every object: per object when none has more than 64
    // edges (k_obj_sort_local, with the gather), else one radix sort of the
    // padded keys (prk_spans.hip)
    local_sort = nt && maxn <= 64 && sw.local_sort;
    PRK_TRY(prk_objtri_emit(&fp, d_objs, d_k0obj, d_k0tri0, nk0, nt, escan, pbits, ybits, c->H, S.d_edges.p,
                            S.d_ekeys.p, (uint32_t *)S.d_evals.p, local_sort ? 0 : 1, s));
    if (nt && !local_sort)
        PRK_TRY(obj_sort(S.d_temp, S.d_ekeys.p, (uint32_t *)S.d_evals.p, S.d_ekeys2.p, ord, 3 * nt,
                         obits + ybits + pbits, s));
    PRK_TRY(S.d_bound.ensure(((size_t)nobj + 1) * 8));
    PRK_TRY(S.d_oslot.ensure(((size_t)nobj + 1) * 8));
    oslot = (unsigned long long *)S.d_oslot.p;
    // The walk's working copy (the triangle edges, the prk_draw_edges lists,
    // the batch lists).
    const uint32_t nwork = 3 * nt + (uint32_t)nk1 + nledge;
    PRK_TRY(S.d_work.ensure(std::max<size_t>(nwork, 1) * kObjEdgeBytes));
    // The small triangle objects' segments (prk_spans.hip k_obj_seg, walk()):
    // a thread per stretch of rows with a non-empty list.
    max_segs = 3 * small_tris + small_ledges;  // (a segment has an edge at least)
    segmented = max_segs && max_segs < 0x7FFFFFFFull && sw.segments;
    if (segmented) PRK_TRY(S.d_wy.ensure((size_t)std::max<uint32_t>(nwork, 1) * 8));
    if (local_sort)
        PRK_TRY(prk_obj_sort_local(d_objs, d_k0obj, nk0, escan, S.d_ekeys.p, S.d_edges.p, S.d_work.p, wy(),
                                   (uint32_t *)S.d_err.p, s));
    if (!local_sort || nk1)
        PRK_TRY(prk_obj_gather(S.d_edges.p, local_sort ? nullptr : ord, total0p, dev(st_edges), d_k1src, (uint32_t)nk1,
                               S.d_work.p, 3 * nt + (uint32_t)nk1, wy(), s));
    // the batch lists' records into it, with their lists' row sums; then the
    // span slots: each object's bound, exclusive-scanned into its first slot
    if (handles)
        PRK_TRY(prk_list_prep_segs(&fp, dev(st_lseg), (uint32_t)S.h_segs.size(), nsegblk, lscan, nlist, lobj, d_objs,
                                   total0p, (uint32_t)nk1, S.d_work.p, wy(), (unsigned long long *)S.d_lrows.p, s));
    else
        PRK_TRY(prk_list_prep(&fp, dev(st_ledges), nledge, lscan, nlist, lobj, d_objs, total0p, (uint32_t)nk1,
                              S.d_work.p, wy(), (unsigned long long *)S.d_lrows.p, s));
    PRK_TRY(prk_obj_bound(&fp, d_objs, nobj, rscan, dev(st_edges), (const unsigned long long *)S.d_lrows.p,
                          (unsigned long long *)S.d_bound.p, s));
    PRK_TRY(scan_u64(S.d_temp, (const unsigned long long *)S.d_bound.p, oslot, nobj + 1, s));
    return PRK_OK;
}

// Each large object's most active edges, rows and entries (they size its
// walk), read back with the slot total: the pass's first wait.  Then the
// span slots' buffers.
int SpanPass::sizes() {
    cls = ClsLayout(nbig);
    if (cls.alloc_bytes() > S.cls_cap) {
        if (S.h_cls) (void)hipHostFree(S.h_cls);
        S.h_cls = nullptr;
        S.cls_cap = 0;
        const size_t want = cls.alloc_bytes() + cls.alloc_bytes() / 4;
        PRK_TRY(hipHostMalloc((void **)&S.h_cls, want, hipHostMallocDefault));
        S.cls_cap = want;
    }
    if (nbig) {
        const uint32_t *d_big = (const uint32_t *)dev(st_big);
        PRK_TRY(S.d_most.ensure((size_t)nbig * 12));
        PRK_TRY(prk_obj_maxact(&fp, d_objs, d_big, nbig, escan, total0p, S.d_work.p, (int32_t *)S.d_most.p,
                               sw.huge_edges, s));
        for (uint32_t &r : S.walk_routes) r = 0;  // (prk_debug_walk_routes: this pass's)
        for (uint32_t b = 0; b < nbig; ++b)  // (objects of sw.huge_edges edges or more: many workgroups each)
            if (big.all_edges[b] >= sw.huge_edges) {
                ++S.walk_routes[8];
                PRK_TRY(S.d_mhuge.ensure(prk_maxact_huge_scratch()));
                PRK_TRY(prk_obj_maxact_huge(&fp, d_objs, d_big, b, nbig, big.all_edges[b], escan, total0p, S.d_work.p,
                                            (int32_t *)S.d_most.p, S.d_mhuge.p, s));
            }
        PRK_TRY(hipMemcpyAsync(S.h_cls, S.d_most.p, (size_t)nbig * 12, hipMemcpyDeviceToHost, s));
    }
    PRK_TRY(hipMemcpyAsync(S.h_rb, oslot + nobj, 8, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    uint64_t nslot64;
    std::memcpy(&nslot64, S.h_rb, 8);
    if (nslot64 >= prk::kMaxPairs) return PRK_ERR_LIMIT;  // 31-bit span tags
    nslot = (uint32_t)nslot64;
    const size_t ns = std::max<uint32_t>(nslot, 1);
    PRK_TRY(S.d_recs.ensure(ns * 64));
    PRK_TRY(S.d_pos.ensure(ns * 16));
    PRK_TRY(S.d_span_tri.ensure(ns * 4));
    if (scalar) PRK_TRY(S.d_srecs.ensure(ns * kScSpanRecBytes));
    if (nbig) PRK_TRY(S.d_raw.ensure(ns * kPairRawBytes));  // the slot walks' pairs
    // slots no span takes stay row -1: binned nowhere.  Without large objects
    // every slot belongs to the thread or segment walks (walk_object,
    // k_obj_seg), which mark their unused ones themselves (C3b as 16-triangle
    // objects: ~21 M slots, a 0.34-GB memset); the large objects' walks rely
    // on this one.
    if (nbig || sw.pos_memset) PRK_TRY(hipMemsetAsync(S.d_pos.p, 0xFF, ns * 16, s));
    return PRK_OK;
}

// The large objects' walks from the readback, on the host alone.
void SpanPass::classify() {
    const ClsView h = cls.view(S.h_cls);
    if (nbig) {
        S.walk_sizes[0] = h.most[0];
        S.walk_sizes[1] = h.rows[0];
        S.walk_sizes[2] = h.ents[0];
    }
    classify_walks(sw, lcap, big, h, walks, S.walk_routes);
    classify_chunked(sw, lcap, big, S.h_big_gl, h, walks);
}

// The chunked walk of the objects classify() gave it.  It is an
// optimisation: when its scratch (up to kPrMaxEntries * ~356 B) cannot be
// had, every object takes the workgroup walk instead (d_prstat stays null) --
// never PRK_ERR_NOMEM.
int SpanPass::chunked() {
    ObjWalks &w = walks;
    if (!w.npr) return PRK_OK;
    hipError_t ae = S.d_prstat.ensure((size_t)nobj * 4);
    if (ae == hipSuccess) ae = S.d_prrow.ensure((size_t)w.npr * 8);
    if (ae == hipSuccess) ae = S.d_prcnt.ensure((size_t)w.pr_rows * 4);
    if (ae == hipSuccess) ae = S.d_preoff.ensure((size_t)w.pr_rows * 4);
    if (ae == hipSuccess) ae = S.d_prfge.ensure((size_t)w.pr_rows * 4);
    if (ae == hipSuccess) ae = S.d_prccur.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_preendm.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_prmatch.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_prsm.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_prsidx.ensure(w.pr_ents * 4);
    if (ae == hipSuccess) ae = S.d_prkey.ensure(w.pr_ents * 16);
    if (ae == hipSuccess) ae = S.d_prest.ensure(w.pr_ents * kObjEdgeBytes);
    if (ae == hipSuccess) ae = S.d_prsst.ensure(w.pr_ents * kObjEdgeBytes);
    if (ae == hipSuccess) ae = S.d_preend.ensure(w.pr_ents * kObjEdgeBytes);
    if (ae == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        DevBuf *bufs[] = {&S.d_prsidx, &S.d_prkey, &S.d_prest, &S.d_prsst, &S.d_preend};
        for (DevBuf *b : bufs) b->release();
        w.npr = 0;
        return PRK_OK;
    }
    PRK_TRY(ae);
    PRK_TRY(hipMemsetAsync(S.d_prstat.p, 0, (size_t)nobj * 4, s));
    const ClsView d = cls.view(S.d_cls.p);
    prk::PrWalkArgs pa{};
    pa.objs = d_objs;
    pa.pro = d.pr;
    pa.npr = w.npr;
    pa.nchunks = w.pr_chunks;
    pa.max_edges = w.pr_max_edges;
    pa.escan = escan;
    pa.total0p = total0p;
    pa.work = S.d_work.p;
    pa.prrow = S.d_prrow.p;
    pa.cnt = (uint32_t *)S.d_prcnt.p;
    pa.eoff = (uint32_t *)S.d_preoff.p;
    pa.fge = (uint32_t *)S.d_prfge.p;
    pa.ccur = (uint32_t *)S.d_prccur.p;
    pa.key = S.d_prkey.p;
    pa.est = S.d_prest.p;
    pa.sst = S.d_prsst.p;
    pa.eend = S.d_preend.p;
    pa.eend_m = (uint32_t *)S.d_preendm.p;
    pa.match = (uint32_t *)S.d_prmatch.p;
    pa.sidx = (uint32_t *)S.d_prsidx.p;
    pa.s_m = (uint32_t *)S.d_prsm.p;
    pa.prstat = (uint32_t *)S.d_prstat.p;
    pa.soff = oslot;
    pa.raw = S.d_raw.p;
    pa.pos = S.d_pos.p;
    pa.span_tri = (uint32_t *)S.d_span_tri.p;
    pa.err = (uint32_t *)S.d_err.p;
    pa.warmup = sw.chunk_warmup;
    PRK_TRY(prk_pr_walk_begin(&fp, &pa, s));
    for (const PrGroup &g : w.prgroups)
        PRK_TRY(prk_pr_walk_group(&fp, &pa, g.mode, g.cap, d.grp + g.start, g.count, g.max_chunks, s));
    PRK_TRY(prk_pr_walk_end(&pa, s));
    d_prstat = (const uint32_t *)S.d_prstat.p;
    return PRK_OK;
}

// The classification's upload and every walk: the chunked walk, the small
// objects' segments and thread walk, the span handles, the walk groups; then
// the slot walks' pairs into span records.
int SpanPass::walk() {
    if (nbig) {
        PRK_TRY(S.d_cls.ensure(cls.end));
        PRK_TRY(hipMemcpyAsync(static_cast<char *>(S.d_cls.p) + cls.big, S.h_cls + cls.big, cls.upload_bytes(),
                               hipMemcpyHostToDevice, s));
        if (walks.pool) PRK_TRY(S.d_pool.ensure(walks.pool * 4));
    }
    {
        const int rc = chunked();
        if (rc != PRK_OK) return rc;
    }
    const void *d_segs = nullptr;  // (the segments)
    const uint32_t *d_nseg = nullptr;
    if (segmented) {
        PRK_TRY(S.d_segcnt.ensure(((size_t)nobj + 1) * 4));
        PRK_TRY(S.d_segoff.ensure(((size_t)nobj + 1) * 4));
        PRK_TRY(S.d_segs.ensure((size_t)max_segs * 24));  // prk_spans.hip ObjSeg
        uint32_t *segcnt = (uint32_t *)S.d_segcnt.p, *segoff = (uint32_t *)S.d_segoff.p;
        PRK_TRY(prk_obj_seg(&fp, d_objs, nobj, escan, total0p, S.d_wy.p, oslot, segcnt, segoff, nullptr, nullptr, s));
        PRK_TRY(scan_u32(S.d_temp, segcnt, segoff, nobj + 1, s));
        PRK_TRY(prk_obj_seg(&fp, d_objs, nobj, escan, total0p, S.d_wy.p, oslot, segcnt, segoff, S.d_segs.p, S.d_pos.p,
                            s));
        d_segs = S.d_segs.p;
        d_nseg = segoff + nobj;
    }
    uint32_t *span_tri = (uint32_t *)S.d_span_tri.p, *err = (uint32_t *)S.d_err.p;
    PRK_TRY(prk_obj_walk(&fp, d_objs, nobj, escan, total0p, S.d_work.p, oslot, S.d_recs.p, srecs(), S.d_pos.p, span_tri,
                         dev(st_spans), err, thread_links ? 1 : 0, d_segs, d_nseg, (uint32_t)max_segs, s));
    for (const HandleRun &h : hruns)  // the span handles' draws, from their own buffers
        PRK_TRY(prk_span_handle_walk(&fp, h.draw, h.g0, h.obj0, h.sp, h.first, h.n, oslot, S.d_recs.p, S.d_pos.p,
                                     span_tri, s));
    const ClsView d = cls.view(S.d_cls.p);
    for (const WalkGroup &g : walks.groups) {
        if (g.big)
            PRK_TRY(prk_big_walk(&fp, g.mode, g.lds ? 1 : 0, d_objs, d.big + g.start, d.off + g.start, d.cap + g.start,
                                 d.meta + 2 * (size_t)g.start, g.count, g.max_rows, (int32_t *)S.d_pool.p, escan,
                                 total0p, S.d_work.p, oslot, S.d_raw.p, S.d_pos.p, span_tri, err, d_prstat, s));
        else
            PRK_TRY(prk_obj_walk_group(&fp, g.mode, g.lcap, d_objs, d.big + g.start, d.off + g.start, d.cap + g.start,
                                       g.count, (int32_t *)S.d_pool.p, escan, total0p, S.d_work.p, oslot, S.d_recs.p,
                                       srecs(), S.d_raw.p, S.d_pos.p, span_tri, err, d_prstat, s));
    }
    if (nbig)  // the slot walks' pairs into span records
        PRK_TRY(prk_span_finish(&fp, S.d_raw.p, nslot, S.d_recs.p, srecs(), S.d_pos.p, s));
    return PRK_OK;
}

// span -> tile bin entries: the tiles' counts and their scan (the total comes
// back with the walks' status: the pass's second wait), then every span
// placed; visibility and shading.
int SpanPass::bin_shade(uint32_t T) {
    PRK_TRY(S.d_scnt.ensure(((size_t)ntiles + 1) * 4));
    PRK_TRY(S.d_offs.ensure(((size_t)ntiles + 1) * 4));
    uint32_t *tcnt = (uint32_t *)S.d_scnt.p, *toff = (uint32_t *)S.d_offs.p;
    PRK_TRY(prk_span_count(&fp, S.d_pos.p, nslot, tcnt, s));
    PRK_TRY(scan_u32(S.d_temp, tcnt, toff, ntiles + 1, s));
    PRK_TRY(hipMemcpyAsync(S.h_rb + 2, toff + ntiles, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipMemcpyAsync(S.h_rb + 3, S.d_err.p, 16, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    const uint32_t total = S.h_rb[2];
    if (S.h_rb[3]) return PRK_ERR_DEVICE;  // a walk outside its LDS list or span slots (never)
    if (sw.pr_debug)
        std::fprintf(stderr, "prk: large objects %u, chunked: taken %u done %u failed %u; chunks %u, walked again %u\n",
                     nbig, walks.npr, S.h_rb[4], S.h_rb[5], walks.pr_chunks, S.h_rb[6]);
    c->stats.objects_chunked += S.h_rb[4];
    c->stats.objects_walked += nbig - S.h_rb[4];
    c->stats.object_chunks += walks.pr_chunks;
    c->stats.object_chunks_rewalked += S.h_rb[6];
    c->stats.triangles = T;
    c->stats.tiles = ntiles;
    c->stats.bin_entries = total;
    PRK_TRY(S.d_vals_b.ensure((size_t)std::max<uint32_t>(total, 1) * 4));
    PRK_TRY(prk_span_bin(&fp, S.d_pos.p, nslot, toff, tcnt, (uint32_t *)S.d_vals_b.p, s));
    PRK_TRY(S.d_nwin.ensure((size_t)ntiles * 4));
    PRK_TRY(S.d_wtag.ensure((size_t)ntiles * fp.tile_w * fp.tile_h * 4));
    PRK_TRY(prk_launch_spans(&fp, (const uint32_t *)S.d_offs.p, (const uint32_t *)S.d_vals_b.p, S.d_pos.p, S.d_recs.p,
                             srecs(), modes, (const uint32_t *)S.d_span_tri.p, (uint32_t *)S.d_nwin.p,
                             (uint32_t *)S.d_wtag.p, s));
    return PRK_OK;
}
}  // namespace

// One pass of whole-object AETs (prk_spans.hip): FillEdgeTable per triangle,
// MergeSort per object (one radix sort), one walk of every object's AET into
// span records (each object writing into its own slots, as many as its edges'
// active rows allow), bin the spans to tiles, then visibility + shading.
// Stream-ordered on s; the host waits at the two sizes it reads back (the
// span slots in sizes(), the bin entry count in bin_shade()).
static int flush_spans(prk_context *c, hipStream_t s, const std::vector<prk::DrawRec> &draws, uint32_t T,
                       uint32_t win_base) {
    c->z_early = false;  // (k_pix / k_span_shade write a span pass's z)
    const bool fuse = c->clear_pending && T > 0;
    SpanPass P(c, s, draws);
    frame_params(c, P.fp);
    P.fp.tri_count = T;
    P.fp.ndraws = (uint32_t)draws.size();
    P.fp.win_base = win_base;
    P.ntiles = (uint32_t)(P.fp.tiles_x * P.fp.tiles_y);
    c->clear_pending = false;
    P.fp.clear_fused = fuse ? 1 : 0;
    if (T == 0) return PRK_OK;
    if (!P.S.h_rb) PRK_TRY(hipHostMalloc((void **)&P.S.h_rb, 8 * sizeof(uint32_t), hipHostMallocDefault));
    P.lcap = prk_obj_walk_lcap();
    int rc = P.plan();
    if (rc == PRK_OK) rc = P.upload();
    if (rc == PRK_OK) rc = P.edges();
    if (rc == PRK_OK) rc = P.sizes();
    if (rc != PRK_OK) return rc;
    P.classify();
    rc = P.walk();
    if (rc == PRK_OK) rc = P.bin_shade(T);
    return rc;
}


int prk_flush(prk_context *c, void *stream) {
    if (!c) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (!c->have_camera) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    {
        const int rc = resolve_count(c);  // the previous frame's count first: it may change the tile
        if (rc != PRK_OK) return rc;
    }
    if (c->tile_auto) {  // the frame's tile (see prk_context::tile_auto)
        const int64_t px = (int64_t)c->W * (c->row1 - c->row0);
        if ((c->auto_small || c->auto_wide) &&
            ((uint64_t)c->pending_tris > 2ull * c->auto_T || 2ull * c->pending_tris < c->auto_T ||
             px > 2 * (int64_t)c->auto_px || 2 * px < (int64_t)c->auto_px))
            c->auto_small = c->auto_wide = 0;  // re-decide from this frame's count
        c->tile_w = c->auto_small ? c->auto_small : (c->auto_wide ? c->auto_wide : 256);
        c->tile_h = 8;
    }
    hipStream_t s = stream ? (hipStream_t)stream : c->own_stream;
    if (c->in_wait) {  // prk_geometry_write copies still in flight: every stream of the frame waits for them
        PRK_TRY(hipStreamWaitEvent(s, c->in_ev, 0));
        PRK_TRY(hipStreamWaitEvent(c->bin_stream, c->in_ev, 0));
        PRK_TRY(hipStreamWaitEvent(c->vis_stream, c->in_ev, 0));
        c->in_wait = false;
    }
    bool any_avx = false;
    for (const auto &d : c->draws) any_avx |= d.mode == prk::MODE_AVX;
    if (any_avx && (c->W % 8)) return PRK_ERR_UNSUPPORTED;  // aligned 8-wide z load, projekt.cpp:2218
    prk::FrameParams probe;
    frame_params(c, probe);
    if (probe.tiles_x > 65535 || probe.tiles_y > 65535) return PRK_ERR_UNSUPPORTED;
    if (!c->d_prof.p) {
        PRK_TRY(c->d_prof.ensure(16 * sizeof(uint64_t)));
        PRK_TRY(hipMemsetAsync(c->d_prof.p, 0, 16 * sizeof(uint64_t), s));
    }
    if (!c->d_negz.p) {
        PRK_TRY(c->d_negz.ensure(4));
        PRK_TRY(hipMemsetAsync(c->d_negz.p, 0, 4, s));
    }
    c->z_early = false;  // (the passes below say whether the frame's last one allows it)
    c->bdbg.valid = false;  // (prk_debug_bins: this flush's last per-triangle pass, if any)
    if (c->debug) {
        PRK_TRY(c->d_winners.ensure((size_t)c->W * (c->row1 - c->row0) * 4));
        PRK_TRY(hipMemsetAsync(c->d_winners.p, 0xFF, (size_t)c->W * (c->row1 - c->row0) * 4, s));
        c->winners_valid = true;
    }
    // Passes: maximal runs of draws of one kind (per-triangle AETs, or
    // whole-object AETs); each pass z-tests against the target as the
    // previous one left it, which is the reference's sequential order.
    std::vector<prk::DrawRec> dr = std::move(c->draws);
    c->draws.clear();
    c->pending_tris = 0;
    struct Clear {  // the frame's edge / span input goes with its draws
        prk_context *c;
        ~Clear() {
            c->pend_edges.clear();
            c->pend_spans.clear();
            c->pend_ledges.clear();
            c->pend_lcnt.clear();
            c->pend_lflag.clear();
        }
    } clear_src{c};
    if (dr.empty()) return c->clear_pending ? fill_pending_clear(c, s) : PRK_OK;
    auto span_path = [](const prk::DrawRec &d) { return d.obj_tris > 1 || d.src_kind != 0; };
    size_t i = 0;
    int rc = PRK_OK;
    while (i < dr.size() && rc == PRK_OK) {
        const bool obj = span_path(dr[i]);
        size_t j = i;
        std::vector<prk::DrawRec> seg;
        uint32_t T = 0;
        const uint32_t base = dr[i].first_global;
        while (j < dr.size() && span_path(dr[j]) == obj) {
            prk::DrawRec d = dr[j];
            d.first_global -= base;
            T += d.tri_count;
            seg.push_back(d);
            ++j;
        }
        // (only the frame's last pass defers its count: a later pass z-tests
        // against this one's output, so an overflow must be re-run first)
        rc = obj ? flush_spans(c, s, seg, T, base) : flush_tris(c, s, seg, T, base, j == dr.size());
        i = j;
    }
    // the frame's last reader of the geometry (the flush stream ends every pass)
    c->read_rec = hipEventRecord(c->read_ev, s) == hipSuccess;
    return rc;
}


int prk_get_target(prk_context *c, void **color, int32_t *pitch_bytes, float **zbuf, int32_t *width,
                   int32_t *height, int32_t *row0, int32_t *row1) {
    if (!c) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (color) *color = c->color;
    if (pitch_bytes) *pitch_bytes = c->pitch;
    if (zbuf) *zbuf = c->zbuf;
    if (width) *width = c->W;
    if (height) *height = c->H;
    if (row0) *row0 = c->row0;
    if (row1) *row1 = c->row1;
    return PRK_OK;
}

int prk_get_device(prk_context *c, int32_t *device, void **stream) {
    if (!c) return PRK_ERR_ARG;
    if (device) *device = c->device;
    if (stream) *stream = (void *)c->own_stream;
    return PRK_OK;
}

// prk_dist.hip: gathers read the band's finished frame (library-internal).
// The pending count is resolved first (an overflowed frame is re-run on its
// own flush stream), then `stream` (the gather's, any stream of the
// context's device) waits for the end of the context's last frame.
__attribute__((visibility("hidden"))) int prk_resolve_pending(prk_context *c, void *stream) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (stream && c->read_rec) {
        PRK_TRY(hipSetDevice(c->device));
        PRK_TRY(hipStreamWaitEvent((hipStream_t)stream, c->read_ev, 0));
    }
    return PRK_OK;
}

int prk_resolve(prk_context *c, void *stream) { return prk_resolve_pending(c, stream); }

int prk_synchronize(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->own_stream));
    PRK_TRY(hipDeviceSynchronize());
    return PRK_OK;
}

int prk_get_stats(prk_context *c, prk_stats *out) {
    if (!c || !out) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    (void)hipSetDevice(c->device);
    for (int i = 1; i <= prk_context::kRing; ++i)  // oldest first
        harvest(c, (int)((c->frame + i) % prk_context::kRing));
    if (c->d_anomaly.p) {
        PRK_TRY(hipDeviceSynchronize());
        static_assert(offsetof(prk_stats, slow_replays) == offsetof(prk_stats, anomalies) + 4, "counter pair");
        PRK_TRY(hipMemcpy(&c->stats.anomalies, c->d_anomaly.p, 8, hipMemcpyDeviceToHost));
    }
    *out = c->stats;
    return PRK_OK;
}

int prk_download_winners(prk_context *c, int32_t *w) {
    if (!c || !w) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (!c->winners_valid || !c->d_winners.p) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    PRK_TRY(hipMemcpy(w, c->d_winners.p, (size_t)c->W * (c->row1 - c->row0) * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

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
    PRK_TRY(S.d_objtab.ensure((size_t)nobj * sizeof(ObjDesc)));
    PRK_TRY(S.d_k0tab.ensure((size_t)nobj * 8));
    void *d_objs = S.d_objtab.p;
    uint32_t *k0tab = (uint32_t *)S.d_k0tab.p;
    const uint32_t *d_k0obj = k0tab, *d_k0tri0 = k0tab + nobj;
    PRK_TRY(prk_obj_tables(static_cast<char *>(S.d_rectab.p) + kRunOff, 1, nobj, kObjWaveTris, d_objs, k0tab,
                           k0tab + nobj, nullptr, nullptr, nullptr, 0u, nullptr, s));
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
        PRK_TRY(S.d_edges.ensure(es * kObjEdgeBytes));
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
        PRK_TRY(prk_rec_emit(&fp, d_objs, d_k0obj, d_k0tri0, nobj, nt, escan, setup, pbits, S.d_edges.p,
                             S.d_ekeys.p, (uint32_t *)S.d_evals.p, local_sort ? 0 : 1, s));
        if (local_sort) {
            PRK_TRY(S.d_work.ensure(es * kObjEdgeBytes));
            PRK_TRY(prk_obj_sort_local(d_objs, d_k0obj, nobj, escan, S.d_ekeys.p, S.d_edges.p, S.d_work.p, nullptr,
                                       (uint32_t *)S.d_err.p, s));
            PRK_TRY(prk_rec_export(S.d_work.p, nullptr, total, d_out, s));
        } else {
            PRK_TRY(S.d_ekeys2.ensure(es * 8));
            PRK_TRY(S.d_ord.ensure(es * 4));
            PRK_TRY(obj_sort(S.d_temp, S.d_ekeys.p, (uint32_t *)S.d_evals.p, S.d_ekeys2.p, (uint32_t *)S.d_ord.p, 3 * nt,
                             obits + ybits + pbits, s));
            PRK_TRY(prk_rec_export(S.d_edges.p, (const uint32_t *)S.d_ord.p, total, d_out, s));
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

int prk_debug_stage_bytes(prk_context *c, uint64_t *bytes_out) {
    if (!c || !bytes_out) return PRK_ERR_ARG;
    *bytes_out = c->spans.last_stage_bytes;
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
    PRK_TRY(S.d_work.ensure((size_t)n * kObjEdgeBytes));
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
        PRK_TRY(S.d_raw.ensure(std::max<size_t>((size_t)plan.nslot * kPairRawBytes, 16)));
        if (tables == 2) PRK_TRY(S.d_pos.ensure(std::max<size_t>((size_t)plan.nslot * 4, 16)));      // the slots' rows
        if (tables == 3) PRK_TRY(S.d_rowslot.ensure(std::max<size_t>((size_t)plan.nrslot * 8, 16)));  // {row, pairs}
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
    a->work = S.d_work.p;
    a->lscan = d_lscan;
    a->nlist = plan.list_count;
    a->route = d_route;
    a->height = height;
    a->sbase = tables > 1 ? d_lscan + nl1 : nullptr;
    a->rbase = tables > 2 ? d_lscan + 2 * nl1 : nullptr;
    a->raw = fill ? S.d_raw.p : nullptr;
    a->prow = fill && tables == 2 ? (int32_t *)S.d_pos.p : nullptr;
    a->rows = fill && tables == 3 ? S.d_rowslot.p : nullptr;
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
    if (records_out || keep) PRK_TRY(prk_rec_export(S.d_work.p, nullptr, n, d_out, s));
    if (next_out) PRK_TRY(prk_adv_next(S.d_work.p, n, (int32_t *)S.d_evals.p, s));
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
            hipError_t e = prk_span_pack(S.d_raw.p, (const int32_t *)S.d_pos.p, d_sbase, d_cscan, list_count, nspan, buf, s);
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
    PRK_TRY(prk_span_pack(S.d_raw.p, (const int32_t *)S.d_pos.p, d_sbase, d_cscan, list_count, nspan, S.d_spanout.p, s));
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
        PRK_TRY(prk_row_pack(S.d_raw.p, S.d_rowslot.p, d_sbase, d_rbase, d_pscan, d_rscan, list_count, npair, nrow,
                             S.d_spanout.p, S.d_rowout.p, s));
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
    // device: lscan | the statistics (24 bytes a list) | the candidates | their most linked
    const size_t stat_off = (plan.nl1 * 4 + 7) & ~(size_t)7, cand_off = stat_off + (size_t)nlist * 24;
    PRK_TRY(S.d_lstat.ensure(cand_off + (size_t)nlist * 8));
    char *base = static_cast<char *>(S.d_lstat.p);
    const uint32_t *d_lscan = reinterpret_cast<const uint32_t *>(base);
    uint32_t *d_cand = reinterpret_cast<uint32_t *>(base + cand_off), *d_most = d_cand + nlist;
    PRK_TRY(hipMemcpyAsync(base, lscan.data(), plan.nl1 * 4, hipMemcpyHostToDevice, s));
    PRK_TRY(prk_list_stats(rec, at, d_lscan, nlist, height, base + stat_off, s));
    std::vector<uint64_t> raw(3 * (size_t)nlist);  // edge-rows, scans, {ymin0 ..., ymax_max ...}
    PRK_TRY(hipMemcpyAsync(raw.data(), base + stat_off, (size_t)nlist * 24, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    const uint64_t *erows = raw.data(), *scans = erows + nlist;
    const int32_t *ymin0 = reinterpret_cast<const int32_t *>(scans + nlist), *ymax_max = ymin0 + nlist;
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

// ConstructSphere (projekt.cpp:4123-4289): the reference's only test mesh.
// 24 inclination x 48 azimuth steps, r = 0.5, 6624 vertices.
int prk_construct_sphere(float *V, float *Col, float *N, float *UV, uint32_t *count_out) {
    if (!V || !Col || !N || !UV || !count_out) return PRK_ERR_ARG;
    const float Pi32 = 3.14159265359f;
    const float Radius = 0.5f;
    const uint32_t StepCount = 24;
    const float Up[4] = {1, 0, 0, 1}, Down[4] = {0, 1, 0, 1};
    float Inc[4];
    for (int k = 0; k < 4; ++k) Inc[k] = (Down[k] - Up[k]) / (float)StepCount;
    const float IncI = Pi32 / StepCount;
    const float IncA = (2.0f * Pi32) / (StepCount * 2);
    float Cur[4] = {Up[0], Up[1], Up[2], Up[3]};
    uint32_t n = 0;
    auto emit = [&](float x, float y, float z, float u, float v, const float *c4, const float *blue, bool inc) {
        V[3 * n] = Radius * x; V[3 * n + 1] = Radius * y; V[3 * n + 2] = Radius * z;
        N[3 * n] = x; N[3 * n + 1] = y; N[3 * n + 2] = z;
        UV[2 * n] = u; UV[2 * n + 1] = v;
        for (int k = 0; k < 4; ++k) Col[4 * n + k] = inc ? (c4[k] + Inc[k]) + blue[k] : c4[k] + blue[k];
        ++n;
    };
    for (uint32_t ii = 0; ii < StepCount; ++ii) {
        for (uint32_t ai = 0; ai < StepCount * 2; ++ai) {
            float I0 = (float)ii * IncI, I1 = (float)(ii + 1) * IncI;
            float A0 = (float)ai * IncA, A1 = (float)(ai + 1) * IncA;
            float Blue[4] = {0, 0, (1.0f + cosf(A0)) / 2.0f, 0};
            float NBlue[4] = {0, 0, (1.0f + cosf(A1)) / 2.0f, 0};
            if (ii == 0) {
                float S[3] = {sinf(I1) * cosf(A0), cosf(I1), sinf(I1) * sinf(A0)};
                float Tt[3] = {sinf(I1) * cosf(A1), cosf(I1), sinf(I1) * sinf(A1)};
                emit(0, 1, 0, 0.5f, 0.5f, Cur, Blue, false);
                emit(S[0], S[1], S[2], S[0], S[2], Cur, Blue, true);
                emit(Tt[0], Tt[1], Tt[2], Tt[0], Tt[2], Cur, NBlue, true);
            } else if (ii == StepCount - 1) {
                float F[3] = {sinf(I0) * cosf(A0), cosf(I0), sinf(I0) * sinf(A0)};
                float Tt[3] = {sinf(I0) * cosf(A1), cosf(I0), sinf(I0) * sinf(A1)};
                emit(F[0], F[1], F[2], 0.5f, 0.5f, Cur, Blue, false);
                emit(0, -1, 0, 0.0f, 0.0f, Cur, Blue, true);
                emit(Tt[0], Tt[1], Tt[2], Tt[0], Tt[2], Cur, NBlue, true);
            } else {
                float F[3] = {sinf(I0) * cosf(A0), cosf(I0), sinf(I0) * sinf(A0)};
                float S[3] = {sinf(I1) * cosf(A0), cosf(I1), sinf(I1) * sinf(A0)};
                float Tt[3] = {sinf(I1) * cosf(A1), cosf(I1), sinf(I1) * sinf(A1)};
                float Fo[3] = {sinf(I0) * cosf(A1), cosf(I0), sinf(I0) * sinf(A1)};
                auto uvx = [](float a) { return (a + 1.0f) / 2.0f; };
                emit(F[0], F[1], F[2], uvx(F[0]), uvx(F[1]), Cur, Blue, false);
                emit(S[0], S[1], S[2], uvx(S[0]), uvx(S[1]), Cur, Blue, true);
                emit(Tt[0], Tt[1], Tt[2], uvx(Tt[0]), uvx(Tt[1]), Cur, NBlue, true);
                emit(F[0], F[1], F[2], uvx(F[0]), uvx(F[1]), Cur, Blue, false);
                emit(Tt[0], Tt[1], Tt[2], uvx(Tt[0]), uvx(Tt[1]), Cur, NBlue, true);
                emit(Fo[0], Fo[1], Fo[2], uvx(Fo[0]), uvx(Fo[1]), Cur, NBlue, false);
            }
        }
        for (int k = 0; k < 4; ++k) Cur[k] = Cur[k] + Inc[k];
    }
    *count_out = n;
    return PRK_OK;
}

}  // extern "C"
