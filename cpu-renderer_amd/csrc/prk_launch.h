// prk_launch.h — the seam between the host runtime (the host files that share
// the context through prk_ctx.h, which lists them, and prk_dist.hip, which
// keeps it opaque) and the kernel files:
// every extern "C" launcher and query that one file defines and another
// calls, and the constants both sides rely on.  The records that cross it are
// prk_types.h's, and the prototypes name them: a buffer of the wrong record
// does not compile.  A parameter left `void *` is raw bytes: packed prk_edge /
// prk_span / prk_row_pair streams (read as uint4), scan and sort scratch and
// sort keys, a layout block (ListStatsLayout), pixels.  Every file that
// defines one of the functions includes this header, so a definition that
// disagrees with its prototype does not compile (C linkage would link it all
// the same).  The comments at the definitions say what each call does in full.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "prk_types.h"  // the records both sides rely on

struct prk_context;  // include/prk.h
struct prk_select_item;   // ... and its plain records that a kernel file reads as they are
struct prk_select_level;
struct prk_xform;
struct prk_bound;

namespace prk {
struct FrameParams;  // prk_device.h
struct DrawRec;

// The record calls' walks (prk_list_walk, prk_list_walk_wg): a call's device
// buffers, set by walk_begin and the run (prk_record_api.hip).  A kind reads only
// its own: 0 prk_advance_edge_lists (work, lscan, nlist, route, height, err),
// 1 prk_span_records (+ sbase, raw, prow, cnt), 2 prk_row_records (+ sbase,
// rbase, raw, rows, cnt, rcnt).  raw == nullptr: the counting variants (no
// slot is read or written).
struct ListWalkArgs {
    ObjEdge *work;          // the working copy (one per record)
    const uint32_t *lscan;  // nlist + 1: the lists' first edges
    uint32_t nlist;
    const uint32_t *route;  // null, or a word a list: 0 the thread walk, c + 1 slot class c
    int32_t height;
    const uint32_t *sbase;  // nlist + 1: the lists' first pair slots
    const uint32_t *rbase;  // nlist + 1: the lists' first row slots
    PairRaw *raw;           // per pair slot
    int32_t *prow;          // kind 1: the pair slots' rows
    RowRec *rows;           // kind 2: per row slot
    uint32_t *cnt, *rcnt;   // per list: its pairs, its rows
    uint32_t *err;          // |= 1 a list passed its slots, |= 2 a row of more than 1000 pairs
};

// ---- constants and sizes of both sides ---------------------------------------
constexpr int kPrepEdges = 256;     // edges a workgroup of k_list_prep* / k_adv_import takes
constexpr int kWaveListArrays = 9;  // WaveList: int32 arrays of cap + 2 entries each
// The workgroup walks' slot classes (listed edges; a class's workgroup has two threads more).
constexpr uint32_t kAdvWgCaps[5] = {62, 126, 254, 510, 1022};
// n packed prk_edge (27 dwords) / prk_span (25 dwords), readable in 16-byte pieces.
constexpr size_t packed_edge_bytes(size_t n) { return ((n * 27 + 3) / 4) * 16; }
constexpr size_t packed_span_bytes(size_t n) { return ((n * 25 + 3) / 4) * 16; }
}  // namespace prk

extern "C" {
// ---- prk_flush.hip (library-internal) ------------------------------------------
// A context's pending frame count, resolved on `stream`.
__attribute__((visibility("hidden"))) int prk_resolve_pending(prk_context *c, void *stream);

// ---- prk_kernels.hip ----------------------------------------------------------
// Each triangle's draw index (tri_draw[tri_count]) from the frame's draws.
hipError_t prk_launch_tri_draw(const prk::DrawRec *draws, uint32_t ndraws, uint32_t *tri_draw, uint32_t tri_count,
                               hipStream_t s);
// k_vis on svis, then the shading on s: k_walk + k_pix (AVX frames) or k_shade.
hipError_t prk_launch_raster(const prk::FrameParams *fp, int modeset, const uint32_t *offs, const prk::BinSlot *bins,
                             const uint32_t *pair_tri, const uint32_t *tri_off, const prk::TileRange *ranges,
                             uint8_t *won,
                             uint8_t *trwon, uint32_t *wlist, void *sel_temp, size_t sel_bytes, uint32_t *list,
                             uint32_t *nwin, uint32_t *wtag, prk::SpanRec *recs, uint32_t *anomaly, hipEvent_t mid,
                             hipEvent_t mid2, hipStream_t svis, hipStream_t s);
// Scratch bytes of k_walk's list build.
hipError_t prk_walk_select_bytes(uint32_t tri_count, size_t *bytes);
// The shared-divisor self-test over n draws; bad: three words, zeroed by the caller.
hipError_t prk_selftest_div_launch(uint32_t n, uint64_t seed, unsigned long long *bad, hipStream_t s);
// prk_selftest_ops: in = 4 x n words (a, b, c, d), out = 4 x n words.
hipError_t prk_selftest_ops_launch(int32_t op, uint32_t n, const uint32_t *in, uint32_t *out, hipStream_t s);
// Span path: visibility, then shading, of the pass's spans (modes: a bit a mode present).
hipError_t prk_launch_spans(const prk::FrameParams *fp, const uint32_t *offs, const uint32_t *bins,
                            const prk::SpanPos *pos,
                            const prk::SpanRec *recs, const prk::ScSpanRec *srecs, uint32_t modes,
                            const uint32_t *span_tri, uint32_t *nwin, uint32_t *wtag, hipStream_t s);

// ---- prk_bin.hip --------------------------------------------------------------
// Per-triangle tile ranges and counts (a band frame with run lists: k_bin_band).
hipError_t prk_bin_count(const prk::FrameParams *fp, uint32_t *tri_n, prk::TileRange *ranges, uint32_t *runlist,
                         uint32_t *run_n, uint8_t *trwon, hipStream_t s);
// A row band's setup records once k_bin_band has listed the runs.
hipError_t prk_band_records(const prk::FrameParams *fp, const uint32_t *runlist, const uint32_t *run_n,
                            hipStream_t s);
uint32_t prk_cs_chunks(uint32_t tri_count);                     // whole-frame counting-sort chunks
uint32_t prk_cs_nchunks(uint32_t tri_count, uint32_t per);      // ... or (per > 0) a band's chunks of `per` runs
uint32_t prk_cs_band_runs_per_chunk(const prk::FrameParams *fp);  // 0: not a band
uint32_t prk_bin_runs(uint32_t tri_count);                      // runs of the band run list
uint32_t prk_bin_run_len(void);                                 // entries of one run
uint32_t prk_cs_max_tiles(void);
uint32_t prk_cs_max_pairs(void);
int prk_cs_ready(uint32_t ntiles);  // the counting sort can bin ntiles tiles on the current device
// The counting sort: ghist nchunks * ntiles, tile_tot ntiles, chunk_tot / chunk_base nchunks;
// info[0] = entry count, info[1] = overflow (count > cap).
hipError_t prk_bin_cs(const prk::FrameParams *fp, const prk::TileRange *ranges, const uint32_t *tri_n, uint32_t *ghist,
                      uint32_t *tile_tot, uint32_t *chunk_tot, uint32_t *chunk_base, uint32_t *offs, uint32_t cap,
                      uint32_t *info, uint32_t *tri_off, prk::BinSlot *bins, uint32_t *pair_tri, uint8_t *won,
                      uint32_t won_stride, uint8_t *trwon, const uint32_t *runlist, const uint32_t *run_n,
                      uint32_t per, hipStream_t s);

// ---- prk_sort.hip -------------------------------------------------------------
// Exclusive scan of n values (temp == nullptr: size query).
hipError_t prk_scan_u32(const uint32_t *in, uint32_t *out, uint32_t n, void *temp, size_t *temp_bytes,
                        hipStream_t s);
hipError_t prk_scan_u64(const unsigned long long *in, unsigned long long *out, uint32_t n, void *temp,
                        size_t *temp_bytes, hipStream_t s);
// Stable sort of n (u64 key, u32 value) pairs (temp == nullptr: size query).  The contract, stated here only:
//   * The order is by the keys' low 8 * ceil(end_bit / 8) bits: whole 8-bit digits, so the bits from end_bit up
//     to the next multiple of 8 TAKE PART in the order; only the bits above that are ignored.  Every key bit,
//     ignored or not, arrives unchanged in keys_out.  end_bit = 0: the input order.
//   * A caller whose order is defined by exactly end_bit bits keeps the bits [end_bit, 8 * ceil(end_bit / 8))
//     equal in every key it wants ordered that way.  Both callers (prk_span_pass.hip's object passes, prk_record_api.hip's edge
//     records) do: a real key is (object, YMin, path) < 2^end_bit, zero above, and its lowest path bit is 0
//     (prk_spans.hip merge_path: pbits exceeds the recursion's depth); a pad key is all ones, so under either
//     mask it is larger than every real key and the pads end up last, in input order.
//   * Equal masked keys keep their input order.  keys_in / vals_in are not written; keys_out / vals_out get n
//     words each; temp is written inside [0, *temp_bytes) of the size query only, and need not be zeroed.
//   * hipErrorInvalidValue, before anything is touched, for end_bit > 64 or n > 2^30 - 1.
hipError_t prk_obj_sort(void *keys_in, uint32_t *vals_in, void *keys_out, uint32_t *vals_out, uint32_t n,
                        uint32_t end_bit, void *temp, size_t *temp_bytes, hipStream_t s);

// ---- prk_xform.hip ------------------------------------------------------------
// prk_geometry_transform: tables = the scan (nruns + 1 words), runs at byte runs_off, matrices at xf_off.
hipError_t prk_xform_launch(const void *tables, size_t runs_off, size_t xf_off, uint32_t nruns, uint32_t total,
                            const float *sV, const float *sC, const float *sN, const float *sUV, float *dV,
                            float *dC, float *dN, float *dUV, hipStream_t s);

// ---- prk_select.hip -----------------------------------------------------------
// prk_geometry_select, stage 1: for each of nitems items its pixel count (item_pixels[i], or without item_pixels
// the difference of two pix_prefix words), the first of its levels that the count passes, and from it chosen[i]
// (the level, or -1), n[i] (its triangles, or 0) and runs[i].  n has nitems + 1 words, the last written 0: the
// scan's input, whose last output word is the total.
// bound_pixels (prk_geometry_select_bounds; else nullptr): an item with id_count == 0 takes bound_pixels[i].
hipError_t prk_sel_choose(const prk_select_item *items, uint32_t nitems, const prk_select_level *levels,
                          const uint32_t *pix_prefix, const uint32_t *item_pixels, const uint32_t *bound_pixels,
                          int32_t *chosen, uint32_t *n, prk::SelRun *runs, hipStream_t s);
// Stage 3 (stage 2 is prk_scan_u32 of n into start): output triangle t of [0, total) belongs to the last item i
// with start[i] <= t; source triangle runs[i].src0 + (t - start[i]) goes through xforms[runs[i].xform] to
// destination triangle dst_first_tri + t.  total = start[nitems], read back by the caller.
hipError_t prk_sel_emit(const uint32_t *start, const prk::SelRun *runs, uint32_t nitems, uint32_t total,
                        uint32_t dst_first_tri, const prk_xform *xforms, const float *sV, const float *sC,
                        const float *sN, const float *sUV, float *dV, float *dC, float *dN, float *dUV,
                        hipStream_t s);

// ---- prk_bounds.hip -----------------------------------------------------------
// prk_visibility_bounds, stage 1: zmin[tiles_y][tiles_x] of the band B describes (z: its first pixel, rows W
// floats apart, 4-byte aligned) -- per 8 x 8 tile the smallest non-NaN z word, +inf without one.
// hipErrorInvalidValue when B's tile counts are not the band's.
hipError_t prk_ztile_min(const float *z, const prk::BoundsFrame *B, float *zmin, hipStream_t s);
// Stage 2: pixels[i] of the `count` boxes against zmin, under B's camera and P (xforms: 16-byte aligned; every
// bounds[i].xform inside it -- the host's check).
hipError_t prk_bounds_test(const prk_bound *bounds, uint32_t count, const prk_xform *xforms,
                           const prk::BoundsFrame *B, const float *zmin, uint32_t *pixels, hipStream_t s);

// ---- prk_tex.hip --------------------------------------------------------------
// prk_texture_from_target: the factor*dw x factor*dh pixels at src (rows spitch bytes apart) box-filtered
// into the dw x dh texels at dst (rows dpitch bytes apart); factor 1, 2 or 4, both addresses 4-byte aligned.
hipError_t prk_tex_from_target_launch(const void *src, size_t spitch, void *dst, size_t dpitch, uint32_t dw,
                                      uint32_t dh, int32_t factor, hipStream_t s);

// ---- prk_layer.hip ------------------------------------------------------------
// prk_layer_from_target / prk_target_from_layer: the w x h pixels (colour words at src_color, rows src_cpitch
// bytes apart; z words at src_z, rows src_zpitch bytes apart) into the pixels at dst_color / dst_z under
// rule (a PRK_MERGE_*: every pixel, or those whose source z wins); all four addresses 4-byte aligned.
hipError_t prk_layer_launch(const void *src_color, size_t src_cpitch, const float *src_z, size_t src_zpitch,
                            void *dst_color, size_t dst_cpitch, float *dst_z, size_t dst_zpitch, uint32_t w,
                            uint32_t h, int32_t rule, hipStream_t s);

// ---- prk_visibility.hip -------------------------------------------------------
// prk_visibility_*: n winner words reduced over id_count ids (temp == nullptr: the scratch size only) -- counts,
// flags, pix_prefix and vis_prefix of id_count + 1 words each, ids of id_count (written up to the visible count).
// natomics: nullptr, or a zeroed word that counts the histogram's atomic adds (the self-test's instantiation).
hipError_t prk_vis_reduce(const int32_t *winners, uint32_t n, uint32_t id_count, uint32_t *counts, uint32_t *flags,
                          uint32_t *pix_prefix, uint32_t *vis_prefix, uint32_t *ids, void *temp, size_t *temp_bytes,
                          uint32_t *natomics, hipStream_t s);
// pixels[g] / visible[g] (either may be null) of the ngroup id ranges [starts[g], starts[g + 1]): prefix differences.
hipError_t prk_vis_groups(const uint32_t *starts, uint32_t ngroup, const uint32_t *pix_prefix,
                          const uint32_t *vis_prefix, uint32_t *pixels, uint32_t *visible, hipStream_t s);

// ---- prk_spans.hip: prk_edge_records ---------------------------------------------
// prk_edge_records: the object triangles' edges with their true-YMin MergeSort keys ...
hipError_t prk_rec_emit(const prk::FrameParams *fp, const prk::ObjDesc *objs, const uint32_t *k0obj,
                        const uint32_t *k0tri0,
                        uint32_t nk0, uint32_t ntri, const uint32_t *escan, int32_t setup, uint32_t pbits,
                        prk::ObjEdge *edges, unsigned long long *keys, uint32_t *vals, int pad, hipStream_t s);
// ... the objects' edge counts ...
hipError_t prk_rec_counts(const prk::ObjDesc *objs, const uint32_t *k0obj, uint32_t nk0, const uint32_t *escan,
                          uint32_t *counts, hipStream_t s);
// ... and `total` edges (ord: null, or their order) as packed prk_edge records.
hipError_t prk_rec_export(const prk::ObjEdge *edges, const uint32_t *ord, uint64_t total, void *out, hipStream_t s);

// ---- prk_records.hip: the record calls' walks, packing and unpacking -------------
// `total` packed records into a->work, then the thread walk of `kind` over a's lists.
hipError_t prk_list_walk(int kind, const void *records, uint32_t total, const prk::ListWalkArgs *a, hipStream_t s);
// The largest slot class the current device grants the workgroup walks (0: none).
uint32_t prk_adv_wg_lcap(void);
// After prk_list_walk: the nl routed lists lists[0, nl) of slot class lcap, a workgroup each.
hipError_t prk_list_walk_wg(int kind, uint32_t lcap, const uint32_t *lists, uint32_t nl,
                            const prk::ListWalkArgs *a, hipStream_t s);
// The working copy's links after a walk: next_out[total].
hipError_t prk_adv_next(const prk::ObjEdge *work, uint32_t total, int32_t *next_out, hipStream_t s);
// The `total` spans a span walk left (cscan: the scanned counts) as packed prk_span.
hipError_t prk_span_pack(const prk::PairRaw *raw, const int32_t *row, const uint32_t *sbase, const uint32_t *cscan,
                         uint32_t nlist, uint32_t total, void *out, hipStream_t s);
// The npair pairs and nrow rows a row walk left as packed prk_row_pair and prk_row.
hipError_t prk_row_pack(const prk::PairRaw *raw, const prk::RowRec *rows, const uint32_t *sbase, const uint32_t *rbase,
                        const uint32_t *pscan, const uint32_t *rscan, uint32_t nlist, uint32_t npair, uint32_t nrow,
                        void *pairs_out, prk::RowRec *rows_out, hipStream_t s);
// prk_draw_rows: the rows' EdgeCounts (nrow + 1 words, the last 0) ...
hipError_t prk_rows_counts(const prk::RowRec *rows, uint32_t nrow, uint32_t *cnt, hipStream_t s);
// ... and npair packed pairs as packed prk_span, each on its row's RowIndex.
hipError_t prk_rows_unpack(const prk::RowRec *rows, const uint32_t *rscan, uint32_t nrow, const void *pairs,
                           uint32_t npair, void *out, hipStream_t s);
// One prk_draw_span_records draw: spans [first, first + count) of a handle into the slots of objects obj0 ...
hipError_t prk_span_handle_walk(const prk::FrameParams *fp, uint32_t draw, uint32_t g0, uint32_t obj0,
                                const void *spans, uint32_t first, uint32_t count, const unsigned long long *soff,
                                prk::SpanRecG *recs, prk::SpanPos *pos, uint32_t *span_tri, hipStream_t s);

// ---- prk_spans.hip: a pass of the span path (flush_spans) ------------------------
// The pass's objects (ObjDesc) and kind-0 tables from the host's runs (ObjRun).
hipError_t prk_obj_tables(const prk::ObjRun *runs, uint32_t nruns, uint32_t nobj, uint32_t wave_tris,
                          prk::ObjDesc *objs,
                          uint32_t *k0obj, uint32_t *k0tri0, const uint32_t *lcnt, const uint32_t *lflag,
                          const uint32_t *lscan, uint32_t wave_edges, uint32_t *lobj, hipStream_t s);
// The batch lists' records into the working copy, and each list's row sum (lrows, zeroed here).
hipError_t prk_list_prep(const prk::FrameParams *fp, const void *records, uint32_t nedge, const uint32_t *lscan,
                         uint32_t nlist, const uint32_t *lobj, const prk::ObjDesc *objs, const uint32_t *total0p,
                         uint32_t ebase, prk::ObjEdge *work, int2 *wy, unsigned long long *lrows, hipStream_t s);
// ... from nseg segments (PrepSeg, nblk workgroups in all) instead of one flat input.
hipError_t prk_list_prep_segs(const prk::FrameParams *fp, const prk::PrepSeg *segs, uint32_t nseg, uint32_t nblk,
                              const uint32_t *lscan, uint32_t nlist, const uint32_t *lobj, const prk::ObjDesc *objs,
                              const uint32_t *total0p, uint32_t ebase, prk::ObjEdge *work, int2 *wy,
                              unsigned long long *lrows, hipStream_t s);
// The pass's list counts (nlist + 1) and sorted flags from the staged tables and the handles' (ListSrc).
hipError_t prk_list_tables(const prk::ObjRun *runs, uint32_t nruns, uint32_t nobj, const uint32_t *cnt0,
                           const uint32_t *flag0, const prk::ListSrc *srcs, uint32_t nlist, uint32_t *lcnt,
                           uint32_t *lflag, hipStream_t s);
// The sorted rule of every list of nedge packed records; lflag: nlist words.
hipError_t prk_list_rule(const void *records, uint32_t nedge, const uint32_t *lscan, uint32_t nlist, uint32_t *lflag,
                         hipStream_t s);
// The walk statistics of every list; stats: 24 bytes a list, zeroed here.
hipError_t prk_list_stats(const void *records, uint32_t nedge, const uint32_t *lscan, uint32_t nlist, int32_t height,
                          void *stats, hipStream_t s);
// The most edges linked at once of the ncand lists cand[] names; most: a word a candidate.
hipError_t prk_list_most(const void *records, const uint32_t *lscan, const uint32_t *cand, uint32_t ncand,
                         int32_t height, uint32_t *most, hipStream_t s);
// FillEdgeTable of the pass's object triangles: per-triangle edge and active-row counts ...
hipError_t prk_objtri_count(const prk::FrameParams *fp, const prk::ObjDesc *objs, const uint32_t *k0obj,
                            const uint32_t *k0tri0, uint32_t nk0, uint32_t ntri, uint32_t *ecnt,
                            unsigned long long *rcnt, hipStream_t s);
// ... then the edges at their exclusive scan, with their MergeSort keys.
hipError_t prk_objtri_emit(const prk::FrameParams *fp, const prk::ObjDesc *objs, const uint32_t *k0obj,
                           const uint32_t *k0tri0, uint32_t nk0, uint32_t ntri, const uint32_t *escan,
                           uint32_t pbits, uint32_t ybits, int32_t ycap, prk::ObjEdge *edges, unsigned long long *keys,
                           uint32_t *vals, int pad, hipStream_t s);
// MergeSort + gather of objects of at most 64 edges.
hipError_t prk_obj_sort_local(const prk::ObjDesc *objs, const uint32_t *k0obj, uint32_t nk0, const uint32_t *escan,
                              const unsigned long long *keys, const prk::ObjEdge *edges, prk::ObjEdge *work, int2 *wy,
                              uint32_t *err, hipStream_t s);
// The walk's working copy: n slots, the triangle edges in order `ord`, then nk1 caller edges.
hipError_t prk_obj_gather(const prk::ObjEdge *edges, const uint32_t *ord, const uint32_t *total0p,
                          const prk::EdgeIn *edges_in,
                          const uint32_t *k1src, uint32_t nk1, prk::ObjEdge *work, uint32_t n, int2 *wy, hipStream_t s);
// Span slots per object (nobj + 1 values, the last 0).
hipError_t prk_obj_bound(const prk::FrameParams *fp, const prk::ObjDesc *objs, uint32_t nobj,
                         const unsigned long long *rscan,
                         const prk::EdgeIn *edges_in, const unsigned long long *lrows, unsigned long long *bound,
                         hipStream_t s);
// The workgroup walk's LDS capacity on the current device (listed edges; 0: none).
uint32_t prk_obj_walk_lcap(void);
// The object walk: a thread per small object or caller edge list (segs: the small objects' segments).
hipError_t prk_obj_walk(const prk::FrameParams *fp, const prk::ObjDesc *objs, uint32_t nobj, const uint32_t *escan,
                        const uint32_t *total0p, prk::ObjEdge *work, const unsigned long long *soff,
                        prk::SpanRecG *recs, prk::ScSpanRec *srecs,
                        prk::SpanPos *pos, uint32_t *span_tri, const prk::SpanIn *spans_in, uint32_t *err, int links,
                        const prk::ObjSeg *segs, const uint32_t *nsegp, uint32_t max_segs, hipStream_t s);
// The small triangle objects' segments: counts when segs is null, else the descriptors at segoff[o].
hipError_t prk_obj_seg(const prk::FrameParams *fp, const prk::ObjDesc *objs, uint32_t nobj, const uint32_t *escan,
                       const uint32_t *total0p, const int2 *wy, const unsigned long long *soff, uint32_t *segcnt,
                       const uint32_t *segoff, prk::ObjSeg *segs, prk::SpanPos *pos, hipStream_t s);
uint32_t prk_obj_link_cap(void);
// The most active entries of the large objects big[0, nbig); most: 3 * nbig values ...
hipError_t prk_obj_maxact(const prk::FrameParams *fp, const prk::ObjDesc *objs, const uint32_t *big, uint32_t nbig,
                          const uint32_t *escan, const uint32_t *total0p, const prk::ObjEdge *work, int32_t *most,
                          uint32_t huge_min, hipStream_t s);
// ... and those of the huge object big[b] over many workgroups (scratch: prk_maxact_huge_scratch bytes).
size_t prk_maxact_huge_scratch(void);
hipError_t prk_obj_maxact_huge(const prk::FrameParams *fp, const prk::ObjDesc *objs, const uint32_t *big, uint32_t b,
                               uint32_t nbig, uint32_t edges, const uint32_t *escan, const uint32_t *total0p,
                               const prk::ObjEdge *work, int32_t *most, void *scratch, hipStream_t s);
// A workgroup per large object of mode `mode`: lcap > 0 the list in LDS, 0 one wave and the pool.
uint32_t prk_obj_walk_threads(uint32_t lcap);
hipError_t prk_obj_walk_group(const prk::FrameParams *fp, int32_t mode, uint32_t lcap, const prk::ObjDesc *objs,
                              const uint32_t *big, const unsigned long long *big_off, const uint32_t *big_cap,
                              uint32_t nbig, int32_t *pool, const uint32_t *escan, const uint32_t *total0p,
                              prk::ObjEdge *work, const unsigned long long *soff, prk::SpanRecG *recs,
                              prk::ScSpanRec *srecs, prk::PairRaw *raw,
                              prk::SpanPos *pos, uint32_t *span_tri, uint32_t *err, const uint32_t *prstat,
                              hipStream_t s);
// The huge-object walk (lds: k_obj_walk_lds, else k_obj_walk_big), then the replay of every pair.
uint32_t prk_big_max_entries(void);
uint64_t prk_big_slice_ints(uint32_t cap, uint32_t rows, uint32_t ents);
uint32_t prk_big_lds_cap(void);
hipError_t prk_big_walk(const prk::FrameParams *fp, int32_t mode, int lds, const prk::ObjDesc *objs,
                        const uint32_t *big,
                        const unsigned long long *big_off, const uint32_t *big_cap, const uint32_t *big_meta,
                        uint32_t nbig, uint32_t max_rows, int32_t *pool, const uint32_t *escan,
                        const uint32_t *total0p, const prk::ObjEdge *work, const unsigned long long *soff,
                        prk::PairRaw *raw,
                        prk::SpanPos *pos, uint32_t *span_tri, uint32_t *err, const uint32_t *prstat, hipStream_t s);
// The chunked walk of large objects: begin, a group call per (mode, LDS capacity), end.
hipError_t prk_pr_walk_begin(const prk::FrameParams *fp, const prk::PrWalkArgs *a, hipStream_t s);
hipError_t prk_pr_walk_group(const prk::FrameParams *fp, const prk::PrWalkArgs *a, int32_t mode, uint32_t cap,
                             const uint32_t *grp, uint32_t ngroup, uint32_t max_chunks, hipStream_t s);
hipError_t prk_pr_walk_end(const prk::PrWalkArgs *a, hipStream_t s);
uint32_t prk_pr_chunk_rows(void);
int32_t prk_pr_max_row_entries(void);
int32_t prk_pr_max_rows(void);
// The slot walks' pairs (PairRaw) into span records, one thread per slot.
hipError_t prk_span_finish(const prk::FrameParams *fp, const prk::PairRaw *raw, uint32_t nslot, prk::SpanRecG *recs,
                           prk::ScSpanRec *srecs, prk::SpanPos *pos, hipStream_t s);
// Span -> tile bin entries: the tiles' counts (ntiles + 1 values), then the bins at their scan.
hipError_t prk_span_count(const prk::FrameParams *fp, const prk::SpanPos *pos, uint32_t nspan, uint32_t *tcnt,
                          hipStream_t s);
hipError_t prk_span_bin(const prk::FrameParams *fp, const prk::SpanPos *pos, uint32_t nspan, const uint32_t *offs,
                        uint32_t *tcur, uint32_t *bins, hipStream_t s);
}  // extern "C"
