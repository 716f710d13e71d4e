// prk_types.h — the plain-data layouts that more than one translation unit
// relies on, each defined here once with its size: the records the host sizes
// buffers by and fills, and the records one kernel file writes and another
// reads.  No device functions, so the host files, the kernel files and
// prk_device.h all include it (prk_launch.h does for the launchers'
// prototypes).  The helpers that read and write the records stay with their
// kernels (prk_spans_dev.h: obj_edge_store, obj_step, obj_span, ...).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace prk {

// ---- what the host fills and the device reads (prk_spans.hip has the full
// comments, next to the kernels that read them) -------------------------------
// One object of the span path, as k_obj_tables expands it from the runs.
struct ObjDesc {
    uint32_t draw;
    uint32_t g0;
    uint32_t tris;
    uint32_t tri0;      // kind 0: its first triangle among the pass's object triangles
    uint32_t kind, src, nsrc;
    uint32_t k1off;     // kind 1, 3: its first edge slot after the pass's triangle edges;
                        // bit 31 (kObjWave): a large object (k_obj_maxact, then its walk)
};
static_assert(sizeof(ObjDesc) == 32);
// A run of objects as the host lists them.
struct ObjRun {
    uint32_t kind, draw, obj0, count, per, tri_count, first_global, tri0, k0base, src_off, src_n, k1off;
};
static_assert(sizeof(ObjRun) == 48);
// A segment of a pass's batch edges (passes that draw from record handles) ...
struct PrepSeg {
    const uint32_t *src;  // its first record (a device address)
    uint32_t e0, n;       // its first edge among the pass's batch edges, its edges
    uint32_t blk0, pad;   // its first workgroup
};
static_assert(sizeof(PrepSeg) == 24);
// ... and where a run's list counts and sorted flags come from.
struct ListSrc {
    const uint32_t *cnt, *flag;
};
static_assert(sizeof(ListSrc) == 16);

// prk_geometry_select (prk_select.hip): what k_sel_choose leaves for an item
// and k_sel_emit reads -- the first source triangle of the chosen level and
// the item's matrix (a dropped item: zeros, never read).  The items and
// levels themselves are prk.h's prk_select_item / prk_select_level.
struct SelRun {
    uint32_t src0, xform;
};
static_assert(sizeof(SelRun) == 8);

// prk_visibility_bounds (prk_bounds.hip): the band both kernels work on, its
// 8 x 8 z tiles, and what the test kernel projects with -- prk_set_camera's
// transform and the call's P, as the host fills them.
struct BoundsFrame {
    int32_t W, row0, row1;       // the band: rows [row0, row1) of W pixels, z rows W floats apart
    int32_t tiles_x, tiles_y;    // (W + 7) / 8, and the tile rows that meet the band
    int32_t first_tile_row;      // row0 / 8: zmin's first row
    float D, F, M2P, Cx, Cy;     // ProjectVertex's constants
    float P[3];
};
static_assert(sizeof(BoundsFrame) == 56);

// Caller edges (prk_edge = edge_info without Next, prk.h) and spans (prk_span).
struct EdgeIn {
    int32_t YMax;
    float XMin, ZMin, OneOverZMin, Gradient, ZGradient, OneOverZGradient;
    int32_t YMin;
    float UMin, VMin, UGradient, VGradient;
    int32_t Left;
    float MinColor[4], ColorGradient[4], MinNormal[3], NormalGradient[3];
};
static_assert(sizeof(EdgeIn) == 27 * 4);
struct SpanEndIn {
    float XMin, ZMin, OneOverZMin, UMin, VMin, MinColor[4], MinNormal[3];
};
struct SpanIn {
    SpanEndIn L, R;
    int32_t Row;
};
static_assert(sizeof(SpanIn) == 25 * 4);

// Tiles a triangle may touch: the rectangle [tx0..tx1] x [ty0..ty1], plus
// for scalar semantics the column-0 tiles of rows [oty0..oty1] that receive
// DrawModel's one-past-the-row store (see span_setup_scalar).
// pad0 / pad1: the triangle's band rows [r0, r1) (prk_bin.hip: row classes)
struct TileRange { uint16_t tx0, ty0, tx1, ty1, oty0, oty1, pad0, pad1; };
static_assert(sizeof(TileRange) == 16);
// A bin entry of the per-triangle pass (prk_bin.hip k_cs_emit): x the
// triangle, y its (triangle, tile) pair.
using BinSlot = uint2;
static_assert(sizeof(BinSlot) == 8);

// ---- the span path's records (prk_spans.hip, prk_records.hip; k_span_vis,
// k_pix and k_span_shade of prk_kernels.hip read the spans) --------------------
// Mutable edge_info of the object's AET (projekt.h:17-37) in global memory:
// the walks' working copy.
struct ObjEdge {
    float X, G, Z, ZG, W, WG, U, UG, V, VG;
    float N0, N1, N2, NG0, NG1, NG2;
    int32_t YMin, YMax, Left, Next;
    float C0, C1, C2, C3, CG0, CG1, CG2, CG3;  // MinColor / ColorGradient (DrawModel's Gouraud colour)
};
static_assert(sizeof(ObjEdge) == 112, "ObjEdge is seven dwordx4");

// Span of the span path: its row and pixel range [minx, maxx) (half-open,
// 1588-1592), DRAW_ST in flags.
struct SpanPos {
    int32_t row, minx, maxx;
    uint32_t flags;
};
static_assert(sizeof(SpanPos) == 16);

// One won row span (FillLineOptimized span setup, 1543-1835: the lane-init
// record), in its two views: the named fields k_walk's queue and k_pix read,
// and the four quads the stores write (walk_record, prk_kernels.hip; obj_span,
// prk_spans_dev.h): q0 = (left_tex, xoff, lw, lu), q1 = (lv, lz, iw, iu),
// q2 = (iv, iz, ln0, ln1), q3 = (ln2, in0, in1, in2).
struct SpanRec {
    int32_t left_tex;  // LeftXa (low 16 bits) | texture index << 16
    float xoff, lw, lu, lv, lz, iw, iu, iv, iz, ln0, ln1, ln2, in0, in1, in2;
};
struct SpanRecG {
    float4 q0, q1, q2, q3;
};
static_assert(sizeof(SpanRec) == 64 && sizeof(SpanRecG) == sizeof(SpanRec), "span record is four dwordx4");
static_assert(offsetof(SpanRec, left_tex) == 0 && offsetof(SpanRec, lv) == 16 && offsetof(SpanRec, iv) == 32 &&
                  offsetof(SpanRec, ln2) == 48,
              "a quad's first field");
static_assert(offsetof(SpanRecG, q0) == 0 && offsetof(SpanRecG, q1) == 16 && offsetof(SpanRecG, q2) == 32 &&
                  offsetof(SpanRecG, q3) == 48,
              "the quads");
// A DrawModel span (scalar semantics) of the span path: the values at MinX
// after the left clip (308-412) and the per-pixel increments, in the float
// slot order of the scalar sweeps (prk_kernels.hip SS_*), plus its texture.
// Its span record slot carries kScalarSpan in its first word, its SpanPos the
// half-open [MinX, MaxX + 1) and SPAN_SCALAR | mode << 8 (prk_device.h).
struct ScSpanRec {
    float f[22];
    int32_t tex, pad;
};
static_assert(sizeof(ScSpanRec) == 96, "scalar span record is six dwordx4");

// A pair of the slot walk, before its span setup (prk_spans_dev.h).
struct PairRaw {
    float4 l0, l1, l2, r0, r1, r2;  // X Z W U | V N0 N1 N2 | C0 C1 C2 C3, left then right edge
};
static_assert(sizeof(PairRaw) == 96, "six dwordx4");
// A row of the row walk (prk_records.hip): x the row, y its pairs.
using RowRec = int2;
static_assert(sizeof(RowRec) == 8);

// A segment of a small triangle object (prk_spans.hip k_obj_seg).
struct ObjSeg {
    uint32_t o;      // object
    uint32_t e0, n;  // its sorted edges [e0, e0 + n) (object-relative)
    uint32_t base, bound;  // span slots
    uint32_t pad;
};
static_assert(sizeof(ObjSeg) == 24);

// k_obj_maxact's block for n large objects: most[n], rows[n], ents[n].
struct MaxactView {
    int32_t *most, *rows, *ents;
};
struct MaxactLayout {
    size_t n;
    size_t bytes() const { return 3 * n * sizeof(int32_t); }
    MaxactView view(void *base) const {
        int32_t *m = static_cast<int32_t *>(base);
        return MaxactView{m, m + n, m + 2 * n};
    }
};
// prk_list_stats' block for n lists, 24 bytes a list: the edge-row sums, the
// insertion-scan sums, the YMin of the first record, the largest YMax.
struct ListStatsView {
    unsigned long long *erows, *scans;
    int32_t *ymin0, *ymaxmax;
};
struct ListStatsLayout {
    size_t n;
    size_t bytes() const { return n * (2 * sizeof(unsigned long long) + 2 * sizeof(int32_t)); }
    ListStatsView view(void *base) const {
        unsigned long long *e = static_cast<unsigned long long *>(base);
        int32_t *y = reinterpret_cast<int32_t *>(e + 2 * n);
        return ListStatsView{e, e + n, y, y + n};
    }
};

// ---- the chunked walk of large objects (prk_spans.hip k_pr_*) -----------------
struct PrObj {                              // per object of the walk (host: classify_chunked)
    uint32_t o;                             // object index
    uint32_t row_off;                       // its first row in the pass's row arrays (rows + 1 each)
    uint32_t rows;                          // MaxY - FirstRow (k_obj_maxact)
    uint32_t chunk_off;                     // its first chunk in the pass's chunk arrays
    uint32_t most;                          // k_obj_maxact's most entries (the list stride per chunk)
    uint32_t ent_off;                       // its first list entry: chunk j's lists at ent_off + j * most
    uint32_t pad0, pad1;
};
static_assert(sizeof(PrObj) == 32);
struct PrRow {                              // per object, set by k_pr_hist
    int32_t first_row, max_y;
};
static_assert(sizeof(PrRow) == 8);
// Its pass-wide buffers and sizes, set by SpanPass::chunked (prk_span_pass.hip).
struct PrWalkArgs {
    const ObjDesc *objs;
    const PrObj *pro;           // npr of them
    uint32_t npr;               // objects
    uint32_t warmup;            // chunks start one chunk early (0: from their own first row)
    uint32_t nchunks;           // their chunks
    uint32_t max_edges;         // most edges of one object
    const uint32_t *escan, *total0p;
    const ObjEdge *work;        // the walk's working copy
    PrRow *prrow;               // npr of them
    uint32_t *cnt, *eoff, *fge; // per row: rows + 1 per object
    uint32_t *ccur;             // per chunk: its first row's entries
    float4 *key;                // per entry (chunk j of an object: ent_off + j * most)
    ObjEdge *est, *sst, *eend;  // per entry: arrival order / canonical list / a walk's end list
    uint32_t *eend_m, *match;   // per chunk
    uint32_t *sidx, *s_m;       // per entry / per chunk: a chunk's list at its first row (edge indices)
    uint32_t *prstat;           // per object of the pass
    const unsigned long long *soff;
    PairRaw *raw;               // per span slot
    SpanPos *pos;               // per span slot
    uint32_t *span_tri, *err;
};
}  // namespace prk
