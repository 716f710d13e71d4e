// prk_records.hip — the record calls' walks of edge lists, no frame (the span
// path: prk_spans.hip): prk_advance_edge_lists, prk_span_records,
// prk_row_records and prk_draw_rows, each by a thread per list and, last in
// this file, by a workgroup per long list; and k_span_handle_walk.
#include <atomic>

#include "prk_slot.h"

namespace prk {
// ---------------------------------------------------------------------------
// prk_advance_edge_lists: the list DrawModel* leaves in the caller's
// edge_info array (3654-3869), for a batch of sorted lists and no frame:
// k_adv_import (k_list_prep's import alone: list o's records at slots
// lscan[o] ..) -> k_adv_walk (a thread per list) -> k_rec_export of the
// working copy and k_adv_next of its links.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kPrepEdges) k_adv_import(const uint4 *__restrict__ in, uint32_t nedge,
                                                           ObjEdge *__restrict__ work) {
    __shared__ uint4 rec4[kPrepPieces];
    prep_records(in, nedge, rec4, work + (size_t)blockIdx.x * kPrepEdges);
}

// The whole edge step (3811-3829): every field, whatever the draw's mode
// reads (obj_step<M> steps only those) -- here the stepped record is the
// result.  The record's quads that hold no stepped field (row range, Left and
// link; the colour gradient) are not written back.
//
// EM is the walk's emission hook: em.half(right, E) sees the record as it
// stands on the row, before the step -- one end of the line_render_work
// DrawModelOptimized(RenderQueue) queues for the pair (3756-3809).  AdvNoEmit
// (prk_advance_edge_lists) compiles to nothing.  em.row(Row) ends every row
// the walk does not skip, paired or not: DrawModelOptimizedLines queues one
// buffer_line_render_work there (3604-3609); only AdvRowEmit listens.
struct AdvNoEmit {
    __device__ __forceinline__ void half(bool, const ObjEdge &) const {}
    __device__ __forceinline__ void pair(int32_t) {}
    __device__ __forceinline__ void row(int32_t) {}
};
// (the arithmetic alone: the thread walk steps the record in device memory,
// the workgroup walk its LDS state -- one text, so one result)
__device__ __forceinline__ void adv_step_fields(ObjEdge &E) {
    E.X += E.G;
    E.Z += E.ZG;
    E.C0 += E.CG0; E.C1 += E.CG1; E.C2 += E.CG2; E.C3 += E.CG3;
    float x = E.N0 + E.NG0, y = E.N1 + E.NG1, z = E.N2 + E.NG2;
    normalize_rcp(x, y, z);
    E.N0 = x; E.N1 = y; E.N2 = z;
    E.U += E.UG;
    E.V += E.VG;
    E.W += E.WG;
}
template <class EM>
__device__ __forceinline__ void adv_step(ObjEdge *p, const EM &em, bool right) {
    PRK_ER(w);
    PRK_ER_LOAD(w, p);
    ObjEdge E = PRK_ER_EDGE(w);
    em.half(right, E);
    adv_step_fields(E);
    PRK_ER_FROM(w, E);
    float4 *d = reinterpret_cast<float4 *>(p);
    d[0] = w0; d[1] = w1; d[2] = w2; d[3] = w3; d[5] = w5;
}

// walk_object's sorted branch without the frame: the same insertion cursor,
// expiry, 3722-3749 removal, pairing with both swaps (P3) and empty-list row
// skip, no span, every field stepped (adv_step), over the rows
// [YMin[0], min(max YMax, height)) -- prk_advance_edge_records' rows, no band
// or target clip.  Under the sorted rule (prk.h) the cursor inserts on every
// row the edges the reference's whole-list scan inserts, in the same order.
// The list is walked whole: an edge that expires on the row later edges are
// inserted on is still linked when they are, and its final Next depends on
// them (k_obj_seg's split would lose that word).  The records are stepped in
// place; the links are LK's (GLinks: the records' own Next).  Every pair goes
// to the emission hook before it is stepped: its two ends (adv_step), then
// em.pair(Row); em.row(Row) once the row's pairs are through.
template <class LK, class EM>
__device__ void adv_walk_list(ObjEdge *E, uint32_t n, int32_t height, const LK lk, EM &em) {
    const int32_t FirstRow = lk.ymin(0);
    int32_t MaxRow = lk.ymax(0);
    for (uint32_t i = 1; i < n; ++i) MaxRow = max(MaxRow, lk.ymax((int)i));
    const int32_t MaxY = min(MaxRow, height);
    for (uint32_t i = 0; i < n; ++i) lk.set_next((int)i, -1);  // 4094
    int32_t Head = -1, Tail = -1;
    uint32_t ins = 0;        // next sorted edge to insert
    int32_t nym = FirstRow;  // its YMin (INT32_MAX past the end)
    for (int32_t Row = FirstRow; Row < MaxY; ++Row) {
        while (ins < n && nym < Row) nym = ++ins < n ? lk.ymin((int)ins) : INT32_MAX;
        const uint32_t i0 = ins;
        while (ins < n && nym == Row) nym = ++ins < n ? lk.ymin((int)ins) : INT32_MAX;
        for (uint32_t ii = i0; ii < ins; ++ii) {  // insertion 3654-3713
            const int32_t c = (int32_t)ii;
            if (Head >= 0) {
                if (lk.before(c, Head)) {
                    lk.set_next(c, Head);
                    Head = c;
                } else {
                    int32_t Cmp = Head, Prev = Head;
                    while (Cmp != Tail) {
                        Cmp = lk.next(Cmp);
                        if (lk.before(c, Cmp)) {
                            lk.set_next(c, Cmp);
                            lk.set_next(Prev, c);
                            Cmp = Tail;
                        } else {
                            Prev = Cmp;
                        }
                    }
                    if (Prev == Cmp) {
                        lk.set_next(Tail, c);
                        Tail = c;
                    }
                }
            } else {
                Head = c;
                Tail = c;
            }
        }
        while (Head >= 0 && lk.ymax(Head) <= Row) {  // expiry 3715-3720
            const int32_t Rm = Head;
            Head = lk.next(Head);
            lk.set_next(Rm, -1);
        }
        if (Head < 0) {  // pin: the row is skipped, and so are the rows before the next insertion
            Tail = -1;
            if (ins >= n) break;
            Row = max(Row, nym - 1);
            continue;
        }
        {
            int32_t Prev = Head, Chk = Head;  // 3722-3749
            while (Chk != Tail) {
                Chk = lk.next(Chk);
                if (lk.ymax(Chk) <= Row) {
                    if (Chk == Tail) {
                        Tail = Prev;
                        lk.set_next(Tail, -1);
                        Chk = Tail;
                    } else {
                        lk.set_next(Prev, lk.next(Chk));
                        Chk = Prev;
                    }
                }
                Prev = Chk;
            }
        }
        int32_t PrevCur = -1, PrevNext = -1;  // pairing 3751-3869
        int32_t Cur = Head, Next = lk.next(Cur);
        while (Next >= 0) {
            adv_step(&E[Cur], em, false);  // 3811-3829
            adv_step(&E[Next], em, true);
            em.pair(Row);
            lk.stepped(Cur);
            lk.stepped(Next);
            if (lk.x(Cur) > lk.x(Next)) {  // 3831-3841
                lk.set_next(Cur, lk.next(Next));
                lk.set_next(Next, Cur);
                if (PrevNext >= 0) lk.set_next(PrevNext, Next);
                else Head = Next;              // P3
                if (Tail == Next) Tail = Cur;  // P3
                Cur = Next;
                Next = lk.next(Cur);
            }
            if (PrevNext >= 0) {  // 3843-3853
                if (lk.x(PrevNext) > lk.x(Cur)) {
                    lk.set_next(PrevNext, lk.next(Cur));
                    lk.set_next(Cur, PrevNext);
                    lk.set_next(PrevCur, Cur);
                    PrevNext = Cur;
                    Cur = lk.next(PrevNext);
                }
            }
            PrevCur = Cur;
            PrevNext = Next;
            if (lk.next(Next) >= 0) {
                Cur = lk.next(Next);
                Next = lk.next(Cur);
            } else {
                Next = -1;
            }
        }
        em.row(Row);
    }
}

// One thread per list; list o: lscan[o + 1] - lscan[o] edges at work +
// lscan[o].  The list fields are the records' own (GLinks): k_obj_walk's LDS
// mirrors of short lists were measured here too and left out (DESIGN
// §4.4.3).  A list of fewer than two edges pairs nothing: it stays as
// imported, every Next -1.
__global__ void __launch_bounds__(kLinkThreads) k_adv_walk(ObjEdge *__restrict__ work,
                                                           const uint32_t *__restrict__ lscan, uint32_t nlist,
                                                           const uint32_t *__restrict__ route, int32_t height) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nlist || (route && route[o])) return;  // (routed: a workgroup walks it, k_adv_walk_wg)
    const uint32_t e0 = lscan[o], n = lscan[o + 1] - e0;
    if (n < 2) return;
    AdvNoEmit em;
    adv_walk_list(work + e0, n, height, GLinks{work + e0}, em);
}

// Each edge's Next, an index within its own list or -1, as one flat array.
__global__ void __launch_bounds__(256) k_adv_next(const ObjEdge *__restrict__ work, uint32_t total,
                                                  int32_t *__restrict__ next_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) next_out[i] = work[i].Next;
}

// ---------------------------------------------------------------------------
// prk_span_records: the line_render_work records DrawModelOptimized
// (RenderQueue) queues for a list (3756-3809), for the same batches and by
// the same walk: k_adv_import -> k_span_walk (k_adv_walk with the emission
// hook: a thread per list, each pair's PairRaw and row into the list's slot
// range, the list's count) -> prk_scan_u32 of the counts -> k_span_pack (the
// used slots as packed prk_span).
// ---------------------------------------------------------------------------
// The hook: pair k of the list at slot at0 + k, both edges as they stand on
// the row (six dwordx4 stores) and the row.  STORE = false counts only: no
// slots, the emission compiled out.  A pair past the list's range is counted
// and not stored (the host's bound rules it out; k_span_walk reports it).
template <bool STORE>
struct AdvSpanEmit {
    PairRaw *raw;
    int32_t *prow;  // the pairs' rows
    uint32_t at, end;
    __device__ __forceinline__ void half(bool right, const ObjEdge &E) const {
        if constexpr (STORE) {
            if (at < end) {
                float4 *q = reinterpret_cast<float4 *>(raw + at) + (right ? 3 : 0);
                pair_raw_half(E, q[0], q[1], q[2]);
            }
        }
    }
    __device__ __forceinline__ void pair(int32_t Row) {
        if constexpr (STORE) {
            if (at < end) prow[at] = Row;
        }
        ++at;
    }
    __device__ __forceinline__ void row(int32_t) {}
};

// sbase: nlist + 1 values, list o's slots [sbase[o], sbase[o + 1]) --
// floor(edge-rows / 2) of them: a pair uses up one row of each of two listed
// edges.  cnt[o]: the list's pairs.  err: set when a list passed its range.
template <bool STORE>
__global__ void __launch_bounds__(kLinkThreads) k_span_walk(ObjEdge *__restrict__ work,
                                                            const uint32_t *__restrict__ lscan, uint32_t nlist,
                                                            const uint32_t *__restrict__ route, int32_t height,
                                                            const uint32_t *__restrict__ sbase,
                                                            PairRaw *__restrict__ raw, int32_t *__restrict__ row,
                                                            uint32_t *__restrict__ cnt, uint32_t *__restrict__ err) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nlist || (route && route[o])) return;  // (routed: k_span_walk_wg walks and counts it)
    const uint32_t e0 = lscan[o], n = lscan[o + 1] - e0;
    uint32_t pairs = 0;
    if (n >= 2) {
        const uint32_t s0 = STORE ? sbase[o] : 0u, s1 = STORE ? sbase[o + 1] : 0xFFFFFFFFu;
        AdvSpanEmit<STORE> em{raw, row, s0, s1};
        adv_walk_list(work + e0, n, height, GLinks{work + e0}, em);
        pairs = em.at - s0;
        if (STORE && em.at > s1) {
            pairs = s1 - s0;
            atomicOr(err, 1u);
        }
    }
    cnt[o] = pairs;
}

// The used slots as packed prk_span records (25 dwords: Left, Right, Row;
// an end is XMin ZMin OneOverZMin UMin VMin MinColor[4] MinNormal[3], prk.h).
// A workgroup takes kPackSpans consecutive packed spans; their 25 * kPackSpans
// dwords are a 16-byte-aligned stretch of the flat output.  Lane t finds span
// k's list by a binary search of the scanned counts (cscan: nlist + 1 values,
// the last = total; the list is the last o with cscan[o] <= k, never an empty
// one), reads its slot sbase[o] + k - cscan[o] (six dwordx4 and the row) and
// puts the 25 dwords in prk_span's order into LDS at dword 25 t: the stride is
// odd, so the 32 lanes of a ds_write_b32 group fall on 32 different banks.
// Then lane t of pass j stores dwordx4 t + 256 j of the stretch from LDS
// (ds_read_b128 of consecutive 16-byte slots, 1 KiB contiguous a wave
// instruction).  `out` holds 25 * total dwords rounded up to four; the last
// piece's spare dwords are zero.
constexpr int kPackSpans = 256;
constexpr uint32_t kPackPieces = 25u * kPackSpans / 4u;
static_assert(25 * kPackSpans % 4 == 0, "a workgroup's spans start on a 16-byte boundary");
__global__ void __launch_bounds__(kPackSpans) k_span_pack(const PairRaw *__restrict__ raw,
                                                          const int32_t *__restrict__ row,
                                                          const uint32_t *__restrict__ sbase,
                                                          const uint32_t *__restrict__ cscan, uint32_t nlist,
                                                          uint32_t total, uint4 *__restrict__ out) {
    __shared__ uint4 st4[kPackPieces];
    float *st = reinterpret_cast<float *>(st4);
    const uint32_t tid = threadIdx.x;
    const uint32_t k0 = blockIdx.x * (uint32_t)kPackSpans;  // (< total: the grid)
    const uint32_t ns = min((uint32_t)kPackSpans, total - k0);
    const uint32_t k = k0 + tid;
    if (tid < ns) {
        uint32_t lo = 0, hi = nlist;  // cscan[lo] <= k < cscan[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cscan[mid] <= k) lo = mid;
            else hi = mid;
        }
        const size_t slot = (size_t)sbase[lo] + (k - cscan[lo]);
        const PairRaw r = raw[slot];
        float *d = st + 25u * tid;
        const float4 q[6] = {r.l0, r.l1, r.l2, r.r0, r.r1, r.r2};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 a = q[3 * h], b = q[3 * h + 1], c = q[3 * h + 2];
            float *e = d + 12 * h;
            e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x;  // X Z W U V
            e[5] = c.x; e[6] = c.y; e[7] = c.z; e[8] = c.w;              // MinColor
            e[9] = b.y; e[10] = b.z; e[11] = b.w;                        // MinNormal
        }
        d[24] = __int_as_float(row[slot]);
    } else if (tid < ns + 1u) {
        st[25u * ns] = st[25u * ns + 1u] = st[25u * ns + 2u] = 0.0f;  // (the last piece's spare dwords; < 25 * 256)
    }
    __syncthreads();
    const uint32_t np = (25u * ns + 3u) / 4u;
    uint4 *dst = out + (size_t)blockIdx.x * kPackPieces;
    for (uint32_t p = tid; p < np; p += (uint32_t)kPackSpans) dst[p] = st4[p];
}

// ---------------------------------------------------------------------------
// prk_row_records: the buffer_line_render_work records DrawModelOptimizedLines
// queues for a list (3509-3609: one a row, RowIndex, EdgeCount and EdgeCount
// thread_edge_info pairs), by the same walk once more: k_adv_import ->
// k_row_walk (the pairs as k_span_walk leaves them, and a {row, pairs} record
// at the end of every row the walk does not skip) -> prk_scan_u32 of the row
// counts and of the pair counts -> k_row_pack (packed prk_row, packed
// prk_row_pair).  prk_draw_rows' k_rows_unpack turns such records back into
// prk_draw_spans' input.
// ---------------------------------------------------------------------------
// The reference's ThreadEdges[1000] (3403): a row with more pairs writes past it.
constexpr uint32_t kRowMaxPairs = 1000u;
// The hook: the halves as AdvSpanEmit's (pair k of the list at slot at0 + k;
// the row is not stored with the pair), and row(): {Row, pairs since the last
// row()} into the list's next row slot.  FILL = false counts only: no slot is
// addressed.  A pair or a row past the list's range is counted and not stored
// (the host's bounds rule both out; k_row_walk reports it).  over: a row
// passed kRowMaxPairs.
template <bool FILL>
struct AdvRowEmit {
    PairRaw *raw;
    int2 *rows;
    uint32_t at, end;    // pair slots
    uint32_t rat, rend;  // row slots
    uint32_t at_row;     // `at` at the last row()
    uint32_t over;
    __device__ __forceinline__ void half(bool right, const ObjEdge &E) const {
        if constexpr (FILL) {
            if (at < end) {
                float4 *q = reinterpret_cast<float4 *>(raw + at) + (right ? 3 : 0);
                pair_raw_half(E, q[0], q[1], q[2]);
            }
        }
    }
    __device__ __forceinline__ void pair(int32_t) { ++at; }
    __device__ __forceinline__ void row(int32_t Row) {
        const uint32_t k = at - at_row;
        if constexpr (FILL) {
            if (rat < rend) rows[rat] = make_int2(Row, (int32_t)k);
        }
        ++rat;
        at_row = at;
        if (k > kRowMaxPairs) over = 1u;
    }
};

// sbase / rbase: nlist + 1 values each, list o's pair slots [sbase[o],
// sbase[o + 1]) (floor(edge-rows / 2), as k_span_walk's) and row slots
// [rbase[o], rbase[o + 1]) (the rows of its walk, max(0, min(max YMax, height)
// - YMin[0])).  pcnt[o], rcnt[o]: the list's pairs and rows.  err bit 0: a
// list passed a range; bit 1: a row passed kRowMaxPairs pairs.  A one-edge
// list is walked too: its rows pair nothing and are queued all the same.
template <bool FILL>
__global__ void __launch_bounds__(kLinkThreads) k_row_walk(ObjEdge *__restrict__ work,
                                                           const uint32_t *__restrict__ lscan, uint32_t nlist,
                                                           const uint32_t *__restrict__ route, int32_t height,
                                                           const uint32_t *__restrict__ sbase,
                                                           const uint32_t *__restrict__ rbase,
                                                           PairRaw *__restrict__ raw, int2 *__restrict__ rows,
                                                           uint32_t *__restrict__ pcnt, uint32_t *__restrict__ rcnt,
                                                           uint32_t *__restrict__ err) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nlist || (route && route[o])) return;  // (routed: k_row_walk_wg walks and counts it)
    const uint32_t e0 = lscan[o], n = lscan[o + 1] - e0;
    uint32_t pairs = 0, nrow = 0;
    if (n >= 1) {
        const uint32_t s0 = FILL ? sbase[o] : 0u, s1 = FILL ? sbase[o + 1] : 0xFFFFFFFFu;
        const uint32_t r0 = FILL ? rbase[o] : 0u, r1 = FILL ? rbase[o + 1] : 0xFFFFFFFFu;
        AdvRowEmit<FILL> em{raw, rows, s0, s1, r0, r1, s0, 0u};
        adv_walk_list(work + e0, n, height, GLinks{work + e0}, em);
        pairs = em.at - s0;
        nrow = em.rat - r0;
        uint32_t bits = em.over ? 2u : 0u;
        if (FILL && (em.at > s1 || em.rat > r1)) {
            pairs = min(pairs, s1 - s0);
            nrow = min(nrow, r1 - r0);
            bits |= 1u;
        }
        if (bits) atomicOr(err, bits);
    }
    pcnt[o] = pairs;
    rcnt[o] = nrow;
}

// The used slots as packed records.  Workgroups [0, npb) pack the pairs,
// kPackSpans consecutive packed pairs each: lane t finds pair k's list as
// k_span_pack does (pscan: the scanned pair counts), reads its slot (six
// dwordx4) and puts the 24 dwords in prk_row_pair's interleaved order into LDS
// at dword kPairStride t.  24 t would put lanes 0, 4, 8, .. of a ds_write_b32
// group on one bank (24 t mod 32 takes four values); 25 is odd, so the 32
// lanes fall on 32 banks.  Then lane t of pass j stores dwordx4 t + 256 j of
// the workgroup's 24 KiB stretch of the output (1 KiB contiguous a wave
// instruction, every store 16-byte aligned: 96 bytes are six dwordx4), read
// from LDS as four dwords -- the odd stride leaves no 16-byte alignment for
// one ds_read_b128.  The workgroups after them copy the rows, one 8-byte
// record a lane, from list slots to packed position (rscan: the scanned row
// counts).
constexpr uint32_t kPairStride = 25u;
__global__ void __launch_bounds__(kPackSpans) k_row_pack(const PairRaw *__restrict__ raw,
                                                         const int2 *__restrict__ rows,
                                                         const uint32_t *__restrict__ sbase,
                                                         const uint32_t *__restrict__ rbase,
                                                         const uint32_t *__restrict__ pscan,
                                                         const uint32_t *__restrict__ rscan, uint32_t nlist,
                                                         uint32_t npair, uint32_t nrow, uint32_t npb,
                                                         uint4 *__restrict__ pairs_out, int2 *__restrict__ rows_out) {
    __shared__ float st[kPairStride * kPackSpans];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x >= npb) {  // (workgroup-uniform)
        const uint32_t k = (blockIdx.x - npb) * (uint32_t)kPackSpans + tid;
        if (k >= nrow) return;
        uint32_t lo = 0, hi = nlist;  // rscan[lo] <= k < rscan[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (rscan[mid] <= k) lo = mid;
            else hi = mid;
        }
        rows_out[k] = rows[(size_t)rbase[lo] + (k - rscan[lo])];
        return;
    }
    const uint32_t k0 = blockIdx.x * (uint32_t)kPackSpans;  // (< npair: npb)
    const uint32_t ns = min((uint32_t)kPackSpans, npair - k0);
    const uint32_t k = k0 + tid;
    if (tid < ns) {
        uint32_t lo = 0, hi = nlist;  // pscan[lo] <= k < pscan[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (pscan[mid] <= k) lo = mid;
            else hi = mid;
        }
        const PairRaw r = raw[(size_t)sbase[lo] + (k - pscan[lo])];
        float *d = st + kPairStride * tid;
        d[0] = r.l0.x; d[1] = r.r0.x;  // XMin
        d[2] = r.l0.y; d[3] = r.r0.y;  // ZMin
        d[4] = r.l0.z; d[5] = r.r0.z;  // OneOverZMin
        d[6] = r.l0.w; d[7] = r.r0.w;  // UMin
        d[8] = r.l1.x; d[9] = r.r1.x;  // VMin
        d[10] = r.l2.x; d[11] = r.l2.y; d[12] = r.l2.z; d[13] = r.l2.w;  // LeftMinColor
        d[14] = r.r2.x; d[15] = r.r2.y; d[16] = r.r2.z; d[17] = r.r2.w;  // RightMinColor
        d[18] = r.l1.y; d[19] = r.l1.z; d[20] = r.l1.w;                  // LeftMinNormal
        d[21] = r.r1.y; d[22] = r.r1.z; d[23] = r.r1.w;                  // RightMinNormal
    }
    __syncthreads();
    uint4 *dst = pairs_out + (size_t)k0 * 6u;
    for (uint32_t p = tid; p < 6u * ns; p += (uint32_t)kPackSpans) {
        const uint32_t t = p / 6u, q = p - 6u * t;
        const float *sp = st + kPairStride * t + 4u * q;
        dst[p] = make_uint4(__float_as_uint(sp[0]), __float_as_uint(sp[1]), __float_as_uint(sp[2]),
                            __float_as_uint(sp[3]));
    }
}

// prk_draw_rows: packed rows and pairs back into prk_draw_spans' records
// (packed prk_span, 25 dwords).  rows: the caller's prk_row records; rscan:
// their scanned EdgeCounts (nrow + 1 values, the last = npair).  A workgroup
// takes kPackSpans consecutive pairs: their 24 KiB come in as dwordx4 (lane t
// of pass j loads piece t + 256 j) and go to LDS at dword kPairStride * pair +
// word; lane t then reads pair t's 24 dwords (the odd stride: 32 banks for a
// group's 32 lanes), finds the pair's row -- the last row r with rscan[r] <=
// k, never one with EdgeCount 0 -- and writes the span's 25 dwords in prk_span's
// order over them: dwords [25 t, 25 t + 25) are lane t's alone, in and out.
// The stretch leaves as k_span_pack's does (`out`: 25 * npair dwords rounded
// up to four, the spare dwords zero).
__global__ void __launch_bounds__(kPackSpans) k_rows_unpack(const int2 *__restrict__ rows,
                                                            const uint32_t *__restrict__ rscan, uint32_t nrow,
                                                            const uint4 *__restrict__ pairs, uint32_t npair,
                                                            uint4 *__restrict__ out) {
    static_assert(kPairStride == 25u, "a pair's LDS stretch holds its span");
    __shared__ uint4 st4[kPackPieces];
    float *st = reinterpret_cast<float *>(st4);
    const uint32_t tid = threadIdx.x;
    const uint32_t k0 = blockIdx.x * (uint32_t)kPackSpans;  // (< npair: the grid)
    const uint32_t ns = min((uint32_t)kPackSpans, npair - k0);
    const uint4 *src = pairs + (size_t)k0 * 6u;
    for (uint32_t p = tid; p < 6u * ns; p += (uint32_t)kPackSpans) {
        const uint32_t t = p / 6u, q = p - 6u * t;
        const uint4 v = src[p];
        float *sp = st + kPairStride * t + 4u * q;
        sp[0] = __uint_as_float(v.x); sp[1] = __uint_as_float(v.y);
        sp[2] = __uint_as_float(v.z); sp[3] = __uint_as_float(v.w);
    }
    __syncthreads();
    if (tid < ns) {
        const uint32_t k = k0 + tid;
        uint32_t lo = 0, hi = nrow;  // rscan[lo] <= k < rscan[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (rscan[mid] <= k) lo = mid;
            else hi = mid;
        }
        float *d = st + kPairStride * tid;
        float w[24];
#pragma unroll
        for (int i = 0; i < 24; ++i) w[i] = d[i];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float *e = d + 12 * h;
            e[0] = w[0 + h]; e[1] = w[2 + h]; e[2] = w[4 + h]; e[3] = w[6 + h]; e[4] = w[8 + h];  // X Z W U V
            e[5] = w[10 + 4 * h]; e[6] = w[11 + 4 * h]; e[7] = w[12 + 4 * h]; e[8] = w[13 + 4 * h];  // MinColor
            e[9] = w[18 + 3 * h]; e[10] = w[19 + 3 * h]; e[11] = w[20 + 3 * h];                      // MinNormal
        }
        d[24] = __int_as_float(rows[lo].x);
    } else if (tid < ns + 1u) {
        st[25u * ns] = st[25u * ns + 1u] = st[25u * ns + 2u] = 0.0f;  // (the last piece's spare dwords; < 25 * 256)
    }
    __syncthreads();
    const uint32_t np = (25u * ns + 3u) / 4u;
    uint4 *dst = out + (size_t)blockIdx.x * kPackPieces;
    for (uint32_t p = tid; p < np; p += (uint32_t)kPackSpans) dst[p] = st4[p];
}
// The rows' EdgeCounts as one array for the scan (cnt[nrow] = 0: its total).
__global__ void __launch_bounds__(256) k_rows_counts(const int2 *__restrict__ rows, uint32_t nrow,
                                                     uint32_t *__restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= nrow) cnt[i] = i < nrow ? (uint32_t)rows[i].y : 0u;
}

// ---------------------------------------------------------------------------
// Span handles (prk_spans_*, prk_draw_span_records): packed prk_span records
// that stay in device memory, drawn from where they are.  One launch per
// recorded draw: spans [first, first + count) of the handle's buffer `spans`
// are the pass's objects obj0 .. obj0 + count - 1 (kind 4: one slot each, no
// other walk takes them) and take the winner ids g0 .. g0 + count - 1.
//
// The mirror image of k_span_pack.  A workgroup takes kHandleSpans consecutive
// spans: their 25 * ns dwords start at dword 25 * (first + j0) of the buffer,
// which is 16-byte aligned only when first + j0 is a multiple of four (25 = 1
// mod 4: the stretch starts `lead` = (first + j0) & 3 dwords into its first
// piece).  Lane t of pass j loads piece t + 256 j of the pieces the stretch
// touches (dwordx4, 1 KiB contiguous a wave instruction; the leading piece's
// first `lead` dwords and the trailing piece's spare ones belong to the
// neighbouring spans, or are the buffer's zero padding: read, never used) into
// LDS as they are (ds_write_b128 of consecutive slots).  Lane t then reads its
// span's 25 dwords at dword lead + 25 t: the stride is odd, so the 32 lanes of
// a ds_read_b32 group fall on 32 different banks.  The buffer holds 25 * total
// dwords rounded up to four (prk_span_pack's / k_rows_unpack's `out`), so the
// trailing piece is inside it.
//
// From there a lane is k_obj_walk's kind-2 branch: the band and target clip
// on Row, emit_span<MODE_AVX> with the draw's DRAW_ST and texture into the
// object's slot, row -1 in a slot no span takes.
constexpr int kHandleSpans = 256;
constexpr uint32_t kHandlePieces = 25u * kHandleSpans / 4u + 1u;  // (a stretch that starts inside a piece)
__global__ void __launch_bounds__(kHandleSpans) k_span_handle_walk(FrameParams fp, uint32_t draw, uint32_t g0,
                                                                   uint32_t obj0, const uint4 *__restrict__ spans,
                                                                   uint32_t first, uint32_t count,
                                                                   const unsigned long long *__restrict__ soff,
                                                                   SpanRecG *__restrict__ recs,
                                                                   SpanPos *__restrict__ pos,
                                                                   uint32_t *__restrict__ span_tri) {
    __shared__ uint4 st4[kHandlePieces];
    const uint32_t tid = threadIdx.x;
    const uint32_t j0 = blockIdx.x * (uint32_t)kHandleSpans;  // (< count: the grid)
    const uint32_t ns = min((uint32_t)kHandleSpans, count - j0);
    const unsigned long long w0 = 25ull * ((unsigned long long)first + j0);  // the stretch's first dword
    const uint32_t lead = (uint32_t)(w0 & 3ull);
    const uint32_t np = (lead + 25u * ns + 3u) / 4u;  // <= kHandlePieces
    const uint4 *src = spans + (w0 >> 2);
    for (uint32_t p = tid; p < np; p += (uint32_t)kHandleSpans) st4[p] = src[p];
    __syncthreads();
    if (tid >= ns) return;
    const float *w = reinterpret_cast<const float *>(st4) + lead + 25u * tid;
    SpanIn sp;
    {
        float v[25];
#pragma unroll
        for (int i = 0; i < 25; ++i) v[i] = w[i];
        static_assert(sizeof(SpanIn) == sizeof(v), "prk_span is 25 dwords");
        __builtin_memcpy(&sp, v, sizeof(sp));
    }
    const DrawRec &d = fp.draws[draw];
    const bool st = (d.flags & DRAW_ST) != 0;
    const uint32_t o = obj0 + j0 + tid;
    const uint32_t base = (uint32_t)soff[o], bound = (uint32_t)(soff[o + 1] - soff[o]);
    uint32_t used = 0;
    if (sp.Row >= fp.row0 && sp.Row < fp.row1 && sp.Row < fp.H && bound)
        used = emit_span<MODE_AVX>(fp, span_end_in(sp.L), span_end_in(sp.R), sp.Row, d, st, g0 + j0 + tid, true, base,
                                   recs, nullptr, pos, span_tri) ? 1u : 0u;
    for (uint32_t q = used; q < bound; ++q) pos[base + q] = SpanPos{-1, 0, 0, 0u};
}

// ---------------------------------------------------------------------------
// Long lists of the three record calls: one workgroup walks one list, the
// slot-list walk (walk_rows<M, false>'s row loop: read-ahead window,
// insert_one_b / insert_batch_b, the expiry compaction, the m == 0 row skip,
// a pair per thread and both swaps) without a frame -- adv_walk_list's rows
// [YMin[0], min(max YMax, height)), no band or target clip, every field
// stepped on the LDS state (adv_step_fields) and the thread walk's emission
// contract: an edge is seen as it stands on the row, before its step.
//
// The records' result.  A slot keeps its edge's sorted index in Next (as
// walk_rows' CHUNK mode does).  An entry's stepped state goes back to
// work[sorted index] -- the five quads adv_step stores, and its final Next --
// when it expires, and for the survivors after the last row.  The ordered
// array gives the reference's Next: on a row, after its insertions and before
// the removal, an expiring entry in the leading run of expiring entries gets
// -1 (the head expiry, 3715-3720); any other expiring entry keeps its
// successor's sorted index, whether that one expires too or not (3722-3749
// never writes the removed edge's own pointer); the last entry has -1.  After
// the last walked row every entry still listed gets its successor's sorted
// index, the last -1.  Edges never inserted stay as imported (Next -1).
//
// The hooks (every member holds the same value in every thread):
//   half(k, right, E, Row)  thread k, pair k of the row: one end before its step
//   row(Row, P, lead)       a row that is not skipped, P pairs (0 when one
//                           edge is listed); lead: the one thread that stores
// ---------------------------------------------------------------------------
struct WgNoEmit {
    __device__ __forceinline__ void half(int, bool, const ObjEdge &, int32_t) const {}
    __device__ __forceinline__ void row(int32_t, uint32_t, bool) {}
};
// Pair k of a row at slot at + k (k_span_pack's layout); the row with it.
template <bool STORE>
struct WgSpanEmit {
    PairRaw *raw;
    int32_t *prow;
    uint32_t at, end;
    __device__ __forceinline__ void half(int k, bool right, const ObjEdge &E, int32_t Row) const {
        if constexpr (STORE) {
            const uint32_t j = at + (uint32_t)k;
            if (j < end) {
                float4 *q = reinterpret_cast<float4 *>(raw + j) + (right ? 3 : 0);
                pair_raw_half(E, q[0], q[1], q[2]);
                if (!right) prow[j] = Row;
            }
        }
    }
    __device__ __forceinline__ void row(int32_t, uint32_t P, bool) { at += P; }
};
// The same pair slots (k_row_pack's layout) and {Row, P} into the next row slot.
template <bool FILL>
struct WgRowEmit {
    PairRaw *raw;
    int2 *rows;
    uint32_t at, end;    // pair slots
    uint32_t rat, rend;  // row slots
    uint32_t over;
    __device__ __forceinline__ void half(int k, bool right, const ObjEdge &E, int32_t) const {
        if constexpr (FILL) {
            const uint32_t j = at + (uint32_t)k;
            if (j < end) {
                float4 *q = reinterpret_cast<float4 *>(raw + j) + (right ? 3 : 0);
                pair_raw_half(E, q[0], q[1], q[2]);
            }
        }
    }
    __device__ __forceinline__ void row(int32_t Row, uint32_t P, bool lead) {
        if constexpr (FILL) {
            if (lead && rat < rend) rows[rat] = make_int2(Row, (int32_t)P);
        }
        ++rat;
        at += P;
        // (kept with the hook's contract; out of reach while the largest class
        // holds 1022 edges, 511 pairs: the 1000-pair rule is the thread walk's to test)
        if (P > kRowMaxPairs) over = 1u;
    }
};

// An entry's state back into its record: the quads adv_step stores, and Next.
__device__ __forceinline__ void adv_write_back(ObjEdge *__restrict__ dst, const ObjEdge &st, int32_t next) {
    const float4 *q = reinterpret_cast<const float4 *>(&st);
    float4 *d = reinterpret_cast<float4 *>(dst);
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2]; d[3] = q[3]; d[5] = q[5];
    dst->Next = next;
}

// E: the list's n >= 1 records (sorted, as imported); cap: the slot class
// (>= the most edges listed at once: the host's sweep); blockDim.x ==
// slot_threads(cap).  Every barrier is reached by the whole workgroup: the
// loop bounds and the branches around them are values every thread holds
// alike (Row, MaxY, m, ins, wb, top, k, lt, nanc, P).  A row with more new
// edges than free slots (never) sets err bit 0 and ends the walk for every
// thread at once; false then.
template <class EM>
__device__ bool adv_walk_rows(ObjEdge *__restrict__ E, uint32_t n, int32_t height, const SlotLds &S, BlockRed &R,
                              uint32_t cap, EM &em, uint32_t *__restrict__ err) {
    const int tid = threadIdx.x;
    const uint32_t NT = blockDim.x;
    int32_t mr = INT32_MIN;
    for (uint32_t i = tid; i < n; i += NT) mr = max(mr, E[i].YMax);
    const int32_t MaxY = min(blk_max(R, mr), height);
    const int32_t FirstRow = E[0].YMin;
    for (uint32_t q = tid; q < cap; q += NT) S.fs[q] = (int32_t)q;
    int top = (int)cap;
    int m = 0;
    uint32_t ins = 0;
    // read-ahead window: thread t holds sorted edge wb + t
    uint32_t wb = 0;
    PRK_WIN(wa);
    PRK_WIN_LOAD(wa, E, wb + (uint32_t)tid, n);
    PRK_WIN_WAIT();
    PRK_WIN_LAUNDER(wa);
    __syncthreads();
    for (int32_t Row = FirstRow; Row < MaxY; ++Row) {
        // insertion (3654-3713): the edges with YMin == Row, in sorted order,
        // a window at a time (batches in order == one at a time)
        for (;;) {
            if (ins == wb + NT) {
                wb += NT;
                PRK_WIN_LOAD(wa, E, wb + tid, n);
                PRK_WIN_WAIT();
                PRK_WIN_LAUNDER(wa);
            }
            const float wx = wa0.x, wg = wa0.y;
            const int32_t wymin = __float_as_int(wa4.x), wl = __float_as_int(wa4.z);
            const int rel = tid - (int)(ins - wb);
            const bool eqr = rel >= 0 && wymin == Row;
            int32_t lt, k, nanc;
            blk_sum3(R, (rel >= 0 && wymin < Row) ? 1 : 0, eqr ? 1 : 0, (eqr && (wx != wx || wg != wg)) ? 1 : 0, lt,
                     k, nanc);
            if (lt) {  // (never: the list is sorted and the walk starts on its first row)
                ins += (uint32_t)lt;
                continue;
            }
            if (k == 0) break;
            if (k > top) {  // (never: cap >= the most listed edges)
                if (tid == 0) atomicOr(err, 1u);
                return false;
            }
            if (rel >= 0 && rel < k) {  // the row's new edges take slots; their keys go to nk*
                const int32_t slot = S.fs[top - 1 - rel];
                PRK_WIN_STORE(&S.st[slot], wa);
                S.st[slot].Next = (int32_t)(ins + (uint32_t)rel);  // (its sorted index)
                S.nkx[rel] = wx;
                S.nkg[rel] = wg;
                S.nkl[rel] = wl;
                S.nks[rel] = slot;
            }
            top -= k;
            __syncthreads();
            if (k <= 2 || nanc) {  // one at a time (any NaN key), 3654-3713
                for (int t = 0; t < k; ++t) insert_one_b(S, R, m, LKey{S.nkx[t], S.nkg[t], S.nkl[t]}, S.nks[t]);
            } else {
                insert_batch_b(S, R, m, k);
            }
            ins += (uint32_t)k;
            if (ins < wb + NT) break;  // the row's edges end inside the window
        }
        {  // expiry 3715-3749: keep entries with YMax > Row, in order; the others' records and slots
            int32_t e = 0, se = -1;
            bool keep = false;
            if (tid < m) {
                e = S.idx[tid];
                keep = !(S.st[e].YMax <= Row);
                if (tid + 1 < m) se = S.idx[tid + 1];  // (its successor before the removal)
            }
            const bool gone = tid < m && !keep;
            int32_t kp, gp, kt, gt;
            blk_excl_sum2(R, keep ? 1 : 0, gone ? 1 : 0, kp, gp, kt, gt);
            if (gone) {  // kp == 0: nothing before it stays, the head expiry
                const int32_t nx = (kp == 0 || se < 0) ? -1 : S.st[se].Next;
                adv_write_back(&E[S.st[e].Next], S.st[e], nx);
                S.fs[top + gp] = e;
            }
            if (keep) S.idx[kp] = e;
            m = kt;
            top += gt;
            __syncthreads();
        }
        if (m == 0) {  // nothing happens on the rows before the next insertion: go there
            const int32_t nx = ins < n ? E[ins].YMin : INT32_MAX;
            Row = max(Row, min(nx, MaxY) - 1);
            continue;
        }
        const int P = m / 2;  // pairing 3751-3869: thread k holds pair k
        const bool valid = tid < P;
        int32_t i0 = 0, i1 = 0;
        float x0 = 0.0f, x1 = 0.0f;
        if (valid) {
            i0 = S.idx[2 * tid];
            i1 = S.idx[2 * tid + 1];
            ObjEdge a = S.st[i0];  // left edge: its values at the row, then its step (3811-3829)
            em.half(tid, false, a, Row);
            adv_step_fields(a);
            S.st[i0] = a;
            x0 = a.X;
            ObjEdge b = S.st[i1];  // right edge
            em.half(tid, true, b, Row);
            adv_step_fields(b);
            S.st[i1] = b;
            x1 = b.X;
            if (x0 > x1) {  // 3831-3841
                const int32_t t = i0; i0 = i1; i1 = t;
                const float f = x0; x0 = x1; x1 = f;
            }
            // pair k's entries after its first swap, for its neighbours
            S.nb[tid] = i0;
            S.bk[tid] = __float_as_int(x0);
            S.aux[tid] = i1;
            S.bk2[tid] = __float_as_int(x1);
        }
        __syncthreads();
        if (valid) {  // 3843-3853: pair k's first entry against pair k-1's second
            const bool sw = tid >= 1 && __int_as_float(S.bk2[tid - 1]) > x0;
            const bool swn = tid + 1 < P && x1 > __int_as_float(S.bk[tid + 1]);  // pair k+1's swap takes my second
            const int32_t nf = sw ? S.aux[tid - 1] : i0, ns = swn ? S.nb[tid + 1] : i1;
            i0 = nf;
            i1 = ns;
        }
        __syncthreads();
        if (valid) {
            S.idx[2 * tid] = i0;
            S.idx[2 * tid + 1] = i1;
        }
        em.row(Row, (uint32_t)P, tid == 0);
        __syncthreads();
    }
    // the list after the last walked row
    if (tid < m) {
        const int32_t e = S.idx[tid];
        const int32_t nx = tid + 1 < m ? S.st[S.idx[tid + 1]].Next : -1;
        adv_write_back(&E[S.st[e].Next], S.st[e], nx);
    }
    return true;
}

// lists: the indices of the lists of one slot class (`lcap` entries), one
// workgroup of slot_threads(lcap) threads each; dynamic LDS slot_lds_bytes(lcap).
__global__ void __launch_bounds__(kSlotMaxThreads) k_adv_walk_wg(ObjEdge *__restrict__ work,
                                                                 const uint32_t *__restrict__ lscan,
                                                                 const uint32_t *__restrict__ lists, uint32_t lcap,
                                                                 int32_t height, uint32_t *__restrict__ err) {
    extern __shared__ int32_t lds_list[];
    __shared__ BlockRed R;
    const uint32_t o = lists[blockIdx.x];
    const uint32_t e0 = lscan[o], n = lscan[o + 1] - e0;
    if (n == 0) return;  // (the whole workgroup; the host routes no empty list)
    SlotLds S;
    S.carve(lds_list, lcap, blockDim.x);
    WgNoEmit em;
    (void)adv_walk_rows(work + e0, n, height, S, R, lcap, em, err);
}
template <bool STORE>
__global__ void __launch_bounds__(kSlotMaxThreads) k_span_walk_wg(ObjEdge *__restrict__ work,
                                                                  const uint32_t *__restrict__ lscan,
                                                                  const uint32_t *__restrict__ lists, uint32_t lcap,
                                                                  int32_t height, const uint32_t *__restrict__ sbase,
                                                                  PairRaw *__restrict__ raw, int32_t *__restrict__ row,
                                                                  uint32_t *__restrict__ cnt,
                                                                  uint32_t *__restrict__ err) {
    extern __shared__ int32_t lds_list[];
    __shared__ BlockRed R;
    const uint32_t o = lists[blockIdx.x];
    const uint32_t e0 = lscan[o], n = lscan[o + 1] - e0;
    if (n == 0) return;
    SlotLds S;
    S.carve(lds_list, lcap, blockDim.x);
    const uint32_t s0 = STORE ? sbase[o] : 0u, s1 = STORE ? sbase[o + 1] : 0xFFFFFFFFu;
    WgSpanEmit<STORE> em{raw, row, s0, s1};
    (void)adv_walk_rows(work + e0, n, height, S, R, lcap, em, err);
    if (threadIdx.x == 0) {
        uint32_t pairs = em.at - s0;
        if (STORE && em.at > s1) {
            pairs = s1 - s0;
            atomicOr(err, 1u);
        }
        cnt[o] = pairs;
    }
}
template <bool FILL>
__global__ void __launch_bounds__(kSlotMaxThreads) k_row_walk_wg(ObjEdge *__restrict__ work,
                                                                 const uint32_t *__restrict__ lscan,
                                                                 const uint32_t *__restrict__ lists, uint32_t lcap,
                                                                 int32_t height, const uint32_t *__restrict__ sbase,
                                                                 const uint32_t *__restrict__ rbase,
                                                                 PairRaw *__restrict__ raw, int2 *__restrict__ rows,
                                                                 uint32_t *__restrict__ pcnt,
                                                                 uint32_t *__restrict__ rcnt,
                                                                 uint32_t *__restrict__ err) {
    extern __shared__ int32_t lds_list[];
    __shared__ BlockRed R;
    const uint32_t o = lists[blockIdx.x];
    const uint32_t e0 = lscan[o], n = lscan[o + 1] - e0;
    if (n == 0) return;
    SlotLds S;
    S.carve(lds_list, lcap, blockDim.x);
    const uint32_t s0 = FILL ? sbase[o] : 0u, s1 = FILL ? sbase[o + 1] : 0xFFFFFFFFu;
    const uint32_t r0 = FILL ? rbase[o] : 0u, r1 = FILL ? rbase[o + 1] : 0xFFFFFFFFu;
    WgRowEmit<FILL> em{raw, rows, s0, s1, r0, r1, 0u};
    (void)adv_walk_rows(work + e0, n, height, S, R, lcap, em, err);
    if (threadIdx.x == 0) {
        uint32_t pairs = em.at - s0, nrow = em.rat - r0;
        uint32_t bits = em.over ? 2u : 0u;
        if (FILL && (em.at > s1 || em.rat > r1)) {
            pairs = min(pairs, s1 - s0);
            nrow = min(nrow, r1 - r0);
            bits |= 1u;
        }
        if (bits) atomicOr(err, bits);
        pcnt[o] = pairs;
        rcnt[o] = nrow;
    }
}

}  // namespace prk

extern "C" {

// The record calls' thread walks.  `total` packed records (readable up to a
// multiple of 16 bytes) of a->nlist lists (a->lscan: their first edges) into
// the working copy a->work, walked over a->height rows there by a thread a
// list (lists with a route word are left to prk_list_walk_wg).
//   kind 0, prk_advance_edge_lists: prk_rec_export(work, nullptr, ...) packs
//     the result, prk_adv_next its links.
//   kind 1, prk_span_records: the walk with the emission: list o's pairs into
//     PairRaw slots [sbase[o], sbase[o + 1]) and their rows (prow), its count
//     into cnt[o]; err |= 1 should a list pass its slots.
//   kind 2, prk_row_records: the walk with the row emission: list o's pairs
//     into its PairRaw slots, its row records into row slots [rbase[o],
//     rbase[o + 1]), its counts into cnt[o] / rcnt[o]; err |= 1 as above, |= 2
//     when a row holds more than 1000 pairs.
// raw == nullptr (kinds 1, 2): the counts and err alone (no slots are read or
// written).
hipError_t prk_list_walk(int kind, const void *records, uint32_t total, const prk::ListWalkArgs *a, hipStream_t s) {
    if (kind < 0 || kind > 2) return hipErrorInvalidValue;
    const uint32_t nlist = a->nlist;
    if (total == 0 || nlist == 0) return hipSuccess;
    prk::ObjEdge *w = a->work;
    hipLaunchKernelGGL(prk::k_adv_import, dim3((total + prk::kPrepEdges - 1) / prk::kPrepEdges),
                       dim3(prk::kPrepEdges), 0, s, reinterpret_cast<const uint4 *>(records), total, w);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((nlist + prk::kLinkThreads - 1) / prk::kLinkThreads), block(prk::kLinkThreads);
    prk::PairRaw *pr = a->raw;
    if (kind == 0)
        hipLaunchKernelGGL(prk::k_adv_walk, grid, block, 0, s, w, a->lscan, nlist, a->route, a->height);
    else if (kind == 1 && pr)
        hipLaunchKernelGGL(prk::k_span_walk<true>, grid, block, 0, s, w, a->lscan, nlist, a->route, a->height,
                           a->sbase, pr, a->prow, a->cnt, a->err);
    else if (kind == 1)
        hipLaunchKernelGGL(prk::k_span_walk<false>, grid, block, 0, s, w, a->lscan, nlist, a->route, a->height,
                           a->sbase, (prk::PairRaw *)nullptr, (int32_t *)nullptr, a->cnt, a->err);
    else if (pr)
        hipLaunchKernelGGL(prk::k_row_walk<true>, grid, block, 0, s, w, a->lscan, nlist, a->route, a->height,
                           a->sbase, a->rbase, pr, a->rows, a->cnt, a->rcnt, a->err);
    else
        hipLaunchKernelGGL(prk::k_row_walk<false>, grid, block, 0, s, w, a->lscan, nlist, a->route, a->height,
                           a->sbase, a->rbase, (prk::PairRaw *)nullptr, (int2 *)nullptr, a->cnt, a->rcnt, a->err);
    return hipGetLastError();
}
// The `total` spans the walk left (cscan: the scanned counts, nlist + 1) as
// packed prk_span; `out` holds 25 * total dwords rounded up to four.
hipError_t prk_span_pack(const prk::PairRaw *raw, const int32_t *row, const uint32_t *sbase, const uint32_t *cscan,
                         uint32_t nlist, uint32_t total, void *out, hipStream_t s) {
    if (total == 0 || nlist == 0) return hipSuccess;
    hipLaunchKernelGGL(prk::k_span_pack, dim3((total + prk::kPackSpans - 1) / prk::kPackSpans),
                       dim3(prk::kPackSpans), 0, s, raw, row, sbase, cscan,
                       nlist, total, reinterpret_cast<uint4 *>(out));
    return hipGetLastError();
}
// The npair pairs and nrow rows the walk left (pscan, rscan: the scanned
// counts, nlist + 1 each) as packed prk_row_pair and prk_row.
hipError_t prk_row_pack(const prk::PairRaw *raw, const prk::RowRec *rows, const uint32_t *sbase, const uint32_t *rbase,
                        const uint32_t *pscan, const uint32_t *rscan, uint32_t nlist, uint32_t npair, uint32_t nrow,
                        void *pairs_out, prk::RowRec *rows_out, hipStream_t s) {
    if (nlist == 0 || (npair == 0 && nrow == 0)) return hipSuccess;
    const uint32_t npb = (npair + prk::kPackSpans - 1) / prk::kPackSpans;
    const uint32_t nrb = (nrow + prk::kPackSpans - 1) / prk::kPackSpans;
    hipLaunchKernelGGL(prk::k_row_pack, dim3(npb + nrb), dim3(prk::kPackSpans), 0, s,
                       raw, rows, sbase, rbase,
                       pscan, rscan, nlist, npair, nrow, npb, reinterpret_cast<uint4 *>(pairs_out), rows_out);
    return hipGetLastError();
}
// prk_draw_rows: the rows' EdgeCounts (nrow + 1 words, the last 0) for the
// scan, and npair packed pairs as packed prk_span (`out`: 25 * npair dwords
// rounded up to four), each on its row's RowIndex.
hipError_t prk_rows_counts(const prk::RowRec *rows, uint32_t nrow, uint32_t *cnt, hipStream_t s) {
    hipLaunchKernelGGL(prk::k_rows_counts, dim3(nrow / 256 + 1), dim3(256), 0, s,
                       rows, nrow, cnt);
    return hipGetLastError();
}
hipError_t prk_rows_unpack(const prk::RowRec *rows, const uint32_t *rscan, uint32_t nrow, const void *pairs,
                           uint32_t npair, void *out, hipStream_t s) {
    if (nrow == 0 || npair == 0) return hipSuccess;
    hipLaunchKernelGGL(prk::k_rows_unpack, dim3((npair + prk::kPackSpans - 1) / prk::kPackSpans),
                       dim3(prk::kPackSpans), 0, s, rows, rscan, nrow,
                       reinterpret_cast<const uint4 *>(pairs), npair, reinterpret_cast<uint4 *>(out));
    return hipGetLastError();
}
// One prk_draw_span_records draw of the pass: spans [first, first + count) of
// a handle's packed buffer into the slots of objects obj0 .. (k_span_handle_walk).
hipError_t prk_span_handle_walk(const prk::FrameParams *fp, uint32_t draw, uint32_t g0, uint32_t obj0,
                                const void *spans, uint32_t first, uint32_t count, const unsigned long long *soff,
                                prk::SpanRecG *recs, prk::SpanPos *pos, uint32_t *span_tri, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(prk::k_span_handle_walk, dim3((count + prk::kHandleSpans - 1) / prk::kHandleSpans),
                       dim3(prk::kHandleSpans), 0, s, *fp, draw, g0, obj0, reinterpret_cast<const uint4 *>(spans),
                       first, count, soff, recs, pos, span_tri);
    return hipGetLastError();
}
hipError_t prk_adv_next(const prk::ObjEdge *work, uint32_t total, int32_t *next_out, hipStream_t s) {
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(prk::k_adv_next, dim3((total + 255) / 256), dim3(256), 0, s,
                       work, total, next_out);
    return hipGetLastError();
}

// The record calls' workgroup walk (k_adv_walk_wg, k_span_walk_wg,
// k_row_walk_wg).  prk_adv_wg_lcap: the largest slot class the current device
// grants them as dynamic LDS (1022, 510 or 254; 0: none, every list stays on
// the thread walk).  `route` words: 0 the thread walk, c + 1 slot class c.
uint32_t prk_adv_wg_lcap(void) {
    static std::atomic<int> cap[64];  // per device: 0 unknown, else cap + 1
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int c = cap[dev].load();
    if (c == 0) {
        c = 1;
        const void *fn[5] = {reinterpret_cast<const void *>(&prk::k_adv_walk_wg),
                             reinterpret_cast<const void *>(&prk::k_span_walk_wg<true>),
                             reinterpret_cast<const void *>(&prk::k_span_walk_wg<false>),
                             reinterpret_cast<const void *>(&prk::k_row_walk_wg<true>),
                             reinterpret_cast<const void *>(&prk::k_row_walk_wg<false>)};
        for (uint32_t k = prk::kSlotCapLds; k >= 254; k = (k + 2) / 2 - 2) {
            const size_t bytes = prk::slot_lds_bytes(k);
            bool ok = true;
            for (int q = 0; q < 5 && ok; ++q)
                ok = hipFuncSetAttribute(fn[q], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
            if (ok) {
                c = (int)k + 1;
                break;
            }
            (void)hipGetLastError();
        }
        cap[dev].store(c);
    }
    return (uint32_t)(c - 1);
}
// The nl lists lists[0, nl) of slot class lcap, a workgroup each, after the
// call's import (prk_list_walk, whose thread kernels skip them); kind, a->raw
// and a->err as there.
hipError_t prk_list_walk_wg(int kind, uint32_t lcap, const uint32_t *lists, uint32_t nl,
                            const prk::ListWalkArgs *a, hipStream_t s) {
    if (nl == 0) return hipSuccess;
    if (lcap == 0 || lcap > prk_adv_wg_lcap()) return hipErrorInvalidValue;
    prk::ObjEdge *w = a->work;
    const dim3 grid(nl), block(prk::slot_threads(lcap));
    const size_t bytes = prk::slot_lds_bytes(lcap);
    prk::PairRaw *pr = a->raw;
    switch (kind) {
        case 0:
            hipLaunchKernelGGL(prk::k_adv_walk_wg, grid, block, bytes, s, w, a->lscan, lists, lcap, a->height,
                               a->err);
            break;
        case 1:
            if (pr)
                hipLaunchKernelGGL(prk::k_span_walk_wg<true>, grid, block, bytes, s, w, a->lscan, lists, lcap,
                                   a->height, a->sbase, pr, a->prow, a->cnt, a->err);
            else
                hipLaunchKernelGGL(prk::k_span_walk_wg<false>, grid, block, bytes, s, w, a->lscan, lists, lcap,
                                   a->height, a->sbase, (prk::PairRaw *)nullptr, (int32_t *)nullptr, a->cnt, a->err);
            break;
        case 2:
            if (pr)
                hipLaunchKernelGGL(prk::k_row_walk_wg<true>, grid, block, bytes, s, w, a->lscan, lists, lcap,
                                   a->height, a->sbase, a->rbase, pr, a->rows, a->cnt, a->rcnt, a->err);
            else
                hipLaunchKernelGGL(prk::k_row_walk_wg<false>, grid, block, bytes, s, w, a->lscan, lists, lcap,
                                   a->height, a->sbase, a->rbase, (prk::PairRaw *)nullptr, (int2 *)nullptr, a->cnt,
                                   a->rcnt, a->err);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // extern "C"
