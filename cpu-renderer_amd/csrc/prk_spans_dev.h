// prk_spans_dev.h — the span path's device functions and row arithmetic that
// prk_spans.hip and prk_records.hip share, each defined here once.  The
// records they read and write (ObjEdge, SpanPos, SpanRecG, ScSpanRec, PairRaw,
// EdgeIn, SpanIn) are prk_types.h's.
#pragma once

#include "prk_device.h"
#include "prk_launch.h"

namespace prk {
// An ObjEdge from FillEdgeTable's edge.
__device__ __forceinline__ void obj_edge_store(ObjEdge &o, const Edge &E) {
    o.X = E.X; o.G = E.G; o.Z = E.Z; o.ZG = E.ZG; o.W = E.W; o.WG = E.WG;
    o.U = E.U; o.UG = E.UG; o.V = E.V; o.VG = E.VG;
    o.N0 = E.N0; o.N1 = E.N1; o.N2 = E.N2; o.NG0 = E.NG0; o.NG1 = E.NG1; o.NG2 = E.NG2;
    o.YMin = E.YMin; o.YMax = E.YMax; o.Left = E.Left; o.Next = -1;
    o.C0 = E.C0; o.C1 = E.C1; o.C2 = E.C2; o.C3 = E.C3;
    o.CG0 = E.CG0; o.CG1 = E.CG1; o.CG2 = E.CG2; o.CG3 = E.CG3;
}

// AET insertion order (3663-3667).
__device__ __forceinline__ bool obj_before(const ObjEdge &A, const ObjEdge &B) {
    return A.X < B.X || (A.X == B.X && (A.G < B.G || (A.G == B.G && A.Left < B.Left)));
}

// Edge step (3811-3829 / DrawModel 542-560), the fields mode M reads: AVX
// semantics X, Z, the normal, U, V, 1/z (the colour lanes are dead,
// 2029-2032); DrawModel also the colour (Gouraud) and drops what its mode
// never reads (ModeTraits).
template <int M>
__device__ __forceinline__ void obj_step(ObjEdge &E) {
    using TR = ModeTraits<M>;
    E.X += E.G;
    E.Z += E.ZG;
    if (TR::color) { E.C0 += E.CG0; E.C1 += E.CG1; E.C2 += E.CG2; E.C3 += E.CG3; }
    if (TR::phong) {
        float x = E.N0 + E.NG0, y = E.N1 + E.NG1, z = E.N2 + E.NG2;
        normalize_rcp(x, y, z);
        E.N0 = x; E.N1 = y; E.N2 = z;
    }
    if (TR::tex) {
        E.U += E.UG;
        E.V += E.VG;
        E.W += E.WG;
    }
}

// FillLineOptimized span setup (1543-1835) of the pair (L, R) at Row: the
// lane-init record and the covered range [MinX, MaxX).  False when the span
// covers nothing.
__device__ __forceinline__ bool obj_span(const FrameParams &fp, const ObjEdge &L, const ObjEdge &R, int32_t Row,
                                         int32_t texi, bool st, SpanRecG &rec, SpanPos &pos) {
    float XOffset;
    int32_t MinX, MaxX, XDiff;
    if (!span_ends(L.X, R.X, fp.W, st, MinX, MaxX, XDiff, XOffset)) return false;  // 1545-1592
    if (MinX >= MaxX) return false;
    int32_t LeftXa = MinX;
    if (MinX & 7) {  // 1594-1609
        LeftXa = MinX & ~7;
        XOffset -= (float)(MinX & 7) * 1.0f;
    }
    const float fXD = (float)XDiff;
    float IW = 0, IU = 0, IV = 0, IZ = 0, IN0 = 0, IN1 = 0, IN2 = 0;
    if (XDiff != 0) {  // 1666-1835
        // the span's increments over XDiff (div_all: one shared reciprocal)
        float q[7] = {R.W - L.W, R.U - L.U, R.V - L.V, R.N0 - L.N0, R.N1 - L.N1, R.N2 - L.N2, R.Z - L.Z};
        div_all(fXD, q);
        IW = q[0]; IU = q[1]; IV = q[2]; IN0 = q[3]; IN1 = q[4]; IN2 = q[5]; IZ = q[6];
    }
    rec.q0 = make_float4(__int_as_float((LeftXa & 0xFFFF) | (texi << 16)), XOffset, L.W, L.U);
    rec.q1 = make_float4(L.V, L.Z, IW, IU);
    rec.q2 = make_float4(IV, IZ, L.N0, L.N1);
    rec.q3 = make_float4(L.N2, IN0, IN1, IN2);
    pos.row = Row;
    pos.minx = MinX;
    pos.maxx = MaxX;
    pos.flags = st ? DRAW_ST : 0u;
    return true;
}

// DrawModel span setup (projekt.cpp:298-412) of the pair (L, R) at Row for
// mode M: the values at MinX (Current* += XOffset * Increment) and the
// per-pixel increments, as span_setup_scalar (prk_kernels.hip) computes them
// for the per-triangle sweeps, and the inclusive range [MinX, MaxX] (MaxX may
// be W: the one-past-the-row store into (Row + 1, 0)).  False when the span
// draws nothing (a NaN end: pinned).
template <int M>
__device__ __forceinline__ bool obj_span_scalar(const FrameParams &fp, const ObjEdge &L, const ObjEdge &R, int32_t Row,
                                                int32_t texi, ScSpanRec &rec, SpanPos &pos) {
    using TR = ModeTraits<M>;
    const int32_t W = fp.W;
    float XOffset = 0.0f;
    const float XDiff = roundf(R.X - L.X);  // 311-312
    float IW = 0, IU = 0, IV = 0, IZ = 0, IN0 = 0, IN1 = 0, IN2 = 0;
    float IC0 = 0, IC1 = 0, IC2 = 0, IC3 = 0;
    if (XDiff != 0.0f) {  // 329-360
        constexpr bool kT = TR::tex, kP = TR::phong, kC = TR::color;
        float q[1 + (kT ? 3 : 0) + (kP ? 3 : 0) + (kC ? 4 : 0)];
        int qi = 0;
        q[qi++] = R.Z - L.Z;
        if (kT) { q[qi++] = R.W - L.W; q[qi++] = R.U - L.U; q[qi++] = R.V - L.V; }
        if (kP) { q[qi++] = R.N0 - L.N0; q[qi++] = R.N1 - L.N1; q[qi++] = R.N2 - L.N2; }
        if (kC) { q[qi++] = R.C0 - L.C0; q[qi++] = R.C1 - L.C1; q[qi++] = R.C2 - L.C2; q[qi++] = R.C3 - L.C3; }
        div_all(XDiff, q);
        qi = 0;
        IZ = q[qi++];
        if (kT) { IW = q[qi++]; IU = q[qi++]; IV = q[qi++]; }
        if (kP) { IN0 = q[qi++]; IN1 = q[qi++]; IN2 = q[qi++]; }
        if (kC) { IC0 = q[qi++]; IC1 = q[qi++]; IC2 = q[qi++]; IC3 = q[qi++]; }
    }
    float LeftX = L.X;  // 381-400
    if (LeftX < 0) { XOffset = -L.X; LeftX = 0; }
    else if (LeftX >= W) LeftX = (float)W - 1;
    float RightX = R.X;
    if (RightX < 0) RightX = 0;
    else if (RightX >= W) RightX = (float)W - 1;
    if (LeftX != LeftX || RightX != RightX) return false;
    const int32_t MinX = round_s32(LeftX), MaxX = round_s32(RightX);  // 402-406
    if (MaxX < MinX) return false;
    for (int k = 0; k < 22; ++k) rec.f[k] = 0.0f;
    rec.f[0] = L.Z + XOffset * IZ;  // 408-412 (SS_Z, SS_IZ)
    rec.f[1] = IZ;
    if (TR::tex) {  // SS_W, SS_U, SS_V, SS_IW, SS_IU, SS_IV
        rec.f[2] = L.W + XOffset * IW; rec.f[5] = IW;
        rec.f[3] = L.U + XOffset * IU; rec.f[6] = IU;
        rec.f[4] = L.V + XOffset * IV; rec.f[7] = IV;
    }
    if (TR::phong) {  // SS_N0..2, SS_IN0..2
        rec.f[8] = L.N0 + XOffset * IN0; rec.f[11] = IN0;
        rec.f[9] = L.N1 + XOffset * IN1; rec.f[12] = IN1;
        rec.f[10] = L.N2 + XOffset * IN2; rec.f[13] = IN2;
    }
    if (TR::color) {  // SS_C0..3, SS_IC0..3
        rec.f[14] = L.C0 + XOffset * IC0; rec.f[18] = IC0;
        rec.f[15] = L.C1 + XOffset * IC1; rec.f[19] = IC1;
        rec.f[16] = L.C2 + XOffset * IC2; rec.f[20] = IC2;
        rec.f[17] = L.C3 + XOffset * IC3; rec.f[21] = IC3;
    }
    rec.tex = TR::tex ? texi : 0;
    rec.pad = 0;
    pos.row = Row;
    pos.minx = MinX;
    pos.maxx = MaxX + 1;
    pos.flags = SPAN_SCALAR | ((uint32_t)M << 8);
    return true;
}

__device__ __forceinline__ void obj_edge_in(ObjEdge &o, const EdgeIn &e) {
    o.X = e.XMin; o.G = e.Gradient; o.Z = e.ZMin; o.ZG = e.ZGradient; o.W = e.OneOverZMin;
    o.WG = e.OneOverZGradient; o.U = e.UMin; o.UG = e.UGradient; o.V = e.VMin; o.VG = e.VGradient;
    o.N0 = e.MinNormal[0]; o.N1 = e.MinNormal[1]; o.N2 = e.MinNormal[2];
    o.NG0 = e.NormalGradient[0]; o.NG1 = e.NormalGradient[1]; o.NG2 = e.NormalGradient[2];
    o.YMin = e.YMin; o.YMax = e.YMax; o.Left = e.Left; o.Next = -1;
    o.C0 = e.MinColor[0]; o.C1 = e.MinColor[1]; o.C2 = e.MinColor[2]; o.C3 = e.MinColor[3];
    o.CG0 = e.ColorGradient[0]; o.CG1 = e.ColorGradient[1]; o.CG2 = e.ColorGradient[2];
    o.CG3 = e.ColorGradient[3];
}
__device__ __forceinline__ ObjEdge span_end_in(const SpanEndIn &e) {  // FillLinesOptimized 648-670
    ObjEdge o;
    o.X = e.XMin; o.Z = e.ZMin; o.W = e.OneOverZMin; o.U = e.UMin; o.V = e.VMin;
    o.N0 = e.MinNormal[0]; o.N1 = e.MinNormal[1]; o.N2 = e.MinNormal[2];
    o.G = o.ZG = o.WG = o.UG = o.VG = o.NG0 = o.NG1 = o.NG2 = 0.0f;
    o.C0 = e.MinColor[0]; o.C1 = e.MinColor[1]; o.C2 = e.MinColor[2]; o.C3 = e.MinColor[3];
    o.CG0 = o.CG1 = o.CG2 = o.CG3 = 0.0f;
    o.YMin = o.YMax = o.Left = 0;
    o.Next = -1;
    return o;
}

// One span of the pair (L, R) at Row, written at span slot `at` (when `write`).
template <int M>
__device__ __forceinline__ bool emit_span(const FrameParams &fp, const ObjEdge &L, const ObjEdge &R, int32_t Row,
                                          const DrawRec &d, bool st, uint32_t g0, bool write, uint32_t at,
                                          SpanRecG *__restrict__ recs, ScSpanRec *__restrict__ srecs,
                                          SpanPos *__restrict__ pos, uint32_t *__restrict__ span_tri) {
    SpanPos sp;
    if constexpr (M != MODE_AVX) {
        ScSpanRec srec;
        if (!obj_span_scalar<M>(fp, L, R, Row, d.tex, srec, sp)) return false;
        if (write) {
            SpanRecG mark;
            mark.q0 = make_float4(__uint_as_float(kScalarSpan), 0.0f, 0.0f, 0.0f);
            mark.q1 = mark.q2 = mark.q3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            recs[at] = mark;
            srecs[at] = srec;
        }
    } else {
        SpanRecG rec;
        if (!obj_span(fp, L, R, Row, d.tex, st, rec, sp)) return false;
        if (write) recs[at] = rec;
    }
    if (write) {
        pos[at] = sp;
        span_tri[at] = g0;
    }
    return true;
}

// The list fields of the thread walk (links, keys, row range), read and
// written through one of two stores: the working copy itself (GLinks), or
// per-thread LDS mirrors (LLinks: objects of at most kLinkCap edges), so the
// list's chains of dependent accesses (insertion scans, expiry, pairing and
// swaps) run at LDS latency; the edge records stay in device memory, read
// for a span and stepped per pair, off those chains.  LLinks steps its X
// mirror with obj_step's own add.
struct GLinks {
    ObjEdge *E;
    __device__ __forceinline__ int32_t next(int i) const { return E[i].Next; }
    __device__ __forceinline__ void set_next(int i, int32_t v) const { E[i].Next = v; }
    __device__ __forceinline__ float x(int i) const { return E[i].X; }
    __device__ __forceinline__ int32_t ymin(int i) const { return E[i].YMin; }
    __device__ __forceinline__ int32_t ymax(int i) const { return E[i].YMax; }
    __device__ __forceinline__ bool before(int a, int b) const { return obj_before(E[a], E[b]); }
    __device__ __forceinline__ void stepped(int) const {}  // (obj_step stepped E[i].X)
    static constexpr bool kCache = false;  // (the list reads the records' X and links)
};
constexpr int kLinkThreads = 64;  // k_obj_walk's workgroup

// An edge record held in seven named float4 registers (ObjEdge's layout): a
// loop-carried ObjEdge went to scratch.
#define PRK_ER(w) float4 w##0, w##1, w##2, w##3, w##4, w##5, w##6
#define PRK_ER_ZERO(w) \
    do { w##0 = w##1 = w##2 = w##3 = w##4 = w##5 = w##6 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); } while (0)
#define PRK_ER_LOAD(w, p)                                                      \
    do {                                                                       \
        const float4 *s_ = reinterpret_cast<const float4 *>(p);               \
        w##0 = s_[0]; w##1 = s_[1]; w##2 = s_[2]; w##3 = s_[3];               \
        w##4 = s_[4]; w##5 = s_[5]; w##6 = s_[6];                             \
    } while (0)
#define PRK_ER_STORE(p, w)                                                     \
    do {                                                                       \
        float4 *d_ = reinterpret_cast<float4 *>(p);                           \
        d_[0] = w##0; d_[1] = w##1; d_[2] = w##2; d_[3] = w##3;               \
        d_[4] = w##4; d_[5] = w##5; d_[6] = w##6;                             \
    } while (0)
#define PRK_ER_SWAP(a, b)                                                                 \
    do {                                                                                  \
        float4 t_;                                                                        \
        t_ = a##0; a##0 = b##0; b##0 = t_; t_ = a##1; a##1 = b##1; b##1 = t_;             \
        t_ = a##2; a##2 = b##2; b##2 = t_; t_ = a##3; a##3 = b##3; b##3 = t_;             \
        t_ = a##4; a##4 = b##4; b##4 = t_; t_ = a##5; a##5 = b##5; b##5 = t_;             \
        t_ = a##6; a##6 = b##6; b##6 = t_;                                                \
    } while (0)
__device__ __forceinline__ ObjEdge er_edge(float4 q0, float4 q1, float4 q2, float4 q3, float4 q4, float4 q5,
                                           float4 q6) {
    ObjEdge e;
    e.X = q0.x; e.G = q0.y; e.Z = q0.z; e.ZG = q0.w;
    e.W = q1.x; e.WG = q1.y; e.U = q1.z; e.UG = q1.w;
    e.V = q2.x; e.VG = q2.y; e.N0 = q2.z; e.N1 = q2.w;
    e.N2 = q3.x; e.NG0 = q3.y; e.NG1 = q3.z; e.NG2 = q3.w;
    e.YMin = __float_as_int(q4.x); e.YMax = __float_as_int(q4.y); e.Left = __float_as_int(q4.z);
    e.Next = __float_as_int(q4.w);
    e.C0 = q5.x; e.C1 = q5.y; e.C2 = q5.z; e.C3 = q5.w;
    e.CG0 = q6.x; e.CG1 = q6.y; e.CG2 = q6.z; e.CG3 = q6.w;
    return e;
}
#define PRK_ER_EDGE(w) er_edge(w##0, w##1, w##2, w##3, w##4, w##5, w##6)
#define PRK_ER_FROM(w, e)                                                                              \
    do {                                                                                               \
        w##0 = make_float4((e).X, (e).G, (e).Z, (e).ZG);                                               \
        w##1 = make_float4((e).W, (e).WG, (e).U, (e).UG);                                              \
        w##2 = make_float4((e).V, (e).VG, (e).N0, (e).N1);                                             \
        w##3 = make_float4((e).N2, (e).NG0, (e).NG1, (e).NG2);                                         \
        w##5 = make_float4((e).C0, (e).C1, (e).C2, (e).C3);                                            \
    } while (0)  /* (q4, q6: row range, link, colour gradient — not stepped) */

// A pair of the slot walk, before its span setup: both edges' values at the
// row (the fields obj_span / obj_span_scalar read), written by the walk; its
// SpanPos holds the row, the draw (in minx) and SPAN_RAW until k_span_finish
// turns it into the span's record (or row -1 when it covers nothing).  The
// setup's ~300 instructions per span leave the walk's row-serial path.
constexpr uint32_t SPAN_RAW = 0x40000000u;
// One edge's half of a PairRaw (pair_raw_in reads it back).
__device__ __forceinline__ void pair_raw_half(const ObjEdge &e, float4 &q0, float4 &q1, float4 &q2) {
    q0 = make_float4(e.X, e.Z, e.W, e.U);
    q1 = make_float4(e.V, e.N0, e.N1, e.N2);
    q2 = make_float4(e.C0, e.C1, e.C2, e.C3);
}
__device__ __forceinline__ void pair_raw_out(const ObjEdge &a, const ObjEdge &b, PairRaw &o) {
    pair_raw_half(a, o.l0, o.l1, o.l2);
    pair_raw_half(b, o.r0, o.r1, o.r2);
}
__device__ __forceinline__ ObjEdge pair_raw_in(const float4 &q0, const float4 &q1, const float4 &q2) {
    ObjEdge e = ObjEdge{};
    e.X = q0.x; e.Z = q0.y; e.W = q0.z; e.U = q0.w;
    e.V = q1.x; e.N0 = q1.y; e.N1 = q1.z; e.N2 = q1.w;
    e.C0 = q2.x; e.C1 = q2.y; e.C2 = q2.z; e.C3 = q2.w;
    return e;
}

// ---- packed prk_edge records into ObjEdges (k_list_prep*; k_adv_import, prk_records.hip) ----
// (kPrepEdges, prk_launch.h: the edges a workgroup takes)
struct PrepMap {
    uint8_t f[28];  // ObjEdge dword -> prk_edge field (27: none, the link)
};
constexpr PrepMap prep_map() {
    // prk_edge field f -> ObjEdge dword (k_rec_export's kWord)
    constexpr uint8_t kWord[27] = {17, 0, 2, 4, 1, 3, 5, 16, 6, 8, 7, 9, 18, 20, 21, 22, 23,
                                   24, 25, 26, 27, 10, 11, 12, 13, 14, 15};
    PrepMap m{};
    for (int d = 0; d < 28; ++d) m.f[d] = 27;
    for (int f = 0; f < 27; ++f) m.f[kWord[f]] = (uint8_t)f;
    return m;
}
// The ne records at `rec` (LDS, 27 dwords each) as ObjEdges at dst_edges[0 .. ne):
// lane t of pass k stores dwordx4 number t + 256 k.
__device__ __forceinline__ void prep_convert(const uint32_t *rec, uint32_t ne, ObjEdge *__restrict__ dst_edges) {
    static constexpr PrepMap kMap = prep_map();
    static_assert(kMap.f[19] == 27 && kMap.f[16] == 7 && kMap.f[17] == 0, "ObjEdge: Next, YMin, YMax");
    const uint32_t tid = threadIdx.x;
    float4 *dst = reinterpret_cast<float4 *>(dst_edges);
    for (uint32_t j = tid; j < 7u * ne; j += (uint32_t)kPrepEdges) {
        const uint32_t e = j / 7u, q = j - 7u * e;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // (q is not a constant: the map is read from a small table)
            const uint32_t f = kMap.f[4 * q + k];
            v[k] = f < 27u ? rec[27u * e + f] : 0xFFFFFFFFu;
        }
        dst[j] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                             __uint_as_float(v[3]));
    }
}
// A workgroup's records into LDS and on into the working copy: edges
// [e_first, e_first + ne) of the flat input as ObjEdges at dst[0 .. ne)
// (shared by k_list_prep and k_adv_import; ends in a barrier, so the callers
// read `rec4` after it).  Returns ne.
constexpr uint32_t kPrepPieces = 27u * kPrepEdges / 4u;  // 16-byte pieces a full workgroup reads
static_assert(27 * kPrepEdges % 4 == 0, "a workgroup's records start on a 16-byte boundary");
__device__ __forceinline__ uint32_t prep_records(const uint4 *__restrict__ in, uint32_t nedge, uint4 *rec4,
                                                 ObjEdge *__restrict__ dst_edges) {
    const uint32_t tid = threadIdx.x;
    const uint32_t e_first = blockIdx.x * (uint32_t)kPrepEdges;  // (< nedge: the grid)
    const uint32_t ne = min((uint32_t)kPrepEdges, nedge - e_first);
    const uint32_t np = (27u * ne + 3u) / 4u;
    const uint4 *src = in + (size_t)blockIdx.x * kPrepPieces;
    for (uint32_t p = tid; p < np; p += (uint32_t)kPrepEdges) rec4[p] = src[p];
    __syncthreads();
    prep_convert(reinterpret_cast<const uint32_t *>(rec4), ne, dst_edges);
    return ne;
}
}  // namespace prk
