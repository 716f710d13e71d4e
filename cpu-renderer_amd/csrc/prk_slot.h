// prk_slot.h — the slot list of the workgroup walks (walk_rows, prk_spans.hip;
// adv_walk_rows, prk_records.hip) and their read-ahead window of sorted edges.
#pragma once

#include "prk_spans_dev.h"
#include "prk_wave.h"

namespace prk {
// ---------------------------------------------------------------------------
// The same walk by a whole workgroup, everything in LDS (objects whose most
// active edges fit the launch's capacity C <= 1022): the listed edges'
// mutable state in C slots (a free-slot stack), and the list as an array of
// slot numbers only — its operations move one int per entry and read the
// keys (X, Gradient, Left, YMax) from the slots.  The workgroup has NT >= C + 2
// threads, so every list operation is one step: thread q holds entry q, the
// scans and searches are workgroup scans (a DPP wave scan plus the waves'
// totals through LDS).  A lone wave walking a long list in 64-entry chunks
// ran each row's chain of dependent steps chunk after chunk (C2 as one
// object: ~80 k clocks a row); here a row is ~20 barriers.  A row touches
// device memory only for the sorted edges it inserts (read ahead NT at a
// time, one per thread) and the pairs it writes.  Pairing: thread k holds
// pair k, does its first swap (3831-3841) itself and its second (3843-3853)
// against pair k-1's second entry through LDS.
// ---------------------------------------------------------------------------
constexpr uint32_t kSlotCapLds = 1022;  // the slot-list walk's largest LDS capacity (listed edges; 1024 threads)
constexpr int kSlotListArrays = 5;  // int arrays of cap + 2: idx (slots), aux, nb, bk, bk2
constexpr uint32_t kSlotMaxThreads = 1024;
__host__ __device__ constexpr uint32_t slot_threads(uint32_t cap) {  // NT: >= cap + 2, a multiple of 64
    return ((cap + 2 + 63) / 64) * 64 > kSlotMaxThreads ? kSlotMaxThreads : ((cap + 2 + 63) / 64) * 64;
}
struct SlotLds {
    int32_t *idx;  // the list: slot of each entry, in list order
    int32_t *aux, *nb, *bk, *bk2;  // insertion / pairing scratch
    float *nkx, *nkg;              // the batch's new edges: keys (x, g, l) and slots, NT each
    int32_t *nkl, *nks;
    int32_t *fs;   // free slots: fs[0, top)
    ObjEdge *st;   // edge state per slot
    __device__ __forceinline__ void carve(int32_t *base, uint32_t cap, uint32_t nt) {
        const size_t s = (size_t)cap + 2;
        idx = base;
        aux = base + s;
        nb = base + 2 * s;
        bk = base + 3 * s;
        bk2 = base + 4 * s;
        int32_t *k = base + kSlotListArrays * s;
        nkx = reinterpret_cast<float *>(k);
        nkg = reinterpret_cast<float *>(k + nt);
        nkl = k + 2 * nt;
        nks = k + 3 * nt;
        fs = k + 4 * nt;
        const size_t off = ((size_t)kSlotListArrays * s + 4 * (size_t)nt + cap) * 4;
        st = reinterpret_cast<ObjEdge *>(reinterpret_cast<char *>(base) + ((off + 15) & ~(size_t)15));
    }
    __device__ __forceinline__ LKey key(int32_t sl) const {
        return entry_key(st[sl].X, st[sl].G, st[sl].Left);
    }
};
__host__ __device__ constexpr size_t slot_lds_bytes(uint32_t cap) {
    return ((((size_t)kSlotListArrays * (cap + 2) + 4 * (size_t)slot_threads(cap) + cap) * 4 + 15) & ~(size_t)15) +
           (size_t)cap * sizeof(ObjEdge);
}
// The record calls' slot classes (prk_launch.h): each fills its workgroup, the largest is the LDS capacity.
static_assert(slot_threads(kAdvWgCaps[0]) == kAdvWgCaps[0] + 2 && slot_threads(kAdvWgCaps[1]) == kAdvWgCaps[1] + 2 &&
                  slot_threads(kAdvWgCaps[2]) == kAdvWgCaps[2] + 2 && slot_threads(kAdvWgCaps[3]) == kAdvWgCaps[3] + 2 &&
                  slot_threads(kAdvWgCaps[4]) == kAdvWgCaps[4] + 2 && kAdvWgCaps[4] == kSlotCapLds,
              "kAdvWgCaps are the slot walk's classes");

// One new edge (key c, slot sl) before the first entry it sorts before
// (3663-3667), else at the tail (thread q: entry q).
__device__ void insert_one_b(const SlotLds &S, BlockRed &R, int &m, const LKey &c, int32_t sl) {
    const int q = threadIdx.x;
    bool b = false;
    if (q < m) {
        const int32_t e = S.idx[q];
        const float x = S.st[e].X, g = S.st[e].G;
        b = c.x < x || (c.x == x && (c.g < g || (c.g == g && c.l < S.st[e].Left)));
    }
    const int p = min(blk_first(R, b), m);
    const bool mv = q >= p && q < m;  // entries [p, m) move up one
    const int32_t v = mv ? S.idx[q] : 0;
    __syncthreads();
    if (mv) S.idx[q + 1] = v;
    if (q == 0) S.idx[p] = sl;
    __syncthreads();
    ++m;
}

// The k new edges of the batch (S.nk*[0, k), in insertion order, no NaN key)
// inserted at once with the result of inserting them one by one (see
// insert_batch: each new edge lands at its gap + the new edges of earlier
// gaps + those of its gap ordered before it; entry q moves up by the new
// edges of gaps <= q).  Thread q: entry q and new edge q.
__device__ void insert_batch_b(const SlotLds &S, BlockRed &R, int &m, int k) {
    const int q = threadIdx.x;
    const bool mine = q < k;
    // 1. PM(q) = the maximum key of entries [0, q], its (x, g, l) in (nb, bk, aux)
    float *pmx = reinterpret_cast<float *>(S.nb), *pmg = reinterpret_cast<float *>(S.bk);
    {
        LKey kk{-INFINITY, -INFINITY, INT32_MIN};
        if (q < m) kk = S.key(S.idx[q]);
        blk_key_prefix_max(R, kk);
        if (q < m) { pmx[q] = kk.x; pmg[q] = kk.g; S.aux[q] = kk.l; }
    }
    __syncthreads();
    // 2. the gap of new edge q: binary search over the non-decreasing PM
    LKey kc{0.0f, 0.0f, 0};
    int32_t rs = 0, gq = 0;
    if (mine) {
        kc = LKey{S.nkx[q], S.nkg[q], S.nkl[q]};
        rs = S.nks[q];
        int lo = 0, hi = m;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key_gt(LKey{pmx[mid], pmg[mid], S.aux[mid]}, kc)) hi = mid;
            else lo = mid + 1;
        }
        gq = lo;
    }
    __syncthreads();
    // 3. gap histogram (aux[0, m + 2)), each new edge's arrival slot in its gap
    if (q < m + 2) S.aux[q] = 0;
    __syncthreads();
    int32_t arr = 0;
    if (mine) arr = atomicAdd(&S.aux[gq], 1);
    __syncthreads();
    {  // 4. exclusive scan: aux[g] = new edges of gaps < g
        const int32_t v = q < m + 2 ? S.aux[q] : 0;
        int32_t tot;
        const int32_t ex = blk_excl_sum(R, v, tot);
        if (q < m + 2) S.aux[q] = ex;
    }
    __syncthreads();
    int32_t s0 = 0, h = 0;
    if (mine) {  // 5. the new edges grouped by gap
        s0 = S.aux[gq];
        h = S.aux[gq + 1] - s0;
        S.bk2[s0 + arr] = q;
    }
    __syncthreads();
    // 6. final positions: gap + new edges of earlier gaps + those of its gap
    //    ordered before it (smaller key, or an equal key inserted earlier)
    //    (a per-thread loop: no barrier inside)
    int32_t r = 0;
    for (int32_t j = 0; j < h; ++j) {
        const int32_t u = S.bk2[s0 + j];
        if (u != q) {
            const LKey ku{S.nkx[u], S.nkg[u], S.nkl[u]};
            r += (key_gt(kc, ku) || (!key_gt(ku, kc) && u < q)) ? 1 : 0;
        }
    }
    // 7. entries move up by the new edges of gaps <= their position; 8. the new edges
    int32_t v = 0, to = 0;
    if (q < m) {
        to = q + S.aux[q + 1];
        v = S.idx[q];
    }
    __syncthreads();
    if (q < m) S.idx[to] = v;
    if (mine) S.idx[gq + s0 + r] = rs;
    __syncthreads();
    m += k;
}

// Read-ahead window of sorted edges as seven dwordx4 (ObjEdge's layout: X, G
// in q0.xy, YMin, YMax, Left in q4.xyz), named registers (an ObjEdge copy in
// a loop-carried variable went to scratch).
#define PRK_WIN(w) float4 w##0, w##1, w##2, w##3, w##4, w##5, w##6
#define PRK_WIN_LOAD(w, E, i, n)                                                      \
    do {                                                                              \
        const float4 *s_ = reinterpret_cast<const float4 *>((E) + min((i), (n) - 1)); \
        w##0 = s_[0]; w##1 = s_[1]; w##2 = s_[2]; w##3 = s_[3];                       \
        w##4 = s_[4]; w##5 = s_[5]; w##6 = s_[6];                                     \
        if ((i) >= (n)) (w##4).x = __int_as_float(INT32_MAX);  /* past the end */     \
    } while (0)
// The window's loads complete right where they are issued (s_waitcnt
// vmcnt(0), once per 64 edges), and the registers are redefined by an empty
// asm, so no later use waits on the load again: a window register still in
// flight across the row loop's back edge made the compiler wait for every
// outstanding access (the previous row's stores included) at the top of
// every row.
#define PRK_WIN_WAIT() __builtin_amdgcn_s_waitcnt(0x0F70)  // vmcnt(0) expcnt(7) lgkmcnt(15)
#define PRK_Q4(q) "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w)
#define PRK_WIN_LAUNDER(w)                                      \
    do {                                                        \
        asm volatile("" : PRK_Q4(w##0), PRK_Q4(w##1));          \
        asm volatile("" : PRK_Q4(w##2), PRK_Q4(w##3));          \
        asm volatile("" : PRK_Q4(w##4), PRK_Q4(w##5));          \
        asm volatile("" : PRK_Q4(w##6));                        \
    } while (0)
#define PRK_WIN_COPY(d, w) \
    do { d##0 = w##0; d##1 = w##1; d##2 = w##2; d##3 = w##3; d##4 = w##4; d##5 = w##5; d##6 = w##6; } while (0)
#define PRK_WIN_STORE(dst, w)                                                          \
    do {                                                                               \
        float4 *d_ = reinterpret_cast<float4 *>(dst);                                  \
        d_[0] = w##0; d_[1] = w##1; d_[2] = w##2; d_[3] = w##3;                        \
        d_[4] = w##4; d_[5] = w##5; d_[6] = w##6;                                      \
    } while (0)
}  // namespace prk
