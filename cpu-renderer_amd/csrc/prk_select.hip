// prk_select.hip — prk_geometry_select's device stages (prk.h):
// for every item of a caller's table, whether it is drawn and from which of
// its meshes, decided from per-id pixel counts that are already on the device
// (prk_visibility_*'s pix_prefix) or from the caller's own counts; then the
// chosen triangles, packed in item order and transformed, written into a
// resident destination geometry.  No table goes back to the host in between.
//
//   k_sel_choose   one thread an item: pixels(i) = item_pixels[i], or the
//                  difference of two pix_prefix words, or (with bound_pixels,
//                  prk_geometry_select_bounds) bound_pixels[i] for an item
//                  without ids; the first of the item's
//                  levels with pixels(i) >= min_pixels wins (no order of the
//                  thresholds is assumed); chosen[i], n[i] and the item's run
//                  (first source triangle, matrix) are written.  Thread
//                  `nitems` writes n[nitems] = 0, so the scan's last word is
//                  the total.
//   prk_scan_u32   start = the exclusive scan of n (nitems + 1 words).
//   k_sel_emit     one flat grid over the output triangles, k_xform's layout
//                  (prk_xform.hip): 64 triangles to a workgroup of 192
//                  threads; the first 64 threads find their triangle's item by
//                  binary search over `start` and leave its source triangle
//                  and matrix in LDS; then thread i takes VERTEX i of the 192,
//                  so consecutive lanes touch consecutive vertices of every
//                  array whatever the item sizes are.  The arithmetic is
//                  prk_xform_dev.h's xform_vertex, the one k_xform runs.
// `start` holds runs of equal words where items were dropped.  The search
// keeps the invariant start[lo] <= t < start[hi] (start[nitems] = total > t)
// and ends at hi = lo + 1: the LAST item with start <= t, whose own count
// start[lo + 1] - start[lo] is then at least 1 -- never a dropped one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/prk.h"
#include "prk_launch.h"
#include "prk_xform_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kTris = 64;            // output triangles a workgroup takes
constexpr uint32_t kThreads = 3 * kTris;  // one thread a vertex
constexpr uint32_t kChooseThreads = 256;

using prk::SelRun;
using prk::XformArrays;

__global__ __launch_bounds__(kChooseThreads) void k_sel_choose(const prk_select_item *__restrict__ items,
                                                               uint32_t nitems,
                                                               const prk_select_level *__restrict__ levels,
                                                               const uint32_t *__restrict__ pix_prefix,
                                                               const uint32_t *__restrict__ item_pixels,
                                                               const uint32_t *__restrict__ bound_pixels,
                                                               int32_t *__restrict__ chosen, uint32_t *__restrict__ n,
                                                               SelRun *__restrict__ runs) {
    const uint64_t i = (uint64_t)blockIdx.x * kChooseThreads + threadIdx.x;
    if (i > nitems) return;
    if (i == nitems) {  // the scan's last input: its last output is the total
        n[i] = 0u;
        return;
    }
    const prk_select_item it = items[i];
    // (the host has checked first_id + id_count against the frame's ids: no wrap, both words inside)
    // (with bound_pixels an item without ids reads no pix_prefix word: there may be no frame)
    const uint32_t pixels = item_pixels                           ? item_pixels[i]
                            : (bound_pixels && it.id_count == 0u) ? bound_pixels[i]
                                                                  : pix_prefix[it.first_id + it.id_count] - pix_prefix[it.first_id];
    int32_t pick = -1;
    uint32_t cnt = 0, src0 = 0;
    for (uint32_t l = 0; l < it.level_count; ++l) {
        const prk_select_level lv = levels[it.first_level + l];
        if (pixels >= lv.min_pixels) {  // the first level that passes
            pick = (int32_t)l;
            cnt = lv.tri_count;
            src0 = lv.src_first_tri;
            break;
        }
    }
    chosen[i] = pick;
    n[i] = cnt;
    runs[i] = SelRun{src0, pick >= 0 ? it.xform : 0u};
}

__global__ __launch_bounds__(kThreads) void k_sel_emit(const uint32_t *__restrict__ start,
                                                       const SelRun *__restrict__ runs, uint32_t nitems,
                                                       uint32_t total, uint32_t dst0,
                                                       const float4 *__restrict__ xforms, const XformArrays A) {
    __shared__ uint32_t s_src[kTris], s_xf[kTris];
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * kTris;  // (total <= 2^31: no wrap)
    if (tid < kTris && t0 + tid < total) {
        const uint32_t t = t0 + tid;
        uint32_t lo = 0, hi = nitems;  // start[lo] <= t < start[hi]: the last item with start <= t
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (start[mid] <= t) lo = mid;
            else hi = mid;
        }
        const SelRun R = runs[lo];
        s_src[tid] = R.src0 + (t - start[lo]);
        s_xf[tid] = R.xform;
    }
    __syncthreads();
    const uint32_t lt = tid / 3u, corner = tid - 3u * lt;
    if (t0 + lt >= total) return;
    const size_t sv = (size_t)s_src[lt] * 3u + corner;        // source and destination vertex
    const size_t dv = ((size_t)dst0 + t0 + lt) * 3u + corner;  // (packed: the grid's order is the destination's)
    prk::xform_vertex(A, sv, dv, xforms + (size_t)s_xf[lt] * 3u);
}

}  // namespace

extern "C" {

hipError_t prk_sel_choose(const prk_select_item *items, uint32_t nitems, const prk_select_level *levels,
                          const uint32_t *pix_prefix, const uint32_t *item_pixels, const uint32_t *bound_pixels,
                          int32_t *chosen, uint32_t *n, prk::SelRun *runs, hipStream_t s) {
    if (nitems == UINT32_MAX) return hipErrorInvalidValue;  // (nitems + 1 words)
    const uint32_t blocks = (uint32_t)(((uint64_t)nitems + 1 + kChooseThreads - 1) / kChooseThreads);
    hipLaunchKernelGGL(k_sel_choose, dim3(blocks), dim3(kChooseThreads), 0, s, items, nitems, levels, pix_prefix,
                       item_pixels, bound_pixels, chosen, n, runs);
    return hipGetLastError();
}

hipError_t prk_sel_emit(const uint32_t *start, const prk::SelRun *runs, uint32_t nitems, uint32_t total,
                        uint32_t dst_first_tri, const prk_xform *xforms, const float *sV, const float *sC,
                        const float *sN, const float *sUV, float *dV, float *dC, float *dN, float *dUV,
                        hipStream_t s) {
    if (!total || !nitems) return hipSuccess;
    if (total > (1u << 31)) return hipErrorInvalidValue;
    const XformArrays A{sV, sC, sN, sUV, dV, dC, dN, dUV};
    const uint32_t blocks = (total + kTris - 1) / kTris;
    hipLaunchKernelGGL(k_sel_emit, dim3(blocks), dim3(kThreads), 0, s, start, runs, nitems, total, dst_first_tri,
                       reinterpret_cast<const float4 *>(xforms), A);
    return hipGetLastError();
}

}  // extern "C"
