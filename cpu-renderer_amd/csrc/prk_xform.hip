// prk_xform.hip — prk_geometry_transform's device pass: runs of triangles of a
// resident source geometry written through a 3x4 matrix each into a resident
// destination geometry (prk.h).  An extension with its own
// definition: the reference transforms on the host, in its absent game layer.
//
// Arithmetic (built with -ffp-contract=off like every kernel here; the pragma
// below says so again for this file): for a position, component i,
//     out[i] = ((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + M[i][3]
// every product and sum rounded to f32 on its own, in this order; a normal
// the same without the last sum; colours and uvs copied as words.
//
// Layout of the work: one flat grid over the call's output triangles, 64 to a
// workgroup of 192 threads.  The first 64 threads find their triangle's run
// by binary search over the exclusive scan of the runs' lengths (as
// k_obj_tables finds an object's run) and leave its source and destination
// triangle and its matrix index in LDS; then thread i of the workgroup takes
// VERTEX i of the 192, so consecutive lanes touch consecutive vertices of
// every array whatever the run lengths are: 12 bytes a lane for positions and
// normals, 16 for colours, 8 for uvs (where consecutive triangles of the grid
// are consecutive in memory, i.e. inside a run).  A lane holds its vertex's
// matrix in registers (three 16-byte loads, one address for the whole wave
// inside a run).  No loop is as long as a run, and there is one launch a call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prk_launch.h"
#include "prk_xform_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kTris = 64;             // output triangles a workgroup takes
constexpr uint32_t kThreads = 3 * kTris;   // one thread a vertex

// One run as the host uploads it (zero-length runs dropped): the source and
// destination triangle of its first triangle, its matrix, and the number of
// output triangles before it (the scan; also in its own array for the search).
struct Run {
    uint32_t src0, dst0, xform, start;
};

using prk::XformArrays;  // the arrays and the per-vertex arithmetic: prk_xform_dev.h

__global__ __launch_bounds__(kThreads) void k_xform(const uint32_t *__restrict__ scan, const Run *__restrict__ runs,
                                                    uint32_t nruns, uint32_t total,
                                                    const float4 *__restrict__ xforms, const XformArrays A) {
    __shared__ uint32_t s_src[kTris], s_dst[kTris], s_xf[kTris];
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * kTris;  // (total <= 2^31: no wrap)
    if (tid < kTris && t0 + tid < total) {
        const uint32_t t = t0 + tid;
        uint32_t lo = 0, hi = nruns;  // the last run with start <= t
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (scan[mid] <= t) lo = mid;
            else hi = mid;
        }
        const Run R = runs[lo];
        const uint32_t j = t - R.start;
        s_src[tid] = R.src0 + j;
        s_dst[tid] = R.dst0 + j;
        s_xf[tid] = R.xform;
    }
    __syncthreads();
    const uint32_t lt = tid / 3u, corner = tid - 3u * lt;
    if (t0 + lt >= total) return;
    const size_t sv = (size_t)s_src[lt] * 3u + corner;  // source and destination vertex
    const size_t dv = (size_t)s_dst[lt] * 3u + corner;
    prk::xform_vertex(A, sv, dv, xforms + (size_t)s_xf[lt] * 3u);
}

}  // namespace

// Host-side layout of the tables in one device buffer (prk_geometry_api.hip fills it):
// words [0, nruns]: the scan (nruns + 1 words, the last the total); runs at
// byte runs_off (16 bytes each); matrices at byte xf_off (48 bytes each);
// both offsets multiples of 16.
extern "C" hipError_t prk_xform_launch(const void *tables, size_t runs_off, size_t xf_off, uint32_t nruns,
                                       uint32_t total, const float *sV, const float *sC, const float *sN,
                                       const float *sUV, float *dV, float *dC, float *dN, float *dUV,
                                       hipStream_t s) {
    if (!total || !nruns) return hipSuccess;
    const uint8_t *b = static_cast<const uint8_t *>(tables);
    const XformArrays A{sV, sC, sN, sUV, dV, dC, dN, dUV};
    const uint32_t blocks = (total + kTris - 1) / kTris;
    hipLaunchKernelGGL(k_xform, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const uint32_t *>(b),
                       reinterpret_cast<const Run *>(b + runs_off), nruns, total,
                       reinterpret_cast<const float4 *>(b + xf_off), A);
    return hipGetLastError();
}
