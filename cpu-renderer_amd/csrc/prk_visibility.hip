// prk_visibility.hip — visibility feedback (prk_visibility_*):
// the winner map a debug-mode flush leaves (n int32 words: -1 or an id of the
// frame's numbering) reduced on the device to per-id pixel counts, their
// prefix sums, and the ascending list of the ids that won a pixel.
//
//   k_vis_hist     counts[id] += the words equal to id.  Winner maps are
//                  coherent along a row (a triangle's span is a run of equal
//                  words), so a wave adds RUNS, not pixels: it walks a chunk
//                  of kVisChunk consecutive words in segments of 256 (a 16-byte
//                  load a lane), finds the run heads of a segment against the
//                  previous word (the previous lane's last word by a lane
//                  move, the previous segment's last run carried in scalars),
//                  turns them into ballot masks, and every head adds its run
//                  with one return-less atomic.  A run that spans segments is
//                  carried and added once, when it ends or the chunk does.
//   k_vis_flags    flag[i] = counts[i] != 0 (and 0 at i == id_count);
//   prk_scan_u32   twice: pix_prefix and vis_prefix, id_count + 1 words each;
//   k_vis_compact  ids[vis_prefix[i]] = i where flag[i];
//   k_vis_groups   prefix differences over caller ranges of ids.
// Counters are plain u32 in device memory: with 2^20 and more ids there is
// nothing to privatise in LDS.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prk_launch.h"

namespace prk {
namespace {

constexpr int kVisThreads = 256;
constexpr uint32_t kVisSegWords = 256;   // a wave's vector segment: 64 lanes x 4 words
constexpr uint32_t kVisChunk = 4096;     // words a wave walks (a multiple of kVisSegWords)

// A run of `len` words equal to `id`: counted if id is one of the frame's.
// (An id < 0 is >= 2^31 as unsigned, and id_count < 2^32 - 16: never indexed.)
template <bool COUNT>
__device__ __forceinline__ void vis_add(uint32_t *__restrict__ counts, uint32_t id_count, int32_t id, uint32_t len,
                                        uint32_t *__restrict__ natomics) {
    if ((uint32_t)id >= id_count) return;
    (void)__hip_atomic_fetch_add(counts + (uint32_t)id, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (COUNT) (void)__hip_atomic_fetch_add(natomics, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The first / last k with bit `lane` of H[k] set (one is).
template <int K>
__device__ __forceinline__ int first_k(const uint64_t (&H)[K], int lane) {
    int r = K - 1;
#pragma unroll
    for (int k = K - 2; k >= 0; --k)
        if ((H[k] >> lane) & 1ull) r = k;
    return r;
}
template <int K>
__device__ __forceinline__ int last_k(const uint64_t (&H)[K], int lane) {
    int r = 0;
#pragma unroll
    for (int k = 1; k < K; ++k)
        if ((H[k] >> lane) & 1ull) r = k;
    return r;
}

// One segment of 64 * K words in lane order (lane l holds words l * K + k).
// (cid, clen): the run that ends at the segment's start, not yet added
// (clen == 0: none -- the wave's first word always starts a run); on return
// the run that ends at the segment's end.  Both are wave-uniform.
template <int K, bool COUNT>
__device__ __forceinline__ void vis_segment(const int32_t (&v)[K], int32_t &cid, uint32_t &clen,
                                            uint32_t *__restrict__ counts, uint32_t id_count,
                                            uint32_t *__restrict__ natomics) {
    const int lane = threadIdx.x & 63;
    int32_t prev = __shfl_up(v[K - 1], 1, 64);  // the previous lane's last word
    if (lane == 0) prev = cid;
    bool head[K];
    head[0] = v[0] != prev || (lane == 0 && clen == 0);
#pragma unroll
    for (int k = 1; k < K; ++k) head[k] = v[k] != v[k - 1];
    uint64_t H[K], A = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        H[k] = __ballot(head[k]);
        A |= H[k];
    }
    if (A == 0) {  // every word continues the carried run
        clen += 64u * K;
        return;
    }
    // the words before the first head end the carried run
    const int lf = (int)__builtin_ctzll(A);
    clen += (uint32_t)(lf * K + first_k<K>(H, lf));
    if (lane == 0 && clen) vis_add<COUNT>(counts, id_count, cid, clen, natomics);
    // every head but the last adds its run: up to the next head
    const int ll = 63 - (int)__builtin_clzll(A);
    const int kl = last_k<K>(H, ll);
    const uint64_t later = A & ~((2ull << lane) - 1ull);  // heads in the lanes after this one
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!head[k] || (lane == ll && k == kl)) continue;
        int nk = -1;
#pragma unroll
        for (int j = K - 1; j > k; --j)
            if (head[j]) nk = j;
        uint32_t len;
        if (nk >= 0) {
            len = (uint32_t)(nk - k);
        } else {  // (not the last head, none later in this lane: a later lane has one)
            const int l2 = (int)__builtin_ctzll(later);
            len = (uint32_t)((l2 - lane) * K + first_k<K>(H, l2) - k);
        }
        vis_add<COUNT>(counts, id_count, v[k], len, natomics);
    }
    // the last head's run is carried on
    int32_t vl = v[0];
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (kl == k) vl = v[k];
    cid = __builtin_amdgcn_readlane(vl, ll);
    clen = (uint32_t)((64 - ll) * K - kl);
}

// vec: w is 16-byte aligned (whole segments are read as one int4 a lane; the
// rest of a chunk, and an unaligned map, one dword a lane, -1 past the end).
template <bool COUNT>
__global__ void __launch_bounds__(kVisThreads) k_vis_hist(const int32_t *__restrict__ w, uint32_t n, uint32_t id_count,
                                                          uint32_t *__restrict__ counts, int vec,
                                                          uint32_t *__restrict__ natomics) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (kVisThreads / 64) + (threadIdx.x >> 6);
    uint64_t pos = wave * kVisChunk;
    if (pos >= n) return;  // (wave-uniform)
    const uint64_t end = pos + kVisChunk < n ? pos + kVisChunk : n;
    int32_t cid = -1;
    uint32_t clen = 0;
    if (vec) {
        for (; pos + kVisSegWords <= end; pos += kVisSegWords) {
            const int4 q = *reinterpret_cast<const int4 *>(w + pos + (uint32_t)lane * 4u);
            const int32_t v[4] = {q.x, q.y, q.z, q.w};
            vis_segment<4, COUNT>(v, cid, clen, counts, id_count, natomics);
        }
    }
    for (; pos < end; pos += 64) {
        const uint64_t i = pos + (uint32_t)lane;
        const int32_t v[1] = {i < end ? w[i] : -1};
        vis_segment<1, COUNT>(v, cid, clen, counts, id_count, natomics);
    }
    if (lane == 0 && clen) vis_add<COUNT>(counts, id_count, cid, clen, natomics);
}

// flag[0 .. id_count]: the scans' input (the last word 0, so their last word is the total).
__global__ void k_vis_flags(const uint32_t *__restrict__ counts, uint32_t id_count, uint32_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > id_count) return;
    flag[i] = i < id_count && counts[i] != 0u ? 1u : 0u;
}

__global__ void k_vis_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ vis_prefix,
                              uint32_t id_count, uint32_t *__restrict__ ids) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= id_count) return;
    if (flag[i]) ids[vis_prefix[i]] = (uint32_t)i;
}

__global__ void k_vis_groups(const uint32_t *__restrict__ starts, uint32_t ngroup,
                             const uint32_t *__restrict__ pix_prefix, const uint32_t *__restrict__ vis_prefix,
                             uint32_t *__restrict__ pixels, uint32_t *__restrict__ visible) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroup) return;
    const uint32_t b = starts[g], e = starts[g + 1];
    if (pixels) pixels[g] = pix_prefix[e] - pix_prefix[b];
    if (visible) visible[g] = vis_prefix[e] - vis_prefix[b];
}

inline unsigned blocks_of(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace prk

extern "C" {

// The whole reduction of n winner words over id_count ids, queued on s (temp
// == nullptr: the scans' scratch size only).  counts, flags, pix_prefix and
// vis_prefix hold id_count + 1 words each, ids id_count; ids is written up to
// the visible count, everything else in full.  natomics: nullptr (the product
// instantiation, no counter), or a zeroed word that counts the histogram's
// atomic adds (prk_selftest_visibility).
hipError_t prk_vis_reduce(const int32_t *winners, uint32_t n, uint32_t id_count, uint32_t *counts, uint32_t *flags,
                          uint32_t *pix_prefix, uint32_t *vis_prefix, uint32_t *ids, void *temp, size_t *temp_bytes,
                          uint32_t *natomics, hipStream_t s) {
    using namespace prk;
    if (id_count == UINT32_MAX) return hipErrorInvalidValue;  // (id_count + 1 words)
    const uint32_t m = id_count + 1;
    if (!temp) return prk_scan_u32(nullptr, nullptr, m, nullptr, temp_bytes, s);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)m * 4, s);
    if (e != hipSuccess) return e;
    if (n && id_count) {
        const unsigned nb = blocks_of(blocks_of(n, kVisChunk), kVisThreads / 64);
        const int vec = (reinterpret_cast<uintptr_t>(winners) & 15u) == 0 ? 1 : 0;
        if (natomics)
            hipLaunchKernelGGL(k_vis_hist<true>, dim3(nb), dim3(kVisThreads), 0, s, winners, n, id_count, counts, vec,
                               natomics);
        else
            hipLaunchKernelGGL(k_vis_hist<false>, dim3(nb), dim3(kVisThreads), 0, s, winners, n, id_count, counts, vec,
                               (uint32_t *)nullptr);
    }
    hipLaunchKernelGGL(k_vis_flags, dim3(blocks_of(m, 256)), dim3(256), 0, s, (const uint32_t *)counts, id_count, flags);
    e = hipGetLastError();
    if (e == hipSuccess) e = prk_scan_u32(counts, pix_prefix, m, temp, temp_bytes, s);
    if (e == hipSuccess) e = prk_scan_u32(flags, vis_prefix, m, temp, temp_bytes, s);
    if (e != hipSuccess) return e;
    if (id_count)
        hipLaunchKernelGGL(k_vis_compact, dim3(blocks_of(id_count, 256)), dim3(256), 0, s, (const uint32_t *)flags,
                           (const uint32_t *)vis_prefix, id_count, ids);
    return hipGetLastError();
}

// pixels[g] / visible[g] (either may be null) of the ngroup id ranges [starts[g], starts[g + 1]).
hipError_t prk_vis_groups(const uint32_t *starts, uint32_t ngroup, const uint32_t *pix_prefix,
                          const uint32_t *vis_prefix, uint32_t *pixels, uint32_t *visible, hipStream_t s) {
    using namespace prk;
    if (ngroup == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vis_groups, dim3(blocks_of(ngroup, 256)), dim3(256), 0, s, starts, ngroup, pix_prefix,
                       vis_prefix, pixels, visible);
    return hipGetLastError();
}

}  // extern "C"
