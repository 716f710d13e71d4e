// prk_bounds.hip — prk_visibility_bounds' device stages (prk.h):
// a min-z map of the target in tiles of 8 x 8 pixels, and every item's bounding
// box tested against it.  Neither kernel is part of a flush.
//
//   k_ztile_min    zmin[ty][tx] = the smallest non-NaN z word of tile (tx, ty)'s
//                  pixels inside the band, +inf if there is none.  A lane takes
//                  PX pixels of a tile row, 8 / PX lanes a tile, and a wave
//                  8 * PX tiles side by side.  The 8 rows of the tile are all
//                  loaded before the first is used (a row outside the band
//                  reads the nearest row inside it and its value is dropped:
//                  no load behind a branch), folded in registers
//                  with fminf (v_min_f32 returns the operand that is no NaN),
//                  the lanes of a tile folded by DPP exchanges, one store a
//                  tile.  PX = 4: 16-byte loads, for a z base on a 16-byte
//                  boundary and W a multiple of 4 (a lane's four pixels are
//                  then all inside W or all outside).  PX = 1: a dword a lane,
//                  for every other target (W no multiple of 4: scalar targets;
//                  a caller-bound z pointer).  The band's first and last tile
//                  rows, where rows of the tile are outside the band, go the
//                  same way in both: the row test is the same for the wave.
//   k_bounds_test  a wave an item.  Lane l takes corner l & 7 (so the 8 groups
//                  of a wave compute the same 8 corners and no value has to be
//                  broadcast): prk_geometry_transform's position arithmetic
//                  (prk_xform_dev.h), + P, ProjectVertex; min and max of px, py
//                  and max of z over the 8 by DPP exchanges; the rectangle,
//                  clamped in float and only then converted; then the 64 lanes
//                  stride over the rectangle's tiles in row-major order, each
//                  adding area(rect ^ tile) where !(znear < zmin[tile]); one
//                  wave sum, one store.
// Both kernels index zmin through the band's tile counts only, and the test
// kernel's rectangle is clamped again as integers, so no index leaves the map
// whatever the floats were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/prk.h"
#include "prk_launch.h"
#include "prk_wave.h"
#include "prk_xform_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kThreads = 256;  // 4 waves: 4 wave-wide strips of tiles, or 4 items

using prk::BoundsFrame;

template <int PX>
struct ZLoad;
template <>
struct ZLoad<4> {
    using T = float4;
    static __device__ __forceinline__ float fold(float m, const float4 v) {
        return fminf(fminf(m, fminf(v.x, v.y)), fminf(v.z, v.w));
    }
};
template <>
struct ZLoad<1> {
    using T = float;
    static __device__ __forceinline__ float fold(float m, const float v) { return fminf(m, v); }
};

template <int PX>
__global__ __launch_bounds__(kThreads) void k_ztile_min(const float *__restrict__ z, const BoundsFrame B,
                                                        uint32_t strips_x, float *__restrict__ zmin) {
    using L = ZLoad<PX>;
    constexpr int kTilesWave = 8 * PX;  // tiles a wave takes, side by side
    const uint32_t wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t trow = wave / strips_x;  // tile row of the band (uniform in the wave)
    if (trow >= (uint32_t)B.tiles_y) return;
    const uint32_t strip = wave - trow * strips_x;
    const int32_t x = (int32_t)(strip * 64u * PX + lane * PX);  // (< W + 64 * PX: no wrap)
    const int32_t y0 = (B.first_tile_row + (int32_t)trow) * 8;
    const bool in_x = x < B.W;  // (PX = 4: W is a multiple of 4, so all four pixels or none)
    // Every load is issued before the first fold, and none sits behind a branch (a load under a condition is
    // waited for on its own): a row or a lane outside the band reads a pixel inside it and drops the value.
    const size_t xs = in_x ? (size_t)x : 0;
    typename L::T v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int32_t yc = min(max(y0 + r, B.row0), B.row1 - 1);
        v[r] = *reinterpret_cast<const typename L::T *>(z + (size_t)(yc - B.row0) * (size_t)B.W + xs);
    }
    float m = INFINITY;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int32_t y = y0 + r;
        const float f = L::fold(INFINITY, v[r]);
        m = fminf(m, (in_x && y >= B.row0 && y < B.row1) ? f : INFINITY);
    }
    m = fminf(m, prk::dpp_f<prk::kDppSwap1>(m, m));
    if (PX == 1) {
        m = fminf(m, prk::dpp_f<prk::kDppSwap2>(m, m));
        m = fminf(m, prk::dpp_f<prk::kDppHalfMirror>(m, m));
    }
    const uint32_t tx = strip * kTilesWave + lane / (8 / PX);
    if (lane % (8 / PX) == 0 && tx < (uint32_t)B.tiles_x) zmin[(size_t)trow * (size_t)B.tiles_x + tx] = m;
}

// min / max over the 8 lanes of a group, in every lane of it.
__device__ __forceinline__ float group8_min(float v) {
    v = fminf(v, prk::dpp_f<prk::kDppSwap1>(v, v));
    v = fminf(v, prk::dpp_f<prk::kDppSwap2>(v, v));
    return fminf(v, prk::dpp_f<prk::kDppHalfMirror>(v, v));
}
__device__ __forceinline__ float group8_max(float v) {
    v = fmaxf(v, prk::dpp_f<prk::kDppSwap1>(v, v));
    v = fmaxf(v, prk::dpp_f<prk::kDppSwap2>(v, v));
    return fmaxf(v, prk::dpp_f<prk::kDppHalfMirror>(v, v));
}

// [lo - 1, hi + 2) of the floors, clamped to [c0, c1] in float, then as integers
// (clamped once more: a no-op while c1 is exact in f32, the bounds' safety beyond).
__device__ __forceinline__ void rect_axis(float lo, float hi, int32_t c0, int32_t c1, int32_t &a, int32_t &b) {
    const float f0 = (float)c0, f1 = (float)c1;
    const float fa = fminf(fmaxf(floorf(lo) - 1.0f, f0), f1);
    const float fb = fminf(fmaxf(floorf(hi) + 2.0f, f0), f1);
    a = min(max((int32_t)fa, c0), c1);
    b = min(max((int32_t)fb, c0), c1);
}

__global__ __launch_bounds__(kThreads) void k_bounds_test(const prk_bound *__restrict__ bounds, uint32_t count,
                                                          const float4 *__restrict__ xforms, const BoundsFrame B,
                                                          const float *__restrict__ zmin,
                                                          uint32_t *__restrict__ pixels) {
    const uint32_t item = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);  // (uniform in the wave)
    if (item >= count) return;
    const uint32_t lane = threadIdx.x & 63;
    const prk_bound b = bounds[item];
    const float4 *M = xforms + (size_t)b.xform * 3u;
    const float4 m0 = M[0], m1 = M[1], m2 = M[2];
    const float x = (lane & 1) ? b.hi[0] : b.lo[0];
    const float y = (lane & 2) ? b.hi[1] : b.lo[1];
    const float zc = (lane & 4) ? b.hi[2] : b.lo[2];
    // prk_geometry_transform's position, then the draw's + P
    const float cx = (prk::xf_row3(m0, x, y, zc) + m0.w) + B.P[0];
    const float cy = (prk::xf_row3(m1, x, y, zc) + m1.w) + B.P[1];
    const float cz = (prk::xf_row3(m2, x, y, zc) + m2.w) + B.P[2];
    // ProjectVertex (prk_device.h project_vertex)
    const float d = B.D - cz;
    const bool front = d > 0.2f;
    const float k = (1.0f / d) * B.F;
    const float px = B.Cx + B.M2P * (k * cx), py = B.Cy + B.M2P * (k * cy);
    const bool whole = __ballot(!front || px != px || py != py) != 0ull;
    float znear = group8_max(cz);
    if (__ballot(cz != cz) != 0ull) znear = NAN;  // (fmaxf drops a NaN: a NaN corner z is a NaN znear)
    int32_t x0 = 0, x1 = B.W, y0 = B.row0, y1 = B.row1;
    if (!whole) {
        rect_axis(group8_min(px), group8_max(px), 0, B.W, x0, x1);
        rect_axis(group8_min(py), group8_max(py), B.row0, B.row1, y0, y1);
    }
    uint32_t sum = 0;
    if (x0 < x1 && y0 < y1) {
        const uint32_t tx0 = (uint32_t)x0 >> 3, ntx = (((uint32_t)x1 + 7u) >> 3) - tx0;
        const uint32_t ty0 = (uint32_t)y0 >> 3, nty = (((uint32_t)y1 + 7u) >> 3) - ty0;
        const uint32_t total = ntx * nty;  // (at most the band's tiles)
        const uint32_t dq = 64u / ntx, dr = 64u - dq * ntx;  // a trip of 64 tiles: dq rows and dr columns on
        uint32_t r = lane / ntx, c = lane - r * ntx;
#pragma unroll 4
        for (uint32_t t = lane; t < total; t += 64u) {
            const int32_t tx = (int32_t)(tx0 + c), ty = (int32_t)(ty0 + r);
            const float zm = zmin[(size_t)(ty - B.first_tile_row) * (size_t)B.tiles_x + (size_t)tx];
            const int32_t w = min(x1, 8 * tx + 8) - max(x0, 8 * tx);
            const int32_t h = min(y1, 8 * ty + 8) - max(y0, 8 * ty);
            if (!(znear < zm)) sum += (uint32_t)w * (uint32_t)h;
            r += dq;
            c += dr;
            if (c >= ntx) {
                c -= ntx;
                ++r;
            }
        }
    }
    sum = (uint32_t)prk::readlane_i(prk::wave_incl_sum_i32((int32_t)sum), 63);
    if (lane == 0) pixels[item] = sum;
}

}  // namespace

extern "C" {

hipError_t prk_ztile_min(const float *z, const prk::BoundsFrame *B, float *zmin, hipStream_t s) {
    if (B->W <= 0 || B->row0 < 0 || B->row1 <= B->row0 || B->tiles_x != (B->W + 7) / 8 ||
        B->first_tile_row != B->row0 / 8 || B->tiles_y != (B->row1 + 7) / 8 - B->first_tile_row)
        return hipErrorInvalidValue;
    const bool vec = (reinterpret_cast<uintptr_t>(z) & 15u) == 0 && (B->W & 3) == 0;
    const uint32_t per_wave = vec ? 32u : 8u;  // tiles a wave takes
    const uint32_t strips_x = ((uint32_t)B->tiles_x + per_wave - 1) / per_wave;
    const uint64_t waves = (uint64_t)strips_x * (uint64_t)B->tiles_y;
    const uint64_t blocks = (waves + kThreads / 64 - 1) / (kThreads / 64);
    if (blocks > 0x3FFFFFFFull) return hipErrorInvalidValue;  // (the wave index stays in 32 bits)
    if (vec)
        hipLaunchKernelGGL(k_ztile_min<4>, dim3((uint32_t)blocks), dim3(kThreads), 0, s, z, *B, strips_x, zmin);
    else
        hipLaunchKernelGGL(k_ztile_min<1>, dim3((uint32_t)blocks), dim3(kThreads), 0, s, z, *B, strips_x, zmin);
    return hipGetLastError();
}

hipError_t prk_bounds_test(const prk_bound *bounds, uint32_t count, const prk_xform *xforms,
                           const prk::BoundsFrame *B, const float *zmin, uint32_t *pixels, hipStream_t s) {
    if (!count) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)count + kThreads / 64 - 1) / (kThreads / 64));
    hipLaunchKernelGGL(k_bounds_test, dim3(blocks), dim3(kThreads), 0, s, bounds, count,
                       reinterpret_cast<const float4 *>(xforms), *B, zmin, pixels);
    return hipGetLastError();
}

}  // extern "C"
