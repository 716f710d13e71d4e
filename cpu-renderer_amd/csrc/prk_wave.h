// prk_wave.h — wave and workgroup primitives: DPP lane moves and the wave64
// scans on them, the insertion order as a key (LKey), BlockRed and blk_*.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prk {
// Lane moves without the LDS (DPP, GFX9): row_shr:n inside each 16-lane row,
// row_bcast:15 / row_bcast:31 across rows; a lane without a source keeps
// `old`.  (__shfl* go through
// ds_bpermute: an LDS round trip each, the one-wave walks' critical path.)
template <int CTRL, int ROW = 0xf>
__device__ __forceinline__ int32_t dpp_i(int32_t old, int32_t v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW, 0xf, false);
}
template <int CTRL, int ROW = 0xf>
__device__ __forceinline__ float dpp_f(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW, 0xf, false));
}
constexpr int kDppShr1 = 0x111, kDppShr2 = 0x112, kDppShr4 = 0x114, kDppShr8 = 0x118;
constexpr int kDppBcast15 = 0x142, kDppBcast31 = 0x143;
// Exchanges inside groups of 8 lanes (every lane has a source): quad_perm
// [1,0,3,2] and [2,3,0,1] swap neighbours and pairs, row_half_mirror reverses
// the 8 -- after the three, a commutative fold has reached all 8 lanes.
constexpr int kDppSwap1 = 0xB1, kDppSwap2 = 0x4E, kDppHalfMirror = 0x141;
__device__ __forceinline__ int32_t wave_incl_sum_i32(int32_t v) {
    v += dpp_i<kDppShr1>(0, v);
    v += dpp_i<kDppShr2>(0, v);
    v += dpp_i<kDppShr4>(0, v);
    v += dpp_i<kDppShr8>(0, v);
    v += dpp_i<kDppBcast15, 0xa>(0, v);
    v += dpp_i<kDppBcast31, 0xc>(0, v);
    return v;
}
__device__ __forceinline__ int32_t wave_incl_max_i32(int32_t v) {
    v = max(v, dpp_i<kDppShr1>(INT32_MIN, v));
    v = max(v, dpp_i<kDppShr2>(INT32_MIN, v));
    v = max(v, dpp_i<kDppShr4>(INT32_MIN, v));
    v = max(v, dpp_i<kDppShr8>(INT32_MIN, v));
    v = max(v, dpp_i<kDppBcast15, 0xa>(INT32_MIN, v));
    v = max(v, dpp_i<kDppBcast31, 0xc>(INT32_MIN, v));
    return v;
}
__device__ __forceinline__ int32_t readlane_i(int32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int wave_max_i32(int v) { return readlane_i(wave_incl_max_i32(v), 63); }
__device__ __forceinline__ int32_t lane_rank(unsigned long long bal) {
    return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// The insertion order as a key.  "Cur sorts before E" (3663-3667) is
// key(E) > key(Cur) for keys compared (X, Gradient, Left) lexicographically
// with float compares, once NaNs are mapped out: an entry with a NaN X never
// compares greater than a new edge (lowest key), one with a NaN Gradient only
// by X (lowest Gradient and Left).  (New edges with a NaN in their key take
// the one-at-a-time insertion.)  +0 and -0 compare equal, as in the reference.
struct LKey {
    float x, g;
    int32_t l;
};
__device__ __forceinline__ LKey entry_key(float x, float g, int32_t l) {
    if (x != x) return LKey{-INFINITY, -INFINITY, INT32_MIN};
    if (g != g) return LKey{x, -INFINITY, INT32_MIN};
    return LKey{x, g, l};
}
__device__ __forceinline__ bool key_gt(const LKey &a, const LKey &b) {
    return a.x > b.x || (a.x == b.x && (a.g > b.g || (a.g == b.g && a.l > b.l)));
}
// Inclusive prefix maximum of the lanes' keys (lane order), with the lane
// position of a maximum as payload.
template <int CTRL, int ROW = 0xf>
__device__ __forceinline__ void key_max_step(LKey &k, int32_t &p) {
    const LKey o{dpp_f<CTRL, ROW>(-INFINITY, k.x), dpp_f<CTRL, ROW>(-INFINITY, k.g), dpp_i<CTRL, ROW>(INT32_MIN, k.l)};
    const int32_t op = dpp_i<CTRL, ROW>(-1, p);
    if (key_gt(o, k)) { k = o; p = op; }
}
__device__ __forceinline__ void wave_key_prefix_max(LKey &k, int32_t &p) {
    key_max_step<kDppShr1>(k, p);
    key_max_step<kDppShr2>(k, p);
    key_max_step<kDppShr4>(k, p);
    key_max_step<kDppShr8>(k, p);
    key_max_step<kDppBcast15, 0xa>(k, p);
    key_max_step<kDppBcast31, 0xc>(k, p);
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// Workgroup reductions and scans over thread order (R: the waves' partials;
// every caller reaches them with the whole workgroup).
struct BlockRed {
    int32_t a[16], b[16], c[16];
    float x[16], g[16];
};
// A workgroup barrier; LO: ordering LDS only (no wait for the workgroup's
// outstanding device-memory accesses -- for walks whose threads share only
// LDS, with device-memory stores that nobody in the workgroup reads back).
template <bool LO = false>
__device__ __forceinline__ void blk_sync() {
    if (LO) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    } else {
        __syncthreads();
    }
}
template <bool LO = false>
__device__ __forceinline__ int32_t blk_excl_sum(BlockRed &R, int32_t v, int32_t &tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int32_t inc = wave_incl_sum_i32(v);
    if (lane == 63) R.a[w] = inc;
    blk_sync<LO>();
    int32_t before = 0, t = 0;
    for (int i = 0; i < nw; ++i) {
        const int32_t x = R.a[i];
        before += i < w ? x : 0;
        t += x;
    }
    blk_sync<LO>();
    tot = t;
    return before + inc - v;
}
// Two exclusive scans at once (one barrier pair).
template <bool LO = false>
__device__ __forceinline__ void blk_excl_sum2(BlockRed &R, int32_t v1, int32_t v2, int32_t &e1, int32_t &e2,
                                              int32_t &t1, int32_t &t2) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int32_t i1 = wave_incl_sum_i32(v1), i2 = wave_incl_sum_i32(v2);
    if (lane == 63) { R.a[w] = i1; R.b[w] = i2; }
    blk_sync<LO>();
    int32_t b1 = 0, b2 = 0, s1 = 0, s2 = 0;
    for (int i = 0; i < nw; ++i) {
        const int32_t x = R.a[i], y = R.b[i];
        b1 += i < w ? x : 0;
        b2 += i < w ? y : 0;
        s1 += x;
        s2 += y;
    }
    blk_sync<LO>();
    e1 = b1 + i1 - v1;
    e2 = b2 + i2 - v2;
    t1 = s1;
    t2 = s2;
}
// Three sums.
template <bool LO = false>
__device__ __forceinline__ void blk_sum3(BlockRed &R, int32_t v1, int32_t v2, int32_t v3, int32_t &t1, int32_t &t2,
                                         int32_t &t3) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int32_t s1 = readlane_i(wave_incl_sum_i32(v1), 63), s2 = readlane_i(wave_incl_sum_i32(v2), 63),
                  s3 = readlane_i(wave_incl_sum_i32(v3), 63);
    if ((threadIdx.x & 63) == 0) { R.a[w] = s1; R.b[w] = s2; R.c[w] = s3; }
    blk_sync<LO>();
    t1 = t2 = t3 = 0;
    for (int i = 0; i < nw; ++i) { t1 += R.a[i]; t2 += R.b[i]; t3 += R.c[i]; }
    blk_sync<LO>();
}
template <bool LO = false>
__device__ __forceinline__ int32_t blk_max(BlockRed &R, int32_t v) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int32_t m = wave_max_i32(v);
    if ((threadIdx.x & 63) == 0) R.a[w] = m;
    blk_sync<LO>();
    int32_t r = INT32_MIN;
    for (int i = 0; i < nw; ++i) r = max(r, R.a[i]);
    blk_sync<LO>();
    return r;
}
// The first thread with b (INT32_MAX: none).
__device__ __forceinline__ int32_t blk_first(BlockRed &R, bool b) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long bal = __ballot(b);
    if ((threadIdx.x & 63) == 0) R.a[w] = bal ? w * 64 + (int)__builtin_ctzll(bal) : INT32_MAX;
    __syncthreads();
    int32_t r = INT32_MAX;
    for (int i = 0; i < nw; ++i) r = min(r, R.a[i]);
    __syncthreads();
    return r;
}
// Inclusive prefix maximum of the threads' keys.
template <bool LO = false>
__device__ __forceinline__ void blk_key_prefix_max(BlockRed &R, LKey &k) {
    const int w = threadIdx.x >> 6;
    int32_t p = 0;
    wave_key_prefix_max(k, p);
    if ((threadIdx.x & 63) == 63) { R.x[w] = k.x; R.g[w] = k.g; R.a[w] = k.l; }
    blk_sync<LO>();
    LKey c{-INFINITY, -INFINITY, INT32_MIN};
    for (int i = 0; i < w; ++i) {
        const LKey o{R.x[i], R.g[i], R.a[i]};
        if (key_gt(o, c)) c = o;
    }
    if (key_gt(c, k)) k = c;
    blk_sync<LO>();
}
}  // namespace prk
