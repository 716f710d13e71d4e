// prk_layer.hip — the device pass of prk_layer_from_target and
// prk_target_from_layer: a rectangle of (colour, z) pixels moved from one
// pair of planes to another, every pixel or only the pixels whose source z
// wins (prk.h).  An extension with its own definition: the
// reference keeps one framebuffer and has no layers.
//
// Per pixel, with (cs, zs) the source's words and (cd, zd) the destination's:
//     PRK_MERGE_COPY           (cd, zd) = (cs, zs)
//     PRK_MERGE_GREATER        the same where zs >  zd
//     PRK_MERGE_GREATER_EQUAL  the same where zs >= zd
// The comparison is IEEE f32 on the z words (a NaN on either side loses,
// -0.0 equals +0.0, denormals compare by value: the library is built without
// flush-to-zero); the words move as bits.  A pixel that does not win is not
// stored, so it keeps both its words.  Save (prk_layer_from_target) is COPY
// with the target as source.
//
// Layout of the work, k_tex_from_target's: a 2-D grid over the rectangle.  A
// lane takes QUADS: the (up to) four pixels of one row that share a 16-byte
// line of the destination's colour plane, so a whole quad's colour leaves in
// one 16-byte store wherever the row starts (pitches, x0 and wrapped
// addresses only promise 4 bytes; the quads of a row are cut from the row's
// actual address).  The other three accesses of a whole quad (source colour,
// source z, destination z) go in the widest pieces their own row addresses
// allow, 16, 8 or 4 bytes; the choice depends on the row alone, and a wave is
// one row, so it is made once a wave on a scalar.  The first and last quad of
// a row may be partial: those pixels go one dword at a time.
// A lane takes kPer quads of its row, a wave apart, and loads all of them
// before it stores any: kPer 16-byte loads a plane in flight per lane.
// Nothing outside the two rectangles is read or written.  No LDS, one launch
// a call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/prk.h"
#include "prk_launch.h"

namespace {

constexpr uint32_t kLanes = 64;  // lanes of one row a workgroup has: one wave
constexpr uint32_t kRows = 4;    // rows a workgroup takes
constexpr uint32_t kPer = 4;     // quads of its row a lane takes

// The widest piece that every whole quad of a row may use in a plane whose
// row starts at p, when the quads start `a` words before p (mod 4): 4 words,
// 2 or 1.  The same for every lane of a wave (a wave is one row).
__device__ __forceinline__ uint32_t piece_words(const uint32_t *p, uint32_t a) {
    const uint32_t m = ((uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) - a) & 3u;
    return __builtin_amdgcn_readfirstlane(m == 0 ? 4u : (m == 2 ? 2u : 1u));
}

__device__ __forceinline__ void load_quad(const uint32_t *p, uint32_t piece, uint32_t (&w)[4]) {
    if (piece == 4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else if (piece == 2) {
        const uint2 u = reinterpret_cast<const uint2 *>(p)[0], v = reinterpret_cast<const uint2 *>(p)[1];
        w[0] = u.x, w[1] = u.y, w[2] = v.x, w[3] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = p[i];
    }
}

__device__ __forceinline__ void store_quad(uint32_t *p, uint32_t piece, const uint32_t (&w)[4]) {
    if (piece == 4) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (piece == 2) {
        reinterpret_cast<uint2 *>(p)[0] = make_uint2(w[0], w[1]);
        reinterpret_cast<uint2 *>(p)[1] = make_uint2(w[2], w[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = w[i];
    }
}

template <int RULE>
__device__ __forceinline__ bool wins(uint32_t zs, uint32_t zd) {
    const float s = __uint_as_float(zs), d = __uint_as_float(zd);
    return RULE == PRK_MERGE_GREATER ? s > d : s >= d;
}

// sc / sz: the source rectangle's first colour word and z word, dc / dz the
// destination's (all 4-byte aligned; rows scp / szp / dcp / dzp bytes apart);
// w x h pixels.  The source and the destination do not overlap.
template <int RULE>
__global__ __launch_bounds__(kLanes *kRows) void k_layer(const uint8_t *__restrict__ sc, size_t scp,
                                                          const uint8_t *__restrict__ sz, size_t szp,
                                                          uint8_t *__restrict__ dc, size_t dcp,
                                                          uint8_t *__restrict__ dz, size_t dzp, uint32_t w, uint32_t h) {
    const uint32_t r = (blockIdx.y + blockIdx.z * gridDim.y) * kRows + threadIdx.y;
    if (r >= h) return;
    const uint32_t *scr = reinterpret_cast<const uint32_t *>(sc + (size_t)r * scp);
    const uint32_t *szr = reinterpret_cast<const uint32_t *>(sz + (size_t)r * szp);
    uint32_t *dcr = reinterpret_cast<uint32_t *>(dc + (size_t)r * dcp);
    uint32_t *dzr = reinterpret_cast<uint32_t *>(dz + (size_t)r * dzp);
    // the row's first pixel is word `a` of its 16-byte line in the destination's
    // colour plane: quad q is that line's words, pixels [4q - a, 4q - a + 4) of
    // the row, cut to [0, w)
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(dcr) >> 2) & 3u;
    const uint32_t psc = piece_words(scr, a), psz = piece_words(szr, a), pdz = piece_words(dzr, a);
    uint32_t tb[kPer], n[kPer];  // a lane's quads: first pixel, pixels (0: none)
    uint32_t cs[kPer][4], zs[kPer][4], zd[kPer][4];
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t q = (blockIdx.x * kPer + j) * kLanes + threadIdx.x;  // (4q + 4 < w + 1040: no wrap, w < 2^29)
        tb[j] = q ? 4u * q - a : 0u;
        const uint32_t te = min(4u * q + 4u - a, w);
        n[j] = tb[j] < te ? te - tb[j] : 0u;
        if (n[j] != 4u) continue;
        load_quad(scr + tb[j], psc, cs[j]);
        load_quad(szr + tb[j], psz, zs[j]);
        if (RULE != PRK_MERGE_COPY) load_quad(dzr + tb[j], pdz, zd[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t t0 = tb[j];
        if (n[j] == 4u) {  // a whole quad: dcr + t0 is 16-byte aligned
            uint32_t win = 15u;
            if (RULE != PRK_MERGE_COPY) {
                win = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) win |= (wins<RULE>(zs[j][i], zd[j][i]) ? 1u : 0u) << i;
            }
            if (win == 15u) {
                store_quad(dcr + t0, 4, cs[j]);
                store_quad(dzr + t0, pdz, zs[j]);
            } else if (win) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (win >> i & 1u) {
                        dcr[t0 + i] = cs[j][i];
                        dzr[t0 + i] = zs[j][i];
                    }
            }
            continue;
        }
        // a row's partial first or last quad: 1 to 3 pixels, dwords
        for (uint32_t i = 0; i < n[j]; ++i) {
            const uint32_t z = szr[t0 + i];
            if (RULE != PRK_MERGE_COPY && !wins<RULE>(z, dzr[t0 + i])) continue;
            dcr[t0 + i] = scr[t0 + i];
            dzr[t0 + i] = z;
        }
    }
}

}  // namespace

// The caller (prk_target_api.hip) has checked both rectangles against the layer and
// the target's band; rule is a PRK_MERGE_*; w, h > 0.
extern "C" hipError_t prk_layer_launch(const void *src_color, size_t src_cpitch, const float *src_z, size_t src_zpitch,
                                       void *dst_color, size_t dst_cpitch, float *dst_z, size_t dst_zpitch, uint32_t w,
                                       uint32_t h, int32_t rule, hipStream_t s) {
    // quads of a row: a row that starts at word a of its line has (a + w + 3) / 4;
    // rows of a pitch that is no multiple of 16 start at every a
    const uint32_t a = (dst_cpitch & 15) ? 3u : (uint32_t)(reinterpret_cast<uintptr_t>(dst_color) >> 2) & 3u;
    const uint32_t nq = (a + w + 3u) / 4u;
    const uint32_t nby = (h + kRows - 1) / kRows;
    const uint32_t gy = nby < 65535u ? nby : 65535u;
    const dim3 grid((nq + kLanes * kPer - 1) / (kLanes * kPer), gy, (nby + gy - 1) / gy), block(kLanes, kRows);
    const uint8_t *sc = static_cast<const uint8_t *>(src_color), *sz = reinterpret_cast<const uint8_t *>(src_z);
    uint8_t *dc = static_cast<uint8_t *>(dst_color), *dz = reinterpret_cast<uint8_t *>(dst_z);
#define PRK_LAYER_LAUNCH(R) \
    hipLaunchKernelGGL(k_layer<R>, grid, block, 0, s, sc, src_cpitch, sz, src_zpitch, dc, dst_cpitch, dz, dst_zpitch, w, h)
    switch (rule) {
    case PRK_MERGE_COPY: PRK_LAYER_LAUNCH(PRK_MERGE_COPY); break;
    case PRK_MERGE_GREATER: PRK_LAYER_LAUNCH(PRK_MERGE_GREATER); break;
    case PRK_MERGE_GREATER_EQUAL: PRK_LAYER_LAUNCH(PRK_MERGE_GREATER_EQUAL); break;
    default: return hipErrorInvalidValue;
    }
#undef PRK_LAYER_LAUNCH
    return hipGetLastError();
}
