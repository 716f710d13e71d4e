// prk_tex.hip — prk_texture_from_target's device pass: a rectangle of the bound
// target's colour box-filtered by 1, 2 or 4 into a rectangle of a texture
// (prk.h).  An extension with its own definition: the
// reference has no render-to-texture.
//
// Arithmetic, per destination texel and per 8-bit channel of the 0xAARRGGBB
// word, integers only:
//     out = (sum of the F*F source channel values + F*F/2) >> (2*log2(F))
// F == 1 copies the word.  The channels are summed as packed 16-bit pairs:
// a word's 0x00FF00FF halves (B and R; A and G after a shift by 8) go into
// two 32-bit accumulators, each field taking at most 16 values of <= 255
// (4080 + 8 < 65536, so no field carries into its neighbour); after the
// shift a field's result is <= 255 and the neighbour's bits that the shift
// moved in lie above bit 7 of the field, where the mask drops them.
//
// Layout of the work: a 2-D grid over the destination rectangle.  A lane takes
// a QUAD: the (up to) four texels of one destination row that share a 16-byte
// line of the texture, so a whole quad leaves in one 16-byte store wherever
// the row starts (a texture's pitch and dst_x only promise 4 bytes; the quads
// of a row are cut from the row's actual address).  The first and last quad of
// a row may be partial: those texels go one dword at a time.  A whole quad
// reads its 4F source pixels of each of the F source rows in the widest pieces
// the row's actual address allows (16, 8 or 4 bytes: a caller-bound target
// promises 4, and x0 is arbitrary); the choice is the same for every lane of
// a row, and a wave is 64 quads of one row, so no wave diverges on it.
// Nothing outside the two rectangles is read or written.  No LDS, no loop as
// long as a row, one launch a call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prk_launch.h"

namespace {

constexpr uint32_t kQuads = 64;  // quads of one row a workgroup takes: one wave
constexpr uint32_t kRows = 4;    // destination rows a workgroup takes

// n consecutive words at p (4-byte aligned) in the widest loads p allows.
template <int N>
__device__ __forceinline__ void load_words(const uint8_t *p, uint32_t (&w)[N]) {
    static_assert(N % 4 == 0, "whole 16-byte pieces");
    const uintptr_t u = reinterpret_cast<uintptr_t>(p);
    if (!(u & 15)) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
        }
    } else if (!(u & 7)) {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const uint2 v = reinterpret_cast<const uint2 *>(p)[i];
            w[2 * i] = v.x, w[2 * i + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = reinterpret_cast<const uint32_t *>(p)[i];
    }
}

// The two accumulators of a texel -> its word (F > 1).
template <int F>
__device__ __forceinline__ uint32_t resolve(uint32_t lo, uint32_t hi) {
    constexpr uint32_t kShift = F == 2 ? 2 : 4;
    constexpr uint32_t kBias = (uint32_t)(F * F / 2) * 0x00010001u;
    lo = ((lo + kBias) >> kShift) & 0x00FF00FFu;
    hi = ((hi + kBias) >> kShift) & 0x00FF00FFu;
    return lo | (hi << 8);
}

// src: the source rectangle's first pixel, dst: the destination rectangle's
// first texel (both 4-byte aligned, rows spitch / dpitch bytes apart); the
// destination is dw x dh texels, the source F*dw x F*dh pixels.
template <int F>
__global__ __launch_bounds__(kQuads *kRows) void k_tex_from_target(const uint8_t *__restrict__ src, size_t spitch,
                                                                    uint8_t *__restrict__ dst, size_t dpitch,
                                                                    uint32_t dw, uint32_t dh) {
    const uint32_t r = (blockIdx.y + blockIdx.z * gridDim.y) * kRows + threadIdx.y;
    if (r >= dh) return;
    uint8_t *drow = dst + (size_t)r * dpitch;
    // the row's first texel is word `a` of its 16-byte line: quad q is the
    // line's words, texels [4q - a, 4q - a + 4) of the row, cut to [0, dw)
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(drow) >> 2) & 3u;
    const uint32_t q = blockIdx.x * kQuads + threadIdx.x;  // (4q + 4 <= dw + 10: no wrap, dw < 2^29)
    const uint32_t tb = q ? 4u * q - a : 0u;
    const uint32_t te = min(4u * q + 4u - a, dw);
    if (tb >= te) return;
    const uint8_t *s = src + (size_t)r * F * spitch + (size_t)tb * F * 4u;
    uint32_t *d = reinterpret_cast<uint32_t *>(drow) + tb;
    if (te - tb == 4u) {  // a whole quad: d is 16-byte aligned
        uint4 o;
        if (F == 1) {
            uint32_t w[4];
            load_words<4>(s, w);
            o = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
#pragma unroll
            for (int y = 0; y < F; ++y) {
                uint32_t w[4 * F];
                load_words<4 * F>(s + (size_t)y * spitch, w);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int x = 0; x < F; ++x) {
                        lo[t] += w[t * F + x] & 0x00FF00FFu;
                        hi[t] += (w[t * F + x] >> 8) & 0x00FF00FFu;
                    }
            }
            o = make_uint4(resolve<F>(lo[0], hi[0]), resolve<F>(lo[1], hi[1]), resolve<F>(lo[2], hi[2]),
                           resolve<F>(lo[3], hi[3]));
        }
        *reinterpret_cast<uint4 *>(d) = o;
        return;
    }
    // a row's partial first or last quad: 1 to 3 texels, dwords
    for (uint32_t t = 0; t < te - tb; ++t) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(s) + t * F;
        if (F == 1) {
            d[t] = p[0];
            continue;
        }
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int y = 0; y < F; ++y) {
            const uint32_t *py = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(p) +
                                                                     (size_t)y * spitch);
#pragma unroll
            for (int x = 0; x < F; ++x) {
                lo += py[x] & 0x00FF00FFu;
                hi += (py[x] >> 8) & 0x00FF00FFu;
            }
        }
        d[t] = resolve<F>(lo, hi);
    }
}

}  // namespace

// The caller (prk_target_api.hip) has checked both rectangles against the target's
// band and the texture; factor is 1, 2 or 4; dw, dh > 0.
extern "C" hipError_t prk_tex_from_target_launch(const void *src, size_t spitch, void *dst, size_t dpitch,
                                                 uint32_t dw, uint32_t dh, int32_t factor, hipStream_t s) {
    // quads of a row: a row that starts at word a of its line has (a + dw + 3) / 4;
    // rows of a pitch that is no multiple of 16 start at every a
    const uint32_t a = (dpitch & 15) ? 3u : (uint32_t)(reinterpret_cast<uintptr_t>(dst) >> 2) & 3u;
    const uint32_t nq = (a + dw + 3u) / 4u;
    const uint32_t nby = (dh + kRows - 1) / kRows;
    const uint32_t gy = nby < 65535u ? nby : 65535u;
    const dim3 grid((nq + kQuads - 1) / kQuads, gy, (nby + gy - 1) / gy), block(kQuads, kRows);
    const uint8_t *sp = static_cast<const uint8_t *>(src);
    uint8_t *dp = static_cast<uint8_t *>(dst);
    switch (factor) {
    case 1: hipLaunchKernelGGL(k_tex_from_target<1>, grid, block, 0, s, sp, spitch, dp, dpitch, dw, dh); break;
    case 2: hipLaunchKernelGGL(k_tex_from_target<2>, grid, block, 0, s, sp, spitch, dp, dpitch, dw, dh); break;
    case 4: hipLaunchKernelGGL(k_tex_from_target<4>, grid, block, 0, s, sp, spitch, dp, dpitch, dw, dh); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
