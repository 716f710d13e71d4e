// prk_xform_dev.h — one vertex of prk_geometry_transform's arithmetic, shared
// by the two passes that write transformed triangles into a resident geometry:
// k_xform (prk_xform.hip, runs listed by the host) and k_sel_emit
// (prk_select.hip, runs chosen on the device).  Device code only; both files
// are built with -ffp-contract=off and say so again with the pragma.
//
// For a position, component i,
//     out[i] = ((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + M[i][3]
// every product and sum rounded to f32 on its own, in this order; a normal
// the same without the last sum; colours and uvs copied as words.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace prk {

// Vertex records of the arrays.  A source geometry may be a caller's device
// pointers (prk_geometry_wrap_device), of which only float alignment is known.
struct __attribute__((packed, aligned(4))) XfV3 {
    float x, y, z;
};
struct __attribute__((packed, aligned(4))) XfV4u {  // colours of a source
    float x, y, z, w;
};
struct __attribute__((packed, aligned(4))) XfV2u {  // uvs of a source
    float x, y;
};

struct XformArrays {
    const float *sV, *sC, *sN, *sUV;  // source (an absent array: nullptr)
    float *dV, *dC, *dN, *dUV;        // destination: library-owned (hipMalloc alignment)
};

__device__ __forceinline__ float xf_row3(const float4 m, float x, float y, float z) {
    return (m.x * x + m.y * y) + m.z * z;
}

// Source vertex sv through the matrix at M (three float4 rows) to destination
// vertex dv, every array the source has.  A lane holds its vertex's matrix in
// registers (three 16-byte loads, one address for the whole wave inside a run).
__device__ __forceinline__ void xform_vertex(const XformArrays &A, size_t sv, size_t dv,
                                             const float4 *__restrict__ M) {
    const float4 m0 = M[0], m1 = M[1], m2 = M[2];
    {
        const XfV3 p = reinterpret_cast<const XfV3 *>(A.sV)[sv];
        XfV3 o;
        o.x = xf_row3(m0, p.x, p.y, p.z) + m0.w;
        o.y = xf_row3(m1, p.x, p.y, p.z) + m1.w;
        o.z = xf_row3(m2, p.x, p.y, p.z) + m2.w;
        reinterpret_cast<XfV3 *>(A.dV)[dv] = o;
    }
    if (A.sN) {
        const XfV3 p = reinterpret_cast<const XfV3 *>(A.sN)[sv];
        XfV3 o;
        o.x = xf_row3(m0, p.x, p.y, p.z);
        o.y = xf_row3(m1, p.x, p.y, p.z);
        o.z = xf_row3(m2, p.x, p.y, p.z);
        reinterpret_cast<XfV3 *>(A.dN)[dv] = o;
    }
    if (A.sC) {
        const XfV4u c = reinterpret_cast<const XfV4u *>(A.sC)[sv];
        reinterpret_cast<float4 *>(A.dC)[dv] = make_float4(c.x, c.y, c.z, c.w);
    }
    if (A.sUV) {
        const XfV2u c = reinterpret_cast<const XfV2u *>(A.sUV)[sv];
        reinterpret_cast<float2 *>(A.dUV)[dv] = make_float2(c.x, c.y);
    }
}

}  // namespace prk
