// prelude.h — what the reference's absent platform and math headers would
// supply, written from SURVEY.md Appendix C.  TEST INFRASTRUCTURE ONLY: it is
// force-included in front of the lane-rewritten copy of the reference that
// oracle/ref/build_ref.py writes under oracle/_ref/ and is never part of the
// product.  Nothing here is taken from the reference; each helper whose
// semantics the absent headers would decide is a PIN (marked below, listed in
// build_ref.PINS and recorded in tests/golden/ref/MANIFEST.json).
#pragma once

#include <immintrin.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define internal static
#define global_variable static
#define local_persist static
// PIN: a failed Assert of the reference throws, so nothing is ever drawn past
// one; the driver decides what a failed one means (ref_driver.cpp)
struct reference_assert {
    int Line;
};
#define Assert(e)                                      \
    do {                                               \
        if (!(e)) throw reference_assert{__LINE__};    \
    } while (0)

typedef float r32;
typedef double r64;
typedef int8_t s8;
typedef int16_t s16;
typedef int32_t s32;
typedef int64_t s64;
typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int32_t b32;
typedef size_t memory_index;

#define Pi32 3.14159265359f
#define BITMAP_BYTES_PER_PIXEL 4

union v2 {
    struct { r32 x, y; };
    struct { r32 u, v; };
    r32 E[2];
};
union v3 {
    struct { r32 x, y, z; };
    struct { r32 r, g, b; };
    struct { v2 xy; r32 Ignored0_; };
    r32 E[3];
};
union v4 {
    struct { r32 r, g, b, a; };
    struct { r32 x, y, z, w; };
    struct { v3 xyz; r32 Ignored0_; };
    struct { v3 rgb; r32 Ignored1_; };
    r32 E[4];
};

inline v2 V2(r32 x, r32 y) { v2 r; r.x = x; r.y = y; return r; }
inline v2 V2i(s32 x, s32 y) { return V2((r32)x, (r32)y); }
inline v2 V2i(u32 x, u32 y) { return V2((r32)x, (r32)y); }
inline v3 V3(r32 x, r32 y, r32 z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
inline v3 V3(v2 xy, r32 z) { return V3(xy.x, xy.y, z); }
inline v4 V4(r32 x, r32 y, r32 z, r32 w) { v4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
inline v4 V4(v3 xyz, r32 w) { return V4(xyz.x, xyz.y, xyz.z, w); }

// component-wise arithmetic: one IEEE operation per component, nothing fused
// (the build has -mno-fma -ffp-contract=off)
inline v2 operator+(v2 a, v2 b) { return V2(a.x + b.x, a.y + b.y); }
inline v2 operator-(v2 a, v2 b) { return V2(a.x - b.x, a.y - b.y); }
inline v2 operator-(v2 a) { return V2(-a.x, -a.y); }
inline v2 operator*(r32 s, v2 a) { return V2(s * a.x, s * a.y); }
inline v2 operator*(v2 a, r32 s) { return s * a; }
inline v2 &operator+=(v2 &a, v2 b) { a = a + b; return a; }
inline v2 &operator-=(v2 &a, v2 b) { a = a - b; return a; }
inline v2 &operator*=(v2 &a, r32 s) { a = s * a; return a; }

inline v3 operator+(v3 a, v3 b) { return V3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline v3 operator-(v3 a, v3 b) { return V3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline v3 operator-(v3 a) { return V3(-a.x, -a.y, -a.z); }
inline v3 operator*(r32 s, v3 a) { return V3(s * a.x, s * a.y, s * a.z); }
inline v3 operator*(v3 a, r32 s) { return s * a; }
inline v3 &operator+=(v3 &a, v3 b) { a = a + b; return a; }
inline v3 &operator-=(v3 &a, v3 b) { a = a - b; return a; }
inline v3 &operator*=(v3 &a, r32 s) { a = s * a; return a; }

inline v4 operator+(v4 a, v4 b) { return V4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
inline v4 operator-(v4 a, v4 b) { return V4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
inline v4 operator-(v4 a) { return V4(-a.x, -a.y, -a.z, -a.w); }
inline v4 operator*(r32 s, v4 a) { return V4(s * a.x, s * a.y, s * a.z, s * a.w); }
inline v4 operator*(v4 a, r32 s) { return s * a; }
inline v4 &operator+=(v4 &a, v4 b) { a = a + b; return a; }
inline v4 &operator-=(v4 &a, v4 b) { a = a - b; return a; }
inline v4 &operator*=(v4 &a, r32 s) { a = s * a; return a; }

inline v2 Hadamard(v2 a, v2 b) { return V2(a.x * b.x, a.y * b.y); }
inline v3 Hadamard(v3 a, v3 b) { return V3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline v4 Hadamard(v4 a, v4 b) { return V4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

// PIN: Inner = (x·x + y·y) + z·z, left to right
inline r32 Inner(v2 a, v2 b) { return a.x * b.x + a.y * b.y; }
inline r32 Inner(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline r32 Inner(v4 a, v4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
inline r32 LengthSq(v3 a) { return Inner(a, a); }
inline r32 SquareRoot(r32 x) { return sqrtf(x); }
inline r32 Length(v3 a) { return sqrtf(Inner(a, a)); }
// PIN: Normalize = (1/sqrtf(Inner(a,a)))·a
inline v3 Normalize(v3 a) { return (1.0f / sqrtf(Inner(a, a))) * a; }
inline v3 Cross(v3 a, v3 b) {
    return V3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// PIN: Clamp01 by compares (a NaN passes through)
inline r32 Clamp01(r32 x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
inline v2 Clamp01(v2 a) { return V2(Clamp01(a.x), Clamp01(a.y)); }
inline v3 Clamp01(v3 a) { return V3(Clamp01(a.x), Clamp01(a.y), Clamp01(a.z)); }
inline v4 Clamp01(v4 a) { return V4(Clamp01(a.x), Clamp01(a.y), Clamp01(a.z), Clamp01(a.w)); }
inline r32 Clamp(r32 lo, r32 x, r32 hi) { return x < lo ? lo : (x > hi ? hi : x); }
inline r32 Maximum(r32 a, r32 b) { return a > b ? a : b; }
inline s32 Maximum(s32 a, s32 b) { return a > b ? a : b; }
inline u32 Maximum(u32 a, u32 b) { return a > b ? a : b; }
inline r32 Minimum(r32 a, r32 b) { return a < b ? a : b; }
inline s32 Minimum(s32 a, s32 b) { return a < b ? a : b; }
inline u32 Minimum(u32 a, u32 b) { return a < b ? a : b; }
inline r32 Square(r32 x) { return x * x; }
inline r32 AbsoluteValue(r32 x) { return fabsf(x); }
inline r32 Lerp(r32 a, r32 t, r32 b) { return (1.0f - t) * a + t * b; }

// PIN: rounding is roundf, halves away from zero
inline s32 RoundR32ToS32(r32 x) { return (s32)roundf(x); }
inline u32 RoundR32ToU32(r32 x) { return (u32)roundf(x); }
inline s32 FloorR32ToS32(r32 x) { return (s32)floorf(x); }
inline s32 CeilR32ToS32(r32 x) { return (s32)ceilf(x); }
inline s32 TruncateR32ToS32(r32 x) { return (s32)x; }
// PIN: libm's single-precision sine, cosine and power
inline r32 Sin(r32 x) { return sinf(x); }
inline r32 Cos(r32 x) { return cosf(x); }
inline r32 Pow(r32 a, r32 b) { return powf(a, b); }
inline r32 Power(r32 a, r32 b) { return powf(a, b); }

inline void *Copy(memory_index Size, const void *Source, void *Dest) { return memcpy(Dest, Source, Size); }
inline void ZeroSize(memory_index Size, void *Ptr) { memset(Ptr, 0, Size); }

struct loaded_bitmap {
    void *Memory;
    s32 Width;
    s32 Height;
    s32 Pitch;
};
struct projective_transform {
    r32 DistanceAboveTarget;
    r32 FocalLength;
    r32 MetersToPixels;
    v2 ScreenCenter;
};
struct light_info {
    v3 P;
    v4 Intensity;
};
struct light_data {
    light_info Lights[8];
    u32 LightCount;
    v4 AmbientIntensity;
};
struct game_render_commands {
    r32 *ZBuffer;
    u8 *ZMask;
    u32 Width;
    void *ThreadMemory;
    u32 ThreadMemorySize;
    u32 ThreadMemorySizeUsed;
    void *SortMemory;
    light_data LightData;
    projective_transform Transform;
};

// PIN: the work queue runs every entry at once, in submission order, on the
// calling thread
struct platform_work_queue {
    u32 Entries;
};
#define PLATFORM_WORK_QUEUE_CALLBACK(name) void name(platform_work_queue *Queue, void *Data)
typedef PLATFORM_WORK_QUEUE_CALLBACK(platform_work_queue_callback);
struct platform_api {
    void (*AddEntry)(platform_work_queue *Queue, platform_work_queue_callback *Callback, void *Data);
    void (*CompleteAllWork)(platform_work_queue *Queue);
};
inline void RefAddEntrySync(platform_work_queue *Queue, platform_work_queue_callback *Callback, void *Data) {
    ++Queue->Entries;
    Callback(Queue, Data);
}
inline void RefCompleteAllWork(platform_work_queue *) {}
global_variable platform_api Platform = {RefAddEntrySync, RefCompleteAllWork};

// PIN: the byte compare-and-swap and the write barrier of the absent compiler,
// by the host compiler's builtins (arguments: destination, exchange, comparand)
#define _InterlockedCompareExchange8(p, x, c) __sync_val_compare_and_swap((p), (char)(c), (char)(x))
#define _WriteBarrier() __asm__ __volatile__("" ::: "memory")

// Lane access of the vector types: the rewrite (build_ref.py) turns member
// access `V.m256i_u32[k]` and its kin into these.  Reads and writes both go
// through a reference to the lane, which GCC's may_alias vector types allow.
template <class T, class V>
inline T &RefLane(V &v, int k) {
    typedef T __attribute__((may_alias)) lane_t;
    return ((lane_t *)&v)[k];
}
#define LANE_256_u32(v, k) RefLane<u32>(v, k)
#define LANE_256_i32(v, k) RefLane<s32>(v, k)
#define LANE_256_f32(v, k) RefLane<r32>(v, k)
#define LANE_128_u32(v, k) RefLane<u32>(v, k)
#define LANE_128_i32(v, k) RefLane<s32>(v, k)
#define LANE_128_f32(v, k) RefLane<r32>(v, k)
