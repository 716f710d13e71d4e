// prk_bounds_api.hip — prk_visibility_bounds (prk.h), one of
// the host files over prk_ctx.h: bounding boxes tested on the device against
// the depth the target holds now, for the items a frame did not draw.  The call
// checks its tables on the host (no status depends on device results), uploads
// them, queues the two kernels of prk_bounds.hip where prk_layer_from_target
// queues its pass -- after the frames already flushed and after the clears,
// uploads and layer calls queued so far -- and waits.  The tile map belongs to
// the target and is rebuilt at every call: nothing here reads or writes
// VisState.  (prk_selftest_bounds is in prk_selftest.hip;
// prk_geometry_select_bounds is in prk_select_api.hip.)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prk_ctx.h"

extern "C" {

// The band's tile counts and the camera as the kernels read them.  false: the
// band has 2^32 pixels or more.
bool bounds_frame(int32_t W, int32_t row0, int32_t row1, const prk_transform &t, const float P[3],
                  prk::BoundsFrame *out) {
    if ((uint64_t)W * (uint64_t)(row1 - row0) >= (1ull << 32)) return false;
    prk::BoundsFrame B{};
    B.W = W;
    B.row0 = row0;
    B.row1 = row1;
    B.tiles_x = (W + 7) / 8;
    B.first_tile_row = row0 / 8;
    B.tiles_y = (row1 + 7) / 8 - B.first_tile_row;
    B.D = t.DistanceAboveTarget;
    B.F = t.FocalLength;
    B.M2P = t.MetersToPixels;
    B.Cx = t.ScreenCenter[0];
    B.Cy = t.ScreenCenter[1];
    for (int k = 0; k < 3; ++k) B.P[k] = P ? P[k] : 0.0f;
    *out = B;
    return true;
}

int prk_visibility_bounds(prk_context *c, const prk_bound *bounds, uint32_t count, const prk_xform *xforms,
                          uint32_t xform_count, const float P[3], uint32_t *pixels) {
    if (!c || (count && (!bounds || !xforms))) return PRK_ERR_ARG;
    if (!c->have_camera) return PRK_ERR_ARG;
    for (uint32_t i = 0; i < count; ++i)
        if (bounds[i].xform >= xform_count) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    prk::BoundsFrame B;
    if (!bounds_frame(c->W, c->row0, c->row1, c->transform, P, &B)) return PRK_ERR_LIMIT;
    RESOLVE_COUNT(c);  // (an overflowed frame is re-run: its z lands first)
    PRK_TRY(hipSetDevice(c->device));
    BoundsState &S = c->bnd;
    for (hipEvent_t &e : S.ev)
        if (!e) PRK_TRY(hipEventCreate(&e));
    // the caller's tables in one buffer, the matrices first (16-byte loads)
    const size_t xb = (size_t)xform_count * sizeof(prk_xform), bb = (size_t)count * sizeof(prk_bound);
    const size_t b_off = (xb + 15) & ~(size_t)15;
    PRK_TRY(S.d_zmin.ensure((size_t)B.tiles_x * (size_t)B.tiles_y * 4));
    PRK_TRY(S.d_tab.ensure(b_off + bb + 16));
    PRK_TRY(S.d_pixels.ensure(std::max<size_t>((size_t)count * 4, 4)));
    S.answered = false;  // (a failure from here on leaves no answer)
    uint8_t *tab = S.d_tab.as<uint8_t>();
    hipStream_t s = c->copy_stream;
    PRK_TRY(side_begin(c, true));  // (the target form; no side_end: the pass only reads, and the call waits)
    if (count) {
        PRK_TRY(hipMemcpyAsync(tab, xforms, xb, hipMemcpyHostToDevice, s));
        PRK_TRY(hipMemcpyAsync(tab + b_off, bounds, bb, hipMemcpyHostToDevice, s));
    }
    PRK_TRY(hipEventRecord(S.ev[0], s));
    PRK_TRY(prk_ztile_min(c->zbuf, &B, S.d_zmin.as<float>(), s));
    PRK_TRY(hipEventRecord(S.ev[1], s));
    PRK_TRY(prk_bounds_test(reinterpret_cast<const prk_bound *>(tab + b_off), count,
                            reinterpret_cast<const prk_xform *>(tab), &B, S.d_zmin.as<float>(),
                            S.d_pixels.as<uint32_t>(), s));
    PRK_TRY(hipEventRecord(S.ev[2], s));
    if (pixels && count)
        PRK_TRY(hipMemcpyAsync(pixels, S.d_pixels.p, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));  // the tables are copied, the answer is complete
    S.answered = S.timed = true;
    S.tested = count != 0;
    S.count = count;
    S.tiles_x = B.tiles_x;
    S.tiles_y = B.tiles_y;
    S.first_tile_row = B.first_tile_row;
    return PRK_OK;
}

int prk_visibility_bounds_device(prk_context *c, const uint32_t **pixels, uint32_t *count) {
    if (!c || !pixels || !count || !c->bnd.answered) return PRK_ERR_ARG;
    *pixels = c->bnd.d_pixels.as<uint32_t>();
    *count = c->bnd.count;
    return PRK_OK;
}

int prk_debug_ztiles(prk_context *c, float *zmin, uint64_t capacity, int32_t *tiles_x, int32_t *tiles_y,
                     int32_t *first_tile_row) {
    if (!c || !tiles_x || !tiles_y || !first_tile_row || !c->bnd.answered) return PRK_ERR_ARG;
    const BoundsState &S = c->bnd;
    const uint64_t n = (uint64_t)S.tiles_x * (uint64_t)S.tiles_y;
    if (zmin && capacity < n) return PRK_ERR_ARG;
    if (zmin) {
        PRK_TRY(hipSetDevice(c->device));
        PRK_TRY(hipMemcpy(zmin, S.d_zmin.p, n * 4, hipMemcpyDeviceToHost));
    }
    *tiles_x = S.tiles_x;
    *tiles_y = S.tiles_y;
    *first_tile_row = S.first_tile_row;
    return PRK_OK;
}

int prk_debug_bounds_ms(prk_context *c, float *ztile_ms, float *test_ms) {
    if (!c || !ztile_ms || !test_ms || !c->bnd.timed) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    BoundsState &S = c->bnd;
    float a = 0.0f, b = 0.0f;
    PRK_TRY(hipEventSynchronize(S.ev[2]));
    PRK_TRY(hipEventElapsedTime(&a, S.ev[0], S.ev[1]));
    if (S.tested) PRK_TRY(hipEventElapsedTime(&b, S.ev[1], S.ev[2]));
    *ztile_ms = a;
    *test_ms = b;
    return PRK_OK;
}

}  // extern "C"
