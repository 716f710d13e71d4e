// prk_visibility_api.hip — visibility feedback (prk.h prk_visibility_*,
// DESIGN.md §2.4), one of the host files over prk_ctx.h: what the last frame
// showed, per id of its winner numbering, answered from the winner map that a
// debug-mode flush leaves on the device.  The first query after a flush
// reduces the map (prk_visibility.hip: histogram, flags, two scans, compact)
// into the context's VisState and waits; later queries of the same frame are
// host copies from those arrays, plus k_vis_groups for caller ranges.
// (prk_selftest_visibility is in prk_selftest.hip.)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prk_ctx.h"

// The frame's answer, reduced if this is the first query since its flush.
// PRK_ERR_ARG: no such frame (prk_download_winners' precondition, and draws).
// (Hidden, prk_ctx.h: prk_geometry_select reads the frame's pix_prefix too.)
extern "C" int vis_ready(prk_context *c) {
    RESOLVE_COUNT(c);  // (an overflowed frame is re-run: its winner words land first)
    VisState &V = c->vis;
    if (!c->winners_valid || !V.frame || !c->d_winners.p) return PRK_ERR_ARG;
    if (V.done) return PRK_OK;
    const uint64_t n = (uint64_t)c->W * (uint64_t)(c->row1 - c->row0);
    if (n >= (1ull << 32)) return PRK_ERR_LIMIT;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // the frame, whichever streams it ran on (as prk_download_winners)
    const uint32_t ids = V.id_count;
    const size_t mb = ((size_t)ids + 1) * 4;
    size_t tb = 0;
    PRK_TRY(prk_vis_reduce(nullptr, (uint32_t)n, ids, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &tb,
                           nullptr, nullptr));
    PRK_TRY(V.d_counts.ensure(mb));
    PRK_TRY(V.d_flags.ensure(mb));
    PRK_TRY(V.d_pix.ensure(mb));
    PRK_TRY(V.d_vis.ensure(mb));
    PRK_TRY(V.d_ids.ensure(std::max<size_t>((size_t)ids * 4, 4)));
    PRK_TRY(V.d_temp.ensure(std::max<size_t>(tb, 16)));
    hipStream_t s = c->own_stream;
    PRK_TRY(prk_vis_reduce(c->d_winners.as<int32_t>(), (uint32_t)n, ids, V.d_counts.as<uint32_t>(),
                           V.d_flags.as<uint32_t>(), V.d_pix.as<uint32_t>(), V.d_vis.as<uint32_t>(),
                           V.d_ids.as<uint32_t>(), V.d_temp.p, &tb, nullptr, s));
    uint32_t tot[2] = {0, 0};  // the prefix arrays' last words
    PRK_TRY(hipMemcpyAsync(&tot[0], V.d_pix.as<uint32_t>() + ids, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipMemcpyAsync(&tot[1], V.d_vis.as<uint32_t>() + ids, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    V.covered = tot[0];
    V.visible = tot[1];
    V.done = true;
    return PRK_OK;
}

extern "C" {

int prk_visibility_info(prk_context *c, uint32_t *id_count, uint64_t *covered, uint32_t *visible_ids) {
    if (!c || !id_count || !covered || !visible_ids) return PRK_ERR_ARG;
    PRK_CHECK(vis_ready(c));
    *id_count = c->vis.id_count;
    *covered = c->vis.covered;
    *visible_ids = c->vis.visible;
    return PRK_OK;
}

int prk_visibility_counts(prk_context *c, uint32_t first_id, uint32_t count, uint32_t *pixels) {
    if (!c || (!pixels && count)) return PRK_ERR_ARG;
    PRK_CHECK(vis_ready(c));
    if ((uint64_t)first_id + count > c->vis.id_count) return PRK_ERR_ARG;
    if (count)
        PRK_TRY(hipMemcpy(pixels, c->vis.d_counts.as<uint32_t>() + first_id, (size_t)count * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_visibility_groups(prk_context *c, const uint32_t *starts, uint32_t group_count, uint32_t *pixels,
                          uint32_t *visible) {
    if (!c || !starts || (!pixels && !visible)) return PRK_ERR_ARG;
    PRK_CHECK(vis_ready(c));
    VisState &V = c->vis;
    for (uint32_t g = 0; g < group_count; ++g)
        if (starts[g] > starts[g + 1]) return PRK_ERR_ARG;
    if (starts[group_count] > V.id_count) return PRK_ERR_ARG;
    if (group_count == 0) return PRK_OK;
    const size_t gb = (size_t)group_count * 4;
    PRK_TRY(V.d_starts.ensure(gb + 4));
    PRK_TRY(V.d_gout.ensure(2 * gb));
    hipStream_t s = c->own_stream;
    uint32_t *dp = pixels ? V.d_gout.as<uint32_t>() : nullptr;
    uint32_t *dv = visible ? V.d_gout.as<uint32_t>() + group_count : nullptr;
    PRK_TRY(hipMemcpyAsync(V.d_starts.p, starts, gb + 4, hipMemcpyHostToDevice, s));
    PRK_TRY(prk_vis_groups(V.d_starts.as<uint32_t>(), group_count, V.d_pix.as<uint32_t>(), V.d_vis.as<uint32_t>(), dp,
                           dv, s));
    // (both outputs land, or neither: the copies follow the one wait)
    PRK_TRY(hipStreamSynchronize(s));
    if (pixels) PRK_TRY(hipMemcpy(pixels, dp, gb, hipMemcpyDeviceToHost));
    if (visible) PRK_TRY(hipMemcpy(visible, dv, gb, hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_visibility_ids(prk_context *c, uint32_t *ids, uint64_t capacity, uint64_t *total_out) {
    if (!c || !total_out) return PRK_ERR_ARG;
    *total_out = 0;
    PRK_CHECK(vis_ready(c));
    const uint32_t total = c->vis.visible;
    *total_out = total;
    if (!ids) return PRK_OK;  // the size only
    if (capacity < total) return PRK_ERR_ARG;
    if (total) PRK_TRY(hipMemcpy(ids, c->vis.d_ids.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_visibility_device(prk_context *c, const uint32_t **counts, const uint32_t **pix_prefix, uint32_t *id_count) {
    if (!c || !counts || !pix_prefix || !id_count) return PRK_ERR_ARG;
    PRK_CHECK(vis_ready(c));
    *counts = c->vis.d_counts.as<uint32_t>();
    *pix_prefix = c->vis.d_pix.as<uint32_t>();
    *id_count = c->vis.id_count;
    return PRK_OK;
}

}  // extern "C"
