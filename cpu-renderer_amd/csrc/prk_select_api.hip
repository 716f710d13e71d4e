// prk_select_api.hip — prk_geometry_select (prk.h), one of
// the host files over prk_ctx.h: cull and pick a level of detail on the
// device.  The call checks its tables against worst cases on the host (no
// status depends on what the device chooses), copies them, queues the choice
// and the scan (prk_select.hip) on the geometry stream and waits for one
// word, the triangle total; it then sizes dst and the grid from it and queues
// the emit pass as prk_geometry_transform queues its pass, without waiting.
// (prk_selftest_select is in prk_selftest.hip; both run select_check and the
// launchers of prk_launch.h.)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "prk_ctx.h"

extern "C" {

// The argument checks that need no context: the tables against each other,
// against a source of src_tris triangles and, when the counts are a frame's
// (frame_ids != nullptr), against its id count.  *worst: for every item its
// largest level, summed (what the device can choose at most).  PRK_ERR_ARG,
// or PRK_OK.  (NULL items with item_count > 0 is the caller's check.)
int select_check(const prk_select_item *items, uint32_t item_count, const prk_select_level *levels,
                 uint32_t level_count, const prk_xform *xforms, uint32_t xform_count, uint32_t src_tris,
                 const uint32_t *frame_ids, uint64_t *worst) {
    uint64_t sum = 0;
    for (uint32_t i = 0; i < item_count; ++i) {
        const prk_select_item &it = items[i];
        if ((uint64_t)it.first_level + it.level_count > level_count) return PRK_ERR_ARG;
        if (frame_ids && (uint64_t)it.first_id + it.id_count > *frame_ids) return PRK_ERR_ARG;
        if (!it.level_count) continue;
        if (!levels || !xforms || it.xform >= xform_count) return PRK_ERR_ARG;
        uint32_t most = 0;
        for (uint32_t l = 0; l < it.level_count; ++l) {
            const prk_select_level &lv = levels[it.first_level + l];
            if (!lv.tri_count) continue;  // (an empty range passes nothing)
            if ((uint64_t)lv.src_first_tri + lv.tri_count > src_tris) return PRK_ERR_ARG;
            most = std::max(most, lv.tri_count);
        }
        sum += most;
    }
    *worst = sum;
    return PRK_OK;
}

}  // extern "C"

// The body of prk_geometry_select and prk_geometry_select_bounds.  `bounds`:
// the second call -- no item_pixels, an item without ids takes its word of the
// last prk_visibility_bounds' answer (which must be there, item_count words),
// and the frame is needed only where some item has ids.
static int select_body(prk_context *c, int32_t src, int32_t dst, uint32_t dst_first_tri, const prk_select_item *items,
                       uint32_t item_count, const prk_select_level *levels, uint32_t level_count,
                       const prk_xform *xforms, uint32_t xform_count, const uint32_t *item_pixels, bool bounds,
                       int32_t *chosen, uint32_t *out_first, uint64_t *total_tris_out) {
    if (!c || !total_tris_out || (item_count && !items)) return PRK_ERR_ARG;
    if (src < 0 || (size_t)src >= c->geoms.size() || dst < 0 || (size_t)dst >= c->geoms.size() || src == dst)
        return PRK_ERR_ARG;
    if (!c->geoms[dst].owned) return PRK_ERR_ARG;
    if (bounds && (!c->bnd.answered || c->bnd.count != item_count)) return PRK_ERR_ARG;
    const uint32_t src_tris = c->geoms[src].vertex_count / 3;
    uint32_t frame_ids = 0;
    bool frame = !item_pixels;
    if (bounds) {
        frame = false;
        for (uint32_t i = 0; i < item_count && !frame; ++i) frame = items[i].id_count != 0;
    }
    if (frame) {  // the frame's counts: there must be a frame (reduced here if no query has yet)
        PRK_CHECK(vis_ready(c));
        frame_ids = c->vis.id_count;
    }
    uint64_t worst = 0;
    PRK_CHECK(select_check(items, item_count, levels, level_count, xforms, xform_count, src_tris,
                           frame ? &frame_ids : nullptr, &worst));
    if (worst && !c->geoms[src].V) return PRK_ERR_ARG;  // (a geometry written without positions)
    // (the total first: 2^31 triangles are past the vertex limit wherever they start)
    if (worst > (1ull << 31)) return PRK_ERR_LIMIT;
    if (((uint64_t)dst_first_tri + worst) * 3 > 0xFFFFFFF0ull) return PRK_ERR_ARG;
    if (item_count == 0) {
        *total_tris_out = 0;
        if (out_first) out_first[0] = dst_first_tri;
        return PRK_OK;
    }
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    SelState &S = c->sel;
    for (hipEvent_t &e : S.ev)
        if (!e) PRK_TRY(hipEventCreate(&e));
    // the caller's tables in one buffer, every part at a multiple of 16 bytes
    const auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t ib = (size_t)item_count * sizeof(prk_select_item);
    const size_t lb = (size_t)level_count * sizeof(prk_select_level);
    const size_t xb = (size_t)xform_count * sizeof(prk_xform);
    const size_t pb = item_pixels ? (size_t)item_count * 4 : 0;
    const size_t lev_off = up16(ib), xf_off = lev_off + up16(levels ? lb : 0), px_off = xf_off + up16(xforms ? xb : 0);
    PRK_TRY(S.d_tab.ensure(px_off + up16(pb) + 16));
    // what the device builds: chosen, n, start (item_count + 1 words each), the runs
    const size_t wb = up16(((size_t)item_count + 1) * 4);
    PRK_TRY(S.d_out.ensure(3 * wb + (size_t)item_count * sizeof(prk::SelRun) + 16));
    size_t tb = 0;
    PRK_TRY(prk_scan_u32(nullptr, nullptr, item_count + 1, nullptr, &tb, nullptr));
    PRK_TRY(S.d_temp.ensure(std::max<size_t>(tb, 16)));
    uint8_t *tab = S.d_tab.as<uint8_t>(), *out = S.d_out.as<uint8_t>();
    const prk_select_item *d_items = reinterpret_cast<const prk_select_item *>(tab);
    const prk_select_level *d_levels = reinterpret_cast<const prk_select_level *>(tab + lev_off);
    const prk_xform *d_xf = reinterpret_cast<const prk_xform *>(tab + xf_off);
    const uint32_t *d_px = item_pixels ? reinterpret_cast<const uint32_t *>(tab + px_off) : nullptr;
    int32_t *d_chosen = reinterpret_cast<int32_t *>(out);
    uint32_t *d_n = reinterpret_cast<uint32_t *>(out + wb), *d_start = reinterpret_cast<uint32_t *>(out + 2 * wb);
    prk::SelRun *d_runs = reinterpret_cast<prk::SelRun *>(out + 3 * wb);
    // Stage 1 and 2 on the geometry stream, behind what is queued there (an
    // earlier emit pass still reads these buffers) but not behind the flushed
    // frames: neither stage touches dst.
    hipStream_t s = c->copy_stream;
    PRK_TRY(hipEventRecord(S.ev[0], s));
    PRK_TRY(hipMemcpyAsync(tab, items, ib, hipMemcpyHostToDevice, s));
    if (levels && lb) PRK_TRY(hipMemcpyAsync(tab + lev_off, levels, lb, hipMemcpyHostToDevice, s));
    if (xforms && xb) PRK_TRY(hipMemcpyAsync(tab + xf_off, xforms, xb, hipMemcpyHostToDevice, s));
    if (pb) PRK_TRY(hipMemcpyAsync(tab + px_off, item_pixels, pb, hipMemcpyHostToDevice, s));
    // (the bounds answer was complete when its call returned: no stream has to wait for it)
    PRK_TRY(prk_sel_choose(d_items, item_count, d_levels, frame ? c->vis.d_pix.as<uint32_t>() : nullptr, d_px,
                           bounds ? c->bnd.d_pixels.as<uint32_t>() : nullptr, d_chosen, d_n, d_runs, s));
    PRK_TRY(prk_scan_u32(d_n, d_start, item_count + 1, S.d_temp.p, &tb, s));
    uint32_t total = 0;
    PRK_TRY(hipMemcpyAsync(&total, d_start + item_count, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipEventRecord(S.ev[1], s));
    PRK_TRY(hipStreamSynchronize(s));  // the one wait: the tables are copied, the total is here
    if (total > worst) return PRK_ERR_DEVICE;  // (never: the choice is among the levels summed above)
    // dst takes every array src has; its size covers the last triangle written
    // (nothing chosen: nothing written, dst as it was)
    if (total) {
        Geometry &sg = c->geoms[src];
        const bool has[4] = {sg.V != nullptr, sg.C != nullptr, sg.N != nullptr, sg.UV != nullptr};
        const uint32_t endv = (uint32_t)(((uint64_t)dst_first_tri + total) * 3);
        const uint32_t end = std::max<uint32_t>(c->geoms[dst].vertex_count, endv);
        PRK_CHECK(geometry_grow(c, dst, has, end));
        Geometry &d = c->geoms[dst];
        // a side pass in the geometry form, as prk_geometry_transform's (s is copy_stream)
        PRK_TRY(side_begin(c, false));
        PRK_TRY(hipEventRecord(S.ev[2], s));
        PRK_TRY(prk_sel_emit(d_start, d_runs, item_count, total, dst_first_tri, d_xf, sg.V, sg.C, sg.N, sg.UV,
                             (float *)d.V, (float *)d.C, (float *)d.N, (float *)d.UV, s));
        PRK_TRY(hipEventRecord(S.ev[3], s));
        PRK_TRY(side_end(c));
        d.vertex_count = end;
    }
    S.timed = true;
    S.emitted = total != 0;
    if (chosen) PRK_TRY(hipMemcpy(chosen, d_chosen, (size_t)item_count * 4, hipMemcpyDeviceToHost));
    if (out_first) {
        PRK_TRY(hipMemcpy(out_first, d_start, ((size_t)item_count + 1) * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i <= item_count; ++i) out_first[i] += dst_first_tri;
    }
    *total_tris_out = total;
    return PRK_OK;
}

extern "C" {

int prk_geometry_select(prk_context *c, int32_t src, int32_t dst, uint32_t dst_first_tri, const prk_select_item *items,
                        uint32_t item_count, const prk_select_level *levels, uint32_t level_count,
                        const prk_xform *xforms, uint32_t xform_count, const uint32_t *item_pixels, int32_t *chosen,
                        uint32_t *out_first, uint64_t *total_tris_out) {
    return select_body(c, src, dst, dst_first_tri, items, item_count, levels, level_count, xforms, xform_count,
                       item_pixels, false, chosen, out_first, total_tris_out);
}

int prk_geometry_select_bounds(prk_context *c, int32_t src, int32_t dst, uint32_t dst_first_tri,
                               const prk_select_item *items, uint32_t item_count, const prk_select_level *levels,
                               uint32_t level_count, const prk_xform *xforms, uint32_t xform_count, int32_t *chosen,
                               uint32_t *out_first, uint64_t *total_tris_out) {
    return select_body(c, src, dst, dst_first_tri, items, item_count, levels, level_count, xforms, xform_count,
                       nullptr, true, chosen, out_first, total_tris_out);
}

int prk_debug_select_ms(prk_context *c, float *choose_ms, float *emit_ms) {
    if (!c || !choose_ms || !emit_ms || !c->sel.timed) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    SelState &S = c->sel;
    float a = 0.0f, b = 0.0f;
    PRK_TRY(hipEventSynchronize(S.ev[1]));
    PRK_TRY(hipEventElapsedTime(&a, S.ev[0], S.ev[1]));
    if (S.emitted) {
        PRK_TRY(hipEventSynchronize(S.ev[3]));
        PRK_TRY(hipEventElapsedTime(&b, S.ev[2], S.ev[3]));
    }
    *choose_ms = a;
    *emit_ms = b;
    return PRK_OK;
}

}  // extern "C"
