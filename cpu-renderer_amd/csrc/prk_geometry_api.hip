// prk_geometry_api.hip — the geometry handles of prk.h, one of
// the host files over prk_ctx.h.  prk_geometry_write and prk_geometry_transform
// (kernel: prk_xform.hip) are side passes in the geometry form (prk_ctx.h:
// side_begin); geometry_grow is also prk_geometry_select's (prk_select_api.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "prk_ctx.h"

extern "C" {

static int upload_array(const float *src, size_t n, const float **dst) {
    *dst = nullptr;
    if (!src) return PRK_OK;
    float *d = nullptr;
    PRK_TRY(hipMalloc((void **)&d, n * sizeof(float)));
    hipError_t e = hipMemcpy(d, src, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return status_of(e);
    }
    *dst = d;
    return PRK_OK;
}

// *dst moved into a new buffer of `bytes`: its first `old` bytes kept, zeros after them.
static int regrow(const float **dst, size_t old, size_t bytes) {
    float *d = nullptr;
    PRK_TRY(hipMalloc((void **)&d, bytes));
    hipError_t e = old ? hipMemcpy(d, *dst, old, hipMemcpyDeviceToDevice) : hipSuccess;
    if (e == hipSuccess) e = hipMemset((uint8_t *)d + old, 0, bytes - old);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return status_of(e);
    }
    (void)hipFree((void *)*dst);
    *dst = d;
    return PRK_OK;
}

int prk_geometry_create(prk_context *c, const float *v, const float *col, const float *n, const float *uv,
                        uint32_t vertex_count, int32_t *handle_out) {
    if (!c || !v || !handle_out || vertex_count % 3) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Geometry g;
    g.vertex_count = vertex_count;
    for (int k = 0; k < 4; ++k) g.cap[k] = vertex_count;
    g.owned = true;
    int rc = upload_array(v, (size_t)vertex_count * 3, &g.V);
    if (rc == PRK_OK) rc = upload_array(col, (size_t)vertex_count * 4, &g.C);
    if (rc == PRK_OK) rc = upload_array(n, (size_t)vertex_count * 3, &g.N);
    if (rc == PRK_OK) rc = upload_array(uv, (size_t)vertex_count * 2, &g.UV);
    if (rc != PRK_OK) {
        for (const float *p : {g.V, g.C, g.N, g.UV}) (void)hipFree((void *)p);
        return rc;
    }
    *handle_out = (int32_t)c->geoms.size();
    c->geoms.push_back(g);
    return PRK_OK;
}

// Replace a library-owned geometry's contents (the reference re-reads
// VertexData at every FillEdgeTable, projekt.cpp:3898-3925).  Buffers are kept
// when large enough; frames in flight finish first.  Draws recorded before
// the update read the new contents.
int prk_geometry_update(prk_context *c, int32_t handle, const float *v, const float *col, const float *n,
                        const float *uv, uint32_t vertex_count) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size() || !v || vertex_count % 3) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    Geometry &g = c->geoms[handle];
    if (!g.owned) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    const float *src[4] = {v, col, n, uv};
    const float **dst[4] = {&g.V, &g.C, &g.N, &g.UV};
    for (int k = 0; k < 4; ++k) {  // an array passed as null keeps its previous contents
        const size_t bytes = (size_t)vertex_count * kGeomComp[k] * sizeof(float);
        if (!src[k]) {
            // ... and grows with the vertex count: its first cap[k] vertices
            // kept, the new ones zero, so no draw reads past its allocation.
            if (*dst[k] && vertex_count > g.cap[k]) {
                PRK_CHECK(regrow(dst[k], (size_t)g.cap[k] * kGeomComp[k] * sizeof(float), bytes));
                g.cap[k] = vertex_count;
            }
            continue;
        }
        if (!*dst[k] || vertex_count > g.cap[k]) {
            float *d = nullptr;
            PRK_TRY(hipMalloc((void **)&d, bytes ? bytes : 4));
            (void)hipFree((void *)*dst[k]);
            *dst[k] = d;
            g.cap[k] = vertex_count;
        }
        PRK_TRY(hipMemcpy((void *)*dst[k], src[k], bytes, hipMemcpyHostToDevice));
    }
    g.vertex_count = vertex_count;
    // recorded draws carry the geometry's device pointers: refresh them
    for (auto &d : c->draws)
        if (d.src_kind == 0 && d.geom == handle) {
            d.V = g.V; d.C = g.C; d.N = g.N; d.UV = g.UV;
        }
    return PRK_OK;
}

// Copies into a library-owned geometry without waiting (prk.h): a side pass
// in the geometry form, ended only if something was copied.
int prk_geometry_write(prk_context *c, int32_t handle, uint32_t first_vertex, uint32_t vertex_count,
                       const float *v, const float *col, const float *n, const float *uv) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size() || first_vertex % 3 || vertex_count % 3)
        return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    const uint64_t end64 = (uint64_t)first_vertex + vertex_count;
    if (end64 > 0xFFFFFFF0ull) return PRK_ERR_ARG;
    const uint32_t end = (uint32_t)end64;
    Geometry &g = c->geoms[handle];
    if (!g.owned) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    const float *src[4] = {v, col, n, uv};
    const float **dst[4] = {&g.V, &g.C, &g.N, &g.UV};
    const bool given[4] = {v != nullptr, col != nullptr, n != nullptr, uv != nullptr};
    PRK_CHECK(geometry_grow(c, handle, given, end));
    PRK_TRY(side_begin(c, false));
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if (!src[k] || !vertex_count) continue;
        const size_t off = (size_t)first_vertex * kGeomComp[k];
        PRK_TRY(hipMemcpyAsync((void *)(*dst[k] + off), src[k], (size_t)vertex_count * kGeomComp[k] * sizeof(float),
                               hipMemcpyHostToDevice, c->copy_stream));
        any = true;
    }
    if (any) PRK_TRY(side_end(c));
    g.vertex_count = end;
    return PRK_OK;
}

// Room for `end` vertices in a library-owned geometry's arrays that exist or
// are wanted now (prk_geometry_write, prk_geometry_transform): buffers that
// must grow do so by half again at least, so a frame streamed in chunks
// reallocates rarely; contents kept, zeros past them (a new array: all zeros),
// recorded draws repointed.  Growing waits for the device.  (Hidden,
// prk_ctx.h: prk_geometry_select grows its destination the same way.)
int geometry_grow(prk_context *c, int32_t handle, const bool want[4], uint32_t end) {
    Geometry &g = c->geoms[handle];
    const float **dst[4] = {&g.V, &g.C, &g.N, &g.UV};
    bool grow = false;
    for (int k = 0; k < 4; ++k) grow |= (want[k] || *dst[k]) && end > g.cap[k];
    if (grow) {
        PRK_TRY(hipDeviceSynchronize());  // frames in flight and earlier writes read / fill the old buffers
        for (int k = 0; k < 4; ++k) {
            if (!(want[k] || *dst[k]) || end <= g.cap[k]) continue;
            const uint64_t need = std::max<uint64_t>(end, (uint64_t)g.cap[k] + g.cap[k] / 2);
            const uint32_t cap = (uint32_t)std::min<uint64_t>(need, 0xFFFFFFF0ull);
            const size_t bytes = (size_t)cap * kGeomComp[k] * sizeof(float);
            const size_t old = *dst[k] ? (size_t)g.cap[k] * kGeomComp[k] * sizeof(float) : 0;
            PRK_CHECK(regrow(dst[k], old, bytes));
            g.cap[k] = cap;
        }
        for (auto &d : c->draws)
            if (d.src_kind == 0 && d.geom == handle) {
                d.V = g.V; d.C = g.C; d.N = g.N; d.UV = g.UV;
            }
        c->read_rec = false;  // the device is idle
    }
    return PRK_OK;
}

int prk_geometry_wrap_device(prk_context *c, const float *v, const float *col, const float *n,
                             const float *uv, uint32_t vertex_count, int32_t *handle_out) {
    if (!c || !v || !handle_out || vertex_count % 3) return PRK_ERR_ARG;
    Geometry g;
    g.V = v; g.C = col; g.N = n; g.UV = uv;
    g.vertex_count = vertex_count;
    g.owned = false;
    *handle_out = (int32_t)c->geoms.size();
    c->geoms.push_back(g);
    return PRK_OK;
}

int prk_geometry_alloc(prk_context *c, int32_t *handle_out) {
    if (!c || !handle_out) return PRK_ERR_ARG;
    Geometry g;  // no vertices, no arrays: prk_geometry_transform / prk_geometry_write give it both
    g.owned = true;
    *handle_out = (int32_t)c->geoms.size();
    c->geoms.push_back(g);
    return PRK_OK;
}

// Runs of src's triangles through a matrix each into dst (prk.h; kernel and
// table layout: prk_xform.hip).  A side pass in the geometry form, the
// tables' copy and the kernel inside it.
int prk_geometry_transform(prk_context *c, int32_t src, int32_t dst, const prk_xform_run *runs, uint32_t run_count,
                           const prk_xform *xforms, uint32_t xform_count) {
    if (!c || src < 0 || (size_t)src >= c->geoms.size() || dst < 0 || (size_t)dst >= c->geoms.size() || src == dst)
        return PRK_ERR_ARG;
    if (!c->geoms[dst].owned) return PRK_ERR_ARG;
    if (run_count && (!runs || !xforms)) return PRK_ERR_ARG;
    const uint32_t src_tris = c->geoms[src].vertex_count / 3;
    uint64_t total = 0, top = 0;  // output triangles; one past the highest triangle written
    uint32_t nruns = 0;
    for (uint32_t i = 0; i < run_count; ++i) {
        const prk_xform_run &r = runs[i];
        if (!r.tri_count) continue;
        if (r.xform >= xform_count) return PRK_ERR_ARG;
        if ((uint64_t)r.src_first_tri + r.tri_count > src_tris) return PRK_ERR_ARG;
        const uint64_t dend = (uint64_t)r.dst_first_tri + r.tri_count;
        if (dend * 3 > 0xFFFFFFF0ull) return PRK_ERR_ARG;
        top = std::max(top, dend);
        total += r.tri_count;
        ++nruns;
    }
    if (!nruns) return PRK_OK;
    if (!c->geoms[src].V) return PRK_ERR_ARG;  // (a geometry written without positions)
    if (total > (1ull << 31)) return PRK_ERR_LIMIT;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    XformState &X = c->xf;
    // the tables: scan (nruns + 1 words), runs, matrices (prk_xform.hip)
    const size_t runs_off = ((size_t)(nruns + 1) * 4 + 15) & ~(size_t)15;
    const size_t xf_off = runs_off + (size_t)nruns * 16;
    const size_t bytes = xf_off + (size_t)xform_count * sizeof(prk_xform);
    if (X.busy) {  // the staging's previous contents have been copied
        PRK_TRY(hipEventSynchronize(X.copied_ev));
        X.busy = false;
    }
    if (bytes > X.h_cap) {
        if (X.h_tab) (void)hipHostFree(X.h_tab);
        X.h_tab = nullptr;
        X.h_cap = 0;
        const size_t want = bytes + bytes / 4;
        PRK_TRY(hipHostMalloc(&X.h_tab, want, hipHostMallocDefault));
        X.h_cap = want;
    }
    if (!X.copied_ev) PRK_TRY(hipEventCreate(&X.copied_ev));
    if (!X.end_ev) PRK_TRY(hipEventCreate(&X.end_ev));
    {
        uint8_t *h = static_cast<uint8_t *>(X.h_tab);
        uint32_t *scan = reinterpret_cast<uint32_t *>(h);
        uint32_t *rr = reinterpret_cast<uint32_t *>(h + runs_off);
        uint32_t at = 0, k = 0;
        for (uint32_t i = 0; i < run_count; ++i) {
            const prk_xform_run &r = runs[i];
            if (!r.tri_count) continue;
            scan[k] = at;
            rr[4 * k + 0] = r.src_first_tri;
            rr[4 * k + 1] = r.dst_first_tri;
            rr[4 * k + 2] = r.xform;
            rr[4 * k + 3] = at;
            at += r.tri_count;
            ++k;
        }
        scan[nruns] = at;
        std::memcpy(h + xf_off, xforms, (size_t)xform_count * sizeof(prk_xform));
    }
    // dst takes every array src has; its size covers the highest triangle written
    Geometry &s = c->geoms[src];
    const bool has[4] = {s.V != nullptr, s.C != nullptr, s.N != nullptr, s.UV != nullptr};
    const uint32_t end = std::max<uint32_t>(c->geoms[dst].vertex_count, (uint32_t)(top * 3));
    PRK_CHECK(geometry_grow(c, dst, has, end));
    Geometry &d = c->geoms[dst];
    PRK_TRY(X.d_tab.ensure(bytes));  // (a larger buffer: hipFree waits for the kernels that read the old one)
    PRK_TRY(side_begin(c, false));
    PRK_TRY(hipMemcpyAsync(X.d_tab.p, X.h_tab, bytes, hipMemcpyHostToDevice, c->copy_stream));
    PRK_TRY(hipEventRecord(X.copied_ev, c->copy_stream));
    X.busy = true;
    PRK_TRY(prk_xform_launch(X.d_tab.p, runs_off, xf_off, nruns, (uint32_t)total, s.V, s.C, s.N, s.UV,
                             (float *)d.V, (float *)d.C, (float *)d.N, (float *)d.UV, c->copy_stream));
    PRK_TRY(hipEventRecord(X.end_ev, c->copy_stream));
    PRK_TRY(side_end(c));
    d.vertex_count = end;
    return PRK_OK;
}

int prk_geometry_info(prk_context *c, int32_t handle, uint32_t *vertex_count_out, uint32_t *arrays_out) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size()) return PRK_ERR_ARG;
    const Geometry &g = c->geoms[handle];
    if (vertex_count_out) *vertex_count_out = g.vertex_count;
    if (arrays_out) *arrays_out = (g.V ? 1u : 0u) | (g.C ? 2u : 0u) | (g.N ? 4u : 0u) | (g.UV ? 8u : 0u);
    return PRK_OK;
}

int prk_debug_transform_ms(prk_context *c, float *kernel_ms) {
    if (!c || !kernel_ms || !c->xf.busy) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipEventSynchronize(c->xf.end_ev));
    PRK_TRY(hipEventElapsedTime(kernel_ms, c->xf.copied_ev, c->xf.end_ev));
    return PRK_OK;
}

int prk_debug_geometry_stream(prk_context *c, void **stream) {
    if (!c || !stream) return PRK_ERR_ARG;
    *stream = (void *)c->copy_stream;
    return PRK_OK;
}

int prk_geometry_download(prk_context *c, int32_t handle, uint32_t first_vertex, uint32_t vertex_count,
                          float *v, float *col, float *n, float *uv) {
    if (!c || handle < 0 || (size_t)handle >= c->geoms.size() || first_vertex % 3 || vertex_count % 3)
        return PRK_ERR_ARG;
    const Geometry &g = c->geoms[handle];
    if ((uint64_t)first_vertex + vertex_count > g.vertex_count) return PRK_ERR_ARG;
    float *dst[4] = {v, col, n, uv};
    const float *src[4] = {g.V, g.C, g.N, g.UV};
    for (int k = 0; k < 4; ++k)
        if (dst[k] && !src[k]) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->copy_stream));  // every queued write of a geometry runs there
    for (int k = 0; k < 4; ++k) {
        if (!dst[k] || !vertex_count) continue;
        PRK_TRY(hipMemcpy(dst[k], src[k] + (size_t)first_vertex * kGeomComp[k],
                          (size_t)vertex_count * kGeomComp[k] * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PRK_OK;
}

}  // extern "C"
