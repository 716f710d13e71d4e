// prk_api.hip — host side of libprk_hip.so: the C-ABI declared in include/prk.h,
// one of the host files over prk_ctx.h (the context).  This one owns the
// context itself -- the runtime check, prk_create and prk_destroy, the cameras,
// the setters, pinned host memory, the timing and debug getters -- and records
// the reference's draw calls:
//   FillEdgeTable + DrawModelOptimized / DrawModel (projekt.cpp:3882, 3615, 162)
//   -> prk_draw records {geometry range, P, semantics, Phong, Bitmap}
// The frame those draws make is queued by prk_flush (prk_flush.hip: the
// per-triangle pass; prk_span_pass.hip: the whole-object pass).  The resources
// the draws name are prk_target_api.hip (target, textures, layers) and
// prk_geometry_api.hip; the record and span handles and the record walks are
// prk_record_api.hip, the self-tests prk_selftest.hip.
// There is no CPU fallback: every entry point that computes pixels needs the
// HIP device and fails with PRK_ERR_DEVICE without one.
#include <hip/hip_runtime.h>
#include <link.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "prk_ctx.h"

using prk::packed_span_bytes;

// ---- one ROCm runtime per process (prk.h prk_create) ------
namespace {
struct MapScan {
    std::vector<std::string> hip, smi;  // distinct mapped files of each library
};
int scan_object(struct dl_phdr_info *info, size_t, void *data) {
    MapScan &m = *static_cast<MapScan *>(data);
    const char *path = info->dlpi_name;
    if (!path || !*path) return 0;
    const char *base = std::strrchr(path, '/');
    base = base ? base + 1 : path;
    std::vector<std::string> *v = nullptr;
    if (std::strncmp(base, "libamdhip64", 11) == 0) v = &m.hip;
    else if (std::strncmp(base, "librocm_smi64", 13) == 0) v = &m.smi;
    if (!v) return 0;
    char real[4096];
    const std::string key = realpath(path, real) ? std::string(real) : std::string(path);
    if (std::find(v->begin(), v->end(), key) == v->end()) v->push_back(key);
    return 0;
}
// Runs before the destructors of every library loaded earlier (exit handlers
// run last-registered first): ends the process with its own exit status
// before the duplicated librocm_smi64 destructors free one map twice.
void exit_guard(int status, void *) {
    std::fflush(nullptr);
    _exit(status);
}
std::atomic<bool> g_guarded{false};
}  // namespace

extern "C" {

int prk_runtime_check(void) {
    MapScan m;
    dl_iterate_phdr(scan_object, &m);
    if (m.hip.size() <= 1 && m.smi.size() <= 1) return PRK_OK;
    if (!g_guarded.exchange(true)) {
        std::fprintf(stderr,
                     "prk: %zu copies of libamdhip64 and %zu of librocm_smi64 are mapped in this process (e.g. "
                     "/opt/rocm's, loaded with libprk_hip.so, and torch's own): load torch (or the framework that "
                     "ships its own ROCm) BEFORE libprk_hip.so (INTEGRATION.md, 'One ROCm stack per process'); "
                     "the process will end at exit before their destructors run\n",
                     m.hip.size(), m.smi.size());
        // The guard ends the process before every exit handler registered
        // earlier (profiler flushes, LSan, earlier libraries' static
        // destructors): without it the duplicated librocm_smi64 destructors
        // abort the process there anyway (SIGABRT, the same handlers lost).
        // PRK_EXIT_GUARD=0 leaves the exit path alone (the host takes the abort).
        const char *g = std::getenv("PRK_EXIT_GUARD");
        if (!(g && g[0] == '0')) on_exit(exit_guard, nullptr);
    }
    return PRK_ERR_RUNTIME_MIX;
}

const char *prk_version(void) { return "prk 0.1 (gfx950)"; }

int prk_device_count(int *out) {
    if (!out) return PRK_ERR_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *out = n;
    return PRK_OK;
}

int prk_create(int device, prk_context **out) {
    if (!out) return PRK_ERR_ARG;
    *out = nullptr;
    PRK_CHECK(prk_runtime_check());
    PRK_CHECK(use_device(device));
    prk_context *c = new (std::nothrow) prk_context();
    if (!c) return PRK_ERR_NOMEM;
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->bin_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->vis_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->s_mark, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->in_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->read_ev, hipEventDisableTiming);
    for (int i = 0; i < prk_context::kSets && e == hipSuccess; ++i) {
        e = hipEventCreateWithFlags(&c->bset[i].free_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bset[i].binned_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bset[i].counted_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bset[i].listed_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipHostMalloc((void **)&c->bset[i].h_info, 2 * sizeof(uint32_t), hipHostMallocDefault);
    }
    for (int i = 0; i < prk_context::kRing && e == hipSuccess; ++i)
        for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipEventCreate(&c->ev[i][k]);
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_total, sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) {
        prk_destroy(c);
        return status_of(e);
    }
    *out = c;
    return PRK_OK;
}

int prk_destroy(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    (void)prk_runtime_check();  // (a runtime loaded since prk_create: guard the exit)
    // Destroy never queues GPU work: a frame whose bin count was never read
    // (PendingCount) is dropped, not re-run — its target may already belong
    // to someone else (a torch tensor freed at interpreter exit, a peer
    // context), and a re-run there is exactly what a caller tearing down does
    // not expect.  Only waits and frees follow.
    c->pcount.active = false;
    c->pcount.draws.clear();
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    (void)hipDeviceSynchronize();
    for (auto &g : c->geoms)
        if (g.owned)
            for (const float *p : {g.V, g.C, g.N, g.UV}) (void)hipFree((void *)p);
    for (auto &t : c->texs) (void)hipFree(t.mem);
    for (auto &r : c->recs) {
        (void)hipFree(r.rec);
        (void)hipFree(r.tab);
    }
    for (auto &b : c->sbatches) (void)hipFree(b.sp);
    for (auto &l : c->layers)
        if (l.live && !l.wrapped) {
            (void)hipFree(l.color);
            (void)hipFree(l.z);
        }
    if (c->owns_target) {
        (void)hipFree(c->color);
        (void)hipFree(c->zbuf);
    }
    for (auto &B : c->bset) {
        DevBuf *bb[] = {&B.d_draws, &B.d_texs, &B.d_tri_draw, &B.d_ranges, &B.d_tri_n, &B.d_tri_off, &B.d_pair_tri,
                        &B.d_bins, &B.d_offs, &B.d_won, &B.d_list, &B.d_nwin, &B.d_wtag, &B.d_recs, &B.d_trwon,
                        &B.d_wlist, &B.d_seltemp, &B.d_trec, &B.d_ghist, &B.d_tile_tot, &B.d_chunk, &B.d_info,
                        &B.d_runlist, &B.d_run_n};
        for (DevBuf *b : bb) b->release();
        for (hipEvent_t e : {B.free_ev, B.binned_ev, B.counted_ev, B.listed_ev})
            if (e) (void)hipEventDestroy(e);
        if (B.h_info) (void)hipHostFree(B.h_info);
    }
    DevBuf *bufs[] = {&c->d_winners, &c->d_anomaly, &c->d_prof, &c->d_negz, &c->xf.d_tab,
                      &c->vis.d_counts, &c->vis.d_flags, &c->vis.d_pix, &c->vis.d_vis, &c->vis.d_ids,
                      &c->vis.d_temp, &c->vis.d_starts, &c->vis.d_gout, &c->sel.d_tab, &c->sel.d_out,
                      &c->sel.d_temp, &c->bnd.d_zmin, &c->bnd.d_tab, &c->bnd.d_pixels};
    for (DevBuf *b : bufs) b->release();
    for (hipEvent_t e : c->bnd.ev)
        if (e) (void)hipEventDestroy(e);
    if (c->xf.h_tab) (void)hipHostFree(c->xf.h_tab);
    if (c->xf.copied_ev) (void)hipEventDestroy(c->xf.copied_ev);
    if (c->xf.end_ev) (void)hipEventDestroy(c->xf.end_ev);
    for (hipEvent_t e : c->sel.ev)
        if (e) (void)hipEventDestroy(e);
    {
        auto &S = c->spans;
        DevBuf *sb[] = {&S.d_stage, &S.d_edges, &S.d_ord, &S.d_temp, &S.d_recs, &S.d_pos, &S.d_span_tri, &S.d_scnt,
                        &S.d_soff, &S.d_vals_b, &S.d_offs, &S.d_nwin,
                        &S.d_wtag, &S.d_srecs, &S.d_work, &S.d_ekeys, &S.d_ekeys2, &S.d_evals, &S.d_ecnt,
                        &S.d_escan, &S.d_rcnt, &S.d_rscan, &S.d_bound, &S.d_oslot, &S.d_pool, &S.d_err,
                        &S.d_raw, &S.d_most, &S.d_cls, &S.d_prrow, &S.d_prcnt, &S.d_preoff, &S.d_prfge,
                        &S.d_prccur, &S.d_prkey, &S.d_prest, &S.d_prsst, &S.d_preend, &S.d_preendm,
                        &S.d_prmatch, &S.d_prsidx, &S.d_prsm, &S.d_prstat, &S.d_segcnt, &S.d_segoff,
                        &S.d_segs, &S.d_wy, &S.d_mhuge, &S.d_objtab, &S.d_k0tab, &S.d_lscan, &S.d_lobj, &S.d_lrows,
                        &S.d_ltab, &S.d_rectab, &S.d_reccnt,
                        &S.d_recout, &S.d_spanout, &S.d_rowslot, &S.d_rowcnt, &S.d_rowscan, &S.d_rowout,
                        &S.d_lstat, &S.d_dr_rows, &S.d_dr_pairs, &S.d_dr_cnt, &S.d_dr_scan, &S.d_dr_temp, &S.d_dr_out};
        for (DevBuf *b : sb) b->release();
        if (S.h_rb) (void)hipHostFree(S.h_rb);
        if (S.stage_ev) {
            if (S.stage_busy) (void)hipEventSynchronize(S.stage_ev);
            (void)hipEventDestroy(S.stage_ev);
        }
        if (S.h_stage) (void)hipHostFree(S.h_stage);
        if (S.h_cls) (void)hipHostFree(S.h_cls);
    }
    for (hipEvent_t e : {c->s_mark, c->in_ev, c->read_ev})
        if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->h_total) (void)hipHostFree(c->h_total);
    for (auto &slot : c->ev)
        for (auto &e : slot)
            if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {c->own_stream, c->bin_stream, c->vis_stream})
        if (s) (void)hipStreamDestroy(s);
    delete c;
    return PRK_OK;
}

int prk_set_camera(prk_context *c, const prk_transform *t, const prk_light_data *l) {
    if (!c || !t || !l || l->LightCount > PRK_MAX_LIGHTS) return PRK_ERR_ARG;
    c->transform = *t;
    c->lights = *l;
    c->shade_transform = *t;
    c->shade_lights = *l;
    c->have_camera = true;
    return PRK_OK;
}

int prk_set_shade_camera(prk_context *c, const prk_transform *t, const prk_light_data *l) {
    if (!c || !t || !l || l->LightCount > PRK_MAX_LIGHTS) return PRK_ERR_ARG;
    if (!c->have_camera) return PRK_ERR_ARG;  // the setup camera first (prk_set_camera)
    c->shade_transform = *t;
    c->shade_lights = *l;
    return PRK_OK;
}

// Allocations of 2 MB and more: heap memory on transparent huge pages,
// page-locked with hipHostRegister, instead of hipHostMalloc's 4-KB pinned
// pages -- the drop-in's staging arena takes ~150 MB of per-call vertex
// snapshots a frame, which the 2-MB pages make cheaper for the CPU (TLB).
// PRK_HOST_ALLOC_THP=0: hipHostMalloc for every size.
static std::mutex g_thp_mu;
static std::map<void *, size_t> g_thp;  // (any context may free)
static bool host_alloc_thp() {
    static const bool on = [] {
        const char *e = std::getenv("PRK_HOST_ALLOC_THP");
        return !(e && e[0] == '0');
    }();
    return on;
}

int prk_host_alloc(prk_context *c, size_t bytes, void **out) {
    if (!c || !out) return PRK_ERR_ARG;
    *out = nullptr;
    PRK_TRY(hipSetDevice(c->device));
    constexpr size_t kHuge = (size_t)2 << 20;
    if (bytes >= kHuge && host_alloc_thp()) {
        const size_t sz = (bytes + kHuge - 1) & ~(kHuge - 1);
        void *p = std::aligned_alloc(kHuge, sz);
        if (!p) return PRK_ERR_NOMEM;
        (void)madvise(p, sz, MADV_HUGEPAGE);  // (best effort)
        memset(p, 0, sz);                      // (faulted in on huge pages before the pinning)
        const hipError_t e = hipHostRegister(p, sz, hipHostRegisterPortable);
        if (e != hipSuccess) {
            std::free(p);
            return status_of(e);
        }
        std::lock_guard<std::mutex> g(g_thp_mu);
        g_thp[p] = sz;
        *out = p;
        return PRK_OK;
    }
    PRK_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return PRK_OK;
}

int prk_host_free(prk_context *c, void *p) {
    if (!c) return PRK_ERR_ARG;
    if (!p) return PRK_OK;
    {
        std::lock_guard<std::mutex> g(g_thp_mu);
        auto it = g_thp.find(p);
        if (it != g_thp.end()) {
            g_thp.erase(it);
            const hipError_t e = hipHostUnregister(p);
            std::free(p);
            return e == hipSuccess ? PRK_OK : status_of(e);
        }
    }
    PRK_TRY(hipHostFree(p));
    return PRK_OK;
}

int prk_host_register(prk_context *c, void *p, size_t bytes) {
    if (!c || !p || !bytes) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return PRK_OK;
}

int prk_host_unregister(prk_context *c, void *p) {
    if (!c || !p) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipHostUnregister(p));
    return PRK_OK;
}

int prk_draw(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count, const float P[3],
             int32_t semantics, int32_t phong, int32_t texture) {
    return prk_draw_objects(c, geometry, first_tri, tri_count, 1, P, semantics, phong, texture);
}

int prk_draw_objects(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                     uint32_t tris_per_object, const float P[3], int32_t semantics, int32_t phong, int32_t texture) {
    return prk_draw_objects_setup(c, geometry, first_tri, tri_count, tris_per_object, P, semantics, phong, texture,
                                  -1);
}

int prk_draw_objects_setup(prk_context *c, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                           uint32_t tris_per_object, const float P[3], int32_t semantics, int32_t phong,
                           int32_t texture, int32_t setup) {
    if (!c || geometry < 0 || geometry >= (int32_t)c->geoms.size() || tris_per_object == 0) return PRK_ERR_ARG;
    const Geometry &g = c->geoms[geometry];
    if ((uint64_t)first_tri + tri_count > g.vertex_count / 3) return PRK_ERR_ARG;
    if (texture >= (int32_t)c->texs.size()) return PRK_ERR_ARG;
    if (setup > (PRK_SETUP_PHONG | PRK_SETUP_BITMAP)) return PRK_ERR_ARG;
    const bool tex = texture >= 0;
    // FillEdgeTable's PhongShading and Object->Bitmap (prk.h prk_setup)
    const bool fe_phong = setup < 0 ? phong != 0 : (setup & PRK_SETUP_PHONG) != 0;
    const bool fe_bitmap = setup < 0 ? tex : (setup & PRK_SETUP_BITMAP) != 0;
    int mode;
    uint32_t flags = 0;
    if (semantics == PRK_SEM_AVX || semantics == PRK_SEM_AVX_ST) {
        // FillLineOptimized dereferences Bitmap at entry (projekt.cpp:1506) and
        // its non-Phong branch stores garbage (2285-2316): undefined -> rejected.
        // The single-thread overload (2350-3358) shares both (2494, 3262-3290).
        if (!tex || !phong) return PRK_ERR_UNSUPPORTED;
        mode = prk::MODE_AVX;
        if (semantics == PRK_SEM_AVX_ST) flags = prk::DRAW_ST;
    } else if (semantics == PRK_SEM_SCALAR) {
        mode = phong ? (tex ? prk::MODE_SC_PHONG_TEX : prk::MODE_SC_PHONG)
                     : (tex ? prk::MODE_SC_GOURAUD_TEX : prk::MODE_SC_GOURAUD);
    } else {
        return PRK_ERR_ARG;
    }
    // Edge fields FillEdgeTable never wrote: MinNormal without PhongShading
    // (4012-4064), the U/V/(1/z) gradients without Object->Bitmap (4078-4089).
    if ((phong && !fe_phong) || (tex && !fe_bitmap)) return PRK_ERR_UNSUPPORTED;
    if (mode == prk::MODE_SC_GOURAUD) {
        if (fe_phong) flags |= prk::DRAW_RAWCOL;        // raw colours, unlit (4014-4015)
        else if (fe_bitmap) flags |= prk::DRAW_WHITELIT;  // lighting from white (4034-4054)
    }
    if ((phong || !tex) && !g.N) return PRK_ERR_ARG;  // (the Gouraud setup kernels load them in every case)
    if (tex && !g.UV) return PRK_ERR_ARG;
    if ((mode == prk::MODE_SC_GOURAUD || mode == prk::MODE_SC_PHONG) && !g.C) return PRK_ERR_ARG;
    if (tri_count == 0) return PRK_OK;
    if ((uint64_t)c->pending_tris + tri_count >= 0xFFFFFFF0ull) return PRK_ERR_ARG;
    // A draw that continues the previous one (same geometry, the next
    // triangles, same object offset, semantics, texture and object size, the
    // previous one ending on an object boundary) extends it: per-object AETs
    // in submission order are unchanged, and a caller submitting one object
    // per call (the reference's render_entry_3d_object pattern) yields a few
    // draws per frame instead of one per triangle.
    if (!c->draws.empty()) {
        prk::DrawRec &b = c->draws.back();
        const float p0 = P ? P[0] : 0.0f, p1 = P ? P[1] : 0.0f, p2 = P ? P[2] : 0.0f;
        if (b.src_kind == 0 && b.geom == geometry && b.geom_tri0 + b.tri_count == first_tri && b.mode == mode &&
            b.flags == flags && b.tex == texture && b.obj_tris == tris_per_object &&
            b.tri_count % tris_per_object == 0 && b.P[0] == p0 && b.P[1] == p1 && b.P[2] == p2 &&
            std::signbit(b.P[0]) == std::signbit(p0) && std::signbit(b.P[1]) == std::signbit(p1) &&
            std::signbit(b.P[2]) == std::signbit(p2)) {
            b.tri_count += tri_count;
            c->pending_tris += tri_count;
            return PRK_OK;
        }
    }
    prk::DrawRec d{};
    d.V = g.V;
    d.C = g.C;
    d.N = g.N;
    d.UV = g.UV;
    d.geom = geometry;
    d.geom_tri0 = first_tri;
    d.first_global = c->pending_tris;
    d.tri_count = tri_count;
    d.mode = mode;
    d.tex = texture;
    d.P[0] = P ? P[0] : 0.0f;
    d.P[1] = P ? P[1] : 0.0f;
    d.P[2] = P ? P[2] : 0.0f;
    d.flags = flags;
    d.obj_tris = tris_per_object;
    c->draws.push_back(d);
    c->pending_tris += tri_count;
    return PRK_OK;
}

// A draw of caller edges or spans (span path): semantics / texture checks as
// prk_draw; it takes `ids` triangle ids of the frame's numbering.
int draw_src(prk_context *c, uint32_t kind, uint32_t off, uint32_t n, uint32_t ids, int32_t semantics,
                    int32_t phong, int32_t texture) {
    if (texture >= (int32_t)c->texs.size()) return PRK_ERR_ARG;
    int mode = prk::MODE_AVX;
    if (semantics == PRK_SEM_SCALAR) {
        // DrawModel on a caller's edge list (projekt.cpp:162-601); work
        // records (kind 2; kind 5: those of a span handle) are FillLineOptimized spans only
        if (kind == 2 || kind == 5) return PRK_ERR_UNSUPPORTED;
        const bool tex = texture >= 0;
        mode = phong ? (tex ? prk::MODE_SC_PHONG_TEX : prk::MODE_SC_PHONG)
                     : (tex ? prk::MODE_SC_GOURAUD_TEX : prk::MODE_SC_GOURAUD);
    } else if (semantics != PRK_SEM_AVX && semantics != PRK_SEM_AVX_ST) {
        return PRK_ERR_ARG;
    } else if (texture < 0 || !phong) {
        return PRK_ERR_UNSUPPORTED;  // projekt.cpp:1506, 2285-2316
    }
    if ((uint64_t)c->pending_tris + ids >= 0xFFFFFFF0ull) return PRK_ERR_ARG;
    prk::DrawRec d{};
    d.first_global = c->pending_tris;
    d.tri_count = ids;
    d.mode = mode;
    d.tex = texture;
    d.flags = semantics == PRK_SEM_AVX_ST ? prk::DRAW_ST : 0u;
    d.obj_tris = 1;
    d.src_kind = kind;
    d.src_off = off;
    d.src_n = n;
    c->draws.push_back(d);
    c->pending_tris += ids;
    return PRK_OK;
}

int prk_draw_edges(prk_context *c, const prk_edge *edges, uint32_t edge_count, int32_t semantics, int32_t phong,
                   int32_t texture) {
    if (!c || (!edges && edge_count)) return PRK_ERR_ARG;
    if (edge_count == 0) return PRK_OK;  // 0 edges: nothing to draw (P1)
    const uint32_t off = (uint32_t)c->pend_edges.size();
    const int rc = draw_src(c, 1, off, edge_count, 1, semantics, phong, texture);
    if (rc == PRK_OK) c->pend_edges.insert(c->pend_edges.end(), edges, edges + edge_count);
    return rc;
}

// Whether a list of a batch takes the walks of a triangle object: sorted by
// YMin (the sorted insertion cursor then inserts exactly what the reference's
// whole-list scan inserts, in the same order), and every edge inside the
// value range FillEdgeTable writes (0 <= YMin <= YMax, Left 0 or 1), which
// those walks' list mirrors are sized for.  Any other list is walked as
// prk_draw_edges walks it.
bool list_walks_sorted(const prk_edge *e, uint32_t n) {
    int32_t prev = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (e[i].YMin < prev || e[i].YMax < e[i].YMin || (uint32_t)e[i].Left > 1u) return false;
        prev = e[i].YMin;
    }
    return true;
}

int prk_draw_edge_lists(prk_context *c, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                        int32_t semantics, int32_t phong, int32_t texture) {
    if (!c || (!counts && list_count)) return PRK_ERR_ARG;
    uint64_t total = 0;
    for (uint32_t o = 0; o < list_count; ++o) total += counts[o];
    if (!records && total) return PRK_ERR_ARG;
    if (list_count == 0) return PRK_OK;
    // the frame's batch records and lists are indexed by 31 bits (as a pass's edge slots, flush_spans)
    if (c->pend_ledges.size() + total >= 0x7FFFFFFFull || c->pend_lcnt.size() + (uint64_t)list_count >= 0x7FFFFFFFull)
        return PRK_ERR_LIMIT;
    const uint32_t off = (uint32_t)c->pend_ledges.size(), l0 = (uint32_t)c->pend_lcnt.size();
    PRK_CHECK(draw_src(c, 3, off, (uint32_t)total, list_count, semantics, phong, texture));
    c->draws.back().geom_tri0 = l0;
    c->pend_ledges.insert(c->pend_ledges.end(), records, records + total);
    c->pend_lcnt.insert(c->pend_lcnt.end(), counts, counts + list_count);
    const prk_edge *e = records;
    for (uint32_t o = 0; o < list_count; e += counts[o], ++o)
        c->pend_lflag.push_back(list_walks_sorted(e, counts[o]) ? 1u : 0u);
    return PRK_OK;
}

int prk_draw_spans(prk_context *c, const prk_span *spans, uint32_t count, int32_t semantics, int32_t phong,
                   int32_t texture) {
    if (!c || (!spans && count)) return PRK_ERR_ARG;
    if (count == 0) return PRK_OK;
    const uint32_t off = (uint32_t)c->pend_spans.size();
    const int rc = draw_src(c, 2, off, count, count, semantics, phong, texture);
    if (rc == PRK_OK) c->pend_spans.insert(c->pend_spans.end(), spans, spans + count);
    return rc;
}

// Row work records (prk_row_records' output, or a caller's own) as a draw of
// their pairs: the rows and pairs go up as they are, k_rows_unpack
// (prk_records.hip) turns every pair into the prk_span of its row on the device
// -- no host loop over the pairs, only the one over the rows that checks the
// arguments -- and the spans come back into the pending frame's span input,
// where the draw is prk_draw_spans' from then on.  The buffers are this
// call's own: frames in flight keep the span scratch.  keep
// (prk_spans_upload_rows; `out` is then NULL): the spans are written into
// that device buffer (25 * npair dwords rounded up to four) and stay there.
int rows_to_spans(prk_context *c, const prk_row *rows, uint32_t nrow, const prk_row_pair *pairs,
                         uint32_t npair, prk_span *out, void *keep) {
    PRK_TRY(hipSetDevice(c->device));
    hipStream_t s = c->own_stream;
    prk_context::SpanScratch &S = c->spans;
    const size_t out_bytes = packed_span_bytes(npair);
    static_assert(sizeof(prk_row) == sizeof(prk::RowRec), "the kernels read a prk_row as {row, pairs}");
    PRK_TRY(S.d_dr_rows.ensure((size_t)nrow * sizeof(prk_row)));
    PRK_TRY(S.d_dr_pairs.ensure((size_t)npair * sizeof(prk_row_pair)));
    PRK_TRY(S.d_dr_cnt.ensure(((size_t)nrow + 1) * 4));
    PRK_TRY(S.d_dr_scan.ensure(((size_t)nrow + 1) * 4));
    if (!keep) PRK_TRY(S.d_dr_out.ensure(out_bytes));
    PRK_TRY(hipMemcpyAsync(S.d_dr_rows.p, rows, (size_t)nrow * sizeof(prk_row), hipMemcpyHostToDevice, s));
    PRK_TRY(hipMemcpyAsync(S.d_dr_pairs.p, pairs, (size_t)npair * sizeof(prk_row_pair), hipMemcpyHostToDevice, s));
    PRK_TRY(prk_rows_counts(S.d_dr_rows.as<prk::RowRec>(), nrow, (uint32_t *)S.d_dr_cnt.p, s));
    PRK_TRY(scan_u32(S.d_dr_temp, (const uint32_t *)S.d_dr_cnt.p, (uint32_t *)S.d_dr_scan.p, nrow + 1, s));
    PRK_TRY(prk_rows_unpack(S.d_dr_rows.as<prk::RowRec>(), (const uint32_t *)S.d_dr_scan.p, nrow, S.d_dr_pairs.p, npair,
                            keep ? keep : S.d_dr_out.p, s));
    if (!keep) PRK_TRY(hipMemcpyAsync(out, S.d_dr_out.p, (size_t)npair * sizeof(prk_span), hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));  // (the caller's arrays are copied at the call)
    return PRK_OK;
}

int prk_draw_rows(prk_context *c, const prk_row *rows, uint64_t row_count, const prk_row_pair *pairs,
                  uint64_t pair_count, int32_t semantics, int32_t phong, int32_t texture) {
    if (!c || (!rows && row_count) || (!pairs && pair_count)) return PRK_ERR_ARG;
    uint64_t sum = 0;
    for (uint64_t r = 0; r < row_count; ++r) {
        if (rows[r].RowIndex < 0) return PRK_ERR_ARG;
        sum += rows[r].EdgeCount;
    }
    if (sum != pair_count) return PRK_ERR_ARG;
    if (row_count == 0 || pair_count == 0) return PRK_OK;
    // the frame's span input is indexed by 31 bits, as the other caller records
    if (row_count >= 0x7FFFFFFFull || c->pend_spans.size() + pair_count >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    const uint32_t off = (uint32_t)c->pend_spans.size(), n = (uint32_t)pair_count;
    int rc = draw_src(c, 2, off, n, n, semantics, phong, texture);
    if (rc != PRK_OK) return rc;
    c->pend_spans.resize((size_t)off + n);
    rc = rows_to_spans(c, rows, (uint32_t)row_count, pairs, n, c->pend_spans.data() + off);
    if (rc != PRK_OK) {  // nothing is recorded
        c->pend_spans.resize(off);
        c->draws.pop_back();
        c->pending_tris -= n;
    }
    return rc;
}

int prk_reset_draws(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    c->draws.clear();
    c->pending_tris = 0;
    c->pend_edges.clear();
    c->pend_spans.clear();
    c->pend_ledges.clear();
    c->pend_lcnt.clear();
    c->pend_lflag.clear();
    return PRK_OK;
}

int prk_set_tile(prk_context *c, int32_t tw, int32_t th) {
    // tile_w: a power of two >= 8 (pixel index <-> (x, y) by shifts)
    if (!c || tw < 8 || th <= 0 || (tw & (tw - 1)) || tw * th > 8192 || tw * th < 64) return PRK_ERR_ARG;
    c->tile_w = tw;
    c->tile_h = th;
    c->tile_auto = false;
    return PRK_OK;
}

int prk_set_early_z(prk_context *c, int on) {
    if (!c) return PRK_ERR_ARG;
    c->early_z = on != 0;
    return PRK_OK;
}

int prk_set_debug(prk_context *c, int32_t enable) {
    if (!c) return PRK_ERR_ARG;
    c->debug = enable != 0;
    return PRK_OK;
}

// Accumulate the kernel times of a timed flush slot (waits for its last event).
void harvest(prk_context *c, int slot) {
    if (!c->pending[slot]) return;
    c->pending[slot] = false;
    if (hipEventSynchronize(c->ev[slot][2]) != hipSuccess) return;
    float a = 0, b = 0, v = 0, sp = 0;
    if (hipEventElapsedTime(&a, c->ev[slot][0], c->ev[slot][1]) != hipSuccess) a = 0;
    if (hipEventElapsedTime(&b, c->ev[slot][5], c->ev[slot][2]) != hipSuccess) b = 0;
    if (hipEventElapsedTime(&v, c->ev[slot][5], c->ev[slot][3]) != hipSuccess) v = 0;
    if (!c->split_span[slot] || hipEventElapsedTime(&sp, c->ev[slot][3], c->ev[slot][4]) != hipSuccess) sp = 0;
    c->stats.sum_ms_bin += a;
    c->stats.sum_ms_raster += b;
    c->stats.sum_ms_vis += v;
    c->stats.sum_ms_span += sp;
    c->stats.frames_timed += 1;
    if (slot == c->last_slot) {
        c->stats.ms_bin = a;
        c->stats.ms_raster = b;
    }
}

int prk_timing_reset(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    for (int i = 0; i < prk_context::kRing; ++i) c->pending[i] = false;
    c->stats.frames_timed = 0;
    c->stats.sum_ms_bin = c->stats.sum_ms_raster = c->stats.sum_ms_vis = c->stats.sum_ms_span = 0.0;
    if (c->d_prof.p) PRK_TRY(hipMemset(c->d_prof.p, 0, 16 * sizeof(uint64_t)));
    return PRK_OK;
}

int prk_debug_counters(prk_context *c, uint64_t *out, int32_t n) {
    if (!c || !out || n < 0 || n > 16) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    for (int i = 0; i < n; ++i) out[i] = 0;
    if (c->d_prof.p && n) PRK_TRY(hipMemcpy(out, c->d_prof.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_get_target(prk_context *c, void **color, int32_t *pitch_bytes, float **zbuf, int32_t *width,
                   int32_t *height, int32_t *row0, int32_t *row1) {
    if (!c) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (color) *color = c->color;
    if (pitch_bytes) *pitch_bytes = c->pitch;
    if (zbuf) *zbuf = c->zbuf;
    if (width) *width = c->W;
    if (height) *height = c->H;
    if (row0) *row0 = c->row0;
    if (row1) *row1 = c->row1;
    return PRK_OK;
}

int prk_get_device(prk_context *c, int32_t *device, void **stream) {
    if (!c) return PRK_ERR_ARG;
    if (device) *device = c->device;
    if (stream) *stream = (void *)c->own_stream;
    return PRK_OK;
}

int prk_synchronize(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->own_stream));
    PRK_TRY(hipDeviceSynchronize());
    return PRK_OK;
}

int prk_get_stats(prk_context *c, prk_stats *out) {
    if (!c || !out) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    (void)hipSetDevice(c->device);
    for (int i = 1; i <= prk_context::kRing; ++i)  // oldest first
        harvest(c, (int)((c->frame + i) % prk_context::kRing));
    if (c->d_anomaly.p) {
        PRK_TRY(hipDeviceSynchronize());
        static_assert(offsetof(prk_stats, slow_replays) == offsetof(prk_stats, anomalies) + 4, "counter pair");
        PRK_TRY(hipMemcpy(&c->stats.anomalies, c->d_anomaly.p, 8, hipMemcpyDeviceToHost));
    }
    *out = c->stats;
    return PRK_OK;
}

int prk_download_winners(prk_context *c, int32_t *w) {
    if (!c || !w) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (!c->winners_valid || !c->d_winners.p) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    PRK_TRY(hipMemcpy(w, c->d_winners.p, (size_t)c->W * (c->row1 - c->row0) * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

// ConstructSphere (projekt.cpp:4123-4289): the reference's only test mesh.
// 24 inclination x 48 azimuth steps, r = 0.5, 6624 vertices.
int prk_construct_sphere(float *V, float *Col, float *N, float *UV, uint32_t *count_out) {
    if (!V || !Col || !N || !UV || !count_out) return PRK_ERR_ARG;
    const float Pi32 = 3.14159265359f;
    const float Radius = 0.5f;
    const uint32_t StepCount = 24;
    const float Up[4] = {1, 0, 0, 1}, Down[4] = {0, 1, 0, 1};
    float Inc[4];
    for (int k = 0; k < 4; ++k) Inc[k] = (Down[k] - Up[k]) / (float)StepCount;
    const float IncI = Pi32 / StepCount;
    const float IncA = (2.0f * Pi32) / (StepCount * 2);
    float Cur[4] = {Up[0], Up[1], Up[2], Up[3]};
    uint32_t n = 0;
    auto emit = [&](float x, float y, float z, float u, float v, const float *c4, const float *blue, bool inc) {
        V[3 * n] = Radius * x; V[3 * n + 1] = Radius * y; V[3 * n + 2] = Radius * z;
        N[3 * n] = x; N[3 * n + 1] = y; N[3 * n + 2] = z;
        UV[2 * n] = u; UV[2 * n + 1] = v;
        for (int k = 0; k < 4; ++k) Col[4 * n + k] = inc ? (c4[k] + Inc[k]) + blue[k] : c4[k] + blue[k];
        ++n;
    };
    for (uint32_t ii = 0; ii < StepCount; ++ii) {
        for (uint32_t ai = 0; ai < StepCount * 2; ++ai) {
            float I0 = (float)ii * IncI, I1 = (float)(ii + 1) * IncI;
            float A0 = (float)ai * IncA, A1 = (float)(ai + 1) * IncA;
            float Blue[4] = {0, 0, (1.0f + cosf(A0)) / 2.0f, 0};
            float NBlue[4] = {0, 0, (1.0f + cosf(A1)) / 2.0f, 0};
            if (ii == 0) {
                float S[3] = {sinf(I1) * cosf(A0), cosf(I1), sinf(I1) * sinf(A0)};
                float Tt[3] = {sinf(I1) * cosf(A1), cosf(I1), sinf(I1) * sinf(A1)};
                emit(0, 1, 0, 0.5f, 0.5f, Cur, Blue, false);
                emit(S[0], S[1], S[2], S[0], S[2], Cur, Blue, true);
                emit(Tt[0], Tt[1], Tt[2], Tt[0], Tt[2], Cur, NBlue, true);
            } else if (ii == StepCount - 1) {
                float F[3] = {sinf(I0) * cosf(A0), cosf(I0), sinf(I0) * sinf(A0)};
                float Tt[3] = {sinf(I0) * cosf(A1), cosf(I0), sinf(I0) * sinf(A1)};
                emit(F[0], F[1], F[2], 0.5f, 0.5f, Cur, Blue, false);
                emit(0, -1, 0, 0.0f, 0.0f, Cur, Blue, true);
                emit(Tt[0], Tt[1], Tt[2], Tt[0], Tt[2], Cur, NBlue, true);
            } else {
                float F[3] = {sinf(I0) * cosf(A0), cosf(I0), sinf(I0) * sinf(A0)};
                float S[3] = {sinf(I1) * cosf(A0), cosf(I1), sinf(I1) * sinf(A0)};
                float Tt[3] = {sinf(I1) * cosf(A1), cosf(I1), sinf(I1) * sinf(A1)};
                float Fo[3] = {sinf(I0) * cosf(A1), cosf(I0), sinf(I0) * sinf(A1)};
                auto uvx = [](float a) { return (a + 1.0f) / 2.0f; };
                emit(F[0], F[1], F[2], uvx(F[0]), uvx(F[1]), Cur, Blue, false);
                emit(S[0], S[1], S[2], uvx(S[0]), uvx(S[1]), Cur, Blue, true);
                emit(Tt[0], Tt[1], Tt[2], uvx(Tt[0]), uvx(Tt[1]), Cur, NBlue, true);
                emit(F[0], F[1], F[2], uvx(F[0]), uvx(F[1]), Cur, Blue, false);
                emit(Tt[0], Tt[1], Tt[2], uvx(Tt[0]), uvx(Tt[1]), Cur, NBlue, true);
                emit(Fo[0], Fo[1], Fo[2], uvx(Fo[0]), uvx(Fo[1]), Cur, NBlue, false);
            }
        }
        for (int k = 0; k < 4; ++k) Cur[k] = Cur[k] + Inc[k];
    }
    *count_out = n;
    return PRK_OK;
}

}  // extern "C"
