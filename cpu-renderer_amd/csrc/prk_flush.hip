// prk_flush.hip — prk_flush: the recorded draws (prk_api.hip) become one GPU
// frame, pass by pass.
//   Platform.CompleteAllWork -> prk_flush runs bin + raster kernels.
// Here: the frame parameters every pass shares (frame_params), the target
// fill of a pending clear, the per-triangle pass (TriPass: draws of one
// triangle per object, binned on bin_stream and rastered on the flush stream)
// with the read of its bin entry count and the re-run of an over-capacity
// frame (resolve_count), and prk_debug_bins.  The whole-object pass is
// prk_span_pass.hip (flush_spans).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "prk_ctx.h"

extern "C" {

__global__ void k_fill_target(uint32_t *color, int32_t pitch, float *z, int32_t W, int32_t rows,
                              uint32_t cval, float zval) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = (size_t)W * rows;
    if (i >= n) return;
    size_t r = i / W, x = i % W;
    reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(color) + r * pitch)[x] = cval;
    z[i] = zval;
}

// k_fill_target over `rows` rows of W pixels (prk_target_clear, fill_pending_clear).
hipError_t launch_fill_target(void *color, int32_t pitch, float *z, int32_t W, int32_t rows, uint32_t cval,
                              float zval, hipStream_t s) {
    const size_t n = (size_t)W * rows;
    hipLaunchKernelGGL(k_fill_target, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint32_t *)color, pitch, z,
                       W, rows, cval, zval);
    return hipGetLastError();
}

}  // extern "C"

namespace {
// A camera and its lights as the kernels read them: FrameParams' own (the
// draws' setup) and its ShadeCam (the spans' shading) have these fields alike.
template <class Cam>
void fill_camera(Cam &o, const prk_transform &t, const prk_light_data &L) {
    o.D = t.DistanceAboveTarget;
    o.F = t.FocalLength;
    o.Cx = t.ScreenCenter[0];
    o.Cy = t.ScreenCenter[1];
    o.InvM2P = 1.0f / t.MetersToPixels;
    int e = 0;
    const float m = std::frexp(o.F, &e);  // F = m * 2^e, |m| in [0.5, 1)
    o.f_pow2 = (std::isfinite(o.F) && (m == 0.5f || m == -0.5f) && e - 1 >= -125 && e - 1 <= 126) ? 1 : 0;
    o.InvF = o.f_pow2 ? 1.0f / o.F : 0.0f;
    o.light_count = L.LightCount;
    for (int k = 0; k < 4; ++k) o.amb[k] = L.AmbientIntensity[k];
    for (uint32_t l = 0; l < PRK_MAX_LIGHTS; ++l) {
        for (int k = 0; k < 3; ++k) o.lp[l][k] = L.Lights[l].P[k];
        for (int k = 0; k < 4; ++k) o.li[l][k] = L.Lights[l].Intensity[k];
    }
}
}  // namespace

extern "C" {

// The frame parameters every pass of a flush shares (camera, lights, target, tiling).
void frame_params(const prk_context *c, prk::FrameParams &fp) {
    fp = prk::FrameParams{};
    fill_camera(fp, c->transform, c->lights);
    fp.M2P = c->transform.MetersToPixels;
    fill_camera(fp.sh, c->shade_transform, c->shade_lights);  // the span shading's (prk_set_shade_camera)
    fp.W = c->W;
    fp.H = c->H;
    fp.row0 = c->row0;
    fp.row1 = c->row1;
    fp.pitch = c->pitch;
    fp.color = (uint32_t *)c->color;
    fp.zbuf = c->zbuf;
    // The context's tile, made taller (then wider) while the frame would have
    // more tiles than the counting-sort binning holds (kCsMaxTiles): results
    // never depend on the tile, and every tile keeps <= 8192 pixels.
    int32_t tw = c->tile_w, th = c->tile_h;
    auto ntl = [&](int32_t w, int32_t h) {
        return (uint64_t)((c->W + w - 1) / w) * (uint64_t)((c->row1 - c->row0 + h - 1) / h);
    };
    while (ntl(tw, th) > prk_cs_max_tiles() && tw * th * 2 <= 8192) {
        if (th < tw / 8) th *= 2;
        else tw *= 2;
    }
    fp.tile_w = tw;
    fp.tile_h = th;
    fp.tile_w_log2 = 0;
    while ((1 << fp.tile_w_log2) < tw) ++fp.tile_w_log2;
    fp.tiles_x = (c->W + tw - 1) / tw;
    fp.tiles_y = (c->row1 - c->row0 + th - 1) / th;
    fp.prof = (unsigned long long *)c->d_prof.p;
    fp.negz = (uint32_t *)c->d_negz.p;
    fp.z_in_vis = c->early_z && c->d_negz.p ? 1 : 0;
    fp.winners = c->debug ? (int32_t *)c->d_winners.p : nullptr;
    fp.clear_color = c->clear_color;
    fp.clear_z = c->clear_z;
}

// A pending clear that the pass cannot fuse into its kernels: fill first.
static int fill_pending_clear(prk_context *c, hipStream_t s) {
    c->z_early = false;
    if (!c->clear_pending) return PRK_OK;
    c->clear_pending = false;
    const size_t n = (size_t)c->W * (c->row1 - c->row0);
    if (n)
        PRK_TRY(launch_fill_target(c->color, c->pitch, c->zbuf, c->W, c->row1 - c->row0, c->clear_color, c->clear_z,
                                   s));
    return PRK_OK;
}

// ---- the per-triangle pass (flush_tris) and its phases ---------------------
namespace {
// One per-triangle pass: what its phases share.  flush_tris runs them in
// order.  The order of the HIP calls, on every stream, is part of the pass:
// binning runs on bin_stream into one of the scratch sets, so it overlaps the
// previous frame's raster on the flush stream, and a host that is only just
// ahead of the GPU holds the sort back with every call it puts in front of it.
struct TriPass {
    prk_context *c;
    hipStream_t s;   // the flush stream
    hipStream_t bs;  // the bin stream
    const std::vector<prk::DrawRec> &draws;
    const uint32_t T, win_base;
    prk::FrameParams fp;
    uint32_t ntiles = 0;
    // begin(): the draws' one mode (or -1), whether the kernels fold a pending
    // clear in, the timing ring's slot
    int modeset = -2;
    bool fuse = false;
    int slot = 0;
    // tables(): the scratch set; its table mirrors are forgotten unless the
    // pass gets as far as commit() (any error leaves them unknown)
    int si = 0;
    prk_context::BinSet *set = nullptr;
    bool queued = false;
    std::vector<prk::TexRec> texs;
    // scratch(): won flags per (pair, row in tile) for span-record (AVX)
    // frames, per pair otherwise; the binning clears them (and trwon) for
    // every pair.  per: a row band's runs per chunk (0: the whole frame's
    // triangles), nch the sort's chunks, cap the pairs the set holds.
    bool span_rec = false;
    uint32_t won_stride = 1;
    size_t sel_bytes = 0;
    uint32_t per = 0, nch = 0, cap = 0;
    // raster(): the stream the raster starts on (k_vis of a span-record frame: the vis stream)
    hipStream_t sv = nullptr;

    TriPass(prk_context *ctx, hipStream_t stream, const std::vector<prk::DrawRec> &d, uint32_t tris, uint32_t base)
        : c(ctx), s(stream), bs(ctx->bin_stream), draws(d), T(tris), win_base(base) {}
    ~TriPass() {
        if (set && !queued) set->h_draws_at = set->h_texs_at = nullptr;
    }
    hipError_t bset_ensure(DevBuf &d, size_t n);
    hipError_t upload_table(DevBuf &d, std::vector<uint8_t> &mirror, const void *&at, const void *src, size_t bytes);
    size_t pairs_held() const;
    hipError_t ensure_pairs(size_t np);
    int begin();
    int tables();
    int scratch();
    int bin();
    int raster();
    int commit(bool defer);
};

// A set buffer that must grow is freed by the host: wait for its reader.
hipError_t TriPass::bset_ensure(DevBuf &d, size_t n) {
    if (d.cap < n && set->used) {
        hipError_t e = hipEventSynchronize(set->free_ev);
        if (e != hipSuccess) return e;
    }
    return d.ensure(n);
}

// Upload a table into this set unless the set already holds the same bytes
// (the set's previous reader, frame k-nsets's raster, is waited for in tables()).
hipError_t TriPass::upload_table(DevBuf &d, std::vector<uint8_t> &mirror, const void *&at, const void *src,
                                 size_t bytes) {
    hipError_t e = bset_ensure(d, bytes);
    if (e != hipSuccess) return e;
    if (at == d.p && mirror.size() == bytes && std::memcmp(mirror.data(), src, bytes) == 0) return hipSuccess;
    at = nullptr;  // unknown until the copy is queued
    mirror.assign((const uint8_t *)src, (const uint8_t *)src + bytes);
    // from the mirror: it outlives this call (the set's next use waits for
    // this frame's raster, which follows the copy on the bin stream)
    e = hipMemcpyAsync(d.p, mirror.data(), bytes, hipMemcpyHostToDevice, bs);
    if (e == hipSuccess) at = d.p;
    return e;
}

// pairs the set's per-pair arrays hold now (they never shrink)
size_t TriPass::pairs_held() const {
    const prk_context::BinSet &B = *set;
    size_t m = std::min(B.d_pair_tri.cap / 4, B.d_bins.cap / sizeof(prk::BinSlot));
    m = std::min(m, B.d_list.cap / 4);
    m = std::min(m, B.d_won.cap / won_stride);
    if (span_rec) m = std::min(m, B.d_recs.cap / (won_stride * sizeof(prk::SpanRec)));
    return m;
}

// Every per-pair array of the set, for `np` pairs.
hipError_t TriPass::ensure_pairs(size_t np) {
    prk_context::BinSet &B = *set;
    const size_t ne = std::max<size_t>(np, 1);
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = bset_ensure(B.d_pair_tri, ne * 4);
    if (e == hipSuccess) e = bset_ensure(B.d_bins, ne * sizeof(prk::BinSlot));
    if (e == hipSuccess) e = bset_ensure(B.d_list, ne * 4);
    if (e == hipSuccess) e = bset_ensure(B.d_won, ne * won_stride);
    // span records: one per (pair, row in tile); only won ones are written
    if (e == hipSuccess && span_rec) e = bset_ensure(B.d_recs, ne * won_stride * sizeof(prk::SpanRec));
    return e;
}

// The frame parameters and stats of the pass, the ring slot's old timings, and
// a pending clear: fused into the kernels or filled now.  (A pass of no
// triangles ends here: flush_tris.)
int TriPass::begin() {
    for (const auto &d : draws) {
        if (modeset == -2) modeset = d.mode;
        else if (modeset != d.mode) modeset = -1;
    }
    if (modeset != prk::MODE_AVX && modeset != prk::MODE_SC_GOURAUD && modeset != prk::MODE_SC_PHONG)
        modeset = -1;
    frame_params(c, fp);
    fp.tri_count = T;
    fp.ndraws = (uint32_t)draws.size();
    fp.win_base = win_base;
    ntiles = (uint32_t)(fp.tiles_x * fp.tiles_y);

    c->stats.triangles = T;
    c->stats.tiles = ntiles;
    c->stats.bin_entries = 0;
    slot = (int)(c->frame % prk_context::kRing);
    harvest(c, slot);  // a flush kRing frames old: long finished
    // A pending fused clear: the span-record kernels (AVX frames) fold it in;
    // every other frame fills the target first, on this stream.
    fuse = c->clear_pending && T > 0 && modeset == prk::MODE_AVX;
    if (!fuse) {
        const int rc = fill_pending_clear(c, s);
        if (rc != PRK_OK) return rc;
    }
    c->clear_pending = false;
    fp.clear_fused = fuse ? 1 : 0;
    return PRK_OK;
}

// The pass's scratch set, and the device-side draw + texture tables in it.
// Consecutive frames take consecutive sets (nsets of them), and a set's reuse
// waits for its own last reader.
int TriPass::tables() {
    const int nsets = (size_t)c->W * (size_t)(c->row1 - c->row0) <= kSmallBandPx ? prk_context::kSets
                                                                                : std::min(prk_context::kSets, 2);
    si = (c->last_set + 1) % nsets;
    c->last_set = si;
    set = &c->bset[si];
    prk_context::BinSet &B = *set;
    if (B.used) PRK_TRY(hipStreamWaitEvent(bs, B.free_ev, 0));  // the raster of frame k-nsets read this set
    tex_table(c, texs);
    PRK_TRY(upload_table(B.d_draws, B.h_draws, B.h_draws_at, draws.data(), draws.size() * sizeof(prk::DrawRec)));
    if (!texs.empty())
        PRK_TRY(upload_table(B.d_texs, B.h_texs, B.h_texs_at, texs.data(), texs.size() * sizeof(prk::TexRec)));
    fp.draws = (const prk::DrawRec *)B.d_draws.p;
    fp.texs = (const prk::TexRec *)B.d_texs.p;
    fp.draw0 = draws[0];
    fp.tex0 = prk::TexRec{};
    if (fp.draw0.tex >= 0 && (size_t)fp.draw0.tex < texs.size()) fp.tex0 = texs[fp.draw0.tex];
    fp.tri_draw = nullptr;
    if (fp.ndraws > 1) {
        PRK_TRY(bset_ensure(B.d_tri_draw, (size_t)T * 4));
        PRK_TRY(prk_launch_tri_draw(fp.draws, fp.ndraws, (uint32_t *)B.d_tri_draw.p, T, bs));
        fp.tri_draw = (const uint32_t *)B.d_tri_draw.p;
    }
    return PRK_OK;
}

// Every other buffer of the set that the pass's kernels use, in the order the
// allocations have always been made (a buffer that grows may wait for the
// set's reader and frees: HIP calls like the rest).  None is queued between
// bin()'s launches; the one allocation that follows them, the context's
// anomaly counters, stays in raster().
int TriPass::scratch() {
    prk_context::BinSet &B = *set;
    PRK_TRY(bset_ensure(B.d_ranges, (size_t)T * sizeof(prk::TileRange)));
    PRK_TRY(bset_ensure(B.d_tri_n, (size_t)(T + 1) * 4));
    PRK_TRY(bset_ensure(B.d_tri_off, (size_t)(T + 1) * 4));
    PRK_TRY(bset_ensure(B.d_offs, (size_t)(ntiles + 1) * 4));
    fp.trec = nullptr;
    if (modeset == prk::MODE_AVX && c->setup_rec) {
        PRK_TRY(bset_ensure(B.d_trec, (size_t)T * sizeof(prk::TriRec)));
        fp.trec = (prk::TriRec *)B.d_trec.p;
    }
    span_rec = modeset == prk::MODE_AVX;
    won_stride = span_rec ? (uint32_t)fp.tile_h : 1u;
    if (span_rec) PRK_TRY(prk_walk_select_bytes(T, &sel_bytes));
    PRK_TRY(bset_ensure(B.d_nwin, (size_t)ntiles * 4));
    PRK_TRY(bset_ensure(B.d_wtag, (size_t)ntiles * fp.tile_w * fp.tile_h * 4));
    if (span_rec) {
        PRK_TRY(bset_ensure(B.d_trwon, T));
        PRK_TRY(bset_ensure(B.d_wlist, ((size_t)T + 1) * 4));  // won triangles + their count
        PRK_TRY(bset_ensure(B.d_seltemp, std::max<size_t>(sel_bytes, 16)));
    }
    // (frame_params keeps every frame within the counting sort's tile count)
    if (ntiles > prk_cs_max_tiles()) return PRK_ERR_LIMIT;
    if (!prk_cs_ready(ntiles)) return PRK_ERR_DEVICE;
    // Counting-sort binning (prk_bin.hip k_cs_*): all sizes stay on the
    // device.  The per-pair arrays hold `cap` pairs (the last frame's count
    // plus room; a first frame guesses 2.5 per triangle, C3b has 3.2); a
    // frame with more entries leaves its bins empty and is re-run once the
    // count is known (resolve_count).
    // a row band's sort walks only its triangles (listed per run by k_bin_band)
    per = prk_cs_band_runs_per_chunk(&fp);
    if (per) {
        PRK_TRY(bset_ensure(B.d_runlist, (size_t)prk_bin_runs(T) * prk_bin_run_len() * 4));
        PRK_TRY(bset_ensure(B.d_run_n, (size_t)prk_bin_runs(T) * 4));
    }
    nch = prk_cs_nchunks(T, per);
    const uint64_t want64 = c->pair_hint ? (uint64_t)c->pair_hint + c->pair_hint / 8 + 4096
                                         : std::max<uint64_t>(5ull * T / 2, 1u << 16);
    const uint32_t want = (uint32_t)std::min<uint64_t>(want64, prk_cs_max_pairs());
    if (pairs_held() > 4ull * want && pairs_held() > (1u << 20)) {
        // far more room than the frames need (a big frame earlier): give
        // it back once the set's last reader is done
        if (B.used) PRK_TRY(hipEventSynchronize(B.free_ev));
        DevBuf *pb[] = {&B.d_pair_tri, &B.d_bins, &B.d_list, &B.d_won, &B.d_recs};
        for (DevBuf *b : pb) b->release();
    }
    if (pairs_held() < want) PRK_TRY(ensure_pairs(want));
    cap = (uint32_t)std::min<size_t>(pairs_held(), prk_cs_max_pairs());
    PRK_TRY(bset_ensure(B.d_ghist, std::max<size_t>((size_t)nch * ntiles * 4, 4)));
    PRK_TRY(bset_ensure(B.d_tile_tot, (size_t)ntiles * 4));
    PRK_TRY(bset_ensure(B.d_chunk, std::max<size_t>((size_t)nch * 8, 8)));
    PRK_TRY(bset_ensure(B.d_info, 8));
    return PRK_OK;
}

// The binning, on the bin stream: the triangles' tile ranges and counts, the
// counting sort into the bins, the entry count's copy to the host.
int TriPass::bin() {
    prk_context::BinSet &B = *set;
    uint8_t *won = (uint8_t *)B.d_won.p;
    uint8_t *trwon = span_rec ? (uint8_t *)B.d_trwon.p : nullptr;
    PRK_TRY(hipEventRecord(c->ev[slot][0], bs));
    uint32_t *runlist = per ? (uint32_t *)B.d_runlist.p : nullptr, *run_n = per ? (uint32_t *)B.d_run_n.p : nullptr;
    PRK_TRY(prk_bin_count(&fp, (uint32_t *)B.d_tri_n.p, B.d_ranges.as<prk::TileRange>(), runlist, run_n, trwon, bs));
    const bool band_rec = runlist && fp.trec;  // a row band's setup records (k_band_rec, below)
    if (band_rec) PRK_TRY(hipEventRecord(B.listed_ev, bs));
    uint32_t *chunk = (uint32_t *)B.d_chunk.p;
    PRK_TRY(prk_bin_cs(&fp, B.d_ranges.as<prk::TileRange>(), (const uint32_t *)B.d_tri_n.p, (uint32_t *)B.d_ghist.p,
                       (uint32_t *)B.d_tile_tot.p, chunk, chunk + nch, (uint32_t *)B.d_offs.p, cap,
                       (uint32_t *)B.d_info.p, (uint32_t *)B.d_tri_off.p, B.d_bins.as<prk::BinSlot>(),
                       (uint32_t *)B.d_pair_tri.p, won, won_stride, trwon, runlist, run_n, per, bs));
    // the entry count's copy to the host, which the host waits for, goes
    // first (behind binned_ev it would queue after k_vis); then the bins are
    // ready and the raster may start
    PRK_TRY(hipMemcpyAsync(B.h_info, B.d_info.p, 8, hipMemcpyDeviceToHost, bs));
    PRK_TRY(hipEventRecord(B.counted_ev, bs));
    PRK_TRY(hipEventRecord(c->ev[slot][1], bs));
    PRK_TRY(hipEventRecord(B.binned_ev, bs));
    // a row band's setup records run on the vis stream beside the counting
    // sort, once k_bin_band has listed the runs (this frame's k_vis follows
    // them there); queued after the sort's launches, so a host that is only
    // just ahead of the GPU (a frame after a wait) does not hold the sort back
    if (band_rec) {
        PRK_TRY(hipStreamWaitEvent(c->vis_stream, B.listed_ev, 0));
        PRK_TRY(prk_band_records(&fp, runlist, run_n, c->vis_stream));
    }
    return PRK_OK;
}

// Raster.  Span-record frames run k_vis on vis_stream once their binning
// is done (so it overlaps the previous frame's k_walk / k_pix on the
// flush stream, while the next frame bins on bin_stream) and shade on the
// flush stream after it; k_vis waits for the flush stream only when it
// reads the target's prior z (no fused clear), writes the debug winner
// map, or writes z itself (early z: the flush stream may still hold an
// earlier frame's z writers -- k_shade, k_pix, k_span_shade, a -0.0
// fix-up -- that must land before this frame's z).
// Other frames run on the flush stream.
int TriPass::raster() {
    prk_context::BinSet &B = *set;
    // (the context's first pass: created here, after the binning is queued,
    // not with the set's buffers in scratch() -- its fill waits for the flush stream)
    if (!c->d_anomaly.p) {
        PRK_TRY(c->d_anomaly.ensure(8));  // [anomalies, slow replays]
        PRK_TRY(hipMemsetAsync(c->d_anomaly.p, 0, 8, s));
        PRK_TRY(hipStreamSynchronize(s));
    }
    sv = s;
    if (span_rec) {
        sv = c->vis_stream;
        PRK_TRY(hipStreamWaitEvent(sv, B.binned_ev, 0));
        if (!fuse || c->debug || fp.z_in_vis) {  // prior z / winner map / early z: after the flush stream's work so far
            PRK_TRY(hipEventRecord(c->s_mark, s));
            PRK_TRY(hipStreamWaitEvent(sv, c->s_mark, 0));
        }
    } else {
        PRK_TRY(hipStreamWaitEvent(s, B.binned_ev, 0));
    }
    PRK_TRY(hipEventRecord(c->ev[slot][5], sv));
    PRK_TRY(prk_launch_raster(&fp, modeset, (const uint32_t *)B.d_offs.p, B.d_bins.as<prk::BinSlot>(),
                              (const uint32_t *)B.d_pair_tri.p, (const uint32_t *)B.d_tri_off.p,
                              B.d_ranges.as<prk::TileRange>(),
                              (uint8_t *)B.d_won.p, (uint8_t *)B.d_trwon.p, (uint32_t *)B.d_wlist.p,
                              B.d_seltemp.p, sel_bytes, (uint32_t *)B.d_list.p,
                              (uint32_t *)B.d_nwin.p, (uint32_t *)B.d_wtag.p, B.d_recs.as<prk::SpanRec>(),
                              (uint32_t *)c->d_anomaly.p, c->ev[slot][3], span_rec ? c->ev[slot][4] : nullptr, sv,
                              s));
    PRK_TRY(hipEventRecord(c->ev[slot][2], s));
    PRK_TRY(hipEventRecord(B.free_ev, s));
    return PRK_OK;
}

// The whole frame is queued: the context's books, then the entry count (the
// binning's first few kernels), which decides whether the frame fitted --
// read here, or, for the frame's last pass once a previous frame has sized
// the scratch, by the next call that needs it (resolve_count).
int TriPass::commit(bool defer) {
    // a span-record pass's z is final after k_vis (ev[slot][3], on the vis stream)
    c->z_early = span_rec && sv != s && fp.z_in_vis;
    c->z_slot = slot;
    set->used = true;
    c->pending[slot] = true;
    c->split_span[slot] = modeset == prk::MODE_AVX;
    c->last_slot = slot;
    c->frame++;
    queued = true;
    c->bdbg.valid = c->debug;
    if (c->debug) {  // (prk_debug_bins reads this set once the frame is done)
        prk_context::BinsDebug &D = c->bdbg;
        D.rerun = false;
        D.set = si;
        D.T = T;
        D.per = per;
        D.tile_w = fp.tile_w;
        D.tile_h = fp.tile_h;
        D.tiles_x = fp.tiles_x;
        D.tiles_y = fp.tiles_y;
        D.row0 = fp.row0;
        D.row1 = fp.row1;
    }
    prk_context::PendingCount &P = c->pcount;
    P.set = si;
    P.s = s;
    P.draws = draws;
    P.T = T;
    P.win_base = win_base;
    P.ntiles = ntiles;
    P.fuse = fuse;
    P.state = pass_state(c);
    P.active = true;
    if (!(defer && c->pair_hint)) return resolve_count(c);
    return PRK_OK;
}
}  // namespace

// One pass of per-triangle AETs (draws of one triangle per object): bin +
// raster into the target.  `draws` number their triangles from 0; winner ids
// are win_base + that index.  Binning runs on bin_stream into one of the
// scratch sets, so it overlaps the previous frame's raster on the flush
// stream; the raster waits for it.  defer: the entry count is left for
// resolve_count (which runs this again, without it, for an over-capacity frame).
static int flush_tris(prk_context *c, hipStream_t s, const std::vector<prk::DrawRec> &draws, uint32_t T,
                      uint32_t win_base, bool defer = false) {
    TriPass P(c, s, draws, T, win_base);
    int rc = P.begin();
    if (rc != PRK_OK || T == 0) return rc;  // (no triangles: the pending clear was the pass)
    rc = P.tables();
    if (rc == PRK_OK) rc = P.scratch();
    if (rc == PRK_OK) rc = P.bin();
    if (rc == PRK_OK) rc = P.raster();
    if (rc == PRK_OK) rc = P.commit(defer);
    return rc;
}

// The entry count of the pending pass (PendingCount): stats, the next
// frame's capacity and tile; an over-capacity pass drew nothing (empty bins;
// with a fused clear its k_pix wrote the clear values, which the re-run
// writes again) and is re-run with room for every entry, with the state it
// was queued with.
int resolve_count(prk_context *c) {
    prk_context::PendingCount &P = c->pcount;
    if (!P.active) return PRK_OK;
    P.active = false;
    PRK_TRY(hipSetDevice(c->device));
    prk_context::BinSet &B = c->bset[P.set];
    PRK_TRY(hipEventSynchronize(B.counted_ev));
    const uint32_t total = B.h_info[0];
    c->stats.bin_entries = total;
    c->pair_hint = total;
    const PassState &Q = P.state;
    if (c->tile_auto && !c->auto_small && Q.tile_w == 256 && total < 64u * P.ntiles &&
        8u * P.ntiles <= prk_cs_max_tiles()) {  // (32x8 tiles stay within the counting sort)
        c->auto_small = total < 8u * P.ntiles ? 64 : 32;  // (from the next frame on)
        c->auto_T = P.T;
        c->auto_px = Q.W * (Q.row1 - Q.row0);
    }
    // (a row band's entries against its share of the triangles, T * rows / H)
    if (c->tile_auto && !c->auto_small && !c->auto_wide && Q.tile_w == 256 && Q.tile_h == 8 && P.T && Q.H > 0 &&
        2ull * total * (uint64_t)Q.H >= 9ull * P.T * (uint64_t)std::max(1, Q.row1 - Q.row0) &&
        std::all_of(P.draws.begin(), P.draws.end(), [](const prk::DrawRec &d) { return d.mode == prk::MODE_AVX; })) {
        c->auto_wide = 512;  // (from the next frame on)
        c->auto_T = P.T;
        c->auto_px = Q.W * (Q.row1 - Q.row0);
    }
    if (!B.h_info[1]) return PRK_OK;
    if (total > prk_cs_max_pairs()) return PRK_ERR_LIMIT;  // 29-bit pair index in the bins
    // re-run with the pass's own state, then give the caller's back
    const PassState callers = pass_state(c);
    apply_pass_state(c, P.state);
    c->clear_pending = P.fuse;
    const std::vector<prk::DrawRec> draws = std::move(P.draws);
    const int rc = flush_tris(c, P.s, draws, P.T, P.win_base);
    // (the re-run ran with the pass's own debug flag, P.state: a prk_set_debug
    // since the flush does not change what prk_debug_bins answers for)
    if (rc == PRK_OK) c->bdbg.rerun = true;
    else c->bdbg.valid = false;
    c->read_rec = hipEventRecord(c->read_ev, P.s) == hipSuccess;  // (geometry writes wait for the re-run)
    c->z_early = false;  // (a re-run: the download takes z after everything)
    apply_pass_state(c, callers);
    return rc;
}

int prk_flush(prk_context *c, void *stream) {
    if (!c) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (!c->have_camera) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    {
        const int rc = resolve_count(c);  // the previous frame's count first: it may change the tile
        if (rc != PRK_OK) return rc;
    }
    if (c->tile_auto) {  // the frame's tile (see prk_context::tile_auto)
        const int64_t px = (int64_t)c->W * (c->row1 - c->row0);
        if ((c->auto_small || c->auto_wide) &&
            ((uint64_t)c->pending_tris > 2ull * c->auto_T || 2ull * c->pending_tris < c->auto_T ||
             px > 2 * (int64_t)c->auto_px || 2 * px < (int64_t)c->auto_px))
            c->auto_small = c->auto_wide = 0;  // re-decide from this frame's count
        c->tile_w = c->auto_small ? c->auto_small : (c->auto_wide ? c->auto_wide : 256);
        c->tile_h = 8;
    }
    hipStream_t s = stream ? (hipStream_t)stream : c->own_stream;
    // side passes still in flight: every stream of the frame waits for them
    PRK_TRY(side_wait(c, s));
    PRK_TRY(side_wait(c, c->bin_stream));
    PRK_TRY(side_wait(c, c->vis_stream));
    c->in_wait = false;
    bool any_avx = false;
    for (const auto &d : c->draws) any_avx |= d.mode == prk::MODE_AVX;
    if (any_avx && (c->W % 8)) return PRK_ERR_UNSUPPORTED;  // aligned 8-wide z load, projekt.cpp:2218
    prk::FrameParams probe;
    frame_params(c, probe);
    if (probe.tiles_x > 65535 || probe.tiles_y > 65535) return PRK_ERR_UNSUPPORTED;
    if (!c->d_prof.p) {
        PRK_TRY(c->d_prof.ensure(16 * sizeof(uint64_t)));
        PRK_TRY(hipMemsetAsync(c->d_prof.p, 0, 16 * sizeof(uint64_t), s));
    }
    if (!c->d_negz.p) {
        PRK_TRY(c->d_negz.ensure(4));
        PRK_TRY(hipMemsetAsync(c->d_negz.p, 0, 4, s));
    }
    c->z_early = false;  // (the passes below say whether the frame's last one allows it)
    c->bdbg.valid = false;  // (prk_debug_bins: this flush's last per-triangle pass, if any)
    c->vis.frame = c->vis.done = false;  // (prk_visibility_*: this flush's frame, if it draws with the winner map)
    const uint32_t frame_ids = c->pending_tris;  // the ids this flush hands out
    if (c->debug) {
        PRK_TRY(c->d_winners.ensure((size_t)c->W * (c->row1 - c->row0) * 4));
        PRK_TRY(hipMemsetAsync(c->d_winners.p, 0xFF, (size_t)c->W * (c->row1 - c->row0) * 4, s));
        c->winners_valid = true;
    }
    // Passes: maximal runs of draws of one kind (per-triangle AETs, or
    // whole-object AETs); each pass z-tests against the target as the
    // previous one left it, which is the reference's sequential order.
    std::vector<prk::DrawRec> dr = std::move(c->draws);
    c->draws.clear();
    c->pending_tris = 0;
    struct Clear {  // the frame's edge / span input goes with its draws
        prk_context *c;
        ~Clear() {
            c->pend_edges.clear();
            c->pend_spans.clear();
            c->pend_ledges.clear();
            c->pend_lcnt.clear();
            c->pend_lflag.clear();
        }
    } clear_src{c};
    if (dr.empty()) return c->clear_pending ? fill_pending_clear(c, s) : PRK_OK;
    auto span_path = [](const prk::DrawRec &d) { return d.obj_tris > 1 || d.src_kind != 0; };
    size_t i = 0;
    int rc = PRK_OK;
    while (i < dr.size() && rc == PRK_OK) {
        const bool obj = span_path(dr[i]);
        size_t j = i;
        std::vector<prk::DrawRec> seg;
        uint32_t T = 0;
        const uint32_t base = dr[i].first_global;
        while (j < dr.size() && span_path(dr[j]) == obj) {
            prk::DrawRec d = dr[j];
            d.first_global -= base;
            T += d.tri_count;
            seg.push_back(d);
            ++j;
        }
        // (only the frame's last pass defers its count: a later pass z-tests
        // against this one's output, so an overflow must be re-run first)
        rc = obj ? flush_spans(c, s, seg, T, base) : flush_tris(c, s, seg, T, base, j == dr.size());
        i = j;
    }
    // the frame's last reader of the geometry (the flush stream ends every pass)
    c->read_rec = hipEventRecord(c->read_ev, s) == hipSuccess;
    if (rc == PRK_OK && c->debug) {  // the frame prk_visibility_* answers for
        c->vis.frame = true;
        c->vis.id_count = frame_ids;
    }
    return rc;
}

// prk_dist.hip: gathers read the band's finished frame (library-internal).
// The pending count is resolved first (an overflowed frame is re-run on its
// own flush stream), then `stream` (the gather's, any stream of the
// context's device) waits for the end of the context's last frame.
__attribute__((visibility("hidden"))) int prk_resolve_pending(prk_context *c, void *stream) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (stream && c->read_rec) {
        PRK_TRY(hipSetDevice(c->device));
        PRK_TRY(hipStreamWaitEvent((hipStream_t)stream, c->read_ev, 0));
    }
    return PRK_OK;
}

int prk_resolve(prk_context *c, void *stream) { return prk_resolve_pending(c, stream); }

int prk_debug_bins(prk_context *c, prk_bins_info *info, uint32_t *tri_n, uint16_t *ranges, uint32_t *tri_off,
                   uint8_t *listed, uint64_t tri_capacity, uint32_t *offs, uint64_t tile_capacity, uint32_t *bins,
                   uint32_t *pair_tri, uint64_t entry_capacity) {
    if (!c || !info) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);  // (an overflowed pass is re-run here: bdbg then names the re-run's set)
    const prk_context::BinsDebug &D = c->bdbg;
    if (!D.valid) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());
    const prk_context::BinSet &B = c->bset[D.set];
    const uint32_t T = D.T, ntiles = (uint32_t)(D.tiles_x * D.tiles_y), total = B.h_info[0];
    *info = prk_bins_info{D.tile_w, D.tile_h, D.tiles_x, D.tiles_y, D.row0, D.row1, T, total, D.rerun ? 1u : 0u,
                          D.per};
    if ((tri_n || ranges || tri_off || listed) && tri_capacity < T) return PRK_ERR_ARG;
    if (offs && tile_capacity < ntiles) return PRK_ERR_ARG;
    if ((bins || pair_tri) && entry_capacity < total) return PRK_ERR_ARG;
    if (tri_n) PRK_TRY(hipMemcpy(tri_n, B.d_tri_n.p, (size_t)T * 4, hipMemcpyDeviceToHost));
    if (ranges) PRK_TRY(hipMemcpy(ranges, B.d_ranges.p, (size_t)T * sizeof(prk::TileRange), hipMemcpyDeviceToHost));
    if (tri_off) PRK_TRY(hipMemcpy(tri_off, B.d_tri_off.p, ((size_t)T + 1) * 4, hipMemcpyDeviceToHost));
    if (listed) std::memset(listed, D.per ? 0 : 1, T);
    if (D.per && (tri_n || ranges || tri_off || listed)) {
        // a row band: k_bin_band and k_cs_emit wrote only the triangles of the
        // run lists; the others hold what an earlier frame left
        const uint32_t nruns = prk_bin_runs(T), len = prk_bin_run_len();
        std::vector<uint32_t> run_n(nruns), list((size_t)nruns * len);
        std::vector<uint8_t> in(T, 0);
        PRK_TRY(hipMemcpy(run_n.data(), B.d_run_n.p, (size_t)nruns * 4, hipMemcpyDeviceToHost));
        PRK_TRY(hipMemcpy(list.data(), B.d_runlist.p, list.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t r = 0; r < nruns; ++r)
            for (uint32_t i = 0; i < std::min(run_n[r], len); ++i) {
                const uint32_t g = list[(size_t)r * len + i];
                if (g < T) in[g] = 1;
            }
        static const uint16_t kEmpty[8] = {1, 1, 0, 0, 1, 0, 0, 0};
        for (uint32_t g = 0; g < T; ++g) {
            if (listed) listed[g] = in[g];
            if (in[g]) continue;
            if (tri_n) tri_n[g] = 0;
            if (ranges) std::memcpy(ranges + 8 * (size_t)g, kEmpty, sizeof(kEmpty));
            if (tri_off) tri_off[g] = UINT32_MAX;
        }
    }
    if (offs) PRK_TRY(hipMemcpy(offs, B.d_offs.p, ((size_t)ntiles + 1) * 4, hipMemcpyDeviceToHost));
    if (bins && total) PRK_TRY(hipMemcpy(bins, B.d_bins.p, (size_t)total * sizeof(prk::BinSlot),
                                         hipMemcpyDeviceToHost));
    if (pair_tri && total) PRK_TRY(hipMemcpy(pair_tri, B.d_pair_tri.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

}  // extern "C"
