// prk_api.hip — host side of libprk_hip.so: the C-ABI declared in include/prk.h,
// one of four host files over prk_ctx.h (the context).  This one owns the
// context and its device resources -- the runtime check, the self-tests,
// targets, textures, layers, pinned host memory, geometry -- and records the
// reference's draw calls:
//   FillEdgeTable + DrawModelOptimized / DrawModel (projekt.cpp:3882, 3615, 162)
//   -> prk_draw records {geometry range, P, semantics, Phong, Bitmap}
// The frame those draws make is queued by prk_flush (prk_flush.hip: the
// per-triangle pass; prk_span_pass.hip: the whole-object pass); the record and
// span handles and the record walks are prk_record_api.hip.
// There is no CPU fallback: every entry point that computes pixels needs the
// HIP device and fails with PRK_ERR_DEVICE without one.
#include <hip/hip_runtime.h>
#include <link.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <functional>
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

#include "../../include/prk.h"
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

// prk_selftest_sort / _scan: a device buffer of `bytes` payload bytes and
// kGuardBytes of kGuardByte after them, filled and read with copies only.
constexpr size_t kGuardBytes = 4096;
constexpr unsigned char kGuardByte = 0xA5;
struct GuardedBuf {
    char *p = nullptr;
    size_t bytes = 0;
    std::vector<unsigned char> host;  // what the buffer was last filled with, then what it holds
    ~GuardedBuf() {
        if (p) (void)hipFree(p);
    }
    // the pattern everywhere, then `src` (may be null) over the payload
    hipError_t fill(size_t payload, const void *src) {
        if (!p) {
            bytes = payload;
            const hipError_t e = hipMalloc(&p, bytes + kGuardBytes);
            if (e != hipSuccess) return e;
        }
        host.assign(bytes + kGuardBytes, kGuardByte);
        if (src && bytes) std::memcpy(host.data(), src, bytes);
        return hipMemcpy(p, host.data(), host.size(), hipMemcpyHostToDevice);
    }
    hipError_t read() { return hipMemcpy(host.data(), p, host.size(), hipMemcpyDeviceToHost); }
    bool guard_intact() const {
        for (size_t i = bytes; i < host.size(); ++i)
            if (host[i] != kGuardByte) return false;
        return true;
    }
    bool holds(const void *src) const { return bytes == 0 || std::memcmp(host.data(), src, bytes) == 0; }
};
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

// Self-test of the shared-divisor quotients against the compiler's division
// (prk.h).  Runs on `device`, synchronously.
int prk_selftest_div_paths(int32_t device, uint32_t n, uint64_t seed, uint64_t *mismatches, uint32_t fast_waves[2]) {
    if (!mismatches || device < 0) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    unsigned long long *d = nullptr;
    PRK_TRY(hipMalloc(&d, 3 * sizeof(unsigned long long)));
    hipError_t e = hipMemset(d, 0, 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = prk_selftest_div_launch(n, seed, d, nullptr);
    unsigned long long h[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return status_of(e);
    *mismatches = h[0];
    if (fast_waves) {
        fast_waves[0] = (uint32_t)h[1];
        fast_waves[1] = (uint32_t)h[2];
    }
    return PRK_OK;
}
int prk_selftest_div(int32_t device, uint32_t n, uint64_t seed, uint64_t *mismatches) {
    return prk_selftest_div_paths(device, n, seed, mismatches, nullptr);
}

// One device primitive on the caller's words (prk.h).  Runs on `device`,
// synchronously; the kernel reads and writes whole 4 x n buffers, so an input
// the op does not read is zeros.
int prk_selftest_ops(int32_t device, int32_t op, uint32_t n, const uint32_t *a, const uint32_t *b,
                     const uint32_t *c, const uint32_t *d, uint32_t *out0, uint32_t *out1, uint32_t *out2,
                     uint32_t *fast) {
    static const uint8_t kInputs[PRK_OP_COUNT] = {2, 2, 4, 4, 4, 4, 4, 2, 1, 1, 3, 3, 1,
                                                  1, 1, 1, 2, 2, 1, 2, 1, 1, 2, 1, 3, 3};
    if (device < 0 || op < 0 || op >= PRK_OP_COUNT || n > (1u << 24) || !out0) return PRK_ERR_ARG;
    const uint32_t *in[4] = {a, b, c, d};
    for (int k = 0; k < kInputs[op]; ++k)
        if (!in[k]) return PRK_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    if (n == 0) return PRK_OK;
    PRK_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    uint32_t *din = nullptr, *dout = nullptr;
    PRK_TRY(hipMalloc(&din, 4 * bytes));
    hipError_t e = hipMalloc(&dout, 4 * bytes);
    if (e == hipSuccess) e = hipMemset(din, 0, 4 * bytes);
    for (int k = 0; k < kInputs[op] && e == hipSuccess; ++k)
        e = hipMemcpy(din + (size_t)k * n, in[k], bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = prk_selftest_ops_launch(op, n, din, dout, nullptr);
    uint32_t *outs[4] = {out0, out1, out2, fast};
    for (int k = 0; k < 4 && e == hipSuccess; ++k)
        if (outs[k]) e = hipMemcpy(outs[k], dout + (size_t)k * n, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return status_of(e);
}

// The radix sort on the caller's pairs (prk.h): guarded buffers, the temp
// buffer at exactly the queried size and left as it is between the repeats.
int prk_selftest_sort(int32_t device, uint32_t n, uint32_t end_bit, const uint64_t *keys, const uint32_t *vals,
                      uint32_t repeats, uint64_t *keys_out, uint32_t *vals_out, uint32_t *damage) {
    if (device < 0 || !keys || !vals || !keys_out || !vals_out || !damage || repeats == 0) return PRK_ERR_ARG;
    size_t tb = 0;
    PRK_TRY(prk_obj_sort(nullptr, nullptr, nullptr, nullptr, n, end_bit, nullptr, &tb, nullptr));  // (host only)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    const size_t kb = (size_t)n * 8, vb = (size_t)n * 4;
    GuardedBuf kin, vin, kout, vout, temp;
    PRK_TRY(kin.fill(kb, keys));
    PRK_TRY(vin.fill(vb, vals));
    PRK_TRY(temp.fill(tb, nullptr));
    for (uint32_t r = 0; r < repeats; ++r) {
        PRK_TRY(kout.fill(kb, nullptr));
        PRK_TRY(vout.fill(vb, nullptr));
        PRK_TRY(prk_obj_sort(kin.p, (uint32_t *)vin.p, kout.p, (uint32_t *)vout.p, n, end_bit, temp.p, &tb, nullptr));
        PRK_TRY(hipDeviceSynchronize());
    }
    PRK_TRY(kin.read());
    PRK_TRY(vin.read());
    PRK_TRY(kout.read());
    PRK_TRY(vout.read());
    PRK_TRY(temp.read());
    *damage = (kin.holds(keys) && vin.holds(vals) && kin.guard_intact() && vin.guard_intact() ? 0u : PRK_DAMAGE_INPUT) |
              (kout.guard_intact() && vout.guard_intact() ? 0u : PRK_DAMAGE_OUTPUT_GUARD) |
              (temp.guard_intact() ? 0u : PRK_DAMAGE_TEMP_GUARD);
    if (n) {
        std::memcpy(keys_out, kout.host.data(), kb);
        std::memcpy(vals_out, vout.host.data(), vb);
    }
    return PRK_OK;
}

// An exclusive scan on the caller's words (prk.h), in and out distinct.
int prk_selftest_scan(int32_t device, int32_t width, uint32_t n, const void *in, void *out, uint32_t *damage) {
    if (device < 0 || (width != 32 && width != 64) || !in || !out || !damage) return PRK_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * (size_t)(width / 8);
    size_t tb = 0;
    GuardedBuf din, dout, temp;
    PRK_TRY(din.fill(bytes, in));
    PRK_TRY(dout.fill(bytes, nullptr));
    if (width == 32) {
        PRK_TRY(prk_scan_u32(nullptr, nullptr, n, nullptr, &tb, nullptr));
        PRK_TRY(temp.fill(tb, nullptr));
        PRK_TRY(prk_scan_u32((const uint32_t *)din.p, (uint32_t *)dout.p, n, temp.p, &tb, nullptr));
    } else {
        PRK_TRY(prk_scan_u64(nullptr, nullptr, n, nullptr, &tb, nullptr));
        PRK_TRY(temp.fill(tb, nullptr));
        PRK_TRY(prk_scan_u64((const unsigned long long *)din.p, (unsigned long long *)dout.p, n, temp.p, &tb,
                             nullptr));
    }
    PRK_TRY(hipDeviceSynchronize());
    PRK_TRY(din.read());
    PRK_TRY(dout.read());
    PRK_TRY(temp.read());
    *damage = (din.holds(in) && din.guard_intact() ? 0u : PRK_DAMAGE_INPUT) |
              (dout.guard_intact() ? 0u : PRK_DAMAGE_OUTPUT_GUARD) | (temp.guard_intact() ? 0u : PRK_DAMAGE_TEMP_GUARD);
    if (bytes) std::memcpy(out, dout.host.data(), bytes);
    return PRK_OK;
}

// The visibility reduction on the caller's words (prk.h): prk_visibility_*'s
// kernels with no context, every device buffer guarded, the histogram in its
// counting instantiation.
int prk_selftest_visibility(int32_t device, uint32_t n, const int32_t *winners, uint32_t id_count, uint32_t *counts,
                            uint32_t *pix_prefix, uint32_t *vis_prefix, uint32_t *ids, uint32_t *visible_out,
                            uint64_t *atomics_out, uint32_t *damage) {
    if (device < 0 || (!winners && n) || ((!counts || !ids) && id_count) || !pix_prefix || !vis_prefix ||
        !visible_out || !atomics_out || !damage || id_count > 0xFFFFFFF0u)
        return PRK_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    const size_t wb = (size_t)n * 4, ib = (size_t)id_count * 4, mb = ib + 4;
    size_t tb = 0;
    PRK_TRY(prk_vis_reduce(nullptr, n, id_count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &tb, nullptr,
                           nullptr));
    GuardedBuf win, cnt, flg, pix, vis, idl, temp, nat;
    const uint32_t zero = 0;
    PRK_TRY(win.fill(wb, winners));
    PRK_TRY(cnt.fill(mb, nullptr));
    PRK_TRY(flg.fill(mb, nullptr));
    PRK_TRY(pix.fill(mb, nullptr));
    PRK_TRY(vis.fill(mb, nullptr));
    PRK_TRY(idl.fill(ib, nullptr));
    PRK_TRY(temp.fill(tb, nullptr));
    PRK_TRY(nat.fill(4, &zero));
    PRK_TRY(prk_vis_reduce((const int32_t *)win.p, n, id_count, (uint32_t *)cnt.p, (uint32_t *)flg.p, (uint32_t *)pix.p,
                           (uint32_t *)vis.p, (uint32_t *)idl.p, temp.p, &tb, (uint32_t *)nat.p, nullptr));
    PRK_TRY(hipDeviceSynchronize());
    GuardedBuf *all[] = {&win, &cnt, &flg, &pix, &vis, &idl, &temp, &nat};
    for (GuardedBuf *b : all) PRK_TRY(b->read());
    *damage = (win.holds(winners) && win.guard_intact() ? 0u : PRK_DAMAGE_INPUT) |
              (cnt.guard_intact() && pix.guard_intact() && vis.guard_intact() && idl.guard_intact() &&
                       nat.guard_intact()
                   ? 0u
                   : PRK_DAMAGE_OUTPUT_GUARD) |
              (temp.guard_intact() && flg.guard_intact() ? 0u : PRK_DAMAGE_TEMP_GUARD);
    uint32_t visible = 0, atomics = 0;
    std::memcpy(&visible, vis.host.data() + ib, 4);
    std::memcpy(&atomics, nat.host.data(), 4);
    if (visible > id_count) visible = id_count;  // (a damaged run: nothing past the caller's arrays)
    if (ib) std::memcpy(counts, cnt.host.data(), ib);
    std::memcpy(pix_prefix, pix.host.data(), mb);
    std::memcpy(vis_prefix, vis.host.data(), mb);
    if (visible) std::memcpy(ids, idl.host.data(), (size_t)visible * 4);
    *visible_out = visible;
    *atomics_out = atomics;
    return PRK_OK;
}

// prk_geometry_select's three stages on the caller's tables and arrays
// (prk.h): the launchers the call itself queues, with no context, every
// device buffer guarded, the outputs starting out as the guard pattern.
int prk_selftest_select(int32_t device, const uint32_t *pix_prefix, uint32_t id_count, const prk_select_item *items,
                        uint32_t item_count, const prk_select_level *levels, uint32_t level_count,
                        const prk_xform *xforms, uint32_t xform_count, const uint32_t *item_pixels,
                        const float *src_vertices, const float *src_colors, const float *src_normals,
                        const float *src_uvs, uint32_t src_tris, uint32_t dst_first_tri, uint32_t dst_tris,
                        float *dst_vertices, float *dst_colors, float *dst_normals, float *dst_uvs, int32_t *chosen,
                        uint32_t *out_first, uint64_t *total_tris_out, uint32_t *damage) {
    if (device < 0 || (item_count && (!items || !chosen)) || !out_first || !total_tris_out || !damage ||
        (!item_pixels && !pix_prefix) || id_count == UINT32_MAX || item_count == UINT32_MAX)
        return PRK_ERR_ARG;
    const float *src[4] = {src_vertices, src_colors, src_normals, src_uvs};
    float *dst[4] = {dst_vertices, dst_colors, dst_normals, dst_uvs};
    const size_t comp[4] = {3, 4, 3, 2};
    for (int k = 0; k < 4; ++k)
        if (src[k] && !dst[k]) return PRK_ERR_ARG;
    uint64_t worst = 0;
    {
        const int rc = select_check(items, item_count, levels, level_count, xforms, xform_count, src_tris,
                                    item_pixels ? nullptr : &id_count, &worst);
        if (rc != PRK_OK) return rc;
    }
    if (worst && !src_vertices) return PRK_ERR_ARG;
    if (worst > (1ull << 31)) return PRK_ERR_LIMIT;
    if ((uint64_t)dst_first_tri + worst > dst_tris || (uint64_t)dst_tris * 3 > 0xFFFFFFF0ull) return PRK_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    const size_t wb = ((size_t)item_count + 1) * 4;
    size_t tb = 0;
    PRK_TRY(prk_scan_u32(nullptr, nullptr, item_count + 1, nullptr, &tb, nullptr));
    GuardedBuf pix, itm, lev, xfm, ipx, sa[4], da[4], cho, cnt, sta, run, temp;
    PRK_TRY(pix.fill(item_pixels ? 0 : ((size_t)id_count + 1) * 4, pix_prefix));
    PRK_TRY(itm.fill((size_t)item_count * sizeof(prk_select_item), items));
    PRK_TRY(lev.fill(levels ? (size_t)level_count * sizeof(prk_select_level) : 0, levels));
    PRK_TRY(xfm.fill(xforms ? (size_t)xform_count * sizeof(prk_xform) : 0, xforms));
    PRK_TRY(ipx.fill(item_pixels ? (size_t)item_count * 4 : 0, item_pixels));
    for (int k = 0; k < 4; ++k) {
        PRK_TRY(sa[k].fill(src[k] ? (size_t)src_tris * 3 * comp[k] * 4 : 0, src[k]));
        PRK_TRY(da[k].fill(src[k] ? (size_t)dst_tris * 3 * comp[k] * 4 : 0, nullptr));
    }
    PRK_TRY(cho.fill((size_t)item_count * 4, nullptr));
    PRK_TRY(cnt.fill(wb, nullptr));
    PRK_TRY(sta.fill(wb, nullptr));
    PRK_TRY(run.fill((size_t)item_count * sizeof(prk::SelRun), nullptr));
    PRK_TRY(temp.fill(tb, nullptr));
    PRK_TRY(prk_sel_choose((const prk_select_item *)itm.p, item_count, (const prk_select_level *)lev.p,
                           item_pixels ? nullptr : (const uint32_t *)pix.p,
                           item_pixels ? (const uint32_t *)ipx.p : nullptr, nullptr, (int32_t *)cho.p, (uint32_t *)cnt.p,
                           (prk::SelRun *)run.p, nullptr));
    PRK_TRY(prk_scan_u32((const uint32_t *)cnt.p, (uint32_t *)sta.p, item_count + 1, temp.p, &tb, nullptr));
    uint32_t total = 0;
    PRK_TRY(hipMemcpy(&total, sta.p + (size_t)item_count * 4, 4, hipMemcpyDeviceToHost));  // (waits for both)
    if (total > worst) return PRK_ERR_DEVICE;  // (never: the emit pass would leave the destination)
    const float *ds[4];
    float *dd[4];
    for (int k = 0; k < 4; ++k) {
        ds[k] = src[k] ? (const float *)sa[k].p : nullptr;
        dd[k] = src[k] ? (float *)da[k].p : nullptr;
    }
    PRK_TRY(prk_sel_emit((const uint32_t *)sta.p, (const prk::SelRun *)run.p, item_count, total, dst_first_tri,
                         (const prk_xform *)xfm.p, ds[0], ds[1], ds[2], ds[3], dd[0], dd[1], dd[2], dd[3], nullptr));
    PRK_TRY(hipDeviceSynchronize());
    GuardedBuf *all[] = {&pix, &itm, &lev, &xfm, &ipx, &sa[0], &sa[1], &sa[2], &sa[3], &da[0], &da[1],
                         &da[2], &da[3], &cho, &cnt, &sta, &run, &temp};
    for (GuardedBuf *b : all) PRK_TRY(b->read());
    bool in_ok = pix.holds(pix_prefix) && pix.guard_intact() && itm.holds(items) && itm.guard_intact() &&
                 lev.holds(levels) && lev.guard_intact() && xfm.holds(xforms) && xfm.guard_intact() &&
                 ipx.holds(item_pixels) && ipx.guard_intact();
    bool out_ok = cho.guard_intact() && sta.guard_intact();
    for (int k = 0; k < 4; ++k) {
        in_ok = in_ok && sa[k].holds(src[k]) && sa[k].guard_intact();
        out_ok = out_ok && da[k].guard_intact();
    }
    *damage = (in_ok ? 0u : PRK_DAMAGE_INPUT) | (out_ok ? 0u : PRK_DAMAGE_OUTPUT_GUARD) |
              (cnt.guard_intact() && run.guard_intact() && temp.guard_intact() ? 0u : PRK_DAMAGE_TEMP_GUARD);
    if (item_count) std::memcpy(chosen, cho.host.data(), (size_t)item_count * 4);
    std::memcpy(out_first, sta.host.data(), wb);
    for (uint32_t i = 0; i <= item_count; ++i) out_first[i] += dst_first_tri;
    for (int k = 0; k < 4; ++k)
        if (src[k] && da[k].bytes) std::memcpy(dst[k], da[k].host.data(), da[k].bytes);
    *total_tris_out = total;
    return PRK_OK;
}

// prk_visibility_bounds' two kernels on the caller's z words and tables
// (prk.h): the launchers the call itself queues, with no context, every device
// buffer guarded, the z words z_offset floats into their buffer.
int prk_selftest_bounds(int32_t device, const float *z, int32_t width, int32_t height, int32_t row0, int32_t row1,
                        uint32_t z_offset, const prk_transform *transform, const float P[3], const prk_bound *bounds,
                        uint32_t count, const prk_xform *xforms, uint32_t xform_count, float *zmin, uint32_t *pixels,
                        uint32_t *damage) {
    if (device < 0 || !z || !transform || !zmin || !damage || (count && (!bounds || !xforms || !pixels)) ||
        width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 >= row1 || z_offset > 1024)
        return PRK_ERR_ARG;
    for (uint32_t i = 0; i < count; ++i)
        if (bounds[i].xform >= xform_count) return PRK_ERR_ARG;
    prk::BoundsFrame B;
    if (!bounds_frame(width, row0, row1, *transform, P, &B)) return PRK_ERR_LIMIT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PRK_ERR_DEVICE;
    if (device >= ndev) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
    const size_t npx = (size_t)width * (size_t)(row1 - row0), nt = (size_t)B.tiles_x * (size_t)B.tiles_y;
    std::vector<float> zin(z_offset + npx, 0.0f);
    std::memcpy(zin.data() + z_offset, z, npx * 4);
    GuardedBuf zb, xfm, bnd, zmn, pix;
    PRK_TRY(zb.fill(zin.size() * 4, zin.data()));
    PRK_TRY(xfm.fill(count ? (size_t)xform_count * sizeof(prk_xform) : 0, xforms));
    PRK_TRY(bnd.fill((size_t)count * sizeof(prk_bound), bounds));
    PRK_TRY(zmn.fill(nt * 4, nullptr));
    PRK_TRY(pix.fill((size_t)count * 4, nullptr));
    PRK_TRY(prk_ztile_min((const float *)zb.p + z_offset, &B, (float *)zmn.p, nullptr));
    PRK_TRY(prk_bounds_test((const prk_bound *)bnd.p, count, (const prk_xform *)xfm.p, &B, (const float *)zmn.p,
                            (uint32_t *)pix.p, nullptr));
    PRK_TRY(hipDeviceSynchronize());
    GuardedBuf *all[] = {&zb, &xfm, &bnd, &zmn, &pix};
    for (GuardedBuf *b : all) PRK_TRY(b->read());
    *damage = (zb.holds(zin.data()) && zb.guard_intact() && xfm.holds(xforms) && xfm.guard_intact() &&
                       bnd.holds(bounds) && bnd.guard_intact()
                   ? 0u
                   : PRK_DAMAGE_INPUT) |
              (zmn.guard_intact() && pix.guard_intact() ? 0u : PRK_DAMAGE_OUTPUT_GUARD);
    std::memcpy(zmin, zmn.host.data(), nt * 4);
    if (count) std::memcpy(pixels, pix.host.data(), (size_t)count * 4);
    return PRK_OK;
}

int prk_create(int device, prk_context **out) {
    if (!out) return PRK_ERR_ARG;
    *out = nullptr;
    {
        const int rc = prk_runtime_check();
        if (rc != PRK_OK) return rc;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PRK_ERR_DEVICE;
    if (device < 0 || device >= n) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(device));
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
        if (g.owned) {
            (void)hipFree((void *)g.V);
            (void)hipFree((void *)g.C);
            (void)hipFree((void *)g.N);
            (void)hipFree((void *)g.UV);
        }
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
        if (B.free_ev) (void)hipEventDestroy(B.free_ev);
        if (B.binned_ev) (void)hipEventDestroy(B.binned_ev);
        if (B.counted_ev) (void)hipEventDestroy(B.counted_ev);
        if (B.listed_ev) (void)hipEventDestroy(B.listed_ev);
        if (B.h_info) (void)hipHostFree(B.h_info);
    }
    DevBuf *bufs[] = {&c->d_winners, &c->d_anomaly, &c->d_prof, &c->d_negz, &c->d_xform,
                      &c->vis.d_counts, &c->vis.d_flags, &c->vis.d_pix, &c->vis.d_vis, &c->vis.d_ids,
                      &c->vis.d_temp, &c->vis.d_starts, &c->vis.d_gout, &c->sel.d_tab, &c->sel.d_out,
                      &c->sel.d_temp, &c->bnd.d_zmin, &c->bnd.d_tab, &c->bnd.d_pixels};
    for (DevBuf *b : bufs) b->release();
    for (hipEvent_t e : c->bnd.ev)
        if (e) (void)hipEventDestroy(e);
    if (c->h_xform) (void)hipHostFree(c->h_xform);
    if (c->xf_ev) (void)hipEventDestroy(c->xf_ev);
    if (c->xf_end_ev) (void)hipEventDestroy(c->xf_end_ev);
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
    if (c->s_mark) (void)hipEventDestroy(c->s_mark);
    if (c->in_ev) (void)hipEventDestroy(c->in_ev);
    if (c->read_ev) (void)hipEventDestroy(c->read_ev);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->h_total) (void)hipHostFree(c->h_total);
    for (auto &slot : c->ev)
        for (auto &e : slot)
            if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->bin_stream) (void)hipStreamDestroy(c->bin_stream);
    if (c->vis_stream) (void)hipStreamDestroy(c->vis_stream);
    delete c;
    return PRK_OK;
}

static void drop_target(prk_context *c) {
    c->z_early = false;
    if (c->owns_target) {
        (void)hipFree(c->color);
        (void)hipFree(c->zbuf);
    }
    c->color = nullptr;
    c->zbuf = nullptr;
    c->owns_target = false;
    c->W = c->H = c->row0 = c->row1 = 0;
}

int prk_target_bind(prk_context *c, void *color, int32_t pitch_bytes, float *zbuf, int32_t width,
                    int32_t height, int32_t row0, int32_t row1) {
    if (!c || !color || !zbuf || width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 >= row1 ||
        pitch_bytes < width * 4 || (pitch_bytes & 3))
        return PRK_ERR_ARG;
    // the pending frame's count first, whoever owns its target: an overflowed
    // frame is re-run into the target it was queued with before a caller
    // hands that memory to anything else (a gather, the next frame)
    RESOLVE_COUNT(c);
    drop_target(c);
    c->color = color;
    c->pitch = pitch_bytes;
    c->zbuf = zbuf;
    c->W = width;
    c->H = height;
    c->row0 = row0;
    c->row1 = row1;
    c->winners_valid = false;
    c->bnd.answered = false;  // (prk_visibility_bounds' answer was the old target's)
    return PRK_OK;
}

int prk_target_alloc(prk_context *c, int32_t width, int32_t height, int32_t row0, int32_t row1,
                     void **color_out, float **zbuf_out) {
    if (!c || width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 >= row1) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    drop_target(c);
    size_t px = (size_t)width * (row1 - row0);
    void *col = nullptr;
    float *z = nullptr;
    hipError_t e = hipMalloc(&col, px * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&z, px * 4);
    if (e != hipSuccess) {
        (void)hipFree(col);
        (void)hipFree(z);
        return status_of(e);
    }
    c->color = col;
    c->zbuf = z;
    c->pitch = width * 4;
    c->W = width;
    c->H = height;
    c->row0 = row0;
    c->row1 = row1;
    c->owns_target = true;
    c->winners_valid = false;
    c->bnd.answered = false;
    if (color_out) *color_out = col;
    if (zbuf_out) *zbuf_out = z;
    return PRK_OK;
}

int prk_target_clear(prk_context *c, uint32_t color, float z) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    c->z_early = false;  // (z written outside a frame)
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    // after a prk_target_upload_async still in flight (it would land on top)
    if (c->in_wait) PRK_TRY(hipStreamWaitEvent(c->own_stream, c->in_ev, 0));
    PRK_TRY(launch_fill_target(c->color, c->pitch, c->zbuf, c->W, c->row1 - c->row0, color, z, c->own_stream));
    return PRK_OK;
}

int prk_target_clear_on_flush(prk_context *c, uint32_t color, float z) {
    if (!c) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    c->clear_pending = true;
    c->clear_color = color;
    c->clear_z = z;
    return PRK_OK;
}

int prk_target_download(prk_context *c, uint32_t *color_host, int32_t host_pitch, float *z_host) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    int rows = c->row1 - c->row0;
    const size_t zbytes = (size_t)c->W * rows * 4;
    // A span-record frame's z is final after its k_vis: it goes down while
    // the frame shades (the copy engine holds the link while k_walk / k_pix
    // run), the colour after the frame.
    const bool early = z_host && c->z_early && c->z_slot >= 0 && c->d_negz.p;
    if (early) {
        PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->ev[c->z_slot][3], 0));
        PRK_TRY(hipMemcpyAsync(z_host, c->zbuf, zbytes, hipMemcpyDeviceToHost, c->copy_stream));
    }
    PRK_TRY(hipStreamSynchronize(c->own_stream));
    PRK_TRY(hipDeviceSynchronize());
    if (color_host)
        PRK_TRY(hipMemcpy2D(color_host, host_pitch, c->color, c->pitch, (size_t)c->W * 4, rows,
                            hipMemcpyDeviceToHost));
    if (early) {  // a -0.0 z written by k_pix after k_vis's +0.0: take z again
        uint32_t negz = 0;
        PRK_TRY(hipMemcpy(&negz, c->d_negz.p, 4, hipMemcpyDeviceToHost));
        if (negz) {
            PRK_TRY(hipMemcpy(z_host, c->zbuf, zbytes, hipMemcpyDeviceToHost));
            PRK_TRY(hipMemset(c->d_negz.p, 0, 4));
        }
    } else if (z_host) {
        PRK_TRY(hipMemcpy(z_host, c->zbuf, zbytes, hipMemcpyDeviceToHost));
    }
    return PRK_OK;
}

int prk_target_upload(prk_context *c, const uint32_t *color_host, int32_t host_pitch, const float *z_host) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    c->z_early = false;  // (z written outside a frame)
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->own_stream));
    if (c->in_wait) PRK_TRY(hipEventSynchronize(c->in_ev));  // an earlier asynchronous upload lands first
    int rows = c->row1 - c->row0;
    if (color_host)
        PRK_TRY(hipMemcpy2D(c->color, c->pitch, color_host, host_pitch, (size_t)c->W * 4, rows,
                            hipMemcpyHostToDevice));
    if (z_host) PRK_TRY(hipMemcpy(c->zbuf, z_host, (size_t)c->W * rows * 4, hipMemcpyHostToDevice));
    return PRK_OK;
}

int prk_target_upload_async(prk_context *c, const uint32_t *color_host, int32_t host_pitch, const float *z_host) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    c->z_early = false;  // (z written outside a frame)
    if (!c->color) return PRK_ERR_NO_TARGET;
    PRK_TRY(hipSetDevice(c->device));
    // after the frames already flushed (they read and write the target) and
    // whatever the context's stream holds (a clear, an earlier upload)
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipEventRecord(c->s_mark, c->own_stream));
    PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->s_mark, 0));
    const int rows = c->row1 - c->row0;
    if (color_host)
        PRK_TRY(hipMemcpy2DAsync(c->color, c->pitch, color_host, host_pitch, (size_t)c->W * 4, rows,
                                 hipMemcpyHostToDevice, c->copy_stream));
    if (z_host)
        PRK_TRY(hipMemcpyAsync(c->zbuf, z_host, (size_t)c->W * rows * 4, hipMemcpyHostToDevice, c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
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

static bool bitmap_ok(const prk_bitmap *b) {
    return b && b->Memory && b->Width > 0 && b->Height > 0 && b->Pitch >= 4 * b->Width && !(b->Pitch & 3);
}

// Copy the caller's Height rows (Pitch bytes each) into a texture holding
// Height + 1 rows, the last one the zeroed guard row that the u == 1 / v == 1
// over-read lands on: the caller's loaded_bitmap is read
// exactly as the reference reads it (Memory, Width, Height, Pitch,
// projekt.cpp:1506, 1881-1935) and never past its last row.
static hipError_t texture_fill(const Texture &t, const prk_bitmap *b) {
    hipError_t e = hipMemcpy(t.mem, b->Memory, (size_t)b->Pitch * b->Height, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t.mem + (size_t)b->Pitch * b->Height, 0, (size_t)b->Pitch);
    return e;
}

int prk_texture_create(prk_context *c, const prk_bitmap *b, int32_t *handle_out) {
    if (!c || !bitmap_ok(b) || !handle_out) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Texture t;
    t.w = b->Width;
    t.h = b->Height;
    t.pitch = b->Pitch;
    PRK_TRY(hipMalloc((void **)&t.mem, (size_t)b->Pitch * (b->Height + 1)));
    hipError_t e = texture_fill(t, b);
    if (e != hipSuccess) {
        (void)hipFree(t.mem);
        return status_of(e);
    }
    *handle_out = (int32_t)c->texs.size();
    c->texs.push_back(t);
    return PRK_OK;
}

int prk_texture_update(prk_context *c, int32_t handle, const prk_bitmap *b) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size() || !bitmap_ok(b)) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    Texture &t = c->texs[handle];
    PRK_TRY(hipDeviceSynchronize());  // frames in flight may still sample it
    if (t.w != b->Width || t.h != b->Height || t.pitch != b->Pitch) {
        uint8_t *m = nullptr;
        PRK_TRY(hipMalloc((void **)&m, (size_t)b->Pitch * (b->Height + 1)));
        (void)hipFree(t.mem);
        t.mem = m;
        t.w = b->Width;
        t.h = b->Height;
        t.pitch = b->Pitch;
    }
    PRK_TRY(texture_fill(t, b));
    return PRK_OK;
}

int prk_texture_alloc(prk_context *c, int32_t width, int32_t height, int32_t *handle_out) {
    if (!c || width <= 0 || height <= 0 || width > INT32_MAX / 4 || !handle_out) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Texture t;
    t.w = width;
    t.h = height;
    t.pitch = 4 * width;
    const size_t bytes = (size_t)t.pitch * ((size_t)height + 1);  // (the guard row with them)
    PRK_TRY(hipMalloc((void **)&t.mem, bytes));
    hipError_t e = hipMemset(t.mem, 0, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the context's streams do not wait for that stream)
    if (e != hipSuccess) {
        (void)hipFree(t.mem);
        return status_of(e);
    }
    *handle_out = (int32_t)c->texs.size();
    c->texs.push_back(t);
    return PRK_OK;
}

// A rectangle of the target's colour into a rectangle of a texture (prk.h;
// kernel: prk_tex.hip).  Ordered as prk_target_upload_async orders its copies:
// on copy_stream after read_ev (the frames already flushed wrote the target
// and sampled the texture) and after what own_stream holds (clears, uploads);
// the next flush waits for in_ev.
int prk_texture_from_target(prk_context *c, int32_t texture, int32_t x0, int32_t y0, int32_t width, int32_t height,
                            int32_t factor, int32_t dst_x, int32_t dst_y) {
    if (!c || texture < 0 || (size_t)texture >= c->texs.size()) return PRK_ERR_ARG;
    if (factor != 1 && factor != 2 && factor != 4) return PRK_ERR_ARG;
    if (width <= 0 || height <= 0 || width % factor || height % factor) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    const Texture &t = c->texs[texture];
    const int32_t dw = width / factor, dh = height / factor;
    if (x0 < 0 || (int64_t)x0 + width > c->W || y0 < c->row0 || (int64_t)y0 + height > c->row1) return PRK_ERR_ARG;
    if (dst_x < 0 || (int64_t)dst_x + dw > t.w || dst_y < 0 || (int64_t)dst_y + dh > t.h) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    const uint8_t *src = static_cast<const uint8_t *>(c->color) + (size_t)(y0 - c->row0) * c->pitch + (size_t)x0 * 4;
    uint8_t *dst = t.mem + (size_t)dst_y * t.pitch + (size_t)dst_x * 4;
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipEventRecord(c->s_mark, c->own_stream));
    PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->s_mark, 0));
    PRK_TRY(prk_tex_from_target_launch(src, (size_t)c->pitch, dst, (size_t)t.pitch, (uint32_t)dw, (uint32_t)dh, factor,
                                       c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
    return PRK_OK;
}

int prk_texture_download(prk_context *c, int32_t handle, void *memory, int32_t pitch_bytes) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size() || !memory) return PRK_ERR_ARG;
    const Texture &t = c->texs[handle];
    if (pitch_bytes < 4 * t.w || (pitch_bytes & 3)) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->copy_stream));  // every queued prk_texture_from_target runs there
    PRK_TRY(hipMemcpy2D(memory, pitch_bytes, t.mem, t.pitch, (size_t)t.w * 4, t.h, hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_texture_info(prk_context *c, int32_t handle, int32_t *width, int32_t *height, int32_t *pitch_bytes) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size()) return PRK_ERR_ARG;
    const Texture &t = c->texs[handle];
    if (width) *width = t.w;
    if (height) *height = t.h;
    if (pitch_bytes) *pitch_bytes = t.pitch;
    return PRK_OK;
}

// ---- target layers (prk.h; kernel: prk_layer.hip) -------------------------------
static Layer *layer_of(prk_context *c, int32_t handle) {
    if (!c || handle < 0 || (size_t)handle >= c->layers.size() || !c->layers[handle].live) return nullptr;
    return &c->layers[handle];
}

int prk_layer_alloc(prk_context *c, int32_t width, int32_t height, int32_t *handle_out) {
    if (!c || width <= 0 || height <= 0 || width > INT32_MAX / 4 || !handle_out) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    Layer l;
    l.w = width;
    l.h = height;
    l.pitch = 4 * width;
    l.live = true;
    const size_t px = (size_t)width * (size_t)height;
    hipError_t e = hipMalloc((void **)&l.color, px * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&l.z, px * 4);
    if (e == hipSuccess) e = hipMemset(l.color, 0, px * 4);
    if (e == hipSuccess) e = hipMemsetD32((hipDeviceptr_t)l.z, (int)0xFF7FFFFFu, px);  // -FLT_MAX
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the context's streams do not wait for that stream)
    if (e != hipSuccess) {
        (void)hipFree(l.color);
        (void)hipFree(l.z);
        return status_of(e);
    }
    *handle_out = (int32_t)c->layers.size();
    c->layers.push_back(l);
    return PRK_OK;
}

int prk_layer_wrap_device(prk_context *c, const void *color, int32_t pitch_bytes, const float *zbuf, int32_t width,
                          int32_t height, int32_t *handle_out) {
    if (!c || !color || !zbuf || width <= 0 || height <= 0 || width > INT32_MAX / 4 || !handle_out) return PRK_ERR_ARG;
    if (pitch_bytes < 4 * width || (pitch_bytes & 3)) return PRK_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(color) & 3) || (reinterpret_cast<uintptr_t>(zbuf) & 3)) return PRK_ERR_ARG;
    Layer l;
    l.color = static_cast<uint8_t *>(const_cast<void *>(color));  // (never written: no call takes it as destination)
    l.z = const_cast<float *>(zbuf);
    l.w = width;
    l.h = height;
    l.pitch = pitch_bytes;
    l.wrapped = l.live = true;
    *handle_out = (int32_t)c->layers.size();
    c->layers.push_back(l);
    return PRK_OK;
}

// Do a layer's rectangle at (lx, ly) and the target's at frame pixel (x0, y0), both width x height, lie inside?
static bool layer_rects_ok(const prk_context *c, const Layer &l, int32_t lx, int32_t ly, int32_t x0, int32_t y0,
                           int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return false;
    if (x0 < 0 || (int64_t)x0 + width > c->W || y0 < c->row0 || (int64_t)y0 + height > c->row1) return false;
    return lx >= 0 && (int64_t)lx + width <= l.w && ly >= 0 && (int64_t)ly + height <= l.h;
}

// One pass between a layer's rectangle at (lx, ly) and the target's at frame
// pixel (x0, y0): rule < 0 saves target to layer, else the layer goes to the
// target under rule.  Ordered as prk_texture_from_target: on copy_stream
// after read_ev (the frames already flushed) and after what own_stream holds
// (clears, uploads); the next flush, clear, upload or layer call waits for
// in_ev.
static int layer_pass(prk_context *c, const Layer &l, int32_t lx, int32_t ly, int32_t x0, int32_t y0, int32_t width,
                      int32_t height, int32_t rule) {
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    const size_t toff = (size_t)(y0 - c->row0) * c->W + (size_t)x0, loff = (size_t)ly * l.w + (size_t)lx;
    uint8_t *tc = static_cast<uint8_t *>(c->color) + (size_t)(y0 - c->row0) * c->pitch + (size_t)x0 * 4;
    uint8_t *lc = l.color + (size_t)ly * l.pitch + (size_t)lx * 4;
    float *tz = c->zbuf + toff, *lz = l.z + loff;
    const size_t tzp = (size_t)c->W * 4, lzp = (size_t)l.w * 4;
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipEventRecord(c->s_mark, c->own_stream));
    PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->s_mark, 0));
    if (rule < 0)
        PRK_TRY(prk_layer_launch(tc, (size_t)c->pitch, tz, tzp, lc, (size_t)l.pitch, lz, lzp, (uint32_t)width,
                                 (uint32_t)height, PRK_MERGE_COPY, c->copy_stream));
    else
        PRK_TRY(prk_layer_launch(lc, (size_t)l.pitch, lz, lzp, tc, (size_t)c->pitch, tz, tzp, (uint32_t)width,
                                 (uint32_t)height, rule, c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
    return PRK_OK;
}

int prk_layer_from_target(prk_context *c, int32_t layer, int32_t x0, int32_t y0, int32_t width, int32_t height,
                          int32_t dst_x, int32_t dst_y) {
    const Layer *l = layer_of(c, layer);
    if (!l || l->wrapped) return PRK_ERR_ARG;
    if (width <= 0 || height <= 0) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (!layer_rects_ok(c, *l, dst_x, dst_y, x0, y0, width, height)) return PRK_ERR_ARG;
    return layer_pass(c, *l, dst_x, dst_y, x0, y0, width, height, -1);
}

int prk_target_from_layer(prk_context *c, int32_t layer, int32_t src_x, int32_t src_y, int32_t width, int32_t height,
                          int32_t x0, int32_t y0, int32_t rule) {
    const Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    if (rule != PRK_MERGE_COPY && rule != PRK_MERGE_GREATER && rule != PRK_MERGE_GREATER_EQUAL) return PRK_ERR_ARG;
    if (width <= 0 || height <= 0) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    if (!layer_rects_ok(c, *l, src_x, src_y, x0, y0, width, height)) return PRK_ERR_ARG;
    c->z_early = false;  // (z written outside a frame)
    return layer_pass(c, *l, src_x, src_y, x0, y0, width, height, rule);
}

int prk_layer_download(prk_context *c, int32_t layer, uint32_t *color_host, int32_t host_pitch, float *z_host) {
    const Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    if (color_host && (host_pitch < 4 * l->w || (host_pitch & 3))) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->copy_stream));  // every queued layer call runs there
    if (color_host)
        PRK_TRY(hipMemcpy2D(color_host, host_pitch, l->color, l->pitch, (size_t)l->w * 4, l->h, hipMemcpyDeviceToHost));
    if (z_host) PRK_TRY(hipMemcpy(z_host, l->z, (size_t)l->w * l->h * 4, hipMemcpyDeviceToHost));
    return PRK_OK;
}

int prk_layer_info(prk_context *c, int32_t layer, int32_t *width, int32_t *height, int32_t *pitch_bytes,
                   int32_t *wrapped) {
    const Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    if (width) *width = l->w;
    if (height) *height = l->h;
    if (pitch_bytes) *pitch_bytes = l->pitch;
    if (wrapped) *wrapped = l->wrapped ? 1 : 0;
    return PRK_OK;
}

int prk_layer_destroy(prk_context *c, int32_t layer) {
    Layer *l = layer_of(c, layer);
    if (!l) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipDeviceSynchronize());  // frames in flight and queued layer calls first
    if (!l->wrapped) {
        (void)hipFree(l->color);
        (void)hipFree(l->z);
    }
    *l = Layer();  // (the slot stays, dead)
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

int prk_texture_set_filter(prk_context *c, int32_t handle, int32_t filter) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size()) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (filter != PRK_FILTER_NEAREST && filter != PRK_FILTER_BILINEAR) return PRK_ERR_ARG;
    c->texs[handle].filter = filter;
    return PRK_OK;
}

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
        (void)hipFree((void *)g.V);
        (void)hipFree((void *)g.C);
        (void)hipFree((void *)g.N);
        (void)hipFree((void *)g.UV);
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
    const size_t comp[4] = {3, 4, 3, 2};
    for (int k = 0; k < 4; ++k) {  // an array passed as null keeps its previous contents
        const size_t bytes = (size_t)vertex_count * comp[k] * sizeof(float);
        if (!src[k]) {
            // ... and grows with the vertex count: its first cap[k] vertices
            // kept, the new ones zero, so no draw reads past its allocation.
            if (*dst[k] && vertex_count > g.cap[k]) {
                const size_t old = (size_t)g.cap[k] * comp[k] * sizeof(float);
                float *d = nullptr;
                PRK_TRY(hipMalloc((void **)&d, bytes));
                hipError_t e = hipMemcpy(d, *dst[k], old, hipMemcpyDeviceToDevice);
                if (e == hipSuccess) e = hipMemset((uint8_t *)d + old, 0, bytes - old);
                if (e != hipSuccess) {
                    (void)hipFree(d);
                    return status_of(e);
                }
                (void)hipFree((void *)*dst[k]);
                *dst[k] = d;
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
    const size_t comp[4] = {3, 4, 3, 2};
    const bool given[4] = {v != nullptr, col != nullptr, n != nullptr, uv != nullptr};
    {
        const int rc = geometry_grow(c, handle, given, end);
        if (rc != PRK_OK) return rc;
    }
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if (!src[k] || !vertex_count) continue;
        const size_t off = (size_t)first_vertex * comp[k];
        PRK_TRY(hipMemcpyAsync((void *)(*dst[k] + off), src[k], (size_t)vertex_count * comp[k] * sizeof(float),
                               hipMemcpyHostToDevice, c->copy_stream));
        any = true;
    }
    if (any) {
        PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
        c->in_wait = true;
    }
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
    const size_t comp[4] = {3, 4, 3, 2};
    bool grow = false;
    for (int k = 0; k < 4; ++k) grow |= (want[k] || *dst[k]) && end > g.cap[k];
    if (grow) {
        PRK_TRY(hipDeviceSynchronize());  // frames in flight and earlier writes read / fill the old buffers
        for (int k = 0; k < 4; ++k) {
            if (!(want[k] || *dst[k]) || end <= g.cap[k]) continue;
            const uint64_t need = std::max<uint64_t>(end, (uint64_t)g.cap[k] + g.cap[k] / 2);
            const uint32_t cap = (uint32_t)std::min<uint64_t>(need, 0xFFFFFFF0ull);
            const size_t bytes = (size_t)cap * comp[k] * sizeof(float);
            const size_t old = *dst[k] ? (size_t)g.cap[k] * comp[k] * sizeof(float) : 0;
            float *d = nullptr;
            PRK_TRY(hipMalloc((void **)&d, bytes));
            hipError_t e = old ? hipMemcpy(d, *dst[k], old, hipMemcpyDeviceToDevice) : hipSuccess;
            if (e == hipSuccess) e = hipMemset((uint8_t *)d + old, 0, bytes - old);
            if (e != hipSuccess) {
                (void)hipFree(d);
                return status_of(e);
            }
            (void)hipFree((void *)*dst[k]);
            *dst[k] = d;
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
    g.V = v;
    g.C = col;
    g.N = n;
    g.UV = uv;
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
// table layout: prk_xform.hip).  Ordered as prk_geometry_write orders its
// copies: on copy_stream after read_ev, the next flush waits for in_ev.
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
    // the tables: scan (nruns + 1 words), runs, matrices (prk_xform.hip)
    const size_t runs_off = ((size_t)(nruns + 1) * 4 + 15) & ~(size_t)15;
    const size_t xf_off = runs_off + (size_t)nruns * 16;
    const size_t bytes = xf_off + (size_t)xform_count * sizeof(prk_xform);
    if (c->xf_busy) {  // the staging's previous contents have been copied
        PRK_TRY(hipEventSynchronize(c->xf_ev));
        c->xf_busy = false;
    }
    if (bytes > c->h_xform_cap) {
        if (c->h_xform) (void)hipHostFree(c->h_xform);
        c->h_xform = nullptr;
        c->h_xform_cap = 0;
        const size_t want = bytes + bytes / 4;
        PRK_TRY(hipHostMalloc(&c->h_xform, want, hipHostMallocDefault));
        c->h_xform_cap = want;
    }
    if (!c->xf_ev) PRK_TRY(hipEventCreate(&c->xf_ev));
    if (!c->xf_end_ev) PRK_TRY(hipEventCreate(&c->xf_end_ev));
    {
        uint8_t *h = static_cast<uint8_t *>(c->h_xform);
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
    {
        const int rc = geometry_grow(c, dst, has, end);
        if (rc != PRK_OK) return rc;
    }
    Geometry &d = c->geoms[dst];
    PRK_TRY(c->d_xform.ensure(bytes));  // (a larger buffer: hipFree waits for the kernels that read the old one)
    if (c->read_rec) PRK_TRY(hipStreamWaitEvent(c->copy_stream, c->read_ev, 0));
    PRK_TRY(hipMemcpyAsync(c->d_xform.p, c->h_xform, bytes, hipMemcpyHostToDevice, c->copy_stream));
    PRK_TRY(hipEventRecord(c->xf_ev, c->copy_stream));
    c->xf_busy = true;
    PRK_TRY(prk_xform_launch(c->d_xform.p, runs_off, xf_off, nruns, (uint32_t)total, s.V, s.C, s.N, s.UV,
                             (float *)d.V, (float *)d.C, (float *)d.N, (float *)d.UV, c->copy_stream));
    PRK_TRY(hipEventRecord(c->xf_end_ev, c->copy_stream));
    PRK_TRY(hipEventRecord(c->in_ev, c->copy_stream));
    c->in_wait = true;
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
    if (!c || !kernel_ms || !c->xf_busy) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipEventSynchronize(c->xf_end_ev));
    PRK_TRY(hipEventElapsedTime(kernel_ms, c->xf_ev, c->xf_end_ev));
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
    const size_t comp[4] = {3, 4, 3, 2};
    for (int k = 0; k < 4; ++k)
        if (dst[k] && !src[k]) return PRK_ERR_ARG;
    PRK_TRY(hipSetDevice(c->device));
    PRK_TRY(hipStreamSynchronize(c->copy_stream));  // every queued write of a geometry runs there
    for (int k = 0; k < 4; ++k) {
        if (!dst[k] || !vertex_count) continue;
        PRK_TRY(hipMemcpy(dst[k], src[k] + (size_t)first_vertex * comp[k],
                          (size_t)vertex_count * comp[k] * sizeof(float), hipMemcpyDeviceToHost));
    }
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
    const int rc = draw_src(c, 3, off, (uint32_t)total, list_count, semantics, phong, texture);
    if (rc != PRK_OK) return rc;
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
