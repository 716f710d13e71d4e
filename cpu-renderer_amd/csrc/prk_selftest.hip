// prk_selftest.hip — the self-tests of prk.h (prk_selftest_*), one of the host
// files over prk_ctx.h: device primitives and the launchers the calls themselves
// queue (prk_launch.h), run on the caller's words with no context, synchronously,
// on `device`; every buffer handed to a launcher is guarded (GuardedBuf).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "prk_ctx.h"

namespace {
// A device buffer of `bytes` payload bytes and kGuardBytes of kGuardByte after
// them, filled and read with copies only.  Its role is the bit of the damage
// word it feeds: an input must come back as it was filled, guard included; an
// output or a temporary must come back with its guard.
constexpr size_t kGuardBytes = 4096;
constexpr unsigned char kGuardByte = 0xA5;
constexpr uint32_t kInput = PRK_DAMAGE_INPUT, kOutput = PRK_DAMAGE_OUTPUT_GUARD, kTemp = PRK_DAMAGE_TEMP_GUARD;
struct GuardedBuf {
    uint32_t role;
    char *p = nullptr;
    size_t bytes = 0;
    const void *src = nullptr;        // what the payload was last filled from (null: the pattern)
    std::vector<unsigned char> host;  // what the buffer was last filled with, then what it holds
    ~GuardedBuf() {
        if (p) (void)hipFree(p);
    }
    // the pattern everywhere, then `from` (may be null) over the payload
    hipError_t fill(size_t payload, const void *from) {
        if (!p) {
            bytes = payload;
            const hipError_t e = hipMalloc(&p, bytes + kGuardBytes);
            if (e != hipSuccess) return e;
        }
        src = from;
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
    bool intact() const {  // (an input: the payload too)
        return (role != kInput || bytes == 0 || std::memcmp(host.data(), src, bytes) == 0) && guard_intact();
    }
};

// The buffers read back in the order given, then the damage word they make.
hipError_t read_back(std::initializer_list<GuardedBuf *> all, uint32_t *damage) {
    for (GuardedBuf *b : all) {
        const hipError_t e = b->read();
        if (e != hipSuccess) return e;
    }
    uint32_t d = 0;
    for (const GuardedBuf *b : all)
        if (!b->intact()) d |= b->role;
    *damage = d;
    return hipSuccess;
}
}  // namespace

extern "C" {

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
    PRK_CHECK(use_device(device, n != 0));  // (no words: the device is checked, not made current)
    if (n == 0) return PRK_OK;
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
    PRK_CHECK(use_device(device));
    const size_t kb = (size_t)n * 8, vb = (size_t)n * 4;
    GuardedBuf kin{kInput}, vin{kInput}, kout{kOutput}, vout{kOutput}, temp{kTemp};
    PRK_TRY(kin.fill(kb, keys));
    PRK_TRY(vin.fill(vb, vals));
    PRK_TRY(temp.fill(tb, nullptr));
    for (uint32_t r = 0; r < repeats; ++r) {
        PRK_TRY(kout.fill(kb, nullptr));
        PRK_TRY(vout.fill(vb, nullptr));
        PRK_TRY(prk_obj_sort(kin.p, (uint32_t *)vin.p, kout.p, (uint32_t *)vout.p, n, end_bit, temp.p, &tb, nullptr));
        PRK_TRY(hipDeviceSynchronize());
    }
    PRK_TRY(read_back({&kin, &vin, &kout, &vout, &temp}, damage));
    if (n) {
        std::memcpy(keys_out, kout.host.data(), kb);
        std::memcpy(vals_out, vout.host.data(), vb);
    }
    return PRK_OK;
}

// An exclusive scan on the caller's words (prk.h), in and out distinct.
int prk_selftest_scan(int32_t device, int32_t width, uint32_t n, const void *in, void *out, uint32_t *damage) {
    if (device < 0 || (width != 32 && width != 64) || !in || !out || !damage) return PRK_ERR_ARG;
    PRK_CHECK(use_device(device));
    const size_t bytes = (size_t)n * (size_t)(width / 8);
    size_t tb = 0;
    GuardedBuf din{kInput}, dout{kOutput}, temp{kTemp};
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
    PRK_TRY(read_back({&din, &dout, &temp}, damage));
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
    PRK_CHECK(use_device(device));
    const size_t wb = (size_t)n * 4, ib = (size_t)id_count * 4, mb = ib + 4;
    size_t tb = 0;
    PRK_TRY(prk_vis_reduce(nullptr, n, id_count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &tb, nullptr,
                           nullptr));
    GuardedBuf win{kInput}, cnt{kOutput}, flg{kTemp}, pix{kOutput}, vis{kOutput}, idl{kOutput}, temp{kTemp},
        nat{kOutput};
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
    PRK_TRY(read_back({&win, &cnt, &flg, &pix, &vis, &idl, &temp, &nat}, damage));
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
    for (int k = 0; k < 4; ++k)
        if (src[k] && !dst[k]) return PRK_ERR_ARG;
    uint64_t worst = 0;
    PRK_CHECK(select_check(items, item_count, levels, level_count, xforms, xform_count, src_tris,
                           item_pixels ? nullptr : &id_count, &worst));
    if (worst && !src_vertices) return PRK_ERR_ARG;
    if (worst > (1ull << 31)) return PRK_ERR_LIMIT;
    if ((uint64_t)dst_first_tri + worst > dst_tris || (uint64_t)dst_tris * 3 > 0xFFFFFFF0ull) return PRK_ERR_ARG;
    PRK_CHECK(use_device(device));
    const size_t wb = ((size_t)item_count + 1) * 4;
    size_t tb = 0;
    PRK_TRY(prk_scan_u32(nullptr, nullptr, item_count + 1, nullptr, &tb, nullptr));
    GuardedBuf pix{kInput}, itm{kInput}, lev{kInput}, xfm{kInput}, ipx{kInput},
        sa[4] = {{kInput}, {kInput}, {kInput}, {kInput}}, da[4] = {{kOutput}, {kOutput}, {kOutput}, {kOutput}},
        cho{kOutput}, cnt{kTemp}, sta{kOutput}, run{kTemp}, temp{kTemp};
    PRK_TRY(pix.fill(item_pixels ? 0 : ((size_t)id_count + 1) * 4, pix_prefix));
    PRK_TRY(itm.fill((size_t)item_count * sizeof(prk_select_item), items));
    PRK_TRY(lev.fill(levels ? (size_t)level_count * sizeof(prk_select_level) : 0, levels));
    PRK_TRY(xfm.fill(xforms ? (size_t)xform_count * sizeof(prk_xform) : 0, xforms));
    PRK_TRY(ipx.fill(item_pixels ? (size_t)item_count * 4 : 0, item_pixels));
    for (int k = 0; k < 4; ++k) {
        PRK_TRY(sa[k].fill(src[k] ? (size_t)src_tris * 3 * kGeomComp[k] * 4 : 0, src[k]));
        PRK_TRY(da[k].fill(src[k] ? (size_t)dst_tris * 3 * kGeomComp[k] * 4 : 0, nullptr));
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
    PRK_TRY(read_back({&pix, &itm, &lev, &xfm, &ipx, &sa[0], &sa[1], &sa[2], &sa[3], &da[0], &da[1], &da[2], &da[3],
                       &cho, &cnt, &sta, &run, &temp},
                      damage));
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
    PRK_CHECK(use_device(device));
    const size_t npx = (size_t)width * (size_t)(row1 - row0), nt = (size_t)B.tiles_x * (size_t)B.tiles_y;
    std::vector<float> zin(z_offset + npx, 0.0f);
    std::memcpy(zin.data() + z_offset, z, npx * 4);
    GuardedBuf zb{kInput}, xfm{kInput}, bnd{kInput}, zmn{kOutput}, pix{kOutput};
    PRK_TRY(zb.fill(zin.size() * 4, zin.data()));
    PRK_TRY(xfm.fill(count ? (size_t)xform_count * sizeof(prk_xform) : 0, xforms));
    PRK_TRY(bnd.fill((size_t)count * sizeof(prk_bound), bounds));
    PRK_TRY(zmn.fill(nt * 4, nullptr));
    PRK_TRY(pix.fill((size_t)count * 4, nullptr));
    PRK_TRY(prk_ztile_min((const float *)zb.p + z_offset, &B, (float *)zmn.p, nullptr));
    PRK_TRY(prk_bounds_test((const prk_bound *)bnd.p, count, (const prk_xform *)xfm.p, &B, (const float *)zmn.p,
                            (uint32_t *)pix.p, nullptr));
    PRK_TRY(hipDeviceSynchronize());
    PRK_TRY(read_back({&zb, &xfm, &bnd, &zmn, &pix}, damage));
    std::memcpy(zmin, zmn.host.data(), nt * 4);
    if (count) std::memcpy(pixels, pix.host.data(), (size_t)count * 4);
    return PRK_OK;
}

}  // extern "C"
