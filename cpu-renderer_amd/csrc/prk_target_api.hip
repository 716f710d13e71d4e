// prk_target_api.hip — the render target, textures and target layers of prk.h
// (DESIGN.md §2.2, §2.3), one of the host files over prk_ctx.h.  What touches the
// target between frames (prk_target_upload_async, prk_texture_from_target, the
// layer passes) is a side pass in the target form (prk_ctx.h: side_begin).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prk_ctx.h"

// Does the width x height rectangle at frame pixel (x0, y0) lie inside the target's band?
static bool target_rect_ok(const prk_context *c, int32_t x0, int32_t y0, int32_t width, int32_t height) {
    return x0 >= 0 && (int64_t)x0 + width <= c->W && y0 >= c->row0 && (int64_t)y0 + height <= c->row1;
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

// The context's target from now on; what was answered for the one before goes with it.
static void set_target(prk_context *c, void *color, int32_t pitch, float *zbuf, int32_t width, int32_t height,
                       int32_t row0, int32_t row1, bool owned) {
    drop_target(c);
    c->color = color;
    c->pitch = pitch;
    c->zbuf = zbuf;
    c->W = width;
    c->H = height;
    c->row0 = row0;
    c->row1 = row1;
    c->owns_target = owned;
    c->winners_valid = false;
    c->bnd.answered = false;  // (prk_visibility_bounds' answer was the old target's)
}

// What a call that writes the target outside a frame does first.
static int target_write_begin(prk_context *c) {
    if (!c) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    c->z_early = false;  // (z written outside a frame)
    if (!c->color) return PRK_ERR_NO_TARGET;
    return status_of(hipSetDevice(c->device));
}

extern "C" {

int prk_target_bind(prk_context *c, void *color, int32_t pitch_bytes, float *zbuf, int32_t width,
                    int32_t height, int32_t row0, int32_t row1) {
    if (!c || !color || !zbuf || width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 >= row1 ||
        pitch_bytes < width * 4 || (pitch_bytes & 3))
        return PRK_ERR_ARG;
    // the pending frame's count first, whoever owns its target: an overflowed
    // frame is re-run into the target it was queued with before a caller
    // hands that memory to anything else (a gather, the next frame)
    RESOLVE_COUNT(c);
    set_target(c, color, pitch_bytes, zbuf, width, height, row0, row1, false);
    return PRK_OK;
}

int prk_target_alloc(prk_context *c, int32_t width, int32_t height, int32_t row0, int32_t row1,
                     void **color_out, float **zbuf_out) {
    if (!c || width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 >= row1) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    drop_target(c);  // (before the new one is allocated: a failure leaves no target)
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
    set_target(c, col, width * 4, z, width, height, row0, row1, true);
    if (color_out) *color_out = col;
    if (zbuf_out) *zbuf_out = z;
    return PRK_OK;
}

int prk_target_clear(prk_context *c, uint32_t color, float z) {
    PRK_CHECK(target_write_begin(c));
    // after a prk_target_upload_async still in flight (it would land on top)
    PRK_TRY(side_wait(c, c->own_stream));
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
    PRK_CHECK(target_write_begin(c));
    PRK_TRY(hipStreamSynchronize(c->own_stream));
    // side_wait's join on the host (the copies below are synchronous): an earlier side pass lands first
    if (c->in_wait) PRK_TRY(hipEventSynchronize(c->in_ev));
    int rows = c->row1 - c->row0;
    if (color_host)
        PRK_TRY(hipMemcpy2D(c->color, c->pitch, color_host, host_pitch, (size_t)c->W * 4, rows,
                            hipMemcpyHostToDevice));
    if (z_host) PRK_TRY(hipMemcpy(c->zbuf, z_host, (size_t)c->W * rows * 4, hipMemcpyHostToDevice));
    return PRK_OK;
}

int prk_target_upload_async(prk_context *c, const uint32_t *color_host, int32_t host_pitch, const float *z_host) {
    PRK_CHECK(target_write_begin(c));
    // after the frames already flushed (they read and write the target) and
    // whatever the context's stream holds (a clear, an earlier upload)
    PRK_TRY(side_begin(c, true));
    const int rows = c->row1 - c->row0;
    if (color_host)
        PRK_TRY(hipMemcpy2DAsync(c->color, c->pitch, color_host, host_pitch, (size_t)c->W * 4, rows,
                                 hipMemcpyHostToDevice, c->copy_stream));
    if (z_host)
        PRK_TRY(hipMemcpyAsync(c->zbuf, z_host, (size_t)c->W * rows * 4, hipMemcpyHostToDevice, c->copy_stream));
    PRK_TRY(side_end(c));
    return PRK_OK;
}

// ---- textures ---------------------------------------------------------------------
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

int prk_texture_set_filter(prk_context *c, int32_t handle, int32_t filter) {
    if (!c || handle < 0 || (size_t)handle >= c->texs.size()) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    if (filter != PRK_FILTER_NEAREST && filter != PRK_FILTER_BILINEAR) return PRK_ERR_ARG;
    c->texs[handle].filter = filter;
    return PRK_OK;
}

// A rectangle of the target's colour into a rectangle of a texture (prk.h;
// kernel: prk_tex.hip).  A side pass in the target form: the frames already
// flushed wrote the target and sampled the texture.
int prk_texture_from_target(prk_context *c, int32_t texture, int32_t x0, int32_t y0, int32_t width, int32_t height,
                            int32_t factor, int32_t dst_x, int32_t dst_y) {
    if (!c || texture < 0 || (size_t)texture >= c->texs.size()) return PRK_ERR_ARG;
    if (factor != 1 && factor != 2 && factor != 4) return PRK_ERR_ARG;
    if (width <= 0 || height <= 0 || width % factor || height % factor) return PRK_ERR_ARG;
    if (!c->color) return PRK_ERR_NO_TARGET;
    const Texture &t = c->texs[texture];
    const int32_t dw = width / factor, dh = height / factor;
    if (!target_rect_ok(c, x0, y0, width, height)) return PRK_ERR_ARG;
    if (dst_x < 0 || (int64_t)dst_x + dw > t.w || dst_y < 0 || (int64_t)dst_y + dh > t.h) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    const uint8_t *src = static_cast<const uint8_t *>(c->color) + (size_t)(y0 - c->row0) * c->pitch + (size_t)x0 * 4;
    uint8_t *dst = t.mem + (size_t)dst_y * t.pitch + (size_t)dst_x * 4;
    PRK_TRY(side_begin(c, true));
    PRK_TRY(prk_tex_from_target_launch(src, (size_t)c->pitch, dst, (size_t)t.pitch, (uint32_t)dw, (uint32_t)dh, factor,
                                       c->copy_stream));
    PRK_TRY(side_end(c));
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
    if (width <= 0 || height <= 0 || !target_rect_ok(c, x0, y0, width, height)) return false;
    return lx >= 0 && (int64_t)lx + width <= l.w && ly >= 0 && (int64_t)ly + height <= l.h;
}

// One pass between a layer's rectangle at (lx, ly) and the target's at frame
// pixel (x0, y0): rule < 0 saves target to layer, else the layer goes to the
// target under rule.  A side pass in the target form, as
// prk_texture_from_target: the next flush, clear, upload or layer call comes
// after it.
static int layer_pass(prk_context *c, const Layer &l, int32_t lx, int32_t ly, int32_t x0, int32_t y0, int32_t width,
                      int32_t height, int32_t rule) {
    RESOLVE_COUNT(c);
    PRK_TRY(hipSetDevice(c->device));
    const size_t toff = (size_t)(y0 - c->row0) * c->W + (size_t)x0, loff = (size_t)ly * l.w + (size_t)lx;
    uint8_t *tc = static_cast<uint8_t *>(c->color) + (size_t)(y0 - c->row0) * c->pitch + (size_t)x0 * 4;
    uint8_t *lc = l.color + (size_t)ly * l.pitch + (size_t)lx * 4;
    float *tz = c->zbuf + toff, *lz = l.z + loff;
    const size_t tzp = (size_t)c->W * 4, lzp = (size_t)l.w * 4;
    PRK_TRY(side_begin(c, true));
    if (rule < 0)
        PRK_TRY(prk_layer_launch(tc, (size_t)c->pitch, tz, tzp, lc, (size_t)l.pitch, lz, lzp, (uint32_t)width,
                                 (uint32_t)height, PRK_MERGE_COPY, c->copy_stream));
    else
        PRK_TRY(prk_layer_launch(lc, (size_t)l.pitch, lz, lzp, tc, (size_t)c->pitch, tz, tzp, (uint32_t)width,
                                 (uint32_t)height, rule, c->copy_stream));
    PRK_TRY(side_end(c));
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

}  // extern "C"
