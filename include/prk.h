/*
 * prk.h — C-ABI of the MI355X-native rasterizer (libprk_hip.so).
 *
 * This is the drop-in boundary for the reference's ONE hot path:
 *
 *     FillEdgeTable            projekt.cpp:3882-4121   (triangle setup)
 *     DrawModelOptimized(Queue) projekt.cpp:3615-3871  (AET walk, per-span tasks)
 *       -> FillLineOptimized   projekt.cpp:1492-2320   (8-px AVX span kernel)
 *     DrawModel                projekt.cpp:162-601     (scalar span kernel)
 *     Platform.CompleteAllWork (absent platform layer, inferred from
 *                               projekt.cpp:3609,3809)
 *
 * The reference exports nothing (every function is `internal`), so the
 * boundary is the set of C++ signatures above plus the caller-owned types
 * they take.  `include/projekt.h` re-declares those C++ signatures and
 * forwards them to the plain-C entry points below.  Signatures here use only
 * plain pointers, sizes and POD structs; no torch or HIP types.
 *
 * Every prk_* function returns an int status (PRK_OK == 0, negative on
 * error) — the reference has no error convention at all (Assert only,
 * projekt.cpp:2327), and crashes on several ordinary inputs;
 * here those inputs are rejected with a status code instead.
 *
 * Semantics: prk_draw submits every triangle as its own AET
 * (one render_entry_3d_object per triangle, "per-triangle submission", SURVEY
 * §0.6); prk_draw_objects submits objects of several triangles, each one AET
 * as FillEdgeTable + DrawModel* build it.  Draws run in submission order and
 * share one z-buffer.
 */
#ifndef PRK_H
#define PRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRK_MAX_LIGHTS 8

enum prk_status {
    PRK_OK = 0,
    PRK_ERR_ARG = -1,          /* bad pointer / size / handle            */
    PRK_ERR_UNSUPPORTED = -2,  /* combination the reference leaves undefined */
    PRK_ERR_DEVICE = -3,       /* HIP runtime error                      */
    PRK_ERR_NOMEM = -4,        /* device allocation failed               */
    PRK_ERR_NO_TARGET = -5,    /* flush without a render target          */
    PRK_ERR_LIMIT = -6,        /* beyond this build's index capacity (more than
                                  2^31 edges, span slots or bin entries in one
                                  pass): a limit of the build, not of the input */
    PRK_ERR_RUNTIME_MIX = -7   /* two copies of the ROCm runtime are mapped in
                                  this process (e.g. /opt/rocm's, pulled in by
                                  this library, and torch's own, loaded after
                                  it): see prk_create */
};

/* Which of the reference's span kernels a draw reproduces. */
enum prk_semantics {
    PRK_SEM_SCALAR = 0,  /* DrawModel            projekt.cpp:162-601   */
    PRK_SEM_AVX = 1,     /* FillLineOptimized    projekt.cpp:1492-2320, driven by
                            DrawModelOptimized(RenderQueue,...) 3615-3871, or by
                            DrawModelOptimizedLines 3362-3613 (FillLinesOptimized
                            629-1490 has the same block math) */
    PRK_SEM_AVX_ST = 2   /* the single-thread overload DrawModelOptimized(Buffer,...)
                            2350-3358: FillLineOptimized's math with two quirks:
                            a left-clipped span keeps XOffset = -0.0f (2508) and the
                            z-test is z >= zbuf (predicate 29, 3205): among equal z
                            the latest fragment wins */
};

/* Texture sampling of a texture handle (prk_texture_set_filter).  The
 * reference samples the nearest texel only (projekt.cpp:1881-2032);
 * PRK_FILTER_BILINEAR is an EXTENSION of this build for the AVX semantics
 * (BASELINE config 4) with its own definition: weights from
 * texel centres at +0.5, clamp to the edge, fp32.  DrawModel (scalar)
 * draws always sample nearest. */
enum prk_filter {
    PRK_FILTER_NEAREST = 0,
    PRK_FILTER_BILINEAR = 1
};

/* projective_transform (absent header; fields as used at projekt.cpp:77-90,
 * 122-141, 152-155). */
typedef struct prk_transform {
    float DistanceAboveTarget;
    float FocalLength;
    float MetersToPixels;
    float ScreenCenter[2];
} prk_transform;

/* light_info / light_data (absent header; projekt.cpp:452-484, 2046-2128,
 * 3885, 4025-4061). */
typedef struct prk_light_info {
    float P[3];
    float Intensity[4]; /* r g b a */
} prk_light_info;

typedef struct prk_light_data {
    uint32_t LightCount;
    float AmbientIntensity[4]; /* r g b a */
    prk_light_info Lights[PRK_MAX_LIGHTS];
} prk_light_data;

/* loaded_bitmap (absent header): 0xAARRGGBB texels, Pitch in bytes.  For a
 * texture, Memory holds Height rows; the library appends the zeroed "guard"
 * row the reference's u==1 / v==1 over-read lands on (SURVEY App. A.2.3,
 * prk_texture_create below). */
typedef struct prk_bitmap {
    void *Memory;
    int32_t Width;
    int32_t Height;
    int32_t Pitch;
} prk_bitmap;

/* Frame statistics.  Kernel times come from HIP events recorded on the
 * launch stream around the binning and raster kernels of every flush; they
 * are harvested without stalling the stream and accumulated until
 * prk_timing_reset. */
typedef struct prk_stats {
    uint64_t triangles;      /* triangles of the last flush            */
    uint64_t bin_entries;    /* (triangle, tile) pairs of the last flush */
    uint32_t tiles;          /* tiles in the render target band        */
    uint32_t frames_timed;   /* flushes accumulated in sum_ms_*        */
    float ms_bin;            /* last flush: project/cull/bin kernels   */
    float ms_raster;         /* last flush: k_vis + shading kernels    */
    double sum_ms_bin;       /* accumulated since prk_timing_reset     */
    double sum_ms_raster;
    uint32_t anomalies;      /* triangles whose AET left the proven
                                per-triangle shape (always 0) */
    uint32_t slow_replays;   /* bin entries whose rows above their tile were
                                replayed row by row (irregular edge list or
                                an X tie); cumulative like
                                anomalies */
    double sum_ms_vis;       /* accumulated: the k_vis (visibility) part
                                of sum_ms_raster */
    double sum_ms_span;      /* accumulated: the k_walk part (AVX frames:
                                raster = k_vis + k_walk + k_pix) */
    uint32_t objects_chunked; /* large objects (48+ triangles) whose AET walk
                                 ran as chunks of rows walked at once, each
                                 from its first row's sorted list, checked and
                                 walked again where that was not the true
                                 list; cumulative */
    uint32_t objects_walked;  /* large objects walked row after row from the
                                 first (an odd row, a NaN key, lists past the
                                 LDS); cumulative */
    uint32_t object_chunks;   /* the chunked walk's chunks; cumulative */
    uint32_t object_chunks_rewalked; /* ... walked a second time (their start
                                 was not the true list); cumulative */
} prk_stats;

typedef struct prk_context prk_context;

/* Library / device lifetime.
 * prk_create checks that the process maps ONE copy of libamdhip64 and of
 * librocm_smi64.  A host that loads this library (and so /opt/rocm's
 * runtime, plus its RCCL once prk_comm_* runs) before a framework that ships
 * its own copies under other names (torch) ends up with two; their
 * librocm_smi64 copies then free one interposed static map twice at exit
 * (glibc "double free", SIGABRT).  prk_create returns
 * PRK_ERR_RUNTIME_MIX then, names the fix on stderr (load the framework
 * before libprk_hip.so), and guards the exit: an on_exit handler registered
 * after both copies' destructors flushes stdio and ends the process with its
 * own exit status before those destructors run.  The guard skips every
 * exit handler registered before it (atexit/on_exit work, earlier libraries'
 * static destructors) -- work the double-free abort would skip as well;
 * PRK_EXIT_GUARD=0 in the environment leaves the exit path untouched.
 * prk_destroy and prk_comm_init run the same check (and install the same
 * guard). */
int prk_create(int device, prk_context **out);
/* prk_destroy queues no GPU work: it waits for the context's streams and frees
 * what the context owns.  A frame whose bin count is still unresolved (prk_flush
 * returned, nothing has read the count since) is DROPPED, not re-run: if its
 * entries overflowed the scratch, a caller-owned target (prk_target_bind) is
 * left with the frame's cleared or partial contents.  A caller that reads its
 * own target after destroying the context calls prk_synchronize (or
 * prk_resolve) first. */
int prk_destroy(prk_context *ctx);
/* The check alone: PRK_OK, or PRK_ERR_RUNTIME_MIX (guard installed). */
int prk_runtime_check(void);
int prk_device_count(int *out);
const char *prk_version(void);

/* Render target: device memory owned by the caller (e.g. a torch tensor) or
 * by the library (prk_target_alloc).  The target covers frame rows
 * [row0, row1) of a frame `height` rows tall; `color` and `zbuf` point at
 * frame row row0.  z-buffer row stride is `width` floats (Commands->Width,
 * projekt.cpp:170,1511); colour row stride is `pitch_bytes`.
 * A target for the AVX semantics needs width % 8 == 0 (the reference's
 * aligned 8-wide z load, projekt.cpp:2218). */
int prk_target_bind(prk_context *ctx, void *color, int32_t pitch_bytes, float *zbuf,
                    int32_t width, int32_t height, int32_t row0, int32_t row1);
int prk_target_alloc(prk_context *ctx, int32_t width, int32_t height, int32_t row0,
                     int32_t row1, void **color_out, float **zbuf_out);
/* Fill the bound target: colour with `color`, z with `z` (reference callers
 * clear z to -FLT_MAX). */
int prk_target_clear(prk_context *ctx, uint32_t color, float z);
/* The same fill, fused into the next prk_flush: the frame's kernels take
 * (color, z) as the target's prior contents and write every pixel of the
 * target (the winners shaded, the rest the fill values), so no separate
 * fill pass runs.  Frames that do not shade through span records (scalar or
 * mixed semantics) and empty flushes fill first, on the flush's stream. */
int prk_target_clear_on_flush(prk_context *ctx, uint32_t color, float z);
/* Copy the bound target to/from host memory (rows [row0,row1)). */
int prk_target_download(prk_context *ctx, uint32_t *color_host, int32_t host_pitch_bytes,
                        float *z_host);
/* Early z (off by default; the drop-in header turns it on): in frames shaded
 * through span records (all-AVX semantics, per triangle) the visibility
 * kernel writes the final z and the shading only the colour, so
 * prk_target_download copies z while the frame still shades (C3b through
 * projekt.h: 0.45 ms less per frame over PCIe).  It costs a frame that is not
 * downloaded ~0.4 % (the z stores move to the frame's busiest kernel).  The
 * result is the same bit for bit (a -0.0 z, which the visibility key holds
 * as +0.0, is written by the shading and makes the download take z again). */
int prk_set_early_z(prk_context *ctx, int on);
int prk_target_upload(prk_context *ctx, const uint32_t *color_host, int32_t host_pitch_bytes,
                      const float *z_host);
/* prk_target_upload on the context's copy stream: returns at once; the next
 * prk_flush's kernels wait for it.  The host buffers must be page-locked
 * (prk_host_register) and stay unchanged until prk_target_download or
 * prk_synchronize returns (the drop-in sends the caller's framebuffer this
 * way at a frame's first draw, so the copy overlaps the caller's calls). */
int prk_target_upload_async(prk_context *ctx, const uint32_t *color_host, int32_t host_pitch, const float *z_host);

/* Pinned host memory for staging (prk_host_alloc / prk_host_free), and
 * page-locking of caller memory (a framebuffer, a z-buffer) so uploads and
 * downloads run as DMA at full PCIe rate.  Allocations of 2 MB and more are
 * heap memory on transparent huge pages, page-locked for every device
 * (cheaper for the CPU to fill than 4-KB pinned pages;
 * PRK_HOST_ALLOC_THP=0 turns this off).  Free with prk_host_free only. */
int prk_host_alloc(prk_context *ctx, size_t bytes, void **out);
int prk_host_free(prk_context *ctx, void *p);
int prk_host_register(prk_context *ctx, void *p, size_t bytes);
int prk_host_unregister(prk_context *ctx, void *p);

/* Camera and lights (game_render_commands::Transform / LightData) of the
 * draws executed by the next prk_flush, for both what FillEdgeTable reads
 * (ProjectVertex 3906-3910, Gouraud vertex lighting 4020-4063) and what the
 * span kernels read (Phong + UnprojectVertex: DrawModel 452-458,
 * FillLineOptimized 2042-2046, the single-thread overload 3030-3034). */
int prk_set_camera(prk_context *ctx, const prk_transform *transform,
                   const prk_light_data *lights);
/* After prk_set_camera: the span shading (Phong lighting and unprojection)
 * of the next flush uses (transform, lights) instead, the setup keeps
 * prk_set_camera's.  The reference's FillEdgeTable and DrawModel* each read
 * Commands when they run, so a caller that changes Commands between an
 * object's FillEdgeTable and its DrawModel* call gets the setup of the first
 * and the shading of the second; the drop-in passes them this way.  (For the
 * queue overload the spans run on workers that read Commands as they go,
 * 2042-2046; the drop-in uses Commands as they are at the DrawModel* call.)
 * PRK_ERR_ARG before any prk_set_camera. */
int prk_set_shade_camera(prk_context *ctx, const prk_transform *transform,
                         const prk_light_data *lights);

/* Textures.  `bitmap->Memory` is host memory of Height rows of Pitch bytes
 * (loaded_bitmap as the reference reads it, projekt.cpp:1506, 1881-1935); the
 * library appends the zeroed guard row the u == 1 / v == 1 over-read lands
 * on and never reads past the caller's last row.
 * Returns a handle >= 0.  prk_texture_update re-reads a bitmap into a handle
 * (the drop-in refreshes every texture once per frame). */
int prk_texture_create(prk_context *ctx, const prk_bitmap *bitmap, int32_t *handle_out);
int prk_texture_update(prk_context *ctx, int32_t handle, const prk_bitmap *bitmap);
int prk_texture_set_filter(prk_context *ctx, int32_t handle, int32_t filter);  /* PRK_FILTER_* */

/* Render to texture: a frame this library drew, sampled by the next one
 * without leaving the device.  An EXTENSION of this build with its own
 * definition: the reference's textures are host bitmaps.
 *
 * prk_texture_alloc: a library-owned texture of width x height texels (both
 * > 0), pitch 4 * width, every texel and the guard row (row `height`) zero,
 * filter PRK_FILTER_NEAREST -- a destination for prk_texture_from_target.
 *
 * prk_texture_from_target: the colour of the bound target, pixels
 * [x0, x0 + width) x [y0, y0 + height) in FRAME coordinates, box-filtered by
 * `factor` (1, 2 or 4) into texels [dst_x, dst_x + width / factor) x
 * [dst_y, dst_y + height / factor) of `texture` (any texture handle, at the
 * pitch it was made with).  Per texel and per 8-bit channel of the 0xAARRGGBB
 * word, in integers:
 *   out = (sum of the factor * factor source channel values + factor * factor / 2)
 *         >> (2 * log2(factor))
 * so factor 1 copies the word bit for bit, and the result is exact and the
 * same on every device.  Rendering at 2W x 2H or 4W x 4H and resolving by 2
 * or 4 is a supersampled frame of W x H.
 * Nothing else is written: texels outside the destination rectangle and the
 * guard row keep their contents; the target and z are only read.
 * The source is the target as the frames already flushed and the clears and
 * uploads already queued leave it; a prk_target_clear_on_flush not yet flushed
 * is not in it.  The source rectangle must lie inside [0, W) x [row0, row1):
 * a band context reads its own rows only.
 * Ordering is prk_geometry_write's: the call returns without waiting and
 * allocates nothing; it runs after the frames already flushed (which wrote the
 * target and sampled the texture) and after the clears and uploads queued so
 * far, before the next prk_flush's kernels, and before a later
 * prk_target_clear / prk_target_upload / prk_texture_update changes either
 * side.  A draw recorded before the call and flushed after it samples the new
 * contents.
 * PRK_ERR_ARG: a NULL context, a bad texture handle, a factor other than 1, 2
 * or 4, a width or height that is not positive or no multiple of factor, a
 * source rectangle outside the target's band, a destination rectangle outside
 * the texture's width x height.  PRK_ERR_NO_TARGET: no target bound.  On any
 * error nothing has been written.
 *
 * prk_texture_download: rows [0, height) of any texture (the guard row is not
 * returned) to host rows of pitch_bytes bytes (>= 4 * width, a multiple of 4),
 * after everything queued that writes the texture.
 *
 * prk_texture_info: a texture's width, height and pitch; any pointer may be
 * NULL.  Host bookkeeping: no device work. */
int prk_texture_alloc(prk_context *ctx, int32_t width, int32_t height, int32_t *handle_out);
int prk_texture_from_target(prk_context *ctx, int32_t texture,
                            int32_t x0, int32_t y0, int32_t width, int32_t height, /* source, frame pixels */
                            int32_t factor,                                        /* 1, 2 or 4 */
                            int32_t dst_x, int32_t dst_y);
int prk_texture_download(prk_context *ctx, int32_t handle, void *memory, int32_t pitch_bytes);
int prk_texture_info(prk_context *ctx, int32_t handle, int32_t *width, int32_t *height, int32_t *pitch_bytes);

/* Target layers: a drawn (colour, z) frame kept on the device, put back
 * before the next frame, or merged into it by depth.  An EXTENSION of this
 * build with its own definition: the reference keeps one
 * framebuffer.
 *
 * A LAYER is a rectangle of width x height pixels, each a 0xAARRGGBB colour
 * word and an f32 z.  The context owns it and names it by a handle >= 0, in a
 * number space of its own (like span handles); a destroyed handle stays dead.
 *
 * prk_layer_alloc: a library-owned layer, colour pitch 4 * width, z rows of
 * width floats; every colour word 0 and every z -FLT_MAX (bits 0xFF7FFFFF).
 *
 * prk_layer_wrap_device: a READ-ONLY layer over device memory that the caller
 * keeps alive until prk_layer_destroy or prk_destroy; no copy is made.  Colour
 * rows are pitch_bytes apart (>= 4 * width, a multiple of 4), z rows width
 * floats.  Both addresses are 4-byte aligned; nothing more is asked.  Intended
 * sources: another context's target on the same device (prk_get_target), a
 * torch tensor.  The caller guarantees that the memory is complete and stays
 * unchanged while a queued call reads it: for a peer context's target that
 * means prk_synchronize on the peer before the call here, and no draw into it
 * until this context has finished (prk_synchronize, or a download).  The
 * memory must not overlap this context's bound target.
 *
 * prk_layer_from_target (save): colour and z of the target's pixels
 * [x0, x0 + width) x [y0, y0 + height), in FRAME coordinates, bit for bit into
 * the layer's pixels at (dst_x, dst_y).  The rectangle must lie inside
 * [0, W) x [row0, row1) (a band context reads its own rows only) and its
 * destination inside the layer.  Nothing else in the layer is written; the
 * target is only read.  A wrapped layer as destination is PRK_ERR_ARG.
 *
 * prk_target_from_layer (restore, merge): for every pixel of the layer's
 * rectangle [src_x, src_x + width) x [src_y, src_y + height), with (cs, zs)
 * the layer's pixel and (cd, zd) the target's pixel at the same offset from
 * (x0, y0) in FRAME coordinates:
 *   PRK_MERGE_COPY           (cd, zd) = (cs, zs)
 *   PRK_MERGE_GREATER        the same where zs >  zd
 *   PRK_MERGE_GREATER_EQUAL  the same where zs >= zd
 * The comparison is IEEE f32: a NaN on either side loses (the target keeps its
 * pixel), -0.0 equals +0.0, denormals compare by value.  Words move as bits; a
 * pixel that does not win keeps both its words.  No pixel outside the
 * rectangle is touched, nor the pad bytes of a caller-bound target's pitch.
 * The rules are the reference's z tests: DrawModel and FillLineOptimized keep
 * the earliest of equal fragments (GREATER: the layer holds the LATER draws),
 * the single-thread overload the latest (GREATER_EQUAL).  So two frames drawn
 * from the same clear, whose z is below every fragment's, one of a frame's
 * draws [0, k) and one of its draws [k, n), merge into exactly the frame of
 * all n draws: restore or keep the first, merge the second under its
 * semantics' rule.
 * Winner ids are not merged: prk_download_winners stays "of the last flush".
 * prk_get_stats is untouched.
 *
 * Ordering of both calls is prk_texture_from_target's: the call returns
 * without waiting and allocates nothing; the pending frame is resolved first
 * (an overflowed one re-run); it runs after the frames already flushed and the
 * clears and uploads queued so far, before the next prk_flush's kernels, and
 * before a later prk_target_clear / prk_target_upload / layer or texture call.
 * A draw recorded before prk_target_from_layer and flushed after it is drawn
 * on top of what the call wrote.  A prk_target_clear_on_flush not yet flushed
 * is not in what prk_layer_from_target reads, and still clears at its flush:
 * it discards what prk_target_from_layer wrote, as it discards an upload.
 *
 * prk_layer_download: the layer's colour (rows host_pitch_bytes apart,
 * >= 4 * width, a multiple of 4) and z (rows of width floats) after every
 * queued call that writes it; either host pointer may be NULL.
 * prk_layer_info: width, height, colour pitch and whether it is wrapped; any
 * pointer may be NULL.  Host bookkeeping: no device work.
 * prk_layer_destroy: after the frames in flight and the queued layer calls;
 * frees a library-owned layer's memory.  prk_destroy frees every layer.
 *
 * PRK_ERR_ARG: a NULL context, a bad or destroyed handle, an unknown rule, a
 * width or height <= 0, a rectangle outside the layer or outside the target's
 * band, a bad pitch or address.  PRK_ERR_NO_TARGET: no target bound.  On any
 * error nothing has been written. */
enum prk_merge {
    PRK_MERGE_COPY = 0,          /* every pixel of the rectangle: colour and z replaced            */
    PRK_MERGE_GREATER = 1,       /* where zs > zd  (DrawModel, FillLineOptimized: earliest wins)   */
    PRK_MERGE_GREATER_EQUAL = 2  /* where zs >= zd (the single-thread overload: latest wins)       */
};
int prk_layer_alloc(prk_context *ctx, int32_t width, int32_t height, int32_t *handle_out);
int prk_layer_wrap_device(prk_context *ctx, const void *color, int32_t pitch_bytes, const float *zbuf,
                          int32_t width, int32_t height, int32_t *handle_out);
int prk_layer_from_target(prk_context *ctx, int32_t layer, int32_t x0, int32_t y0, int32_t width, int32_t height,
                          int32_t dst_x, int32_t dst_y);
int prk_target_from_layer(prk_context *ctx, int32_t layer, int32_t src_x, int32_t src_y, int32_t width,
                          int32_t height, int32_t x0, int32_t y0, int32_t rule);
int prk_layer_download(prk_context *ctx, int32_t layer, uint32_t *color_host, int32_t host_pitch_bytes, float *z_host);
int prk_layer_info(prk_context *ctx, int32_t layer, int32_t *width, int32_t *height, int32_t *pitch_bytes, int32_t *wrapped);
int prk_layer_destroy(prk_context *ctx, int32_t layer);

/* Visibility feedback: what the last frame showed, per id, without moving the
 * frame to the host -- which draws, objects or triangles won pixels, and how
 * many.  An EXTENSION of this build with its own definition:
 * the reference has no such query.
 *
 * THE FRAME is the most recent prk_flush, if it had draws and was queued with
 * prk_set_debug(ctx, 1) (prk_download_winners' precondition: the answer is a
 * reduction of that winner map, on the device).  A flush without draws or with
 * debug off leaves no frame, and neither does a target bound or allocated
 * since.
 * IDS are the frame's winner numbering, in submission order from 0: one per
 * triangle of prk_draw and of prk_draw_objects' range (an object's pixels
 * carry the id of its first triangle; its other ids stay at 0 pixels), one
 * per prk_draw_edges call, per list of prk_draw_edge_lists / prk_draw_records
 * (an empty list takes its id all the same), per span of prk_draw_spans /
 * prk_draw_span_records and per pair of prk_draw_rows.  id_count is the number
 * of ids that flush handed out.
 * pixels[i] is the number of pixels of the context's band, rows [row0, row1),
 * whose winner word is i.  A pixel that kept an earlier flush's contents
 * belongs to no id.  covered is the sum of pixels[i], visible_ids the number
 * of ids with pixels[i] > 0.  A band context answers for its own rows, so a
 * frame's counts are the sums of its ranks'.  Winner ids are not merged by
 * prk_target_from_layer (above), so a later merge does not change the answer.
 *
 * prk_visibility_info: id_count, covered and visible_ids (all three required).
 * prk_visibility_counts: pixels[0 .. count) = the counts of ids first_id ...
 * prk_visibility_groups: for group g = ids [starts[g], starts[g + 1]) -- an
 * object's triangles, a batch's lists; starts has group_count + 1 words --
 * pixels[g] = the sum of the group's counts and visible[g] = how many of its
 * ids have any.  Either output may be NULL, not both; an empty group gets 0.
 * prk_visibility_ids: the ids with pixels[i] > 0, ascending.  *total_out is
 * always written (0 where there is no frame); ids == NULL: the size only; a
 * capacity below the total: PRK_ERR_ARG with `ids` untouched.
 * prk_visibility_device: the library's own device arrays, complete when the
 * call returns: counts of id_count words and pix_prefix of id_count + 1
 * (pix_prefix[i] = pixels[0] + ... + pixels[i - 1]; the last word is covered).
 * Read-only, valid until the next prk_flush, prk_target_alloc / prk_target_bind
 * or prk_destroy: for a caller that wants the counts as a tensor, no copy.
 *
 * Ordering and cost: every call resolves the pending frame first (an
 * overflowed one is re-run, as prk_download_winners does).  The first call
 * after a flush waits for the frame, queues the reduction (a histogram of the
 * map, two scans, a compaction) and waits for it; later calls for the same
 * frame reuse the result: host copies, and one small kernel for the groups.
 * Nothing here touches the flush: a frame queued without the winner map costs
 * what it did.  The winner map is debug mode's, which forgoes the fused clear
 * (prk_target_clear_on_flush then fills before the frame).
 *
 * PRK_ERR_ARG: a NULL context, no such frame, a NULL required pointer,
 * first_id + count > id_count, starts not non-decreasing or
 * starts[group_count] > id_count.  PRK_ERR_LIMIT: a band of 2^32 pixels or
 * more.  count == 0 or group_count == 0: PRK_OK, nothing written.  On any
 * error nothing is written, except *total_out as stated. */
int prk_visibility_info(prk_context *ctx, uint32_t *id_count, uint64_t *covered, uint32_t *visible_ids);
int prk_visibility_counts(prk_context *ctx, uint32_t first_id, uint32_t count, uint32_t *pixels);
int prk_visibility_groups(prk_context *ctx, const uint32_t *starts, uint32_t group_count,
                          uint32_t *pixels, uint32_t *visible); /* either output may be NULL, not both */
int prk_visibility_ids(prk_context *ctx, uint32_t *ids, uint64_t capacity, uint64_t *total_out);
int prk_visibility_device(prk_context *ctx, const uint32_t **counts, const uint32_t **pix_prefix, uint32_t *id_count);

/* Geometry: non-indexed SoA vertex arrays exactly as render_entry_3d_object
 * (projekt.h:2-15): positions v3, colours v4, normals v3, uvs v2, three
 * vertices per triangle.  Copied to HBM once; a draw references a range. */
int prk_geometry_create(prk_context *ctx, const float *vertices, const float *colors,
                        const float *normals, const float *uvs, uint32_t vertex_count,
                        int32_t *handle_out);
/* New contents for a library-owned geometry (grows its buffers if needed);
 * an array passed as NULL keeps its previous contents (vertices past them
 * read as zero); draws already recorded read the new contents.  Waits for
 * frames in flight; synchronous. */
int prk_geometry_update(prk_context *ctx, int32_t handle, const float *vertices, const float *colors,
                        const float *normals, const float *uvs, uint32_t vertex_count);
/* Asynchronous partial update: vertices [first_vertex, first_vertex +
 * vertex_count) of the arrays given (NULL: that array unchanged there) are
 * copied on the context's copy stream, after the frames already flushed have
 * read the geometry and before the next prk_flush's kernels read it.  The
 * geometry's vertex count becomes first_vertex + vertex_count; buffers grow
 * (kept contents, zeros past them) when needed, which waits for the device.
 * The host arrays must be page-locked (prk_host_alloc / prk_host_register)
 * and stay unchanged until prk_synchronize or prk_target_download returns.
 * The drop-in streams FillEdgeTable's vertices this way while the caller is
 * still submitting objects.  first_vertex and vertex_count are multiples of 3. */
int prk_geometry_write(prk_context *ctx, int32_t handle, uint32_t first_vertex, uint32_t vertex_count,
                       const float *vertices, const float *colors, const float *normals, const float *uvs);
/* Same as prk_geometry_create, but from device pointers the caller keeps
 * alive (no copy). */
int prk_geometry_wrap_device(prk_context *ctx, const float *vertices, const float *colors,
                             const float *normals, const float *uvs, uint32_t vertex_count,
                             int32_t *handle_out);

/* Objects that move: a transform pass on the device.  An EXTENSION of this
 * build with its own definition: the reference's camera has
 * no rotation and its callers re-fill Vertices on the host before every
 * FillEdgeTable; here a resident source geometry is written through 3x4
 * matrices into a resident destination geometry, and one prk_draw_objects or
 * prk_records_from_geometry on the destination (P = 0) takes every object.
 *
 * prk_geometry_alloc: a library-owned geometry of 0 vertices and no arrays --
 * a destination to transform (or prk_geometry_write) into.
 *
 * prk_geometry_transform: for every run, triangles [src_first_tri, +tri_count)
 * of src go to triangles [dst_first_tri, +tri_count) of dst through
 * M = xforms[run.xform].M (row-major):
 *   positions, component i:  out[i] = ((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + M[i][3]
 *   normals:                 out[i] =  (M[i][0]*x + M[i][1]*y) + M[i][2]*z
 *   colours, uvs:            copied bit for bit.
 * Every product and every sum is rounded to f32 on its own, in this order;
 * nothing is fused.  So the identity matrix returns values equal to the
 * source's, except that a -0.0 may come out as +0.0 (-0.0 + 0.0).  Normals
 * are NOT renormalised: pass rigid transforms (rotation + translation), or
 * accept the normals as they come out.
 * dst receives every array src has: one dst lacked is allocated, zero where
 * no run writes; an array dst has and src lacks is left alone.  dst grows as
 * prk_geometry_write grows a geometry (contents kept, zeros past them,
 * recorded draws repointed); its vertex count becomes the larger of its old
 * value and three times the highest triangle written.
 * A run of 0 triangles is skipped.  The same source range may appear in many
 * runs (instancing); runs may come in any order.  Destination ranges that
 * overlap are NOT checked: the overlap holds unspecified values (of one run
 * or another, per word), everything else what its run writes.
 * PRK_ERR_ARG: a NULL context, a bad handle, src == dst, a dst that is wrapped
 * (prk_geometry_wrap_device), run_count > 0 with NULL runs or xforms, a run
 * whose xform >= xform_count, whose source range passes the end of src, or
 * whose destination end passes prk_geometry_write's vertex limit.
 * PRK_ERR_LIMIT: more than 2^31 output triangles in one call.  On any error
 * nothing has been written.
 * Ordering is prk_geometry_write's: the call returns without waiting (unless
 * dst must grow); it runs after the frames already flushed have read dst,
 * before the next prk_flush's kernels read it and before any later
 * prk_records_from_geometry / prk_edge_records reads it.  runs and xforms are
 * copied at the call.  src is read at that same point of the order: an earlier
 * prk_geometry_write (or transform) to src is seen, a later one is not.
 *
 * prk_geometry_download: vertices [first_vertex, +vertex_count) of any
 * geometry to host memory, after everything queued that writes it.  A NULL
 * pointer skips that array.  PRK_ERR_ARG: an array asked for that the geometry
 * lacks, a range past the vertex count, first_vertex or vertex_count no
 * multiple of 3. */
typedef struct prk_xform {
    float M[3][4]; /* row-major: out = M[:, 0:3] * v + M[:, 3] */
} prk_xform;
typedef struct prk_xform_run {
    uint32_t src_first_tri, tri_count, dst_first_tri, xform; /* xform: index into the call's xforms */
} prk_xform_run;
int prk_geometry_alloc(prk_context *ctx, int32_t *handle_out);
int prk_geometry_transform(prk_context *ctx, int32_t src, int32_t dst,
                           const prk_xform_run *runs, uint32_t run_count,
                           const prk_xform *xforms, uint32_t xform_count);
int prk_geometry_download(prk_context *ctx, int32_t handle, uint32_t first_vertex, uint32_t vertex_count,
                          float *vertices, float *colors, float *normals, float *uvs);
/* A geometry's vertex count and which arrays it has (bit 0 vertices, 1
 * colours, 2 normals, 3 uvs), as the calls queued so far leave them; either
 * pointer may be NULL.  Host bookkeeping: no device work. */
int prk_geometry_info(prk_context *ctx, int32_t handle, uint32_t *vertex_count_out, uint32_t *arrays_out);
/* Debug/bench: the stream (a hipStream_t) prk_geometry_write's copies and
 * prk_geometry_transform's pass are queued on, for timing them with events
 * (tools/xform_bench.py).  Queue nothing else there. */
int prk_debug_geometry_stream(prk_context *ctx, void **stream);
/* Debug/bench: the device time of the most recent prk_geometry_transform's
 * kernel alone (events after its table upload and after the kernel); waits
 * for it.  PRK_ERR_ARG before any transform. */
int prk_debug_transform_ms(prk_context *ctx, float *kernel_ms);

/* Cull and pick a level of detail on the device.  An EXTENSION of this build
 * with its own definition: it acts on prk_visibility_*'s
 * counts without moving them to the host.  For every ITEM (an object, a group
 * of them) the call decides on the device whether the item is drawn and from
 * which of its LEVELS (meshes of the source geometry, finest first as a rule),
 * and writes the chosen triangles, packed in item order and transformed, into
 * dst.  One word comes back before the draw: the triangle total.  The library
 * still decides nothing on its own: thresholds and tables are the caller's.
 *
 * pixels(i): with item_pixels, item_pixels[i] -- no frame is needed, first_id
 *   and id_count are ignored.  Without (NULL), the sum of the frame's
 *   pixels[id] over ids [first_id, first_id + id_count): THE FRAME is
 *   prk_visibility_*'s, with the same "no such frame" rule; the sum is a
 *   difference of two pix_prefix words (it fits in 32 bits); id_count == 0
 *   gives 0.
 * chosen(i): the smallest l in [0, item.level_count) with
 *   pixels(i) >= levels[item.first_level + l].min_pixels; -1 when no level
 *   passes or the item has no levels.  Nothing is assumed about the order of
 *   the thresholds: the first level that passes wins.  min_pixels == 0 always
 *   passes: an always-drawn item (a new object, the occluders) has one level
 *   with min_pixels == 0.
 * n(i): the chosen level's tri_count, or 0.
 * out_first[i] = dst_first_tri + n(0) + ... + n(i - 1); out_first[item_count]
 *   is the end; *total_tris_out = the sum of the n(i).
 * Triangles [out_first[i], out_first[i] + n(i)) of dst are source triangles
 *   [level.src_first_tri, +n(i)) through xforms[item.xform], in exactly
 *   prk_geometry_transform's arithmetic (the same expression order, nothing
 *   fused, colours and uvs copied bit for bit).  When the total is not 0, dst
 *   grows and receives the arrays src has by prk_geometry_transform's rule,
 *   and its vertex count becomes max(old, 3 * end); triangles outside
 *   [dst_first_tri, end) keep their contents.  A call that chooses nothing
 *   (total 0) writes nothing and leaves dst as it was.
 *
 * Ordering: the choice and the scan run at the call, on the geometry stream,
 * and the call waits for them -- it needs the total to size dst and the grid,
 * and returns it.  The emit pass is queued as prk_geometry_transform's pass
 * is: after the frames already flushed have read dst, before the next
 * prk_flush's kernels read it; the call does not wait for it.  All tables are
 * copied at the call.  src is read where the emit pass stands in that order.
 *
 * Errors are decided on the host from the arguments and from worst cases; no
 * status depends on what the device chose, and on any error nothing is
 * written.  PRK_ERR_ARG: a NULL context or total_tris_out; a bad handle,
 * src == dst, a wrapped dst; item_count > 0 with NULL items; NULL levels or
 * xforms where an item has levels; an item's first_level + level_count past
 * level_count; xform >= xform_count on an item that has levels; a level of a
 * listed item (with tri_count > 0) whose source range passes the end of src;
 * without item_pixels, no frame, or an item's first_id + id_count past the
 * frame's id_count; a worst-case end -- dst_first_tri plus every item's
 * largest level -- past prk_geometry_write's vertex limit.  PRK_ERR_LIMIT: a
 * worst-case total above 2^31 (checked before the vertex limit, which such a
 * total always passes).  item_count == 0: PRK_OK, total 0, out_first[0] =
 * dst_first_tri.
 *
 * Ids after a compacted draw: after prk_draw(dst, dst_first_tri, total, ...)
 * as the frame's first draw, item i's ids next frame are
 * [out_first[i] - dst_first_tri, +n(i)).  A dropped item has no ids and leaves
 * no pixels to count: whether it could be seen again is answered by
 * prk_visibility_bounds, and acted on by prk_geometry_select_bounds (below).
 * Band contexts: a band context's frame counts cover its own rows only; ranks
 * that must draw the same geometry pass the summed counts as item_pixels.
 *
 * chosen: item_count words or NULL; out_first: item_count + 1 words or NULL. */
typedef struct prk_select_level {
    uint32_t min_pixels, src_first_tri, tri_count;
} prk_select_level;
typedef struct prk_select_item {
    uint32_t first_id, id_count, first_level, level_count, xform; /* xform: index into the call's xforms */
} prk_select_item;
int prk_geometry_select(prk_context *ctx, int32_t src, int32_t dst, uint32_t dst_first_tri,
                        const prk_select_item *items, uint32_t item_count,
                        const prk_select_level *levels, uint32_t level_count,
                        const prk_xform *xforms, uint32_t xform_count,
                        const uint32_t *item_pixels, int32_t *chosen, uint32_t *out_first,
                        uint64_t *total_tris_out);
/* Debug/bench: the device times of the most recent prk_geometry_select that
 * reached the device -- choose_ms from before its table uploads to the copy of
 * the total (uploads, choice, scan), emit_ms its emit pass alone (0 when the
 * total was 0); waits for the pass.  PRK_ERR_ARG before any such call. */
int prk_debug_select_ms(prk_context *ctx, float *choose_ms, float *emit_ms);

/* Bounds occlusion test on the device: bring culled items back.  An EXTENSION
 * of this build with its own definition.  An item that was
 * not drawn has no pixels to count; this call tests its bounding box against
 * the depth the target holds now, without moving the z-buffer to the host.
 * Pixel counts rule the items that were drawn, this test the ones that were
 * not.  The library still decides nothing: boxes, padding and thresholds are
 * the caller's.
 *
 * Z TILES.  The target band, rows [row0, row1) of the W x H frame, is cut into
 * tiles of 8 x 8 pixels aligned to frame coordinates: tile (tx, ty) covers
 * x in [8tx, 8tx + 8) ^ [0, W) and y in [8ty, 8ty + 8) ^ [row0, row1).
 * zmin[ty][tx] is the smallest non-NaN z word of the tile's pixels, or +inf if
 * every word is NaN.  -0.0 and +0.0 are one value (either may be stored);
 * denormals compare by value.  W need not be a multiple of 8, row0 need not
 * be one, and the z pointer of a caller-bound target need only be 4-byte
 * aligned.  The map has tiles_x = (W + 7) / 8 columns and the tile rows
 * row0 / 8 ... (row1 + 7) / 8 - 1.
 *
 * BOUNDS.  Item i has 8 corners, every choice of lo / hi per axis.  Each goes
 * through xforms[bound.xform] in exactly prk_geometry_transform's position
 * arithmetic (((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + M[i][3], nothing fused),
 * then + P component by component as a draw adds its P (a NULL P is 0), then
 * through ProjectVertex under prk_set_camera's transform as it stands at the
 * call: d = D - z; if d > 0.2: k = (1 / d) * F, px = Cx + M2P * (k * x),
 * py = Cy + M2P * (k * y).
 * znear(i) is the largest camera-space z (after + P, before projection) of the
 *   8 corners, NaN if any of them is NaN.  The z-buffer holds camera-space z,
 *   and a larger z is nearer (z > zbuf wins; clears are -FLT_MAX).
 * rect(i) is x0 = floor(min px) - 1, x1 = floor(max px) + 2 and the same in
 *   y, half-open, each of the four clamped in float (max with the low edge,
 *   then min with the high edge) to [0, W] and [row0, row1] before any integer
 *   conversion.  The pixel of margin on each side absorbs the fill rules.  If
 *   any corner fails d > 0.2 (a NaN d included) or any projected coordinate
 *   is NaN, rect(i) is the whole band.
 * pixels(i) is the sum of area(rect(i) ^ t) over the tiles t that meet rect(i)
 *   and satisfy !(znear(i) < zmin[t]).  Equality passes: the single-thread
 *   semantics draw on >=, and an item tested against a frame that holds its
 *   own flat face must not hide itself.  A NaN znear passes everywhere.  An
 *   empty rectangle gives 0.
 * pixels(i) is an upper bound on the pixels any geometry inside the box could
 * win over the target's current z, and 0 only if the box cannot win a pixel --
 * exact up to the rounding of the rasteriser's span recurrences (an edge's x
 * and z are stepped row by row in f32 and may leave the hull of the vertices
 * by a few ulps).  PADDING THE BOX AGAINST THAT ROUNDING IS THE CALLER'S JOB.
 * A band context answers for its own rows on band-clipped tiles; the sum over
 * ranks is again an upper bound, and equals the one-context answer only when
 * the band edges are multiples of 8.
 *
 * prk_visibility_bounds.  Ordering is prk_layer_from_target's, except that the
 * call waits for its result: the pending frame is resolved first (an
 * overflowed one is re-run); the two kernels run after the frames already
 * flushed and after the clears, uploads and layer calls queued so far; a
 * prk_target_clear_on_flush not flushed yet is not in what the call reads.
 * The tile map is rebuilt at every call.  The answer -- count words on the
 * device, and in `pixels` if that is not NULL -- is complete when the call
 * returns and stays valid until the next prk_visibility_bounds,
 * prk_target_alloc, prk_target_bind or prk_destroy.  A later prk_flush does
 * not invalidate it: which z it was tested against is the caller's business.
 * Errors are decided on the host, nothing written and the previous answer as
 * it was: PRK_ERR_ARG for a NULL context, NULL bounds or xforms with
 * count > 0, a bound's xform >= xform_count, a call before any
 * prk_set_camera; PRK_ERR_NO_TARGET without a target; PRK_ERR_LIMIT for a
 * band of 2^32 pixels or more.  count == 0: PRK_OK and an empty answer.
 * prk_visibility_bounds_device: the answer's device array and its count
 * (read-only; PRK_ERR_ARG when there is none).
 *
 * prk_geometry_select_bounds is prk_geometry_select with item_pixels == NULL,
 * except that an item with id_count == 0 takes pixels(i) = answer[i] of the
 * last prk_visibility_bounds.  PRK_ERR_ARG if there is no answer or its count
 * is not item_count.  A frame is needed only when some item has
 * id_count > 0 (its ids are then checked against the frame's for every item,
 * as there).  Everything else is prk_geometry_select's, word for word:
 * chosen, out_first, the emit arithmetic, the errors from worst cases, the
 * ordering, and dst left untouched when the total is 0.
 *
 * Debug/bench: prk_debug_ztiles copies the last call's tile map (row-major,
 * tiles_y rows of tiles_x; zmin NULL: the sizes only; a capacity in floats
 * below tiles_x * tiles_y: PRK_ERR_ARG) and says which tile row is its first;
 * prk_debug_bounds_ms gives the device times of the last call's two kernels
 * (test_ms 0 when count was 0).  Both are PRK_ERR_ARG before any call. */
typedef struct prk_bound {
    float lo[3], hi[3];
    uint32_t xform; /* index into the call's xforms */
} prk_bound;
int prk_visibility_bounds(prk_context *ctx, const prk_bound *bounds, uint32_t count,
                          const prk_xform *xforms, uint32_t xform_count, const float *P,
                          uint32_t *pixels);
int prk_visibility_bounds_device(prk_context *ctx, const uint32_t **pixels, uint32_t *count);
int prk_geometry_select_bounds(prk_context *ctx, int32_t src, int32_t dst, uint32_t dst_first_tri,
                               const prk_select_item *items, uint32_t item_count,
                               const prk_select_level *levels, uint32_t level_count,
                               const prk_xform *xforms, uint32_t xform_count,
                               int32_t *chosen, uint32_t *out_first, uint64_t *total_tris_out);
int prk_debug_ztiles(prk_context *ctx, float *zmin, uint64_t capacity, int32_t *tiles_x, int32_t *tiles_y,
                     int32_t *first_tile_row);
int prk_debug_bounds_ms(prk_context *ctx, float *ztile_ms, float *test_ms);

/* Record one draw: triangles [first_tri, first_tri+tri_count) of a geometry,
 * object offset P (render_entry_3d_object::P), semantics PRK_SEM_*,
 * PhongShading flag, texture handle (-1 = no Bitmap).
 * PRK_SEM_AVX requires a texture and PhongShading != 0: the reference
 * dereferences Bitmap unconditionally (projekt.cpp:1506) and its non-Phong
 * branch writes garbage (projekt.cpp:2285-2316). */
int prk_draw(prk_context *ctx, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
             const float P[3], int32_t semantics, int32_t phong, int32_t texture);
/* The same draw as consecutive render_entry_3d_objects of `tris_per_object`
 * triangles each (the last one may be smaller): every object is ONE active
 * edge table, as FillEdgeTable + DrawModelOptimized(RenderQueue,...) build it
 * (projekt.cpp:3894-4117, 3654-3869), so spans pair edges of different
 * triangles of the object.  tris_per_object == 1 is prk_draw.  Objects of
 * more than one triangle are supported for every semantics (DrawModel's
 * AET, 162-601, has the same list logic), of any size: the active edge list
 * has no length limit (a wave walks it in LDS, or in device memory once it
 * outgrows LDS).  The edges are set up as FillEdgeTable(Object, Commands,
 * phong) does for an object whose Bitmap is set iff texture >= 0. */
int prk_draw_objects(prk_context *ctx, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                     uint32_t tris_per_object, const float P[3], int32_t semantics, int32_t phong,
                     int32_t texture);

/* FillEdgeTable's own inputs, which shape the edge records independently of
 * the later DrawModel* call (projekt.cpp:3882-4121):
 *   PRK_SETUP_PHONG   its PhongShading argument != 0: raw vertex colours and
 *                     normals (4012-4019); 0: per-vertex Gouraud lighting
 *                     (4020-4063) and no normals;
 *   PRK_SETUP_BITMAP  Object->Bitmap != 0: the lighting starts from white
 *                     (4034-4054) and the U/V/(1/z) gradients are set
 *                     (4078-4089); 0: no gradients.
 * prk_draw_objects_setup draws with explicit setup flags (setup < 0: derived
 * from the draw, as prk_draw_objects).  Combinations the reference leaves
 * undefined are PRK_ERR_UNSUPPORTED: a Phong draw (any semantics) of edges
 * set up without PRK_SETUP_PHONG (MinNormal never written, 4012-4064), and a
 * textured draw of edges set up without PRK_SETUP_BITMAP (UGradient,
 * VGradient, OneOverZGradient never written, 4078-4089).  So
 * FillEdgeTable(..., 1) + DrawModel(..., Bitmap = 0, Phong = 0) interpolates
 * the raw colours unlit, and an object with a Bitmap drawn by
 * DrawModel(..., Bitmap = 0, Phong = 0) after FillEdgeTable(..., 0) gets the
 * white-based lighting. */
enum prk_setup {
    PRK_SETUP_PHONG = 1,
    PRK_SETUP_BITMAP = 2
};
int prk_draw_objects_setup(prk_context *ctx, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                           uint32_t tris_per_object, const float P[3], int32_t semantics, int32_t phong,
                           int32_t texture, int32_t setup);

/* edge_info (projekt.h:17-37) without its list pointer: what the reference's
 * FillEdgeTable leaves in EdgeMemory and DrawModel* walk.  prk_draw_edges
 * draws one object from such a list, already sorted by YMin as FillEdgeTable
 * leaves it, exactly as DrawModelOptimized(RenderQueue,...) (3615-3871), the
 * single-thread overload (2350-3358) or DrawModel (162-601, PRK_SEM_SCALAR)
 * walks it.  The winner id of its pixels is the draw's position in the
 * frame's triangle numbering (it counts as one). */
typedef struct prk_edge {
    int32_t YMax;
    float XMin, ZMin, OneOverZMin, Gradient, ZGradient, OneOverZGradient;
    int32_t YMin;
    float UMin, VMin, UGradient, VGradient;
    int32_t Left;
    float MinColor[4], ColorGradient[4], MinNormal[3], NormalGradient[3];
} prk_edge;
int prk_draw_edges(prk_context *ctx, const prk_edge *edges, uint32_t edge_count, int32_t semantics, int32_t phong,
                   int32_t texture);
/* A batch of such lists in one call, in the packed layout prk_edge_records
 * produces: list o is records[sum(counts[0..o)) ...], counts[o] entries long.
 * Each list is drawn exactly as one prk_draw_edges call of it would draw it,
 * the lists in order, one after another, at this point of the frame's
 * submission order; the records are copied at the call.  Semantics, phong and
 * texture are checked as prk_draw_edges checks them.
 *
 * Winner ids: list o takes id base + o of the frame's numbering, base being
 * the id the next draw would have had.  EVERY list takes one id, empty or
 * not, so ids map to list indices -- unlike prk_draw_edges, which takes no id
 * for an empty list (a loop of prk_draw_edges calls over the same lists
 * numbers the lists after an empty one differently).
 *
 * A list whose YMin is non-decreasing (what FillEdgeTable's MergeSort and
 * prk_edge_records leave) and whose edges lie in FillEdgeTable's value range
 * (0 <= YMin <= YMax, Left 0 or 1) is walked as a triangle object of as many
 * edges is: the sorted insertion cursor inserts on every row exactly the
 * edges the reference's whole-list scan (3654-3713) inserts, in the same
 * order, so the frame is the same, and long lists take the parallel walks
 * (144 edges or more: the large-object walks, counted by
 * prk_debug_walk_routes and prk_stats.objects_chunked / objects_walked).
 * Any other list is walked as prk_draw_edges walks it, by one thread that
 * scans the whole list on every row.
 *
 * PRK_ERR_ARG: a NULL context, NULL counts with list_count > 0, NULL records
 * with a non-zero total, a bad semantics or texture, ids past the frame's
 * numbering.  PRK_ERR_UNSUPPORTED: as prk_draw_edges.  PRK_ERR_LIMIT: the
 * frame's batch records or lists pass 31 bits (prk_flush returns it when a
 * pass's edge slots do).  list_count == 0: PRK_OK, nothing recorded.  On any
 * error nothing is recorded. */
int prk_draw_edge_lists(prk_context *ctx, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                        int32_t semantics, int32_t phong, int32_t texture);

/* One span end as line_render_work carries it by value (projekt.h:65-74) or
 * thread_edge_info holds it (39-63): what FillLineOptimized /
 * FillLinesOptimized read of an edge (1543-1835; 648-670). */
typedef struct prk_span_end {
    float XMin, ZMin, OneOverZMin, UMin, VMin;
    float MinColor[4];
    float MinNormal[3];
} prk_span_end;
typedef struct prk_span {
    prk_span_end Left, Right;
    int32_t Row;
} prk_span;
/* Draw caller-built spans (the work records DoLineRenderWork /
 * DoBufferLineRenderWork run, 2336-2348), in order, each with
 * FillLineOptimized's span body.  Each span counts as one triangle id.
 * prk_span_records (below) returns the spans of batches of edge lists. */
int prk_draw_spans(prk_context *ctx, const prk_span *spans, uint32_t count, int32_t semantics, int32_t phong,
                   int32_t texture);

/* Execute every recorded draw, in submission order, into the bound target
 * (the reference's Platform.CompleteAllWork).  `stream` is a hipStream_t or
 * NULL for the library's own stream.  Asynchronous w.r.t. the host: it
 * returns once the frame is queued, without waiting for its binning.  The
 * frame's bin entry count (scratch sizing, prk_stats.bin_entries) is read by
 * the next call that needs it: the next prk_flush, prk_synchronize,
 * prk_resolve, prk_target_download / upload / clear, prk_get_stats, a texture
 * or geometry update, a gather, prk_target_alloc, or prk_target_bind (any
 * target: rebinding waits on the host for the previous frame's count, so a
 * caller rotating its own buffers pays that wait at the bind).  A frame whose entries overflowed the scratch is
 * re-run there, into the target and with the camera, tile and clear it was
 * queued with, before anything else is queued — so a caller that reads the
 * target through its own device pointers (not prk_target_download) after a
 * flush calls prk_synchronize first.  (The first frame of a context is
 * counted at once.) */
int prk_flush(prk_context *ctx, void *stream);
/* Drop recorded draws without executing them. */
int prk_reset_draws(prk_context *ctx);
int prk_synchronize(prk_context *ctx);
/* Resolve the last flush's pending bin count (re-running an overflowed frame,
 * as above) and make `stream` (a hipStream_t of the context's device, or NULL
 * for none) wait for the end of the context's last frame, without blocking
 * the host on the frame's raster.  For callers that read the target through
 * their own device pointers on their own stream (a torch RCCL strip gather):
 * the asynchronous counterpart of prk_synchronize. */
int prk_resolve(prk_context *ctx, void *stream);
int prk_get_stats(prk_context *ctx, prk_stats *out); /* waits for timed flushes */
int prk_timing_reset(prk_context *ctx);

/* Debug/test: per-pixel winning triangle index of the last flush (-1 = none),
 * rows [row0,row1).  Requires prk_set_debug(ctx, 1) before the flush. */
int prk_set_debug(prk_context *ctx, int32_t enable);
int prk_download_winners(prk_context *ctx, int32_t *winners_host);
/* Debug: the raster kernels' phase cycle counters (written only by builds
 * with -DPRK_PROF; zeroed by prk_timing_reset), n <= 16. */
int prk_debug_counters(prk_context *ctx, uint64_t *out, int32_t n);
/* Debug/test: which walk the large objects (whole-object draws of 64
 * triangles or more) of the most recent flush that had any were given, from
 * the host's bookkeeping (no kernel reports in).  out[0..4]: objects in the
 * workgroup walk's LDS slot classes of 62 / 126 / 254 / 510 / 1022 entries;
 * out[5]: the huge-object walk with the list in LDS; out[6]: the same with
 * the list in device memory; out[7]: one wave each; out[8]: objects whose
 * sizes the many-workgroup histogram counted; out[9..11]: the first large
 * object's most active edges, rows and list entries as read back (int32_t
 * bits; INT32_MAX: past the histogram).  n <= 12 words are written. */
int prk_debug_walk_routes(prk_context *ctx, uint32_t *out, int32_t n);
/* Debug/test: which walk the lists of the most recent prk_advance_edge_lists,
 * prk_span_records or prk_row_records call were given, from the host's
 * bookkeeping (no kernel reports in).  out[0]: lists walked by one GPU thread
 * each (empty lists among them); out[1..5]: lists walked by a workgroup each,
 * in the slot classes of 62 / 126 / 254 / 510 / 1022 entries.  A refused call
 * leaves the words of the call before it.  n <= 6 words are written. */
int prk_debug_list_routes(prk_context *ctx, uint32_t *out, int32_t n);
/* Debug/test: the tile binning of the last per-triangle pass (draws of one
 * triangle per object) of the most recent flush, as the binning kernels left
 * it.  Requires prk_set_debug(ctx, 1) before that flush; PRK_ERR_ARG before
 * any such flush, without debug, or when the flush had no per-triangle pass.
 * The pending entry count is resolved first: a pass whose entries overflowed
 * the scratch is re-run, and the call answers for the re-run (info->rerun).
 * It then waits for the frame and copies to host memory; no kernel runs for
 * it, and a flush without debug records nothing for it.
 *
 * Triangles are numbered from 0 within the pass, pairs (bin entries) in
 * triangle order: triangle g's entries are pairs tri_off[g] .. tri_off[g] +
 * tri_n[g] - 1, in the order rectangle row-major (ty, then tx), then the
 * column-0 row-overflow tiles oty0..oty1 that are not in the rectangle.
 *   tri_n    [tri_count]      entries of each triangle (0: culled or outside)
 *   ranges   [tri_count][8]   tx0 ty0 tx1 ty1 oty0 oty1 pad0 pad1 (an empty
 *                             rectangle or overflow range reads 1, 0; pad0 /
 *                             pad1: the band rows [r0, r1) the triangle can
 *                             cover, meaningful only where tri_n != 0)
 *   tri_off  [tri_count + 1]  first pair of each triangle; the last word is
 *                             the entry count
 *   listed   [tri_count]      1 where the binning wrote the three above.  A
 *                             whole-frame pass writes every triangle.  A row
 *                             band's pass writes only the triangles with
 *                             entries (its run lists); the others read
 *                             tri_n 0, an empty range and tri_off UINT32_MAX
 *   offs     [ntiles + 1]     bin starts, tile = ty * tiles_x + tx
 *   bins     [entry_count][2] (triangle, pair) of every bin slot, grouped by
 *                             row class within windows of 2048 slots, in no
 *                             particular order within a class
 *   pair_tri [entry_count]    the triangle of each pair
 * Any of the array pointers may be NULL (not wanted).  Sizing follows
 * prk_edge_records: *info is always written; a wanted array whose capacity
 * (tri_capacity triangles, tile_capacity tiles, entry_capacity entries) is
 * short of the frame's gives PRK_ERR_ARG and copies nothing. */
typedef struct prk_bins_info {
    int32_t tile_w, tile_h, tiles_x, tiles_y; /* the frame's tile (as widened to fit the sort) */
    int32_t row0, row1;                       /* the band the pass drew */
    uint32_t tri_count, entry_count;
    uint32_t rerun;                           /* 1: the pass overflowed its scratch and was run again */
    uint32_t band_per;                        /* 0: a whole-frame pass.  Else a row band, binned through run
                                               * lists (see listed) of 2048 triangles: the runs one chunk of
                                               * the counting sort takes (1..64) */
} prk_bins_info;
int prk_debug_bins(prk_context *ctx, prk_bins_info *info, uint32_t *tri_n, uint16_t *ranges, uint32_t *tri_off,
                   uint8_t *listed, uint64_t tri_capacity, uint32_t *offs, uint64_t tile_capacity,
                   uint32_t *bins, uint32_t *pair_tri, uint64_t entry_capacity);

/* Test: the raster kernels divide several values by one divisor through a
 * shared reciprocal; this checks n hashed (x, d) draws and
 * normalisations on `device` against the compiler's own division, bit for
 * bit.  *mismatches = quotient mismatches | normalisation mismatches << 32. */
int prk_selftest_div(int32_t device, uint32_t n, uint64_t seed, uint64_t *mismatches);
/* The same, and how many 64-lane waves took the shared-reciprocal path:
 * fast_waves[0] of the quotient, fast_waves[1] of the normalisation.  Odd
 * waves draw every lane inside the fast range with non-zero numerators, so
 * half of the waves take it by construction; even waves mix lanes, zeros and
 * out-of-range exponents.  prk_selftest_div is this call without the counts. */
int prk_selftest_div_paths(int32_t device, uint32_t n, uint64_t seed, uint64_t *mismatches, uint32_t fast_waves[2]);

/* Test: one arithmetic primitive of the kernels (csrc/prk_device.h) on the
 * caller's words.  Element i is computed by thread i of a 1-D launch of 256
 * threads a block, so elements 64k .. 64k+63 share a wave.  Every value
 * travels as a raw 32-bit word (float bits, or an integer).  a, b, c, d: host
 * inputs of n words; PRK_ERR_ARG when one the op reads is NULL, the others
 * are ignored.  out0..out2: host outputs of n words, out0 required, the
 * others may be NULL (words an op does not produce are 0).  fast: n words or
 * NULL: for DIV_ALL* and NORMALIZE_DIV bit 0 is set when the element's wave
 * took the shared-reciprocal path, as reported by the function itself; 0 for
 * every other op.  n <= 2^24.  A NaN result may differ from x86's in sign and
 * payload.  tests/test_gpu_arith.py holds each op to a host reference written
 * from the definitions (tests/arithref.py). */
enum {
    PRK_OP_DIV = 0,            /* out0 = a / b */
    PRK_OP_DIV_ALL1 = 1,       /* div_all<1>: out0 = a / b */
    PRK_OP_DIV_ALL3 = 2,       /* div_all<K>, K = 3, 4, 5, 7, 8 (every size the raster kernels use): the */
    PRK_OP_DIV_ALL4 = 3,       /* numerators a, b, c, a, b, ... over the divisor d; out0..2 = a / d, b / d, */
    PRK_OP_DIV_ALL5 = 4,       /* c / d; bit 1 of fast is set when a later quotient of the same numerator */
    PRK_OP_DIV_ALL7 = 5,       /* differs from them in any bit */
    PRK_OP_DIV_ALL8 = 6,
    PRK_OP_DIV_FOCAL = 7,      /* out0 = div_focal of a by the focal length b (its not-a-power-of-two branch) */
    PRK_OP_SQRT = 8,           /* out0 = sqrtf(a) */
    PRK_OP_SQRT_MID = 9,       /* out0 = sqrt_mid(a) */
    PRK_OP_NORMALIZE_DIV = 10, /* out0..2 = normalize_div(a, b, c) */
    PRK_OP_NORMALIZE_RCP = 11, /* out0..2 = normalize_rcp(a, b, c) */
    PRK_OP_CVTT_S32 = 12,      /* out0 = cvtt_s32(a) */
    PRK_OP_ROUND_S32 = 13,
    PRK_OP_ROUND_U32 = 14,
    PRK_OP_CVT_RNE_S32 = 15,
    PRK_OP_MINPS = 16,         /* out0 = minps(a, b) */
    PRK_OP_MAXPS = 17,
    PRK_OP_CLAMP01 = 18,       /* out0 = clamp01(a) */
    PRK_OP_MUL16_TRICK = 19,   /* out0 = mul16_trick(a, b) */
    PRK_OP_U8_UNIT = 20,       /* out0 = u8_unit(a), a in [0, 255] */
    PRK_OP_ZKEY = 21,          /* out0 = zkey(a), out1 = zkey_z(out0) */
    PRK_OP_PAIR_TAG = 22,      /* out0 = pair_tag(a, b != 0); out1, out2 = tag_pair(out0): j (0 when false), result */
    PRK_OP_TAG_PAIR = 23,      /* out0, out1 = tag_pair(a): j (0 when false), result */
    PRK_OP_SPAN_ENDS = 24,     /* span_ends(LX = a, RX = b, W = c & 0x7FFFFFFF, st = c >> 31): MinX, MaxX, XDiff */
    PRK_OP_SPAN_OFFSET = 25,   /* the same call: out0 = XOffset, out1 = its result (false: MinX.. are 0 above) */
    PRK_OP_COUNT = 26
};
int prk_selftest_ops(int32_t device, int32_t op, uint32_t n, const uint32_t *a, const uint32_t *b,
                     const uint32_t *c, const uint32_t *d, uint32_t *out0, uint32_t *out1, uint32_t *out2,
                     uint32_t *fast);

/* Test: the span path's radix sort and exclusive scans (csrc/prk_sort.hip)
 * on the caller's host arrays, synchronously on `device`, no context needed.
 * Every device buffer is followed by a guard region of a known pattern, the
 * outputs and the temp buffer start out as that pattern, and the temp buffer
 * is exactly as large as the size query answered.  *damage gets the
 * PRK_DAMAGE_* bits, found by copying back and comparing on the host: an
 * input buffer changed, the guard after an output changed, the guard after
 * the temp buffer changed.  tests/test_gpu_sort_scan.py holds both to the
 * definitions in tests/sortref.py, every word equal and *damage == 0.
 *
 * prk_selftest_sort: `repeats` (>= 1) stable sorts of the n (keys[i],
 * vals[i]) pairs with the same temp buffer, left as the sort before left it;
 * the outputs are reset to the guard pattern before each.  The order is by
 * the keys' low 8 * ceil(end_bit / 8) bits (whole 8-bit digits; the bits
 * above are ignored and carried).  keys_out / vals_out: n words each, of the
 * last sort.  PRK_ERR_ARG: a NULL pointer, repeats == 0, a bad device.  A
 * size the sort refuses (end_bit > 64, n > 2^30 - 1) returns the status of
 * hipErrorInvalidValue (PRK_ERR_DEVICE) before anything is allocated or read.
 *
 * prk_selftest_scan: out[i] = in[0] + ... + in[i - 1] modulo 2^width over n
 * words of `width` (32 or 64) bits; in and out are distinct device buffers.
 * PRK_ERR_ARG: a NULL pointer, another width, a bad device. */
enum { PRK_DAMAGE_INPUT = 1, PRK_DAMAGE_OUTPUT_GUARD = 2, PRK_DAMAGE_TEMP_GUARD = 4 };
int prk_selftest_sort(int32_t device, uint32_t n, uint32_t end_bit, const uint64_t *keys, const uint32_t *vals,
                      uint32_t repeats, uint64_t *keys_out, uint32_t *vals_out, uint32_t *damage);
int prk_selftest_scan(int32_t device, int32_t width, uint32_t n, const void *in, void *out, uint32_t *damage);
/* Test: prk_visibility_*'s kernels (csrc/prk_visibility.hip) on the caller's
 * n winner words and id_count ids, synchronously on `device`, no context
 * needed, guarded and compared as above (the flags the scans read count as
 * temp).  counts: id_count words; pix_prefix, vis_prefix: id_count + 1 words;
 * ids: room for id_count words, *visible_out (= vis_prefix[id_count]) of them
 * written.  *atomics_out: the atomic adds the histogram issued -- counted by
 * an instantiation of its own, which this call alone runs (the one behind
 * prk_visibility_* carries no counter).  PRK_ERR_ARG: a NULL pointer (winners
 * with n > 0, counts / ids with id_count > 0, any other), a bad device,
 * id_count > 2^32 - 16.  tests/test_gpu_visibility.py holds every word to
 * tests/visref.py, *damage == 0. */
int prk_selftest_visibility(int32_t device, uint32_t n, const int32_t *winners, uint32_t id_count,
                            uint32_t *counts, uint32_t *pix_prefix, uint32_t *vis_prefix, uint32_t *ids,
                            uint32_t *visible_out, uint64_t *atomics_out, uint32_t *damage);
/* Test: prk_geometry_select's three stages (csrc/prk_select.hip: the choice,
 * the scan, the emit pass) on host-supplied inputs, synchronously on `device`,
 * no context needed, guarded and compared as above.  pix_prefix: id_count + 1
 * words, read when item_pixels is NULL (else it may be NULL).  The source is
 * src_tris triangles of the arrays given (src_vertices required when any
 * level has triangles; the others may be NULL).  The destination is dst_tris
 * triangles of every array the source has, on the device pre-filled with the
 * guard pattern (bytes of 0xA5) and returned whole: the words outside
 * [dst_first_tri, dst_first_tri + total) come back as that pattern.  A dst_*
 * pointer is required where the source has the array and ignored where not.
 * chosen: item_count words; out_first: item_count + 1 words.  *damage: an
 * input (a table, pix_prefix, item_pixels, a source array) changed or its
 * guard did; the guard after chosen, the scan's output or a destination array
 * changed; the guard after the counts, the runs or the scan's scratch changed.
 * PRK_ERR_ARG: a NULL required pointer, a bad device, prk_geometry_select's
 * table errors (with id_count as the frame's), a worst-case end past dst_tris.
 * PRK_ERR_LIMIT as there.  tests/test_gpu_select.py holds every word to
 * tests/selectref.py, *damage == 0. */
int prk_selftest_select(int32_t device, const uint32_t *pix_prefix, uint32_t id_count,
                        const prk_select_item *items, uint32_t item_count,
                        const prk_select_level *levels, uint32_t level_count,
                        const prk_xform *xforms, uint32_t xform_count, const uint32_t *item_pixels,
                        const float *src_vertices, const float *src_colors, const float *src_normals,
                        const float *src_uvs, uint32_t src_tris, uint32_t dst_first_tri, uint32_t dst_tris,
                        float *dst_vertices, float *dst_colors, float *dst_normals, float *dst_uvs,
                        int32_t *chosen, uint32_t *out_first, uint64_t *total_tris_out, uint32_t *damage);
/* Test: prk_visibility_bounds' two kernels (csrc/prk_bounds.hip) on
 * host-supplied inputs, synchronously on `device`, no context needed, guarded
 * and compared as above.  z: the band's width * (row1 - row0) words, placed
 * z_offset floats (at most 1024) into their device buffer, so that 1 gives the
 * kernel a base that is only 4-byte aligned.  zmin: (width + 7) / 8 columns by
 * (row1 + 7) / 8 - row0 / 8 rows; pixels: count words.  *damage: an input
 * changed or its guard did; the guard after zmin or pixels changed.
 * PRK_ERR_ARG: a NULL required pointer (P may be NULL: 0), a bad device or
 * band, a bound's xform >= xform_count.  PRK_ERR_LIMIT as
 * prk_visibility_bounds.  tests/test_gpu_bounds.py holds every word to
 * tests/boundsref.py, *damage == 0. */
int prk_selftest_bounds(int32_t device, const float *z, int32_t width, int32_t height, int32_t row0,
                        int32_t row1, uint32_t z_offset, const prk_transform *transform, const float *P,
                        const prk_bound *bounds, uint32_t count, const prk_xform *xforms,
                        uint32_t xform_count, float *zmin, uint32_t *pixels, uint32_t *damage);

/* The bound target (any pointer may be NULL) and the context's device and
 * own stream (a hipStream_t; prk_flush(ctx, NULL) runs on it). */
int prk_get_target(prk_context *ctx, void **color, int32_t *pitch_bytes, float **zbuf, int32_t *width,
                   int32_t *height, int32_t *row0, int32_t *row1);
int prk_get_device(prk_context *ctx, int32_t *device, void **stream);

/* ---- Multi-GPU: row bands and the frame gather ------------
 * The reference has no distribution; this is the build's.  Rank r of N binds
 * (or allocates) a target for frame rows prk_band_rows(H, r, N) and records
 * the same draws as every other rank: each rank bins all triangles against
 * its band, so every pixel has one owner and submission order holds.  The
 * only exchange is the gather of the band strips into one frame on rank 0
 * (colour, and z when with_z).  A caller that wants the frame in host memory
 * needs no gather: each rank downloads its band into its rows.
 *
 * One process per GPU: RCCL over xGMI.  Rank 0 makes a unique id
 * (PRK_COMM_ID_BYTES bytes), the caller hands it to every rank (its own
 * channel: MPI, a socket, torch.distributed ...), and every rank creates its
 * communicator with prk_comm_init.  librccl is loaded on first use;
 * PRK_ERR_UNSUPPORTED when it is absent (prk_comm_available() == 0). */
#define PRK_COMM_ID_BYTES 128
typedef struct prk_comm prk_comm;
int prk_band_rows(int32_t height, int32_t rank, int32_t nranks, int32_t *row0, int32_t *row1);
int prk_comm_available(void);
int prk_comm_unique_id(void *id);
int prk_comm_init(prk_context *ctx, const void *id, int32_t nranks, int32_t rank, prk_comm **out);
/* One process driving N GPUs: one communicator per context (ncclCommInitAll). */
int prk_comm_init_all(prk_context *const *ctxs, int32_t n, prk_comm **comms_out);
int prk_comm_destroy(prk_comm *comm);
/* Every rank's band into rank 0's device frame (W x H; colour rows of
 * frame_pitch == 4*W bytes, z rows of W floats).  Rank 0 passes the frame,
 * other ranks pass NULL (their bands must be packed: pitch 4*W).  Enqueued on
 * `stream` (NULL: the context's own stream) after the work already there;
 * rank 0's own band is copied unless its target is the frame's slice. */
int prk_gather_frame(prk_context *ctx, prk_comm *comm, int32_t with_z, void *frame_color, int32_t frame_pitch,
                     float *frame_z, void *stream);
/* The same for N contexts of one process, as one RCCL group (ctxs[r] and
 * comms[r] are rank r; each rank's ops go on its context's own stream). */
int prk_gather_frame_all(prk_context *const *ctxs, prk_comm *const *comms, int32_t n, int32_t with_z,
                         void *frame_color, int32_t frame_pitch, float *frame_z);
/* One process driving N GPUs without RCCL: each band's device copies its
 * strip into ctxs[0]'s frame over xGMI (peer access), after the work on its
 * own stream; ctxs[0]'s own stream waits for every copy (prk_synchronize on
 * ctxs[0] waits for the whole frame).  Contexts may share a device. */
int prk_gather_frame_local(prk_context *const *ctxs, int32_t n, int32_t with_z, void *frame_color,
                           int32_t frame_pitch, float *frame_z);

/* Tunables (testing / benchmarking). tile_w must be a power of two >= 8,
 * 64 <= tile_w * tile_h <= 8192.  Without a call the context picks its tile
 * itself: 256x8, or 32x8 / 64x8 once a frame shows fewer than 64 / 8 bin
 * entries per 256x8 tile, or 512x8 once an all-AVX frame shows 4.5 or more
 * entries a triangle (large triangles; a band: per its share of the
 * triangles), kept while the triangle count and the band stay within 2x.
 * Results never depend on the tile. */
int prk_set_tile(prk_context *ctx, int32_t tile_w, int32_t tile_h);

/* Host utility: FillEdgeTable's return value (projekt.cpp:3882-4121, 4119)
 * for one object of vertex_count vertices (positions v3, three per
 * triangle) at offset P (may be NULL: 0) under transform T: the number of
 * edges of its front-facing triangles (3926-3943) with MaxY > 0 (3968) and
 * MinY != MaxY (4066), 0 for an object that draws nothing.  The drop-in's
 * FillEdgeTable returns it at the call; the setup runs on the GPU. */
int prk_fill_edge_count(const float *vertices, uint32_t vertex_count, const float P[3],
                        const prk_transform *transform, uint32_t *count_out);

/* Host utilities: edge_info records in the caller's own memory (the drop-in's
 * opt-in record mode, projekt.h PRK_SetEdgeRecords).  The frame never comes
 * from these: the GPU sets objects up from their vertices (prk_draw_objects)
 * and draws edge lists from their copies (prk_draw_edges).  They reproduce
 * what the reference leaves in the caller's memory, in place: `edges` is an
 * array of elements of `stride` bytes whose first 108 bytes are edge_info's
 * 27 fields in prk_edge order and whose list pointer (edge_info.Next) sits at
 * byte `next_offset` (x86-64 edge_info: stride 120, next_offset 112).  A field
 * the reference does not write keeps the caller's bytes.
 *
 * prk_fill_edge_records: FillEdgeTable (projekt.cpp:3894-4117) of one object
 * of vertex_count vertices at offset P under T / L, with its own PhongShading
 * and Bitmap != 0 as PRK_SETUP_* bits in `setup`: the visible edges written
 * at edges[0 ..), Next = NULL, then MergeSort (2-72) with sort_memory
 * (Commands->SortMemory, >= count elements; NULL: a library buffer) as its
 * scratch.  *count_out = FillEdgeTable's return value (4119). */
int prk_fill_edge_records(const float *vertices, const float *colors, const float *normals, const float *uvs,
                          uint32_t vertex_count, const float P[3], const prk_transform *transform,
                          const prk_light_data *lights, int32_t setup, void *edges, size_t stride,
                          size_t next_offset, void *sort_memory, uint32_t *count_out);
/* prk_advance_edge_records: what DrawModel* (every overload: the same list
 * walk and edge step, 3654-3869, 3811-3829) leaves in the list it drew over a
 * frame of `height` rows: every edge stepped once per row it was paired on,
 * the list pointers as the walk left them (real addresses into `edges`).
 * The reference's crashes are pinned as the draw pins them (prk.h above): a
 * first-pair swap moves the list head (P3), an emptied list skips the row. */
int prk_advance_edge_records(void *edges, uint32_t count, size_t stride, size_t next_offset, int32_t height);

/* FillEdgeTable's records (projekt.cpp:3894-4117) of consecutive objects of
 * tris_per_object triangles (the last may be smaller), set up on the GPU
 * under prk_set_camera's transform and lights with explicit PRK_SETUP_* bits.
 * Object o's records, MergeSorted (2-72), are packed one after another:
 * records[sum(counts[0..o)) ...], counts[o] = FillEdgeTable's return value.
 * Every record is what prk_fill_edge_records leaves in zero-filled memory:
 * a field the reference does not write for this setup is all-zero bits.
 * records == NULL: counts and *total_out only.  Needs no render target,
 * records no draw, touches no recorded draw; synchronous.
 *
 * For a caller that wants the records of many objects at once (to keep them,
 * or to draw them later: all at once with prk_draw_edge_lists, which takes
 * records and counts as they are, or one list at a time with
 * prk_draw_edges).  PRK_ERR_ARG: a NULL context or
 * total_out, a bad geometry handle or triangle range, tris_per_object == 0,
 * setup outside 0..3, a call before any prk_set_camera, or a capacity (in
 * records) below the total -- *total_out is written all the same, so the
 * caller can size its buffer and call again.  PRK_ERR_LIMIT: the object
 * index, the 31-bit YMin and the MergeSort path bits (bit length of
 * 3 * tris_per_object, plus one) do not fit the 64-bit sort key.  Frames in
 * flight finish first.  The drop-in's record mode (projekt.h) does not use
 * this: there FillEdgeTable must leave the records in the caller's own
 * memory before it returns and keep the caller's bytes in unwritten fields,
 * which a batched call cannot do.  The lists DrawModel* leaves come from
 * prk_advance_edge_lists (below) for such a batch; the record mode still
 * uses the host call prk_advance_edge_records there, since DrawModel* must
 * leave its list in the caller's memory at its return, with real addresses. */
int prk_edge_records(prk_context *ctx, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                     uint32_t tris_per_object, const float P[3], int32_t setup,
                     prk_edge *records, uint64_t capacity, uint32_t *counts, uint64_t *total_out);

/* Record handles: a batch of lists in prk_edge_records' packed layout that
 * stays in device memory -- the reference's EdgeMemory of a static mesh:
 * FillEdgeTable once, DrawModel* from the records every frame.  The context
 * owns the batch and names it by a handle >= 0, as geometries and textures;
 * the host keeps each list's edge count and whether it is inside
 * prk_draw_edge_lists' sorted rule (8 bytes a list, computed on the device
 * when the handle is made), and no copy of the records.  A handle belongs to
 * its context (each band context makes its own).
 *
 * prk_records_from_geometry: prk_edge_records' records of the same arguments,
 * written into the handle's buffer instead of the caller's -- no record
 * crosses to the host.  Arguments and errors are prk_edge_records' (minus
 * records / capacity / counts); *list_count_out = the objects, *total_out =
 * the records (either may be NULL).  Synchronous; needs no target, records no
 * draw, touches no recorded draw and no prk_stats; frames in flight finish
 * first.  tri_count == 0 makes a handle of no lists.
 *
 * prk_records_upload: the same for a caller's own lists (records / counts as
 * prk_draw_edge_lists takes them), copied once at the call; the host does not
 * read the records.  PRK_ERR_ARG: NULL counts with list_count > 0, NULL
 * records with a non-zero total.  PRK_ERR_LIMIT: records or lists pass 31 bits.
 *
 * prk_records_info / prk_records_lists: the handle's lists and records; each
 * list's count and sorted-rule flag (1: inside the rule), list_count words
 * each, either pointer may be NULL.  Host bookkeeping: no device work.
 *
 * prk_records_download: the packed records, word for word what
 * prk_edge_records returns for the arguments the handle was made from (or
 * what was uploaded).  PRK_ERR_ARG: capacity (in records) below the total.
 *
 * prk_records_destroy: frames in flight finish first (as prk_geometry_update
 * waits).  PRK_ERR_ARG while a recorded, unflushed draw names the handle
 * (prk_reset_draws releases it), and for a bad or destroyed handle.
 * prk_destroy frees every handle. */
int prk_records_from_geometry(prk_context *ctx, int32_t geometry, uint32_t first_tri, uint32_t tri_count,
                              uint32_t tris_per_object, const float P[3], int32_t setup, int32_t *handle_out,
                              uint32_t *list_count_out, uint64_t *total_out);
int prk_records_upload(prk_context *ctx, const prk_edge *records, const uint32_t *counts, uint32_t list_count,
                       int32_t *handle_out);
int prk_records_info(prk_context *ctx, int32_t handle, uint32_t *list_count_out, uint64_t *total_out);
int prk_records_lists(prk_context *ctx, int32_t handle, uint32_t *counts, uint32_t *sorted_flags);
int prk_records_download(prk_context *ctx, int32_t handle, prk_edge *records, uint64_t capacity);
int prk_records_destroy(prk_context *ctx, int32_t handle);
/* One draw of lists [first_list, first_list + list_count) of a handle, at
 * this point of the frame's submission order: the frame, the winner ids
 * (base + o, one per list, empty or not), the semantics / phong / texture
 * checks and the routing (the sorted rule, the 144-edge threshold, the
 * parallel walks) are exactly prk_draw_edge_lists' for the same lists passed
 * from host memory -- but nothing is copied: the flush reads the records where
 * they are, and its staging holds the pass's tables only.  A handle may be
 * drawn any number of times, in one frame or across frames, mixed with every
 * other kind of draw.  PRK_ERR_ARG: a bad handle, a range past the handle's
 * lists, and prk_draw_edge_lists' cases.  PRK_ERR_UNSUPPORTED: as
 * prk_draw_edges.  list_count == 0: PRK_OK, nothing recorded.  On any error
 * nothing is recorded. */
int prk_draw_records(prk_context *ctx, int32_t handle, uint32_t first_list, uint32_t list_count,
                     int32_t semantics, int32_t phong, int32_t texture);
/* Debug/test: the bytes the most recent whole-object pass (any flush with a
 * whole-object, edge, span or record draw) copied from the host in its one
 * staging upload: the pass's tables, and the records of its prk_draw_edges /
 * prk_draw_edge_lists / prk_draw_spans draws -- none for prk_draw_records
 * and none for prk_draw_span_records (below). */
int prk_debug_stage_bytes(prk_context *ctx, uint64_t *bytes_out);

/* What DrawModel* leaves in the lists of a batch (projekt.cpp:3654-3869),
 * walked on the GPU: records / counts in the packed layout of
 * prk_edge_records and prk_draw_edge_lists, all pointers host memory.  List
 * o's part of records_out (the same layout; may be `records` itself: in
 * place) and of next_out (one word per record, or NULL) is what
 * prk_advance_edge_records(mem, counts[o], 120, 112, height) leaves in an
 * edge_info array `mem` made of list o with every Next NULL (what
 * FillEdgeTable leaves, 4094): the 27 fields word for word, and next_out[i]
 * = the Next of record i as an index within its own list, -1 for NULL.  One
 * allowance: where the host's word is a NaN the word here is a NaN too, of
 * any sign and payload (Normalize of a zero normal is inf * 0: x86's default
 * NaN has the sign bit set, gfx950's has not).  Such NaNs sit in normals and
 * colours only, never in what orders the list; every word that is not a NaN
 * on the host is equal.
 *
 * Only lists inside prk_draw_edge_lists' sorted rule are taken (YMin
 * non-decreasing, 0 <= YMin <= YMax, Left 0 or 1: what FillEdgeTable's
 * MergeSort and prk_edge_records leave): there the sorted insertion cursor
 * inserts what the reference's whole-list scan inserts, in its order.  Any
 * other list goes to prk_advance_edge_records.  A list is walked over at
 * most `height` rows, by one GPU thread -- or, when that thread's walk would
 * be long (its steps, below, reach a measured threshold; PRK_ADV_WG_MIN_STEPS
 * in the environment replaces it) and the list never links
 * more than 1022 edges at once, by one workgroup with the list in LDS: a mesh
 * passed as ONE list.  A batch may mix both; the results are the same words
 * (prk_debug_list_routes tells which walk a call's lists took).
 *
 * Synchronous; needs no render target, records no draw, touches no recorded
 * draw and no prk_stats; frames in flight finish first.  PRK_ERR_ARG: a NULL
 * context, NULL counts with list_count > 0, NULL records or records_out with a
 * non-zero total, height < 0.  PRK_ERR_UNSUPPORTED: a list outside the sorted
 * rule.  PRK_ERR_LIMIT: the total passes 31 bits, height > 65536, or a list's
 * walk is too long: its edge-rows, the sum over its edges of max(0, min(YMax,
 * height) - YMin), pass 2^21 -- or, for a list one thread walks (in particular
 * every list that links more than 1022 edges at once), its edge-rows plus its
 * insertion scans, for every edge the edges still linked when it is inserted
 * (the earlier ones whose YMax is not below its YMin), pass 2^21 steps; the
 * workgroup walk inserts a row's edges as one batch and has no such scan.  The
 * cap keeps a call from holding the GPU for seconds (a thread walks 1.6 M
 * edge-rows a second); it is no tuned number.  list_count == 0 or a zero
 * total: PRK_OK.  On any error nothing is written to records_out or next_out.  The
 * spans the same walk queues on its way: prk_span_records (below). */
int prk_advance_edge_lists(prk_context *ctx, const prk_edge *records, const uint32_t *counts,
                           uint32_t list_count, int32_t height, prk_edge *records_out, int32_t *next_out);

/* The work records DrawModelOptimized(RenderQueue, ...) queues for the lists
 * of a batch (projekt.cpp:3756-3809), from the same walk on the GPU: records
 * / counts as for prk_advance_edge_lists, all pointers host memory.  For
 * every pair the walk meets on every row it emits one prk_span before it
 * steps the pair (3811-3829): Left is CurrentEdgeInList, Right is
 * NextEdgeInList as they stand on that row (XMin, ZMin, OneOverZMin, UMin,
 * VMin, MinColor, MinNormal), Row is RowIndex -- what prk_draw_spans and the
 * drop-in's DoLineRenderWork take.  List o's spans are packed at
 * spans[span_counts[0] + ... + span_counts[o - 1]] in queue order: rows
 * ascending, the pairs of a row in list order; a row with one listed edge
 * emits nothing, an odd list leaves its last edge unpaired.  span_counts
 * (list_count words, or NULL) gets every list's number of spans, *total_out
 * their sum.  Span k of list o is, word for word, the k-th work record a
 * walk of 3654-3869 over list o with every Next NULL queues; the walk's rows
 * and rules are prk_advance_edge_lists' ([YMin[0], min(max YMax, height)), no
 * band or target clip), and so is the one allowance: where the expected
 * MinColor or MinNormal word is a NaN the word here is a NaN of any sign and
 * payload.  Every other word, Row included, is equal.
 *
 * Calling pattern, as prk_edge_records: spans == NULL sizes -- span_counts
 * and *total_out are written by a counting walk that takes no span memory;
 * with spans and a `capacity` (in spans) below the total the call returns
 * PRK_ERR_ARG with span_counts and *total_out written and `spans` untouched.
 *
 * Only lists inside the sorted rule are taken.  A thread or a workgroup
 * walks a list, as in prk_advance_edge_lists: ConstructSphere as one list is
 * a workgroup's (DESIGN §4.4.6 has its times beside a host walk's).
 *
 * Synchronous; needs no render target, records no draw, touches no recorded
 * draw and no prk_stats; frames in flight finish first.  PRK_ERR_ARG: a NULL
 * context or total_out, NULL counts with list_count > 0, NULL records with a
 * non-zero record total, height < 0.  PRK_ERR_UNSUPPORTED: a list outside the
 * sorted rule.  PRK_ERR_LIMIT: the record total or list_count passes 31 bits,
 * height > 65536, a list's walk passes prk_advance_edge_lists' 2^21 cap (its
 * edge-rows; with its insertion scans where a thread walks it), or the batch's
 * span slots pass 31 bits (a list gets half its edge-rows, the sum over its
 * edges of max(0, min(YMax, height) - YMin): a span uses up one row of each of
 * two edges).  list_count == 0 or no records: PRK_OK, *total_out = 0,
 * span_counts zero.  On any error but the short capacity nothing is written to
 * spans or span_counts. */
int prk_span_records(prk_context *ctx, const prk_edge *records, const uint32_t *counts,
                     uint32_t list_count, int32_t height,
                     prk_span *spans, uint64_t capacity,
                     uint32_t *span_counts, uint64_t *total_out);

/* thread_edge_info, field for field (projekt.h:39-63): 24 words, 96 bytes */
typedef struct prk_row_pair {
    float LeftXMin, RightXMin, LeftZMin, RightZMin, LeftOneOverZMin, RightOneOverZMin,
          LeftUMin, RightUMin, LeftVMin, RightVMin;
    float LeftMinColor[4], RightMinColor[4], LeftMinNormal[3], RightMinNormal[3];
} prk_row_pair;
/* buffer_line_render_work's RowIndex / EdgeCount (EdgeCount counts PAIRS, 3521) */
typedef struct prk_row { int32_t RowIndex; uint32_t EdgeCount; } prk_row;

/* The row work records DrawModelOptimizedLines queues for the lists of a batch
 * (projekt.cpp:3362-3613: one buffer_line_render_work a row, followed by its
 * EdgeCount thread_edge_info pairs), from the same walk on the GPU: records /
 * counts / height are the packed batch of prk_advance_edge_lists, all pointers
 * host memory; the walk's rows, the sorted rule, the choice between a thread
 * and a workgroup per list and the 2^21 cap are that call's.  For list o
 * RowIndex runs over [YMin[0], min(max YMax, height)), ascending, and every
 * row the walk reaches emits one prk_row whose EdgeCount is the number of
 * pairs the walk meets on it -- 0 for a row with one listed edge (a one-edge
 * list emits nothing else; 3509-3516, 3604-3609).  A row on which the list is
 * empty after the head expiry (3467-3472, where the reference dereferences
 * NULL) emits no record: a row of the range is emitted if and only if some
 * edge of the list has YMin <= RowIndex < YMax.  Pair k of a row has Left* =
 * CurrentEdgeInList and Right* = NextEdgeInList as they stand before the
 * pair's step (3523-3542 precede 3546-3564), whatever their X order.  List o's
 * rows are packed at rows[row_counts[0] + ... + row_counts[o - 1]]; `pairs`
 * holds every pair of the batch in queue order (lists in order, rows
 * ascending, a row's pairs in list order), so row r's pairs start at the sum
 * of EdgeCount over the batch's earlier rows.  Pair k of the batch holds the
 * 24 values of span k of prk_span_records on the same input, re-ordered, and
 * the allowance is that call's: where the expected MinColor or MinNormal word
 * is a NaN the word here is a NaN of any sign and payload.  Every other word,
 * RowIndex and EdgeCount included, is equal. row_counts (list_count words, or
 * NULL) gets every list's number of rows, *row_total_out their sum,
 * *pair_total_out the batch's pairs.
 *
 * Calling pattern: rows == NULL and pairs == NULL size -- row_counts and both
 * totals are written by a counting walk that takes no row or pair memory;
 * with both arrays and either capacity (in records) below its total the call
 * returns PRK_ERR_ARG with row_counts and the totals written and both arrays
 * untouched.  One array NULL and the other not: PRK_ERR_ARG.
 *
 * Synchronous; needs no render target, records no draw, touches no recorded
 * draw and no prk_stats; frames in flight finish first.  PRK_ERR_ARG: a NULL
 * context or total pointer, NULL counts with list_count > 0, NULL records
 * with a non-zero record total, height < 0.  PRK_ERR_UNSUPPORTED: a list
 * outside the sorted rule, or a row with more than 1000 pairs (the reference
 * writes past its ThreadEdges[1000], 3403) -- the walk itself finds such a
 * row, so the counting call refuses it too.  PRK_ERR_LIMIT: whatever
 * prk_span_records refuses, or the batch's row slots pass 31 bits (a list
 * gets max(0, min(max YMax, height) - YMin[0])).  list_count == 0 or no
 * records: PRK_OK, both totals 0, row_counts zero.  On any error but the
 * short capacity nothing is written to any output. */
int prk_row_records(prk_context *ctx, const prk_edge *records, const uint32_t *counts,
                    uint32_t list_count, int32_t height,
                    prk_row *rows, uint64_t row_capacity,
                    prk_row_pair *pairs, uint64_t pair_capacity,
                    uint32_t *row_counts, uint64_t *row_total_out, uint64_t *pair_total_out);

/* Draw row work records (what DoBufferLineRenderWork runs, 2341-2348): the
 * pairs in order, each with FillLineOptimized's span body on its row's
 * RowIndex (FillLinesOptimized, 629-1490, has the same block math) -- exactly
 * what prk_draw_spans draws for the same pairs regrouped as prk_spans, frame
 * and winner ids: one id per pair, a row with EdgeCount == 0 takes none.  Row
 * r's pairs are pairs[sum of EdgeCount over rows before r ..].  The records
 * are copied at the call (the GPU regroups them; the call waits for that).
 * Semantics, phong and texture as prk_draw_spans: PRK_SEM_SCALAR is
 * PRK_ERR_UNSUPPORTED.  PRK_ERR_ARG: the EdgeCounts do not sum to pair_count,
 * an array is NULL with a non-zero count, a RowIndex is negative.
 * PRK_ERR_LIMIT: row_count or the frame's spans pass 31 bits.  row_count == 0
 * or pair_count == 0: PRK_OK, nothing recorded.  On any error nothing is
 * recorded. */
int prk_draw_rows(prk_context *ctx, const prk_row *rows, uint64_t row_count,
                  const prk_row_pair *pairs, uint64_t pair_count,
                  int32_t semantics, int32_t phong, int32_t texture);

/* The three record walks for lists [first_list, first_list + list_count) of a
 * record handle (prk_records_*): FillEdgeTable once into the handle, then
 * what DrawModel* leaves and queues every frame, without the records crossing
 * to the host.  Each call returns the status of its host-input call
 * (prk_advance_edge_lists, prk_span_records, prk_row_records) given
 * prk_records_download's records of that range and the handle's counts, and
 * writes the same words bit for bit: the range is copied on the device into
 * the walk's input and the same kernels run.  The sizing calls (NULL arrays),
 * the short-capacity behaviour, the limits and prk_debug_list_routes are
 * those calls'.  Synchronous; needs no target, records no draw, touches no
 * recorded draw and no prk_stats; frames in flight finish first.
 *
 * What the host-input calls decide in a host pass over the records -- the
 * 2^21 cap, the thread / workgroup route and its slot class, every list's
 * pair and row slots -- is decided here from a few words a list that the
 * device computes where the records are, by the same code.
 * The one difference: the host pass stops adding a list's insertion scans
 * once its cost is past 2^21, the device's sum is exact.  The two costs can
 * differ only in values above 2^21, and a route only where
 * PRK_ADV_WG_MIN_STEPS is set between them; the exact sum governs here.
 *
 * Differences: a list of the range whose sorted flag is 0 is
 * PRK_ERR_UNSUPPORTED before any walk (the flag is the sorted rule).
 * PRK_ERR_ARG: a handle that does not exist or was destroyed, a range past
 * the handle's lists, height < 0, a NULL context (and the NULL pointers the
 * host-input calls refuse).  On any error but the short capacity nothing is
 * written to any output.
 *
 * prk_records_advance: records_out (NULL, or as prk_advance_edge_lists'),
 * next_out (NULL, or as there; it needs no records_out) and advanced_out
 * (NULL, or receives a new handle of list_count lists that holds the
 * advanced records: same counts, every flag 1 -- nothing crosses to the host,
 * and prk_draw_records of it draws what prk_draw_edge_lists of records_out
 * draws).  All three NULL: PRK_ERR_ARG.  On any error no handle is made and
 * *advanced_out is -1.  The handle given is not changed.
 *
 * prk_debug_list_stats: the raw numbers, five words a list -- its edge-rows
 * sum of max(0, min(YMax, height) - YMin), its insertion scans, its most
 * edges linked at once (0 unless the list is a route candidate), YMin of its
 * first record and its largest YMax. */
int prk_records_advance(prk_context *ctx, int32_t handle, uint32_t first_list, uint32_t list_count,
                        int32_t height, int32_t *advanced_out, prk_edge *records_out, int32_t *next_out);
int prk_records_spans(prk_context *ctx, int32_t handle, uint32_t first_list, uint32_t list_count,
                      int32_t height, prk_span *spans, uint64_t capacity, uint32_t *span_counts,
                      uint64_t *total_out);
int prk_records_rows(prk_context *ctx, int32_t handle, uint32_t first_list, uint32_t list_count,
                     int32_t height, prk_row *rows, uint64_t row_capacity,
                     prk_row_pair *pairs, uint64_t pair_capacity,
                     uint32_t *row_counts, uint64_t *row_total_out, uint64_t *pair_total_out);
int prk_debug_list_stats(prk_context *ctx, int32_t handle, uint32_t first_list, uint32_t list_count,
                         int32_t height, uint64_t *out);

/* Span handles: packed prk_span records that stay in device memory -- the
 * work records DrawModelOptimized(RenderQueue, ...) queues (projekt.cpp:
 * 3756-3809), kept where the walk leaves them and drawn from there as
 * DoLineRenderWork draws them (2336-2348): the span-queue counterpart of the
 * record handles.  The context owns a batch and names it by a handle >= 0 in
 * a number space of its own (not the record handles'); the host keeps the span
 * count and each list's number of spans (4 bytes a list), and no copy of the
 * spans.  A handle belongs to its context.  prk_destroy frees every handle.
 *
 * prk_spans_from_records: prk_records_spans' walk of lists [first_list,
 * first_list + list_count) of a record handle, the packed spans written into
 * the new handle's buffer instead of the caller's -- no span crosses to the
 * host.  Its status is what prk_records_spans returns for the same handle,
 * range and height with a sufficient `spans` buffer (the same PRK_ERR_ARG /
 * PRK_ERR_UNSUPPORTED / PRK_ERR_LIMIT cases), and PRK_ERR_ARG for a NULL
 * spans_out; the handle's contents are, bit for bit, the words that call
 * writes.  span_counts (list_count words) and total_out may be NULL.  The
 * handle has list_count lists; no lists or no spans: PRK_OK and a handle of no
 * spans.  On any error no handle is made and *spans_out is -1.  Synchronous;
 * needs no target, records no draw, touches no recorded draw and no prk_stats;
 * frames in flight finish first.  A record handle's row work needs no handle
 * of its own: pair k of prk_records_rows holds span k of prk_records_spans
 * re-ordered and prk_draw_rows draws what prk_draw_spans draws (above), so
 * this handle serves DrawModelOptimizedLines' callers too.
 *
 * prk_spans_upload: a caller's own spans, copied once at the call; the host
 * does not read them.  One list of `count` spans; count == 0: an empty handle.
 * PRK_ERR_ARG: NULL spans with count > 0.  PRK_ERR_LIMIT: count passes 31 bits.
 *
 * prk_spans_upload_rows: row work records (prk_row_records' output or a
 * caller's), regrouped into spans on the device as prk_draw_rows regroups
 * them; the spans stay there.  Argument checks and errors are prk_draw_rows'
 * (the EdgeCounts must sum to pair_count, no negative RowIndex, 31-bit
 * limits).  One list of pair_count spans; no rows or no pairs: an empty handle.
 *
 * prk_spans_info / prk_spans_lists: the handle's lists and spans; each list's
 * number of spans (list_count words).  Any pointer may be NULL.  Host
 * bookkeeping: no device work.
 *
 * prk_spans_download: the packed spans.  PRK_ERR_ARG: capacity (in spans)
 * below the total.
 *
 * prk_spans_destroy: as prk_records_destroy.  Frames in flight finish first.
 * PRK_ERR_ARG while a recorded, unflushed draw names the handle
 * (prk_reset_draws releases it), and for a bad or destroyed handle. */
int prk_spans_from_records(prk_context *ctx, int32_t records_handle, uint32_t first_list, uint32_t list_count,
                           int32_t height, int32_t *spans_out, uint32_t *span_counts, uint64_t *total_out);
int prk_spans_upload(prk_context *ctx, const prk_span *spans, uint32_t count, int32_t *spans_out);
int prk_spans_upload_rows(prk_context *ctx, const prk_row *rows, uint64_t row_count,
                          const prk_row_pair *pairs, uint64_t pair_count, int32_t *spans_out);
int prk_spans_info(prk_context *ctx, int32_t handle, uint32_t *list_count_out, uint64_t *total_out);
int prk_spans_lists(prk_context *ctx, int32_t handle, uint32_t *span_counts);
int prk_spans_download(prk_context *ctx, int32_t handle, prk_span *spans, uint64_t capacity);
int prk_spans_destroy(prk_context *ctx, int32_t handle);
/* One draw of spans [first_span, first_span + span_count) of a span handle, at
 * this point of the frame's submission order: the frame, the winner ids
 * (base + k, one per span) and the semantics / phong / texture checks are
 * exactly prk_draw_spans' for the same spans passed from host memory
 * (PRK_SEM_SCALAR is PRK_ERR_UNSUPPORTED, the AVX semantics need a texture and
 * phong, the frame's id capacity applies) -- but nothing is copied, at the
 * call or at the flush: the flush reads the spans where they are, and its
 * staging holds the pass's tables only.  A handle may be drawn any number of
 * times, in one frame or across frames, mixed in one pass with every other
 * kind of draw (prk_draw_spans' staged spans, record handles and edge lists,
 * triangle objects, other span handles).  PRK_ERR_ARG: a bad handle, a range
 * past the handle's spans.  span_count == 0: PRK_OK, nothing recorded.  On
 * any error nothing is recorded. */
int prk_draw_span_records(prk_context *ctx, int32_t handle, uint32_t first_span, uint32_t span_count,
                          int32_t semantics, int32_t phong, int32_t texture);

/* Host utility: the reference's test mesh, ConstructSphere
 * (projekt.cpp:4123-4289).  Arrays must hold 6624 vertices; returns the
 * vertex count through *count_out. */
int prk_construct_sphere(float *vertices, float *colors, float *normals, float *uvs,
                         uint32_t *count_out);

#ifdef __cplusplus
}
#endif

#endif /* PRK_H */
