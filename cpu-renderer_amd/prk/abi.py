"""ctypes mirror of include/prk.h (plain structs only).

These are the caller-owned types the reference takes at its draw entry
points and that live in its absent platform header: projective_transform,
light_info / light_data, loaded_bitmap (projekt.cpp:77-90, 452-484, 1506,
3885).  See include/prk.h for the field-by-field citations.
"""
import ctypes as C

PRK_MAX_LIGHTS = 8

PRK_OK = 0
PRK_ERR_ARG = -1
PRK_ERR_UNSUPPORTED = -2
PRK_ERR_DEVICE = -3
PRK_ERR_NOMEM = -4
PRK_ERR_NO_TARGET = -5
PRK_ERR_LIMIT = -6
PRK_ERR_RUNTIME_MIX = -7

PRK_SEM_SCALAR = 0  # DrawModel            projekt.cpp:162-601
PRK_SEM_AVX = 1     # FillLineOptimized    projekt.cpp:1492-2320
PRK_SEM_AVX_ST = 2  # DrawModelOptimized(Buffer,...) single-thread overload, projekt.cpp:2350-3358

# FillEdgeTable's own inputs (prk_draw_objects_setup): its PhongShading
# argument and Object->Bitmap != 0 (projekt.cpp:4012-4089)
PRK_SETUP_PHONG = 1
PRK_SETUP_BITMAP = 2

PRK_FILTER_NEAREST = 0   # the reference's sampling (projekt.cpp:1881-2032)
PRK_FILTER_BILINEAR = 1  # extension (AVX semantics)

# prk_selftest_ops: one device primitive of csrc/prk_device.h each
(PRK_OP_DIV, PRK_OP_DIV_ALL1, PRK_OP_DIV_ALL3, PRK_OP_DIV_ALL4, PRK_OP_DIV_ALL5, PRK_OP_DIV_ALL7, PRK_OP_DIV_ALL8,
 PRK_OP_DIV_FOCAL, PRK_OP_SQRT, PRK_OP_SQRT_MID, PRK_OP_NORMALIZE_DIV, PRK_OP_NORMALIZE_RCP, PRK_OP_CVTT_S32,
 PRK_OP_ROUND_S32, PRK_OP_ROUND_U32, PRK_OP_CVT_RNE_S32, PRK_OP_MINPS, PRK_OP_MAXPS, PRK_OP_CLAMP01,
 PRK_OP_MUL16_TRICK, PRK_OP_U8_UNIT, PRK_OP_ZKEY, PRK_OP_PAIR_TAG, PRK_OP_TAG_PAIR, PRK_OP_SPAN_ENDS,
 PRK_OP_SPAN_OFFSET, PRK_OP_COUNT) = range(27)

# prk_selftest_sort / prk_selftest_scan: the damage word's bits, and each
# entry point's argument types
PRK_DAMAGE_INPUT = 1
PRK_DAMAGE_OUTPUT_GUARD = 2
PRK_DAMAGE_TEMP_GUARD = 4
SORT_SELFTEST_SIGS = {
    "prk_selftest_sort": [C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                          C.c_void_p, C.POINTER(C.c_uint32)],
    "prk_selftest_scan": [C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)],
}

STATUS_NAMES = {
    PRK_OK: "PRK_OK", PRK_ERR_ARG: "PRK_ERR_ARG", PRK_ERR_UNSUPPORTED: "PRK_ERR_UNSUPPORTED",
    PRK_ERR_DEVICE: "PRK_ERR_DEVICE", PRK_ERR_NOMEM: "PRK_ERR_NOMEM",
    PRK_ERR_NO_TARGET: "PRK_ERR_NO_TARGET", PRK_ERR_RUNTIME_MIX: "PRK_ERR_RUNTIME_MIX",
    PRK_ERR_LIMIT: "PRK_ERR_LIMIT",
}


class PrkTransform(C.Structure):
    _fields_ = [("DistanceAboveTarget", C.c_float), ("FocalLength", C.c_float),
                ("MetersToPixels", C.c_float), ("ScreenCenter", C.c_float * 2)]


class PrkLightInfo(C.Structure):
    _fields_ = [("P", C.c_float * 3), ("Intensity", C.c_float * 4)]


class PrkLightData(C.Structure):
    _fields_ = [("LightCount", C.c_uint32), ("AmbientIntensity", C.c_float * 4),
                ("Lights", PrkLightInfo * PRK_MAX_LIGHTS)]


class PrkBitmap(C.Structure):
    _fields_ = [("Memory", C.c_void_p), ("Width", C.c_int32), ("Height", C.c_int32),
                ("Pitch", C.c_int32)]


class PrkStats(C.Structure):
    _fields_ = [("triangles", C.c_uint64), ("bin_entries", C.c_uint64), ("tiles", C.c_uint32),
                ("frames_timed", C.c_uint32), ("ms_bin", C.c_float), ("ms_raster", C.c_float),
                ("sum_ms_bin", C.c_double), ("sum_ms_raster", C.c_double),
                ("anomalies", C.c_uint32), ("slow_replays", C.c_uint32), ("sum_ms_vis", C.c_double), ("sum_ms_span", C.c_double),
                ("objects_chunked", C.c_uint32), ("objects_walked", C.c_uint32),
                ("object_chunks", C.c_uint32), ("object_chunks_rewalked", C.c_uint32)]


class PrkRowPair(C.Structure):
    """prk_row_pair: thread_edge_info, left and right interleaved (24 words)."""
    _fields_ = [("LeftXMin", C.c_float), ("RightXMin", C.c_float), ("LeftZMin", C.c_float), ("RightZMin", C.c_float),
                ("LeftOneOverZMin", C.c_float), ("RightOneOverZMin", C.c_float),
                ("LeftUMin", C.c_float), ("RightUMin", C.c_float), ("LeftVMin", C.c_float), ("RightVMin", C.c_float),
                ("LeftMinColor", C.c_float * 4), ("RightMinColor", C.c_float * 4),
                ("LeftMinNormal", C.c_float * 3), ("RightMinNormal", C.c_float * 3)]


class PrkRow(C.Structure):
    """prk_row: buffer_line_render_work's RowIndex and EdgeCount (pairs)."""
    _fields_ = [("RowIndex", C.c_int32), ("EdgeCount", C.c_uint32)]


class PrkXform(C.Structure):
    """prk_xform: a row-major 3x4 matrix, out = M[:, 0:3] * v + M[:, 3]."""
    _fields_ = [("M", (C.c_float * 4) * 3)]


class PrkXformRun(C.Structure):
    """prk_xform_run: triangles [src_first_tri, +tri_count) of the source to
    [dst_first_tri, +tri_count) of the destination through xforms[xform]."""
    _fields_ = [("src_first_tri", C.c_uint32), ("tri_count", C.c_uint32), ("dst_first_tri", C.c_uint32),
                ("xform", C.c_uint32)]


# The device transform pass (prk.h): each entry point and its argument types
GEOMETRY_TRANSFORM_SIGS = {
    "prk_geometry_alloc": [C.c_void_p, C.POINTER(C.c_int32)],
    "prk_geometry_transform": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(PrkXformRun), C.c_uint32,
                               C.POINTER(PrkXform), C.c_uint32],
    "prk_geometry_download": [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p],
    "prk_geometry_info": [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "prk_debug_geometry_stream": [C.c_void_p, C.POINTER(C.c_void_p)],
    "prk_debug_transform_ms": [C.c_void_p, C.c_void_p],
}

class PrkSelectLevel(C.Structure):
    """prk_select_level: source triangles [src_first_tri, +tri_count), chosen
    when the item's pixel count is at least min_pixels."""
    _fields_ = [("min_pixels", C.c_uint32), ("src_first_tri", C.c_uint32), ("tri_count", C.c_uint32)]


class PrkSelectItem(C.Structure):
    """prk_select_item: the item's ids [first_id, +id_count) of the frame, its
    levels [first_level, +level_count) of the call's table, its matrix."""
    _fields_ = [("first_id", C.c_uint32), ("id_count", C.c_uint32), ("first_level", C.c_uint32),
                ("level_count", C.c_uint32), ("xform", C.c_uint32)]


# Cull and pick a level of detail on the device (prk.h): each entry point and its argument types
SELECT_SIGS = {
    "prk_geometry_select": [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(PrkSelectItem), C.c_uint32,
                            C.POINTER(PrkSelectLevel), C.c_uint32, C.POINTER(PrkXform), C.c_uint32, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)],
    "prk_selftest_select": [C.c_int32, C.c_void_p, C.c_uint32, C.POINTER(PrkSelectItem), C.c_uint32,
                            C.POINTER(PrkSelectLevel), C.c_uint32, C.POINTER(PrkXform), C.c_uint32, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)],
    "prk_debug_select_ms": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)],
}

class PrkBound(C.Structure):
    """prk_bound: an axis-aligned box lo .. hi in the space of its matrix."""
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("xform", C.c_uint32)]


# The bounds occlusion test (prk.h): each entry point and its argument types
BOUNDS_SIGS = {
    "prk_visibility_bounds": [C.c_void_p, C.POINTER(PrkBound), C.c_uint32, C.POINTER(PrkXform), C.c_uint32,
                              C.c_void_p, C.c_void_p],
    "prk_visibility_bounds_device": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)],
    "prk_geometry_select_bounds": [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(PrkSelectItem),
                                   C.c_uint32, C.POINTER(PrkSelectLevel), C.c_uint32, C.POINTER(PrkXform),
                                   C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)],
    "prk_debug_ztiles": [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                         C.POINTER(C.c_int32)],
    "prk_debug_bounds_ms": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "prk_selftest_bounds": [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                            C.POINTER(PrkTransform), C.c_void_p, C.POINTER(PrkBound), C.c_uint32,
                            C.POINTER(PrkXform), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)],
}

# Render to texture (prk.h): each entry point and its argument types
TEXTURE_TARGET_SIGS = {
    "prk_texture_alloc": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)],
    "prk_texture_from_target": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32],
    "prk_texture_download": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32],
    "prk_texture_info": [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
}

# Target layers (prk.h): the merge rules, and each entry point and its argument types
PRK_MERGE_COPY = 0           # every pixel of the rectangle
PRK_MERGE_GREATER = 1        # where zs > zd  (DrawModel, FillLineOptimized: the earliest of equals wins)
PRK_MERGE_GREATER_EQUAL = 2  # where zs >= zd (the single-thread overload: the latest wins)
TARGET_LAYER_SIGS = {
    "prk_layer_alloc": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)],
    "prk_layer_wrap_device": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                              C.POINTER(C.c_int32)],
    "prk_layer_from_target": [C.c_void_p] + [C.c_int32] * 7,
    "prk_target_from_layer": [C.c_void_p] + [C.c_int32] * 8,
    "prk_layer_download": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p],
    "prk_layer_info": [C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 4,
    "prk_layer_destroy": [C.c_void_p, C.c_int32],
}

# Visibility feedback (prk.h): each entry point and its argument types
VISIBILITY_SIGS = {
    "prk_visibility_info": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)],
    "prk_visibility_counts": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "prk_visibility_groups": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "prk_visibility_ids": [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)],
    "prk_visibility_device": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)],
    "prk_selftest_visibility": [C.c_int32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)],
}


# prk_row_pair word w holds prk_span word ROW_PAIR_SPAN_WORD[w] (an end is
# XMin ZMin OneOverZMin UMin VMin MinColor[4] MinNormal[3]; Right at +12)
ROW_PAIR_SPAN_WORD = ([h * 12 + k for k in range(5) for h in (0, 1)] + [5, 6, 7, 8] + [17, 18, 19, 20] +
                      [9, 10, 11] + [21, 22, 23])


# The record walks of a handle (prk.h): each entry point and its arguments
RECORD_WALK_ARGS = {
    "prk_records_advance": 8,
    "prk_records_spans": 9,
    "prk_records_rows": 12,
    "prk_debug_list_stats": 6,
}
# Span handles (prk.h): each entry point and its arguments
SPAN_HANDLE_ARGS = {
    "prk_spans_from_records": 8,
    "prk_spans_upload": 4,
    "prk_spans_upload_rows": 6,
    "prk_spans_info": 4,
    "prk_spans_lists": 3,
    "prk_spans_download": 4,
    "prk_spans_destroy": 2,
    "prk_draw_span_records": 7,
}
# prk_debug_list_stats: the words of a list
LIST_STATS_FIELDS = ("edge_rows", "scans", "most", "ymin0", "ymax_max")


class PrkBinsInfo(C.Structure):
    """prk_bins_info: the frame sizes prk_debug_bins answers for."""
    _fields_ = [("tile_w", C.c_int32), ("tile_h", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("row0", C.c_int32), ("row1", C.c_int32), ("tri_count", C.c_uint32), ("entry_count", C.c_uint32),
                ("rerun", C.c_uint32), ("band_per", C.c_uint32)]


# prk_debug_bins: a triangle's eight range words, and the call's argument types
TILE_RANGE_FIELDS = ("tx0", "ty0", "tx1", "ty1", "oty0", "oty1", "pad0", "pad1")
DEBUG_BINS_ARGS = [C.c_void_p, C.POINTER(PrkBinsInfo), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                   C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]


def make_transform(D, F, M2P, cx, cy):
    t = PrkTransform()
    t.DistanceAboveTarget = D
    t.FocalLength = F
    t.MetersToPixels = M2P
    t.ScreenCenter[0] = cx
    t.ScreenCenter[1] = cy
    return t


def make_lights(lights, ambient):
    """lights: list of ((px,py,pz), (r,g,b,a)); ambient: (r,g,b,a)."""
    if len(lights) > PRK_MAX_LIGHTS:
        raise ValueError("at most %d lights" % PRK_MAX_LIGHTS)
    ld = PrkLightData()
    ld.LightCount = len(lights)
    for c in range(4):
        ld.AmbientIntensity[c] = ambient[c]
    for i, (p, inten) in enumerate(lights):
        for c in range(3):
            ld.Lights[i].P[c] = p[c]
        for c in range(4):
            ld.Lights[i].Intensity[c] = inten[c]
    return ld
