"""prk — Python binding of libprk_hip.so (the MI355X rasterizer C-ABI).

Mirrors the reference's draw interface (projekt.cpp, MacSpain/cpu-renderer):

    reference                                   here
    ------------------------------------------  ---------------------------------
    FillEdgeTable(Object, Commands, Phong)      Renderer.draw_* record the object
    DrawModelOptimized(Queue, Buffer, Edges,    Renderer.draw_model_optimized()
        EdgeCount, Commands, Bitmap, Phong)     (FillLineOptimized semantics)
    DrawModel(Buffer, Edges, EdgeCount,         Renderer.draw_model()
        Commands, Bitmap, Phong)                (scalar DrawModel semantics)
    Platform.CompleteAllWork(Queue)             Renderer.complete_all_work()

The HIP library is the only compute path: there is no CPU fallback, and every
entry point raises PrkError if libprk_hip.so or the GPU is missing.
"""
import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

from . import abi
from . import scenes as scenes_mod
from .abi import PRK_SEM_AVX, PRK_SEM_AVX_ST, PRK_SEM_SCALAR  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(os.path.dirname(_HERE), "libprk_hip.so")
LIB_PATH = os.environ.get("PRK_LIB") or _DEFAULT_LIB
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "prk.h")

_LIB = None


class PrkError(RuntimeError):
    def __init__(self, fn, code):
        super().__init__("%s failed: %s (%d)" % (fn, abi.STATUS_NAMES.get(code, "?"), code))
        self.code = code


_SIGS = {
    "prk_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "prk_destroy": (C.c_int, [C.c_void_p]),
    "prk_runtime_check": (C.c_int, []),
    "prk_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "prk_version": (C.c_char_p, []),
    "prk_target_bind": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32]),
    "prk_target_alloc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "prk_target_clear": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float]),
    "prk_target_clear_on_flush": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float]),
    "prk_target_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "prk_target_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "prk_target_upload_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "prk_set_camera": (C.c_int, [C.c_void_p, C.POINTER(abi.PrkTransform), C.POINTER(abi.PrkLightData)]),
    "prk_set_shade_camera": (C.c_int, [C.c_void_p, C.POINTER(abi.PrkTransform), C.POINTER(abi.PrkLightData)]),
    "prk_texture_create": (C.c_int, [C.c_void_p, C.POINTER(abi.PrkBitmap), C.POINTER(C.c_int32)]),
    "prk_texture_set_filter": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "prk_texture_update": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(abi.PrkBitmap)]),
    "prk_geometry_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32]),
    "prk_geometry_write": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "prk_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "prk_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "prk_host_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "prk_host_unregister": (C.c_int, [C.c_void_p, C.c_void_p]),
    "prk_geometry_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.POINTER(C.c_int32)]),
    "prk_geometry_wrap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint32, C.POINTER(C.c_int32)]),
    "prk_draw": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                           C.c_int32, C.c_int32, C.c_int32]),
    "prk_draw_objects": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_int32]),
    "prk_draw_objects_setup": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "prk_draw_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]),
    "prk_draw_spans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]),
    "prk_draw_edge_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32,
                                      C.c_int32]),
    "prk_flush": (C.c_int, [C.c_void_p, C.c_void_p]),
    "prk_reset_draws": (C.c_int, [C.c_void_p]),
    "prk_synchronize": (C.c_int, [C.c_void_p]),
    "prk_resolve": (C.c_int, [C.c_void_p, C.c_void_p]),
    "prk_get_stats": (C.c_int, [C.c_void_p, C.POINTER(abi.PrkStats)]),
    "prk_timing_reset": (C.c_int, [C.c_void_p]),
    "prk_set_debug": (C.c_int, [C.c_void_p, C.c_int32]),
    "prk_set_early_z": (C.c_int, [C.c_void_p, C.c_int]),
    "prk_download_winners": (C.c_int, [C.c_void_p, C.c_void_p]),
    "prk_debug_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]),
    "prk_debug_walk_routes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int32]),
    "prk_debug_list_routes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int32]),
    "prk_debug_bins": (C.c_int, abi.DEBUG_BINS_ARGS),
    "prk_set_tile": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "prk_construct_sphere": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_uint32)]),
    "prk_fill_edge_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.POINTER(C.c_float), C.POINTER(abi.PrkTransform),
                                        C.POINTER(abi.PrkLightData), C.c_int32, C.c_void_p, C.c_size_t,
                                        C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]),
    "prk_advance_edge_records": (C.c_int, [C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int32]),
    "prk_fill_edge_count": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(abi.PrkTransform),
                                      C.POINTER(C.c_uint32)]),
    "prk_edge_records": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                   C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "prk_records_from_geometry": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "prk_records_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]),
    "prk_records_info": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "prk_records_lists": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "prk_records_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64]),
    "prk_records_destroy": (C.c_int, [C.c_void_p, C.c_int32]),
    "prk_draw_records": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]),
    "prk_debug_stage_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "prk_advance_edge_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p,
                                         C.c_void_p]),
    "prk_span_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.POINTER(C.c_uint64)]),
    "prk_row_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "prk_draw_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32,
                                C.c_int32]),
    "prk_records_advance": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_int32),
                                      C.c_void_p, C.c_void_p]),
    "prk_records_spans": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64,
                                    C.c_void_p, C.POINTER(C.c_uint64)]),
    "prk_records_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "prk_debug_list_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p]),
    "prk_spans_from_records": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32,
                                         C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_uint64)]),
    "prk_spans_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]),
    "prk_spans_upload_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_int32)]),
    "prk_spans_info": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "prk_spans_lists": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "prk_spans_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64]),
    "prk_spans_destroy": (C.c_int, [C.c_void_p, C.c_int32]),
    "prk_draw_span_records": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                        C.c_int32]),
    "prk_get_target": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32)]),
    "prk_get_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "prk_band_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "prk_selftest_div": (C.c_int, [C.c_int32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "prk_selftest_div_paths": (C.c_int, [C.c_int32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32)]),
    "prk_selftest_ops": (C.c_int, [C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "prk_comm_available": (C.c_int, []),
    "prk_comm_unique_id": (C.c_int, [C.c_void_p]),
    "prk_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "prk_comm_init_all": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]),
    "prk_comm_destroy": (C.c_int, [C.c_void_p]),
    "prk_gather_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "prk_gather_frame_all": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_void_p]),
    "prk_gather_frame_local": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_void_p]),
}

_SIGS.update({name: (C.c_int, args) for name, args in abi.GEOMETRY_TRANSFORM_SIGS.items()})
_SIGS.update({name: (C.c_int, args) for name, args in abi.TEXTURE_TARGET_SIGS.items()})
_SIGS.update({name: (C.c_int, args) for name, args in abi.TARGET_LAYER_SIGS.items()})
_SIGS.update({name: (C.c_int, args) for name, args in abi.SORT_SELFTEST_SIGS.items()})
_SIGS.update({name: (C.c_int, args) for name, args in abi.VISIBILITY_SIGS.items()})
_SIGS.update({name: (C.c_int, args) for name, args in abi.SELECT_SIGS.items()})
_SIGS.update({name: (C.c_int, args) for name, args in abi.BOUNDS_SIGS.items()})

COMM_ID_BYTES = 128  # PRK_COMM_ID_BYTES


def exported_symbols():
    return list(_SIGS)


def lib(path=None):
    """Load libprk_hip.so (fails loudly if it has not been built)."""
    global _LIB
    if _LIB is None:
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise PrkError("load libprk_hip.so (%s: not built; run __graft_entry__.build())" % p, -3)
        # One ROCm runtime per process: torch ships its own libamdhip64 /
        # librccl / librocm_smi64 under names (libamdhip64.so, librccl.so) that
        # do not match this library's (libamdhip64.so.7 via /opt/rocm, and the
        # librccl.so.1 prk_comm_* dlopens).  Loaded first, torch's copies
        # satisfy ours by SONAME; loaded after us, torch would map a second
        # copy of each, and two librocm_smi64 copies destroy the same
        # interposed static map at exit (glibc "double free").
        # PRK_NO_TORCH_PRELOAD=1 skips this (a process that never imports
        # torch: the library's own /opt/rocm stack alone, no torch import cost).
        if os.environ.get("PRK_NO_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:  # no (usable) torch: this library's own ROCm stack alone
                pass
        atexit.register(_close_all)  # after torch's handlers: runs before them
        L = C.CDLL(p)
        # (A/B tools load older builds through PRK_LIB that may lack newer entry points)
        variant = os.path.abspath(p) != os.path.abspath(_DEFAULT_LIB)
        for name, (res, args) in _SIGS.items():
            if variant and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def _check(fn, rc):
    if rc != abi.PRK_OK:
        raise PrkError(fn, rc)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def device_count():
    n = C.c_int(0)
    _check("prk_device_count", lib().prk_device_count(C.byref(n)))
    return n.value


def construct_sphere():
    """ConstructSphere (projekt.cpp:4123-4289) -> (V[6624,3], C[6624,4], N[6624,3], UV[6624,2])."""
    V = np.zeros((6624, 3), np.float32)
    Cc = np.zeros((6624, 4), np.float32)
    N = np.zeros((6624, 3), np.float32)
    UV = np.zeros((6624, 2), np.float32)
    n = C.c_uint32(0)
    _check("prk_construct_sphere", lib().prk_construct_sphere(_ptr(V), _ptr(Cc), _ptr(N), _ptr(UV),
                                                               C.byref(n)))
    return V[: n.value], Cc[: n.value], N[: n.value], UV[: n.value]


def fill_edge_count(vertices, P, transform):
    """prk_fill_edge_count: FillEdgeTable's return value (projekt.cpp:4119)
    for one object (host-side, no device needed)."""
    v = np.ascontiguousarray(vertices, np.float32)
    Pc = (C.c_float * 3)(*(P or (0.0, 0.0, 0.0)))
    n = C.c_uint32(0)
    _check("prk_fill_edge_count", lib().prk_fill_edge_count(_ptr(v), v.shape[0], Pc, C.byref(transform),
                                                             C.byref(n)))
    return n.value


# x86-64 edge_info (projekt.h:17-37): 27 four-byte fields, pad, Next pointer
EDGE_INFO_STRIDE, EDGE_INFO_NEXT = 120, 112


def fill_edge_records(vertices, colors, normals, uvs, P, transform, lights, setup, memory=None):
    """prk_fill_edge_records: FillEdgeTable's records (projekt.cpp:3894-4117)
    written in place into `memory` (uint8 [>= 3T, 120]: x86-64 edge_info
    elements; default zeros).  Returns (memory, count)."""
    arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (vertices, colors, normals, uvs)]
    nv = arrs[0].shape[0]
    if memory is None:
        memory = np.zeros((max(1, nv), EDGE_INFO_STRIDE), np.uint8)
    Pc = (C.c_float * 3)(*(P or (0.0, 0.0, 0.0)))
    n = C.c_uint32(0)
    _check("prk_fill_edge_records", lib().prk_fill_edge_records(
        *[_ptr(a) for a in arrs], nv, Pc, C.byref(transform), C.byref(lights), int(setup), _ptr(memory),
        EDGE_INFO_STRIDE, EDGE_INFO_NEXT, None, C.byref(n)))
    return memory, n.value


def advance_edge_records(memory, count, height):
    """prk_advance_edge_records on an edge_info array (uint8 [n, 120]) in
    place: what DrawModel* leaves in it (projekt.cpp:3654-3869)."""
    _check("prk_advance_edge_records", lib().prk_advance_edge_records(
        _ptr(memory), count, EDGE_INFO_STRIDE, EDGE_INFO_NEXT, int(height)))
    return memory


def edge_record_words(memory, count):
    """(fields as uint32 [count, 27], Next as an element index or -1)."""
    w = memory[:count, :108].copy().view(np.uint32).reshape(count, 27)
    ptr = memory[:count, EDGE_INFO_NEXT:EDGE_INFO_NEXT + 8].copy().view(np.uint64).reshape(count)
    base = memory.ctypes.data
    nxt = np.where(ptr == 0, -1, (ptr.astype(np.int64) - base) // EDGE_INFO_STRIDE).astype(np.int32)
    return w, nxt


def selftest_div(n=1 << 22, seed=1, device=0):
    """prk_selftest_div: (quotient mismatches, normalisation mismatches) of the
    shared-divisor division against the compiler's x / d over n draws."""
    out = C.c_uint64()
    _check("prk_selftest_div", lib().prk_selftest_div(device, n, seed, C.byref(out)))
    return out.value & 0xFFFFFFFF, out.value >> 32


def selftest_div_paths(n=1 << 22, seed=1, device=0):
    """prk_selftest_div_paths: selftest_div's two counts, and how many 64-lane
    waves took the quotient's and the normalisation's shared-reciprocal path."""
    out = C.c_uint64()
    fast = (C.c_uint32 * 2)()
    _check("prk_selftest_div_paths", lib().prk_selftest_div_paths(device, n, seed, C.byref(out), fast))
    return out.value & 0xFFFFFFFF, out.value >> 32, int(fast[0]), int(fast[1])


def selftest_ops(op, a, b=None, c=None, d=None, device=0):
    """prk_selftest_ops: device primitive `op` (abi.PRK_OP_*) on uint32 word
    arrays of one length.  Returns (out0, out1, out2, fast) as uint32 arrays;
    element i is thread i of the launch, so 64 consecutive elements share a wave."""
    ins = [None if x is None else np.ascontiguousarray(x, np.uint32) for x in (a, b, c, d)]
    n = ins[0].shape[0]
    assert all(x is None or x.shape == (n,) for x in ins)
    outs = [np.zeros(n, np.uint32) for _ in range(4)]
    _check("prk_selftest_ops", lib().prk_selftest_ops(device, int(op), n, *[_ptr(x) for x in ins],
                                                       *[_ptr(x) for x in outs]))
    return tuple(outs)


def selftest_sort(keys, vals, end_bit, repeats=1, device=0):
    """prk_selftest_sort: the span path's radix sort (prk_obj_sort) of the
    (keys[i], vals[i]) pairs, `repeats` times on one temp buffer.  Returns
    (keys_out uint64, vals_out uint32, damage): damage is 0 or abi.PRK_DAMAGE_*
    bits (inputs changed, a guard after an output or after temp changed)."""
    k = np.ascontiguousarray(keys, np.uint64)
    v = np.ascontiguousarray(vals, np.uint32)
    n = k.shape[0]
    assert k.shape == (n,) and v.shape == (n,)
    ko, vo = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    dmg = C.c_uint32(0xFFFFFFFF)
    _check("prk_selftest_sort", lib().prk_selftest_sort(device, n, int(end_bit), _ptr(k), _ptr(v), int(repeats),
                                                        _ptr(ko), _ptr(vo), C.byref(dmg)))
    return ko, vo, dmg.value


def selftest_scan(x, width, device=0):
    """prk_selftest_scan: the span path's exclusive scan (prk_scan_u32 /
    prk_scan_u64) of x as `width`-bit words.  Returns (out, damage)."""
    dt = {32: np.uint32, 64: np.uint64}.get(int(width), np.uint64)
    a = np.ascontiguousarray(x, dt)
    assert a.ndim == 1
    out = np.zeros(a.shape[0], dt)
    dmg = C.c_uint32(0xFFFFFFFF)
    _check("prk_selftest_scan", lib().prk_selftest_scan(device, int(width), a.shape[0], _ptr(a), _ptr(out),
                                                        C.byref(dmg)))
    return out, dmg.value


def selftest_visibility(winners, id_count, device=0):
    """prk_selftest_visibility: the visibility reduction (prk_visibility_*'s
    kernels) of the int32 winner words over id_count ids, no context.
    Returns a dict: counts [id_count], pix_prefix and vis_prefix
    [id_count + 1], ids [visible] (all uint32), visible, atomics (the atomic
    adds the histogram issued) and damage (0 or abi.PRK_DAMAGE_* bits)."""
    w = np.ascontiguousarray(winners, np.int32).reshape(-1)
    m = int(id_count)
    counts, ids = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    pix, vis = np.zeros(m + 1, np.uint32), np.zeros(m + 1, np.uint32)
    nvis, nat, dmg = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0xFFFFFFFF)
    _check("prk_selftest_visibility", lib().prk_selftest_visibility(
        device, w.shape[0], _ptr(w), m, _ptr(counts), _ptr(pix), _ptr(vis), _ptr(ids), C.byref(nvis), C.byref(nat),
        C.byref(dmg)))
    return dict(counts=counts, pix_prefix=pix, vis_prefix=vis, ids=ids[:nvis.value], visible=nvis.value,
                atomics=nat.value, damage=dmg.value)


def _select_tables(items, levels, xforms):
    """(items uint32 [n, 5], levels uint32 [m, 3], xforms float32 [k, 3, 4]) and their typed pointers (None: NULL)."""
    it = np.ascontiguousarray(items, np.uint32).reshape(-1, 5)
    lv = None if levels is None else np.ascontiguousarray(levels, np.uint32).reshape(-1, 3)
    xf = None if xforms is None else np.ascontiguousarray(xforms, np.float32).reshape(-1, 3, 4)
    ptrs = (C.cast(it.ctypes.data, C.POINTER(abi.PrkSelectItem)) if it.shape[0] else None,
            None if lv is None else C.cast(lv.ctypes.data, C.POINTER(abi.PrkSelectLevel)),
            None if xf is None else C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform)))
    return (it, lv, xf), ptrs


def selftest_select(items, levels, xforms, src, dst_tris, dst_first_tri=0, pix_prefix=None, item_pixels=None,
                    device=0):
    """prk_selftest_select: prk_geometry_select's stages (choice, scan, emit)
    on host tables, no context.  items uint32 [n, 5] of (first_id, id_count,
    first_level, level_count, xform), levels uint32 [m, 3] of (min_pixels,
    src_first_tri, tri_count), xforms float32 [k, 3, 4]; src: (vertices,
    colors, normals, uvs), None for an absent array; counts from pix_prefix
    (uint32 [ids + 1]) or item_pixels (uint32 [n]).  Returns a dict: chosen
    int32 [n], out_first uint32 [n + 1], total, dst (the dst_tris triangles of
    every array src has, as uint32 words -- 0xA5A5A5A5 where nothing was
    written), damage (0 or abi.PRK_DAMAGE_* bits)."""
    (it, lv, xf), (ip, lp, xp) = _select_tables(items, levels, xforms)
    n = it.shape[0]
    pp = None if pix_prefix is None else np.ascontiguousarray(pix_prefix, np.uint32).reshape(-1)
    px = None if item_pixels is None else np.ascontiguousarray(item_pixels, np.uint32).reshape(-1)
    assert px is None or px.shape[0] == n
    arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in src]
    src_tris = 0 if arrs[0] is None else arrs[0].shape[0] // 3
    out = [None if a is None else np.zeros((3 * int(dst_tris), comp), np.float32)
           for a, comp in zip(arrs, (3, 4, 3, 2))]
    chosen, first = np.zeros(n, np.int32), np.zeros(n + 1, np.uint32)
    total, dmg = C.c_uint64(0), C.c_uint32(0xFFFFFFFF)
    _check("prk_selftest_select", lib().prk_selftest_select(
        device, _ptr(pp), 0 if pp is None else pp.shape[0] - 1, ip, n, lp, 0 if lv is None else lv.shape[0], xp,
        0 if xf is None else xf.shape[0], _ptr(px), *[_ptr(a) for a in arrs], src_tris, int(dst_first_tri),
        int(dst_tris), *[_ptr(a) for a in out], _ptr(chosen), _ptr(first), C.byref(total), C.byref(dmg)))
    return dict(chosen=chosen, out_first=first, total=total.value,
                dst=tuple(None if a is None else a.view(np.uint32) for a in out), damage=dmg.value)


def _bound_tables(bounds, xforms):
    """(bounds as float32 [n, 7] rows of lo[3], hi[3] and the xform index as a
    uint32 word, xforms float32 [k, 3, 4]) and their typed pointers (None: NULL)."""
    b = np.ascontiguousarray(bounds, np.float32).reshape(-1, 7)
    xf = None if xforms is None else np.ascontiguousarray(xforms, np.float32).reshape(-1, 3, 4)
    return (b, xf), (C.cast(b.ctypes.data, C.POINTER(abi.PrkBound)) if b.shape[0] else None,
                     None if xf is None else C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform)))


def pack_bounds(lo, hi, xform):
    """prk_bound records as float32 [n, 7]: lo, hi float [n, 3], xform the
    matrix index of each (stored as a uint32 word in the last column)."""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    out = np.zeros((lo.shape[0], 7), np.float32)
    out[:, 0:3] = lo
    out[:, 3:6] = np.asarray(hi, np.float32).reshape(-1, 3)
    out.view(np.uint32)[:, 6] = np.broadcast_to(np.asarray(xform, np.uint32), (lo.shape[0],))
    return out


def selftest_bounds(z, row0, height, transform, bounds, xforms, P=None, z_offset=0, device=0):
    """prk_selftest_bounds: prk_visibility_bounds' two kernels on host inputs,
    no context.  z float32 [row1 - row0, W] (the band of a W x height frame
    from row0 on), placed z_offset floats into its device buffer; transform an
    abi.PrkTransform; bounds from pack_bounds; xforms float32 [k, 3, 4].
    Returns a dict: zmin float32 [tiles_y, tiles_x], pixels uint32 [n], damage
    (0 or abi.PRK_DAMAGE_* bits)."""
    zz = np.ascontiguousarray(z, np.float32)
    rows, W = zz.shape
    row1 = int(row0) + rows
    (b, xf), (bp, xp) = _bound_tables(bounds, xforms)
    n = b.shape[0]
    zmin = np.zeros(((row1 + 7) // 8 - int(row0) // 8, (W + 7) // 8), np.float32)
    pix = np.zeros(n, np.uint32)
    Pc = None if P is None else (C.c_float * 3)(*P)
    dmg = C.c_uint32(0xFFFFFFFF)
    _check("prk_selftest_bounds", lib().prk_selftest_bounds(
        device, _ptr(zz), W, int(height), int(row0), row1, int(z_offset), C.byref(transform),
        None if Pc is None else C.cast(Pc, C.c_void_p), bp, n, xp, 0 if xf is None else xf.shape[0], _ptr(zmin),
        _ptr(pix), C.byref(dmg)))
    return dict(zmin=zmin, pixels=pix, damage=dmg.value)


def band_rows(height, rank, nranks):
    """prk_band_rows: frame rows [row0, row1) of rank `rank` of `nranks`."""
    a, b = C.c_int32(0), C.c_int32(0)
    _check("prk_band_rows", lib().prk_band_rows(height, rank, nranks, C.byref(a), C.byref(b)))
    return a.value, b.value


def comm_available():
    """True when librccl can be loaded (prk_comm_*)."""
    return bool(lib().prk_comm_available())


def comm_unique_id():
    """prk_comm_unique_id (rank 0): the RCCL unique id as bytes."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check("prk_comm_unique_id", lib().prk_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """An RCCL communicator of one rank (prk_comm_init) or of one context of
    a single-process group (Comm.init_all)."""

    def __init__(self, handle, rank, nranks):
        self._h, self.rank, self.nranks = handle, rank, nranks
        _LIVE.add(self)

    @classmethod
    def init(cls, renderer, uid, nranks, rank):
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        _check("prk_comm_init", lib().prk_comm_init(renderer._h, buf, nranks, rank, C.byref(h)))
        return cls(h, rank, nranks)

    @classmethod
    def init_all(cls, renderers):
        n = len(renderers)
        ctxs = (C.c_void_p * n)(*[r._h.value for r in renderers])
        out = (C.c_void_p * n)()
        _check("prk_comm_init_all", lib().prk_comm_init_all(ctxs, n, out))
        return [cls(C.c_void_p(out[i]), i, n) for i in range(n)]

    def close(self):
        if getattr(self, "_h", None):
            lib().prk_comm_destroy(self._h)
            self._h = None

    def gather(self, renderer, frame_color_ptr=None, frame_z_ptr=None, with_z=False, stream=None):
        """prk_gather_frame: rank 0 passes its device frame (packed rows),
        the other ranks nothing."""
        pitch = renderer.width * 4
        _check("prk_gather_frame", lib().prk_gather_frame(
            renderer._h, self._h, int(bool(with_z)), C.c_void_p(frame_color_ptr) if frame_color_ptr else None,
            pitch, C.c_void_p(frame_z_ptr) if frame_z_ptr else None,
            None if stream is None else C.c_void_p(stream)))


def gather_frame_all(renderers, comms, frame_color_ptr, frame_z_ptr=None, with_z=False):
    """prk_gather_frame_all: one process, N contexts, one RCCL group."""
    n = len(renderers)
    ctxs = (C.c_void_p * n)(*[r._h.value for r in renderers])
    cms = (C.c_void_p * n)(*[c._h.value for c in comms])
    _check("prk_gather_frame_all", lib().prk_gather_frame_all(
        ctxs, cms, n, int(bool(with_z)), C.c_void_p(frame_color_ptr), renderers[0].width * 4,
        C.c_void_p(frame_z_ptr) if frame_z_ptr else None))


def gather_frame_local(renderers, frame_color_ptr, frame_pitch, frame_z_ptr=None, with_z=False):
    """prk_gather_frame_local: every band's device copies its strip into
    renderers[0]'s device frame (peer copies, no RCCL)."""
    n = len(renderers)
    ctxs = (C.c_void_p * n)(*[r._h.value for r in renderers])
    _check("prk_gather_frame_local", lib().prk_gather_frame_local(
        ctxs, n, int(bool(with_z)), C.c_void_p(frame_color_ptr), frame_pitch,
        C.c_void_p(frame_z_ptr) if frame_z_ptr else None))


_LIVE = weakref.WeakSet()  # open Renderers / Comms, closed in a defined order at exit


def _close_all():
    """Interpreter exit: close every context still open, communicators first,
    while the HIP runtime (and torch, whose tensors a target may use) is still
    alive.  atexit runs the last-registered handler first; lib() registers
    this one right after it imports torch, so it runs before torch's.
    prk_destroy never queues GPU work (prk_api.hip), so a context whose last
    frame was never read just drops it."""
    objs = list(_LIVE)
    for o in sorted(objs, key=lambda o: 0 if isinstance(o, Comm) else 1):
        try:
            o.close()
        except Exception:
            pass


def _finalizing():
    return sys.is_finalizing()


class Records:
    """A record handle (prk_records_*): lists in edge_records' packed layout
    kept in device memory by the Renderer that made it, drawn with
    Renderer.draw_records any number of times."""

    def __init__(self, renderer, handle):
        self._r, self.handle = renderer, handle
        n, t = C.c_uint32(0), C.c_uint64(0)
        _check("prk_records_info", renderer._L.prk_records_info(renderer._h, handle, C.byref(n), C.byref(t)))
        self.list_count, self.total = n.value, t.value

    def _lists(self, which):
        out = np.zeros(self.list_count, np.uint32)
        args = (_ptr(out), None) if which == 0 else (None, _ptr(out))
        _check("prk_records_lists", self._r._L.prk_records_lists(self._r._h, self.handle, *args))
        return out

    def counts(self):
        """uint32 [list_count]: each list's records."""
        return self._lists(0)

    def sorted_flags(self):
        """uint32 [list_count]: 1 for a list inside draw_edge_lists' sorted
        rule (computed on the device when the handle was made)."""
        return self._lists(1)

    def download(self):
        """uint32 [total, 27]: the packed records (edge_records' words)."""
        w = np.empty((self.total, 27), np.uint32)
        _check("prk_records_download", self._r._L.prk_records_download(self._r._h, self.handle, _ptr(w), self.total))
        return w

    def _range(self, first_list, list_count):
        first = int(first_list)
        n = self.list_count - first if list_count is None else int(list_count)
        if first < 0 or n < 0 or first + n > self.list_count:
            raise ValueError("lists [%d, %d) of a handle of %d" % (first, first + n, self.list_count))
        return first, n, int(self.counts()[first:first + n].sum(dtype=np.uint64))

    def advance(self, height, first_list=0, list_count=None, keep=False, host=True):
        """prk_records_advance: what DrawModel* leaves in lists [first_list,
        first_list + list_count) over a frame of `height` rows, the records
        never leaving the device.  host: (words_out, next) as
        Renderer.advance_edge_lists returns them; keep: a new Records that
        holds the advanced lists; both: (words_out, next, Records)."""
        first, n, total = self._range(first_list, list_count)
        if not (keep or host):
            raise ValueError("advance: neither keep nor host")
        out = np.empty((total, 27), np.uint32) if host else None
        nxt = np.empty(total, np.int32) if host else None
        h = C.c_int32(-1)
        _check("prk_records_advance", self._r._L.prk_records_advance(
            self._r._h, self.handle, first, n, int(height), C.byref(h) if keep else None,
            _ptr(out) if host else None, _ptr(nxt) if host else None))
        if not keep:
            return out, nxt
        adv = Records(self._r, h.value)
        return (out, nxt, adv) if host else adv

    def spans(self, height, first_list=0, list_count=None, keep=False):
        """prk_records_spans: what Renderer.span_records returns for the
        same lists, (span_words uint32 [total, 25], span_counts).  keep:
        prk_spans_from_records instead -- a Spans that holds the same words
        on the device (no span crosses to the host)."""
        first, n, _ = self._range(first_list, list_count)
        L, rh = self._r._L, self._r._h
        if keep:
            h = C.c_int32(-1)
            _check("prk_spans_from_records", L.prk_spans_from_records(rh, self.handle, first, n, int(height),
                                                                      C.byref(h), None, None))
            return Spans(self._r, h.value)
        sc = np.zeros(n, np.uint32)
        total = C.c_uint64(0)
        _check("prk_records_spans", L.prk_records_spans(rh, self.handle, first, n, int(height), None, 0, _ptr(sc),
                                                        C.byref(total)))
        spans = np.empty((total.value, 25), np.uint32)
        _check("prk_records_spans", L.prk_records_spans(rh, self.handle, first, n, int(height), _ptr(spans),
                                                        total.value, _ptr(sc), C.byref(total)))
        return spans, sc

    def rows(self, height, first_list=0, list_count=None):
        """prk_records_rows: what Renderer.row_records returns for the same
        lists, (rows int32 [k, 2], pairs uint32 [m, 24], row_counts)."""
        first, n, _ = self._range(first_list, list_count)
        L, rh = self._r._L, self._r._h
        rc = np.zeros(n, np.uint32)
        nrow, npair = C.c_uint64(0), C.c_uint64(0)
        _check("prk_records_rows", L.prk_records_rows(rh, self.handle, first, n, int(height), None, 0, None, 0,
                                                      _ptr(rc), C.byref(nrow), C.byref(npair)))
        rows = np.empty((nrow.value, 2), np.int32)
        pairs = np.empty((npair.value, 24), np.uint32)
        _check("prk_records_rows", L.prk_records_rows(rh, self.handle, first, n, int(height), _ptr(rows), nrow.value,
                                                      _ptr(pairs), npair.value, _ptr(rc), C.byref(nrow),
                                                      C.byref(npair)))
        return rows, pairs, rc

    def list_stats(self, height, first_list=0, list_count=None):
        """prk_debug_list_stats: int64 [list_count, 5] -- each list's
        edge-rows, insertion scans, most edges linked at once (0 unless a
        route candidate), first YMin and largest YMax, as the device
        computes them for the walks above."""
        first, n, _ = self._range(first_list, list_count)
        out = np.zeros((n, 5), np.uint64)
        _check("prk_debug_list_stats", self._r._L.prk_debug_list_stats(self._r._h, self.handle, first, n, int(height),
                                                                       _ptr(out)))
        return out.view(np.int64)

    def close(self):
        """prk_records_destroy (the Renderer's close frees what is left)."""
        if self.handle is not None and getattr(self._r, "_h", None):
            _check("prk_records_destroy", self._r._L.prk_records_destroy(self._r._h, self.handle))
        self.handle = None


class Spans:
    """A span handle (prk_spans_*): packed prk_span records kept in device
    memory by the Renderer that made it, drawn with
    Renderer.draw_span_records any number of times."""

    def __init__(self, renderer, handle):
        self._r, self.handle = renderer, handle
        n, t = C.c_uint32(0), C.c_uint64(0)
        _check("prk_spans_info", renderer._L.prk_spans_info(renderer._h, handle, C.byref(n), C.byref(t)))
        self.list_count, self.total = n.value, t.value

    def counts(self):
        """uint32 [list_count]: each list's spans."""
        out = np.zeros(self.list_count, np.uint32)
        _check("prk_spans_lists", self._r._L.prk_spans_lists(self._r._h, self.handle, _ptr(out)))
        return out

    def download(self):
        """uint32 [total, 25]: the packed spans (span_records' words)."""
        w = np.empty((self.total, 25), np.uint32)
        _check("prk_spans_download", self._r._L.prk_spans_download(self._r._h, self.handle, _ptr(w), self.total))
        return w

    def close(self):
        """prk_spans_destroy (the Renderer's close frees what is left)."""
        if self.handle is not None and getattr(self._r, "_h", None):
            _check("prk_spans_destroy", self._r._L.prk_spans_destroy(self._r._h, self.handle))
        self.handle = None


class Renderer:
    """One GPU context: render target, camera/lights, resident geometry and
    textures, and the list of recorded draws of the current frame."""

    def __init__(self, device=0):
        self._L = lib()
        h = C.c_void_p()
        _check("prk_create", self._L.prk_create(int(device), C.byref(h)))
        self._h = h
        self._keep = []
        self.width = self.height = self.row0 = self.row1 = 0
        _LIVE.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._L.prk_destroy(self._h)
            self._h = None

    def __del__(self):
        # no GPU calls while the interpreter is tearing down (module globals,
        # torch's allocator and the HIP runtime may already be gone): the
        # atexit handler above closed every context before that began
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    # ---- target -----------------------------------------------------------
    def target_alloc(self, width, height, row0=0, row1=None):
        row1 = height if row1 is None else row1
        _check("prk_target_alloc", self._L.prk_target_alloc(self._h, width, height, row0, row1, None, None))
        self.width, self.height, self.row0, self.row1 = width, height, row0, row1

    def target_bind(self, color_ptr, pitch_bytes, z_ptr, width, height, row0=0, row1=None):
        """Bind caller-owned device memory (e.g. torch tensors' data_ptr())."""
        row1 = height if row1 is None else row1
        _check("prk_target_bind", self._L.prk_target_bind(self._h, C.c_void_p(color_ptr), pitch_bytes,
                                                          C.c_void_p(z_ptr), width, height, row0, row1))
        self.width, self.height, self.row0, self.row1 = width, height, row0, row1

    def clear(self, color=0xFF000000, z=None):
        z = -float(np.finfo(np.float32).max) if z is None else z
        _check("prk_target_clear", self._L.prk_target_clear(self._h, C.c_uint32(color), C.c_float(z)))

    def clear_on_flush(self, color=0xFF000000, z=None):
        """The same fill, fused into the next complete_all_work()."""
        z = -float(np.finfo(np.float32).max) if z is None else z
        _check("prk_target_clear_on_flush",
               self._L.prk_target_clear_on_flush(self._h, C.c_uint32(color), C.c_float(z)))

    def upload(self, color, z):
        color = np.ascontiguousarray(color, np.uint32)
        z = np.ascontiguousarray(z, np.float32)
        _check("prk_target_upload", self._L.prk_target_upload(self._h, _ptr(color), self.width * 4, _ptr(z)))

    def download(self):
        rows = self.row1 - self.row0
        color = np.empty((rows, self.width), np.uint32)
        z = np.empty((rows, self.width), np.float32)
        _check("prk_target_download", self._L.prk_target_download(self._h, _ptr(color), self.width * 4,
                                                                  _ptr(z)))
        return color, z

    def winners(self):
        rows = self.row1 - self.row0
        w = np.empty((rows, self.width), np.int32)
        _check("prk_download_winners", self._L.prk_download_winners(self._h, _ptr(w)))
        return w

    # ---- visibility feedback ----------------------------------------------
    def visibility(self):
        """prk_visibility_info: (id_count, covered, visible_ids) of the last
        frame -- the ids its flush handed out, the pixels of this context's
        band that any of them won, and how many ids won at least one.  Needs
        set_debug(True) at the flush; the first call after a flush reduces
        the winner map on the device, later ones reuse the result."""
        n, cov, vis = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        _check("prk_visibility_info", self._L.prk_visibility_info(self._h, C.byref(n), C.byref(cov), C.byref(vis)))
        return n.value, cov.value, vis.value

    def visibility_counts(self, first=0, count=None):
        """prk_visibility_counts: uint32 [count], the pixels ids first ...
        first + count won (None: to the frame's last id)."""
        if count is None:
            count = self.visibility()[0] - int(first)
        out = np.zeros(max(0, int(count)), np.uint32)
        _check("prk_visibility_counts", self._L.prk_visibility_counts(self._h, int(first), int(count), _ptr(out)))
        return out

    def visibility_groups(self, starts):
        """prk_visibility_groups: for the groups of ids [starts[g],
        starts[g + 1]) (uint32 [groups + 1], non-decreasing), (pixels, visible):
        uint32 [groups] each -- a group's pixels, and how many of its ids won any."""
        st = np.ascontiguousarray(starts, np.uint32).reshape(-1)
        if st.shape[0] < 1:
            raise ValueError("visibility_groups: starts needs groups + 1 words")
        g = st.shape[0] - 1
        pix, vis = np.zeros(g, np.uint32), np.zeros(g, np.uint32)
        _check("prk_visibility_groups", self._L.prk_visibility_groups(self._h, _ptr(st), g, _ptr(pix), _ptr(vis)))
        return pix, vis

    def visibility_ids(self):
        """prk_visibility_ids: uint32 [visible_ids], the ids that won a pixel, ascending."""
        total = C.c_uint64(0)
        _check("prk_visibility_ids", self._L.prk_visibility_ids(self._h, None, 0, C.byref(total)))
        out = np.zeros(total.value, np.uint32)
        _check("prk_visibility_ids", self._L.prk_visibility_ids(self._h, _ptr(out), total.value, C.byref(total)))
        return out

    def visibility_device(self):
        """prk_visibility_device: (counts_ptr, pix_prefix_ptr, id_count) -- the
        library's device arrays of id_count and id_count + 1 uint32 words,
        complete, read-only, valid until the next flush or target change."""
        cp, pp, n = C.c_void_p(), C.c_void_p(), C.c_uint32(0)
        _check("prk_visibility_device", self._L.prk_visibility_device(self._h, C.byref(cp), C.byref(pp), C.byref(n)))
        return cp.value or 0, pp.value or 0, n.value

    # ---- bounds occlusion test ---------------------------------------------
    def visibility_bounds(self, bounds, xforms, P=None):
        """prk_visibility_bounds: uint32 [n], for every box (pack_bounds rows;
        xforms float32 [k, 3, 4]) an upper bound on the pixels anything inside
        it could win over the z the target holds now -- 0: it cannot be seen.
        Rebuilds the target's min-z tile map, tests on the device, waits."""
        (b, xf), (bp, xp) = _bound_tables(bounds, xforms)
        out = np.zeros(b.shape[0], np.uint32)
        Pc = None if P is None else (C.c_float * 3)(*P)
        _check("prk_visibility_bounds", self._L.prk_visibility_bounds(
            self._h, bp, b.shape[0], xp, 0 if xf is None else xf.shape[0],
            None if Pc is None else C.cast(Pc, C.c_void_p), _ptr(out)))
        return out

    def visibility_bounds_device(self):
        """prk_visibility_bounds_device: (pixels_ptr, count) -- the last
        answer's device array, valid until the next visibility_bounds or
        target change."""
        pp, n = C.c_void_p(), C.c_uint32(0)
        _check("prk_visibility_bounds_device", self._L.prk_visibility_bounds_device(self._h, C.byref(pp), C.byref(n)))
        return pp.value or 0, n.value

    def ztiles(self):
        """prk_debug_ztiles: (zmin float32 [tiles_y, tiles_x], first tile row)
        of the last visibility_bounds."""
        tx, ty, t0 = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check("prk_debug_ztiles", self._L.prk_debug_ztiles(self._h, None, 0, C.byref(tx), C.byref(ty), C.byref(t0)))
        out = np.zeros((ty.value, tx.value), np.float32)
        _check("prk_debug_ztiles", self._L.prk_debug_ztiles(self._h, _ptr(out), out.size, C.byref(tx), C.byref(ty),
                                                            C.byref(t0)))
        return out, t0.value

    def bounds_ms(self):
        """prk_debug_bounds_ms: (ztile_ms, test_ms), the device times of the
        last visibility_bounds' two kernels."""
        a, b = C.c_float(0.0), C.c_float(0.0)
        _check("prk_debug_bounds_ms", self._L.prk_debug_bounds_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def geometry_select_bounds(self, src, dst, items, levels, xforms, dst_first_tri=0):
        """prk_geometry_select_bounds: geometry_select from the last frame's
        counts, except that an item with id_count == 0 takes its word of the
        last visibility_bounds (one box an item).  Returns (total, chosen
        int32 [n], out_first uint32 [n + 1])."""
        (it, lv, xf), (ip, lp, xp) = _select_tables(items, levels, xforms)
        n = it.shape[0]
        chosen, first = np.zeros(n, np.int32), np.zeros(n + 1, np.uint32)
        total = C.c_uint64(0)
        _check("prk_geometry_select_bounds", self._L.prk_geometry_select_bounds(
            self._h, src, dst, int(dst_first_tri), ip, n, lp, 0 if lv is None else lv.shape[0], xp,
            0 if xf is None else xf.shape[0], _ptr(chosen), _ptr(first), C.byref(total)))
        return total.value, chosen, first

    # ---- state ------------------------------------------------------------
    def set_camera(self, transform, lights):
        self._cam = (transform, lights)
        _check("prk_set_camera", self._L.prk_set_camera(self._h, C.byref(transform), C.byref(lights)))

    def set_shade_camera(self, transform, lights):
        """After set_camera: the span shading (Phong, unprojection) uses these
        instead -- Commands as DrawModel* sees them when the caller changed
        them after FillEdgeTable (projekt.cpp:452-458, 2042-2046)."""
        self._shade_cam = (transform, lights)
        _check("prk_set_shade_camera", self._L.prk_set_shade_camera(self._h, C.byref(transform),
                                                                    C.byref(lights)))

    def texture(self, tex):
        """tex: scenes.Texture (uint32 texels with the zeroed guard row)."""
        texels = np.ascontiguousarray(tex.texels, np.uint32)
        bm = abi.PrkBitmap(texels.ctypes.data, tex.width, tex.height, texels.shape[1] * 4)
        h = C.c_int32(-1)
        _check("prk_texture_create", self._L.prk_texture_create(self._h, C.byref(bm), C.byref(h)))
        if getattr(tex, "filter", abi.PRK_FILTER_NEAREST) != abi.PRK_FILTER_NEAREST:
            self.set_filter(h.value, tex.filter)
        return h.value

    def texture_update(self, handle, tex):
        """Re-read a texture's bitmap into `handle` (prk_texture_update)."""
        texels = np.ascontiguousarray(tex.texels, np.uint32)
        bm = abi.PrkBitmap(texels.ctypes.data, tex.width, tex.height, texels.shape[1] * 4)
        _check("prk_texture_update", self._L.prk_texture_update(self._h, handle, C.byref(bm)))

    def texture_alloc(self, width, height):
        """prk_texture_alloc: a zeroed library-owned texture, a destination
        for texture_from_target."""
        h = C.c_int32(-1)
        _check("prk_texture_alloc", self._L.prk_texture_alloc(self._h, int(width), int(height), C.byref(h)))
        return h.value

    def texture_from_target(self, tex, rect=None, factor=1, dst=(0, 0)):
        """prk_texture_from_target: the target's colour over rect = (x0, y0,
        width, height) in frame pixels (None: the whole band), box-filtered
        by factor 1, 2 or 4 into texture `tex` at texel dst = (x, y).  Does
        not wait for the device."""
        x0, y0, w, h = (0, self.row0, self.width, self.row1 - self.row0) if rect is None else rect
        _check("prk_texture_from_target", self._L.prk_texture_from_target(
            self._h, tex, int(x0), int(y0), int(w), int(h), int(factor), int(dst[0]), int(dst[1])))

    def texture_info(self, tex):
        """prk_texture_info: (width, height, pitch in bytes)."""
        v = [C.c_int32(0) for _ in range(3)]
        _check("prk_texture_info", self._L.prk_texture_info(self._h, tex, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def texture_download(self, tex):
        """prk_texture_download: uint32 [height, width], the texture's texels
        (without the guard row) after everything queued that writes them."""
        w, h, _ = self.texture_info(tex)
        out = np.empty((h, w), np.uint32)
        _check("prk_texture_download", self._L.prk_texture_download(self._h, tex, _ptr(out), 4 * w))
        return out

    # ---- target layers ----------------------------------------------------
    def layer_alloc(self, width, height):
        """prk_layer_alloc: a library-owned layer of width x height (colour,
        z) pixels, every colour word 0 and every z -FLT_MAX."""
        h = C.c_int32(-1)
        _check("prk_layer_alloc", self._L.prk_layer_alloc(self._h, int(width), int(height), C.byref(h)))
        return h.value

    def layer_wrap(self, color_ptr, pitch_bytes, z_ptr, width, height):
        """prk_layer_wrap_device: a read-only layer over caller-owned device
        memory (a peer context's target after its synchronize(), a torch
        tensor's data_ptr()); no copy is made."""
        h = C.c_int32(-1)
        _check("prk_layer_wrap_device", self._L.prk_layer_wrap_device(
            self._h, C.c_void_p(color_ptr), int(pitch_bytes), C.c_void_p(z_ptr), int(width), int(height), C.byref(h)))
        return h.value

    def layer_from_target(self, layer, rect=None, dst=(0, 0)):
        """prk_layer_from_target: colour and z of the target over rect = (x0,
        y0, width, height) in frame pixels (None: the whole band) into layer
        `layer` at pixel dst = (x, y).  Does not wait for the device."""
        x0, y0, w, h = (0, self.row0, self.width, self.row1 - self.row0) if rect is None else rect
        _check("prk_layer_from_target", self._L.prk_layer_from_target(
            self._h, layer, int(x0), int(y0), int(w), int(h), int(dst[0]), int(dst[1])))

    def target_from_layer(self, layer, rect=None, dst=None, rule=abi.PRK_MERGE_COPY):
        """prk_target_from_layer: the layer's pixels over rect = (src_x,
        src_y, width, height) (None: the whole layer) into the target at frame
        pixel dst = (x0, y0) (None: the band's first pixel), every pixel
        (PRK_MERGE_COPY) or where the layer's z wins (PRK_MERGE_GREATER,
        PRK_MERGE_GREATER_EQUAL).  Does not wait for the device."""
        sx, sy, w, h = (0, 0) + self.layer_info(layer)[:2] if rect is None else rect
        x0, y0 = (0, self.row0) if dst is None else dst
        _check("prk_target_from_layer", self._L.prk_target_from_layer(
            self._h, layer, int(sx), int(sy), int(w), int(h), int(x0), int(y0), int(rule)))

    def layer_info(self, layer):
        """prk_layer_info: (width, height, colour pitch in bytes, wrapped)."""
        v = [C.c_int32(0) for _ in range(4)]
        _check("prk_layer_info", self._L.prk_layer_info(self._h, layer, *[C.byref(x) for x in v]))
        return v[0].value, v[1].value, v[2].value, bool(v[3].value)

    def layer_download(self, layer):
        """prk_layer_download: (uint32 [height, width], float32 [height,
        width]), the layer's colour and z after everything queued that writes
        them."""
        w, h = self.layer_info(layer)[:2]
        color = np.empty((h, w), np.uint32)
        z = np.empty((h, w), np.float32)
        _check("prk_layer_download", self._L.prk_layer_download(self._h, layer, _ptr(color), 4 * w, _ptr(z)))
        return color, z

    def layer_destroy(self, layer):
        """prk_layer_destroy (the Renderer's close frees what is left)."""
        _check("prk_layer_destroy", self._L.prk_layer_destroy(self._h, layer))

    def geometry_update(self, handle, vertices, colors=None, normals=None, uvs=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float32)
                for a in (vertices, colors, normals, uvs)]
        _check("prk_geometry_update", self._L.prk_geometry_update(self._h, handle, *[_ptr(a) for a in arrs],
                                                                  arrs[0].shape[0]))

    def geometry_write(self, handle, first_vertex, vertices=None, colors=None, normals=None, uvs=None,
                       count=None):
        """prk_geometry_write of vertices [first_vertex, first_vertex+count)
        (count: the given arrays' length); waits for the copy, since the
        arrays here are temporaries."""
        arrs = [None if a is None else np.ascontiguousarray(a, np.float32)
                for a in (vertices, colors, normals, uvs)]
        if count is None:
            count = next(a.shape[0] for a in arrs if a is not None)
        _check("prk_geometry_write", self._L.prk_geometry_write(self._h, handle, first_vertex, count,
                                                                *[_ptr(a) for a in arrs]))
        self.synchronize()

    def set_filter(self, texture, filt):
        """Texture sampling: PRK_FILTER_NEAREST (the reference's) or
        PRK_FILTER_BILINEAR (an extension, AVX semantics only)."""
        _check("prk_texture_set_filter", self._L.prk_texture_set_filter(self._h, texture, filt))

    def geometry(self, vertices, colors=None, normals=None, uvs=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float32)
                for a in (vertices, colors, normals, uvs)]
        h = C.c_int32(-1)
        nv = arrs[0].shape[0]
        _check("prk_geometry_create", self._L.prk_geometry_create(self._h, *[_ptr(a) for a in arrs],
                                                                  nv, C.byref(h)))
        return h.value

    def geometry_device(self, v_ptr, c_ptr, n_ptr, uv_ptr, vertex_count):
        h = C.c_int32(-1)
        ptrs = [C.c_void_p(p) if p else None for p in (v_ptr, c_ptr, n_ptr, uv_ptr)]
        _check("prk_geometry_wrap_device", self._L.prk_geometry_wrap_device(self._h, *ptrs, vertex_count,
                                                                            C.byref(h)))
        return h.value

    def geometry_alloc(self):
        """prk_geometry_alloc: an empty library-owned geometry, a destination
        for geometry_transform."""
        h = C.c_int32(-1)
        _check("prk_geometry_alloc", self._L.prk_geometry_alloc(self._h, C.byref(h)))
        return h.value

    def geometry_transform(self, src, dst, runs, xforms):
        """prk_geometry_transform: runs uint32 [n, 4] of (src_first_tri,
        tri_count, dst_first_tri, xform), xforms float32 [m, 3, 4] row-major;
        both are copied at the call, which does not wait for the device."""
        r = np.ascontiguousarray(runs, np.uint32).reshape(-1, 4)
        x = np.ascontiguousarray(xforms, np.float32).reshape(-1, 3, 4)
        _check("prk_geometry_transform", self._L.prk_geometry_transform(
            self._h, src, dst, C.cast(r.ctypes.data, C.POINTER(abi.PrkXformRun)), r.shape[0],
            C.cast(x.ctypes.data, C.POINTER(abi.PrkXform)), x.shape[0]))

    def geometry_select(self, src, dst, items, levels, xforms, dst_first_tri=0, item_pixels=None):
        """prk_geometry_select: cull and pick a level of detail on the device.
        items uint32 [n, 5] of (first_id, id_count, first_level, level_count,
        xform), levels uint32 [m, 3] of (min_pixels, src_first_tri, tri_count),
        xforms float32 [k, 3, 4]; item_pixels uint32 [n], or None for the last
        frame's counts (set_debug(True) at its flush).  The chosen triangles
        go to dst from dst_first_tri on, packed in item order; the call waits
        for the total, not for the pass that writes them.  Returns (total,
        chosen int32 [n], out_first uint32 [n + 1])."""
        (it, lv, xf), (ip, lp, xp) = _select_tables(items, levels, xforms)
        n = it.shape[0]
        px = None if item_pixels is None else np.ascontiguousarray(item_pixels, np.uint32).reshape(-1)
        if px is not None and px.shape[0] != n:
            raise ValueError("geometry_select: item_pixels needs a word an item")
        chosen, first = np.zeros(n, np.int32), np.zeros(n + 1, np.uint32)
        total = C.c_uint64(0)
        _check("prk_geometry_select", self._L.prk_geometry_select(
            self._h, src, dst, int(dst_first_tri), ip, n, lp, 0 if lv is None else lv.shape[0], xp,
            0 if xf is None else xf.shape[0], _ptr(px), _ptr(chosen), _ptr(first), C.byref(total)))
        return total.value, chosen, first

    def select_ms(self):
        """prk_debug_select_ms: (choose_ms, emit_ms), the device times of the
        last geometry_select's uploads + choice + scan and of its emit pass."""
        a, b = C.c_float(0.0), C.c_float(0.0)
        _check("prk_debug_select_ms", self._L.prk_debug_select_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def geometry_download(self, geom, first_tri=0, tri_count=None, arrays=(True, True, True, True)):
        """prk_geometry_download of triangles [first_tri, first_tri +
        tri_count) (None: to the geometry's end, found by asking): (vertices
        [n, 3], colors [n, 4], normals [n, 3], uvs [n, 2]), None for an array
        the geometry lacks (or `arrays` leaves out)."""
        nv, have = self.geometry_info(geom)
        if tri_count is None:
            tri_count = max(0, nv // 3 - first_tri)
        n = 3 * tri_count
        out = [np.empty((n, comp), np.float32) if arrays[k] and have[k] else None
               for k, comp in enumerate((3, 4, 3, 2))]
        _check("prk_geometry_download", self._L.prk_geometry_download(self._h, geom, 3 * first_tri, n,
                                                                      *[_ptr(a) for a in out]))
        return tuple(out)

    def geometry_info(self, geom):
        """prk_geometry_info: (vertex count, (has vertices, colors, normals, uvs))."""
        n, m = C.c_uint32(0), C.c_uint32(0)
        _check("prk_geometry_info", self._L.prk_geometry_info(self._h, geom, C.byref(n), C.byref(m)))
        return n.value, tuple(bool(m.value >> k & 1) for k in range(4))

    def target(self):
        """prk_get_target: (color_ptr, pitch, z_ptr, W, H, row0, row1)."""
        cp, zp = C.c_void_p(), C.c_void_p()
        v = [C.c_int32(0) for _ in range(5)]
        _check("prk_get_target", self._L.prk_get_target(self._h, C.byref(cp), C.byref(v[0]), C.byref(zp),
                                                        *[C.byref(x) for x in v[1:]]))
        return cp.value, v[0].value, zp.value, v[1].value, v[2].value, v[3].value, v[4].value

    def device_stream(self):
        """prk_get_device: (device, own stream as an int)."""
        d, s = C.c_int32(0), C.c_void_p()
        _check("prk_get_device", self._L.prk_get_device(self._h, C.byref(d), C.byref(s)))
        return d.value, s.value or 0

    def set_tile(self, tw, th):
        _check("prk_set_tile", self._L.prk_set_tile(self._h, tw, th))

    def set_debug(self, on=True):
        _check("prk_set_debug", self._L.prk_set_debug(self._h, int(bool(on))))

    def set_early_z(self, on=True):
        """prk_set_early_z: span-record frames write z in the visibility
        kernel, so download() copies it while the frame shades."""
        _check("prk_set_early_z", self._L.prk_set_early_z(self._h, int(bool(on))))

    # ---- draws (the reference's entry points) -----------------------------
    def _draw(self, geom, first_tri, tri_count, P, semantics, phong, texture, tris_per_object=1, setup=None):
        Pc = (C.c_float * 3)(*(P or (0.0, 0.0, 0.0)))
        tex = -1 if texture is None else texture
        if setup is None:
            _check("prk_draw_objects", self._L.prk_draw_objects(self._h, geom, first_tri, tri_count,
                                                                tris_per_object, Pc, semantics, int(bool(phong)), tex))
        else:  # FillEdgeTable's own PhongShading / Object->Bitmap (abi.PRK_SETUP_*)
            _check("prk_draw_objects_setup", self._L.prk_draw_objects_setup(
                self._h, geom, first_tri, tri_count, tris_per_object, Pc, semantics, int(bool(phong)), tex,
                int(setup)))

    def draw_model_optimized(self, geom, tri_count, first_tri=0, P=None, bitmap=None, phong=True):
        """DrawModelOptimized(RenderQueue, ...) -> FillLineOptimized semantics
        (projekt.cpp:3615-3871, 1492-2320).  Needs bitmap + phong."""
        self._draw(geom, first_tri, tri_count, P, abi.PRK_SEM_AVX, phong, bitmap)

    def draw_model(self, geom, tri_count, first_tri=0, P=None, bitmap=None, phong=False):
        """DrawModel (projekt.cpp:162-601) scalar semantics."""
        self._draw(geom, first_tri, tri_count, P, abi.PRK_SEM_SCALAR, phong, bitmap)

    def draw_model_optimized_st(self, geom, tri_count, first_tri=0, P=None, bitmap=None, phong=True):
        """The single-thread overload DrawModelOptimized(Buffer, ...)
        (projekt.cpp:2350-3358): FillLineOptimized's math with its left-clip
        XOffset quirk (2508) and the >= z-test (3205).  Needs bitmap + phong."""
        self._draw(geom, first_tri, tri_count, P, abi.PRK_SEM_AVX_ST, phong, bitmap)

    def draw(self, semantics, geom, tri_count, first_tri=0, P=None, bitmap=None, phong=True, tris_per_object=1,
             setup=None):
        """Any PRK_SEM_* draw; tris_per_object > 1: consecutive objects of that
        many triangles, one active edge table each (prk_draw_objects).
        setup: FillEdgeTable's own PhongShading / Object->Bitmap as
        abi.PRK_SETUP_* bits (None: as the draw; prk_draw_objects_setup)."""
        self._draw(geom, first_tri, tri_count, P, semantics, phong, bitmap, tris_per_object, setup)

    def draw_edges(self, edge_words, semantics=abi.PRK_SEM_AVX, bitmap=None, phong=True):
        """DrawModelOptimized* on a ready edge_info list: uint32 [n, 27] in
        prk_edge layout (prk.h), sorted by YMin as FillEdgeTable leaves it."""
        w = np.ascontiguousarray(edge_words, np.uint32)
        self._keep.append(w)
        _check("prk_draw_edges", self._L.prk_draw_edges(self._h, _ptr(w), w.shape[0], semantics, int(bool(phong)),
                                                        -1 if bitmap is None else bitmap))

    def edge_records(self, geom, tri_count, first_tri=0, P=None, setup=3, tris_per_object=None):
        """prk_edge_records: FillEdgeTable's records of consecutive objects of
        tris_per_object triangles (None: one object), set up on the GPU under
        set_camera's transform and lights with abi.PRK_SETUP_* bits `setup`.
        Returns (words, counts): uint32 [total, 27] in prk_edge layout (what
        draw_edges takes), object o's MergeSorted records at
        words[counts[:o].sum():][:counts[o]], and uint32 [nobj]."""
        per = max(1, tri_count) if tris_per_object is None else int(tris_per_object)
        nobj = (tri_count + per - 1) // per if per > 0 else 0
        words = np.empty((3 * tri_count, 27), np.uint32)  # (FillEdgeTable writes at most 3 edges a triangle)
        counts = np.zeros(nobj, np.uint32)
        total = C.c_uint64(0)
        Pc = (C.c_float * 3)(*(P or (0.0, 0.0, 0.0)))
        _check("prk_edge_records", self._L.prk_edge_records(self._h, geom, first_tri, tri_count, per, Pc, int(setup),
                                                            _ptr(words), words.shape[0], _ptr(counts),
                                                            C.byref(total)))
        return words[:total.value], counts

    def draw_edge_lists(self, words, counts, semantics=abi.PRK_SEM_AVX, bitmap=None, phong=True):
        """prk_draw_edge_lists: a batch of edge_info lists in one call, the two
        arrays edge_records returns (uint32 [total, 27] in prk_edge layout,
        uint32 [nobj]).  List o is drawn as draw_edges(words of list o) draws
        it and takes winner id base + o, empty or not; lists sorted by YMin
        run through the walks of triangle objects of their size."""
        w = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
        n = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if int(n.sum(dtype=np.uint64)) != w.shape[0]:
            raise ValueError("draw_edge_lists: counts sum to %d, %d records given" % (int(n.sum(dtype=np.uint64)),
                                                                                   w.shape[0]))
        _check("prk_draw_edge_lists", self._L.prk_draw_edge_lists(self._h, _ptr(w), _ptr(n), n.shape[0], semantics,
                                                                  int(bool(phong)),
                                                                  -1 if bitmap is None else bitmap))

    def records_from_geometry(self, geom, tri_count, first_tri=0, P=None, setup=3, tris_per_object=None):
        """prk_records_from_geometry: edge_records' records of the same
        arguments, kept on the device -> Records."""
        per = max(1, tri_count) if tris_per_object is None else int(tris_per_object)
        Pc = (C.c_float * 3)(*(P or (0.0, 0.0, 0.0)))
        h = C.c_int32(-1)
        _check("prk_records_from_geometry", self._L.prk_records_from_geometry(
            self._h, geom, first_tri, tri_count, per, Pc, int(setup), C.byref(h), None, None))
        return Records(self, h.value)

    def records_upload(self, words, counts):
        """prk_records_upload: the two arrays draw_edge_lists takes, copied to
        the device once -> Records."""
        w = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
        n = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if int(n.sum(dtype=np.uint64)) != w.shape[0]:
            raise ValueError("records_upload: counts sum to %d, %d records given" % (int(n.sum(dtype=np.uint64)),
                                                                                  w.shape[0]))
        h = C.c_int32(-1)
        _check("prk_records_upload", self._L.prk_records_upload(self._h, _ptr(w), _ptr(n), n.shape[0], C.byref(h)))
        return Records(self, h.value)

    def draw_records(self, rec, first_list=0, list_count=None, semantics=abi.PRK_SEM_AVX, bitmap=None, phong=True):
        """prk_draw_records: lists [first_list, first_list + list_count) of a
        Records (None: to its last list), drawn as draw_edge_lists draws the
        same lists from host arrays -- from where they are on the device."""
        n = rec.list_count - first_list if list_count is None else list_count
        _check("prk_draw_records", self._L.prk_draw_records(self._h, rec.handle, first_list, n, semantics,
                                                            int(bool(phong)), -1 if bitmap is None else bitmap))

    def stage_bytes(self):
        """prk_debug_stage_bytes: the bytes the last whole-object pass copied
        from the host in its staging upload."""
        out = C.c_uint64(0)
        _check("prk_debug_stage_bytes", self._L.prk_debug_stage_bytes(self._h, C.byref(out)))
        return out.value

    def advance_edge_lists(self, words, counts, height):
        """prk_advance_edge_lists: what DrawModel* leaves in every list of a
        batch over a frame of `height` rows, walked on the GPU -- the two
        arrays edge_records returns in, (words_out uint32 [total, 27],
        next int32 [total]: each record's Next as an index within its own
        list, -1 for NULL) out.  Lists sorted by YMin only (prk.h)."""
        w = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
        n = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if int(n.sum(dtype=np.uint64)) != w.shape[0]:
            raise ValueError("advance_edge_lists: counts sum to %d, %d records given" % (int(n.sum(dtype=np.uint64)),
                                                                                      w.shape[0]))
        out = np.empty_like(w)
        nxt = np.empty(w.shape[0], np.int32)
        _check("prk_advance_edge_lists", self._L.prk_advance_edge_lists(self._h, _ptr(w), _ptr(n), n.shape[0],
                                                                        int(height), _ptr(out), _ptr(nxt)))
        return out, nxt

    def span_records(self, words, counts, height):
        """prk_span_records: the spans DrawModelOptimized(RenderQueue) queues
        for every list of a batch over a frame of `height` rows, walked on
        the GPU (two calls: size, then fill) -- (span_words uint32
        [total, 25] in prk_span layout, list o's at sum(span_counts[:o]),
        span_counts uint32 [nlist]).  Lists sorted by YMin only (prk.h)."""
        w = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
        n = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if int(n.sum(dtype=np.uint64)) != w.shape[0]:
            raise ValueError("span_records: counts sum to %d, %d records given" % (int(n.sum(dtype=np.uint64)),
                                                                                w.shape[0]))
        sc = np.zeros(n.shape[0], np.uint32)
        total = C.c_uint64(0)
        _check("prk_span_records", self._L.prk_span_records(self._h, _ptr(w), _ptr(n), n.shape[0], int(height), None,
                                                            0, _ptr(sc), C.byref(total)))
        spans = np.empty((total.value, 25), np.uint32)
        _check("prk_span_records", self._L.prk_span_records(self._h, _ptr(w), _ptr(n), n.shape[0], int(height),
                                                            _ptr(spans), total.value, _ptr(sc), C.byref(total)))
        return spans, sc

    def draw_spans(self, span_words, semantics=abi.PRK_SEM_AVX, bitmap=None, phong=True):
        """Caller spans (the work records of DoLineRenderWork): uint32 [n, 25]
        in prk_span layout (prk.h)."""
        w = np.ascontiguousarray(span_words, np.uint32)
        self._keep.append(w)
        _check("prk_draw_spans", self._L.prk_draw_spans(self._h, _ptr(w), w.shape[0], semantics, int(bool(phong)),
                                                        -1 if bitmap is None else bitmap))

    def spans_upload(self, span_words):
        """prk_spans_upload: the array draw_spans takes (uint32 [n, 25]),
        copied to the device once -> Spans of one list."""
        w = np.ascontiguousarray(span_words, np.uint32).reshape(-1, 25)
        h = C.c_int32(-1)
        _check("prk_spans_upload", self._L.prk_spans_upload(self._h, _ptr(w), w.shape[0], C.byref(h)))
        return Spans(self, h.value)

    def spans_upload_rows(self, rows, pairs):
        """prk_spans_upload_rows: row work records (the arrays row_records
        returns), regrouped into spans on the device and kept there ->
        Spans of one list."""
        r = np.ascontiguousarray(rows, np.int32).reshape(-1, 2)
        p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 24)
        h = C.c_int32(-1)
        _check("prk_spans_upload_rows", self._L.prk_spans_upload_rows(self._h, _ptr(r), r.shape[0], _ptr(p),
                                                                      p.shape[0], C.byref(h)))
        return Spans(self, h.value)

    def draw_span_records(self, sp, first_span=0, span_count=None, semantics=abi.PRK_SEM_AVX, bitmap=None,
                          phong=True):
        """prk_draw_span_records: spans [first_span, first_span + span_count)
        of a Spans (None: to its last span), drawn as draw_spans draws the
        same spans from a host array -- from where they are on the device."""
        n = sp.total - first_span if span_count is None else span_count
        _check("prk_draw_span_records", self._L.prk_draw_span_records(self._h, sp.handle, first_span, n, semantics,
                                                                      int(bool(phong)),
                                                                      -1 if bitmap is None else bitmap))

    def row_records(self, words, counts, height):
        """prk_row_records: the row work DrawModelOptimizedLines queues for
        every list of a batch over a frame of `height` rows, walked on the
        GPU (two calls: size, then fill) -- (rows int32 [k, 2]: RowIndex and
        EdgeCount, list o's at sum(row_counts[:o]); pairs uint32 [m, 24] in
        prk_row_pair layout, row r's at sum(rows[:r, 1]); row_counts uint32
        [nlist]).  Lists sorted by YMin only (prk.h)."""
        w = np.ascontiguousarray(words, np.uint32).reshape(-1, 27)
        n = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if int(n.sum(dtype=np.uint64)) != w.shape[0]:
            raise ValueError("row_records: counts sum to %d, %d records given" % (int(n.sum(dtype=np.uint64)),
                                                                               w.shape[0]))
        rc = np.zeros(n.shape[0], np.uint32)
        nrow, npair = C.c_uint64(0), C.c_uint64(0)
        _check("prk_row_records", self._L.prk_row_records(self._h, _ptr(w), _ptr(n), n.shape[0], int(height), None,
                                                          0, None, 0, _ptr(rc), C.byref(nrow), C.byref(npair)))
        rows = np.empty((nrow.value, 2), np.int32)
        pairs = np.empty((npair.value, 24), np.uint32)
        _check("prk_row_records", self._L.prk_row_records(self._h, _ptr(w), _ptr(n), n.shape[0], int(height),
                                                          _ptr(rows), nrow.value, _ptr(pairs), npair.value,
                                                          _ptr(rc), C.byref(nrow), C.byref(npair)))
        return rows, pairs, rc

    def draw_rows(self, rows, pairs, semantics=abi.PRK_SEM_AVX, bitmap=None, phong=True):
        """prk_draw_rows: row work records (the arrays row_records returns)
        drawn as draw_spans draws their pairs, one winner id a pair."""
        r = np.ascontiguousarray(rows, np.int32).reshape(-1, 2)
        p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 24)
        _check("prk_draw_rows", self._L.prk_draw_rows(self._h, _ptr(r), r.shape[0], _ptr(p), p.shape[0], semantics,
                                                      int(bool(phong)), -1 if bitmap is None else bitmap))

    def complete_all_work(self, stream=None):
        """Platform.CompleteAllWork: run every recorded draw (asynchronous)."""
        _check("prk_flush", self._L.prk_flush(self._h, None if stream is None else C.c_void_p(stream)))

    flush = complete_all_work

    def reset_draws(self):
        _check("prk_reset_draws", self._L.prk_reset_draws(self._h))

    def synchronize(self):
        _check("prk_synchronize", self._L.prk_synchronize(self._h))

    def resolve(self, stream=None):
        """Resolve the last flush's bin count (an overflowed frame is re-run
        first) and make `stream` wait for the frame's end, host-asynchronously:
        call before reading the target on another stream (prk.dist gathers)."""
        _check("prk_resolve", self._L.prk_resolve(self._h, None if stream is None else C.c_void_p(stream)))

    def timing_reset(self):
        _check("prk_timing_reset", self._L.prk_timing_reset(self._h))

    def debug_counters(self, n=16):
        out = (C.c_uint64 * n)()
        _check("prk_debug_counters", self._L.prk_debug_counters(self._h, out, n))
        return list(out)

    def walk_routes(self):
        """Which walk the large objects of the last flush that had any took
        (prk_debug_walk_routes): objects per class -- slots (the five LDS slot
        classes), huge_lds, huge_mem, wave -- how many were sized by the
        many-workgroup histogram (sized_huge), and the first large object's
        sizes as the device counted them (most, rows, ents)."""
        out = (C.c_uint32 * 12)()
        _check("prk_debug_walk_routes", self._L.prk_debug_walk_routes(self._h, out, 12))
        sizes = [v - (1 << 32) if v >> 31 else v for v in out[9:12]]  # (int32_t bits)
        return dict(slots=tuple(out[0:5]), huge_lds=out[5], huge_mem=out[6], wave=out[7], sized_huge=out[8],
                    most=sizes[0], rows=sizes[1], ents=sizes[2])

    def list_routes(self):
        """Which walk the lists of the last advance_edge_lists / span_records
        / row_records call took (prk_debug_list_routes): thread (one GPU
        thread a list, empty lists among them) and slots (a workgroup a list,
        per LDS slot class of 62 / 126 / 254 / 510 / 1022 entries)."""
        out = (C.c_uint32 * 6)()
        _check("prk_debug_list_routes", self._L.prk_debug_list_routes(self._h, out, 6))
        return dict(thread=out[0], slots=tuple(out[1:6]))

    def debug_bins(self):
        """The tile binning of the last per-triangle pass of the most recent
        flush made with set_debug on (prk_debug_bins): a dict of the frame's
        sizes (abi.PrkBinsInfo's fields) and the arrays tri_n [T], ranges
        [T, 8] uint16 (abi.TILE_RANGE_FIELDS), tri_off [T + 1], listed [T]
        uint8, offs [ntiles + 1], bins [entries, 2] (triangle, pair) and
        pair_tri [entries]."""
        fn = self._L.prk_debug_bins
        info = abi.PrkBinsInfo()
        _check("prk_debug_bins", fn(self._h, C.byref(info), None, None, None, None, 0, None, 0, None, None, 0))
        T, ne, nt = info.tri_count, info.entry_count, info.tiles_x * info.tiles_y
        out = dict(tri_n=np.zeros(T, np.uint32), ranges=np.zeros((T, 8), np.uint16),
                   tri_off=np.zeros(T + 1, np.uint32), listed=np.zeros(T, np.uint8),
                   offs=np.zeros(nt + 1, np.uint32), bins=np.zeros((ne, 2), np.uint32),
                   pair_tri=np.zeros(ne, np.uint32))
        p = {k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()}
        _check("prk_debug_bins", fn(self._h, C.byref(info), p["tri_n"], p["ranges"], p["tri_off"], p["listed"], T,
                                    p["offs"], nt, p["bins"], p["pair_tri"], ne))
        out.update({k: getattr(info, k) for k, _ in abi.PrkBinsInfo._fields_})
        return out

    def stats(self):
        s = abi.PrkStats()
        _check("prk_get_stats", self._L.prk_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in abi.PrkStats._fields_}


class Stats(dict):
    """render_scene's stats: prk_get_stats as a dict, and the flush's walk
    routes (Renderer.walk_routes) as the attribute walk_routes."""
    walk_routes = None


def render_scene(scene, semantics=abi.PRK_SEM_AVX, phong=True, device=0, tile=None, debug=True,
                 color=None, z=None, rows=None, fused_clear=False, tris_per_object=1, setup=None,
                 shade_camera=None, early_z=False):
    """Convenience: draw a whole scenes.Scene (per-triangle submission) and
    return (color, z, winners or None, stats).  fused_clear: upload
    color / z, then clear through prk_target_clear_on_flush (the frame must
    overwrite them).  setup: FillEdgeTable's own inputs (abi.PRK_SETUP_*) of
    every draw.  shade_camera: a scene whose transform / lights shade the
    spans (set_shade_camera); `scene`'s set the draws up.  early_z:
    set_early_z (z written by the visibility kernel, copied early)."""
    r = Renderer(device)
    try:
        r0, r1 = (0, scene.height) if rows is None else rows
        r.target_alloc(scene.width, scene.height, r0, r1)
        if color is None and z is None:
            r.clear()
        else:
            r.upload(color[r0:r1], z[r0:r1])
        if fused_clear:
            r.clear_on_flush()
        if tile:
            r.set_tile(*tile)
        r.set_debug(debug)
        if early_z:
            r.set_early_z(True)
        r.set_camera(scene.prk_transform(), scene.prk_lights())
        if shade_camera is not None:
            r.set_shade_camera(shade_camera.prk_transform(), shade_camera.prk_lights())
        g = r.geometry(scene.vertices, scene.colors, scene.normals, scene.uvs)
        draws = scene.draws if scene.draws is not None else [(0, scene.tri_count, scene.texture)]
        handles = {}
        for d in draws:
            first, count, texture, sem, tpo = scenes_mod.draw_spec(d, semantics, tris_per_object)
            tex = None
            if texture is not None:
                if id(texture) not in handles:
                    handles[id(texture)] = r.texture(texture)
                tex = handles[id(texture)]
            r.draw(sem, g, count, first_tri=first, P=scene.P, bitmap=tex, phong=phong, tris_per_object=tpo,
                   setup=setup)
        r.complete_all_work()
        r.synchronize()
        col, zb = r.download()
        win = r.winners() if debug else None
        st = Stats(r.stats())
        st.walk_routes = r.walk_routes()
        return col, zb, win, st
    finally:
        r.close()
