"""CPU tests of the device transform pass's boundary (no GPU compute): the
ctypes mirror against include/prk.h, the numpy restatement of its arithmetic
(tests/xform_ref.py) against float64, and the host stub.  What the pass
computes is checked on the GPU (tests/test_gpu_geometry_transform.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prk
import xform_ref as X
from prk import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the C parameter types of the three calls (and prk_geometry_info) -> ctypes
CTYPES = {
    "prk_context *": C.c_void_p, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "float *": C.c_void_p,
    "int32_t *": C.POINTER(C.c_int32), "uint32_t *": C.POINTER(C.c_uint32), "void **": C.POINTER(C.c_void_p),    "const prk_xform_run *": C.POINTER(abi.PrkXformRun), "const prk_xform *": C.POINTER(abi.PrkXform),
}


def header():
    with open(os.path.join(ROOT, "include", "prk.h")) as f:
        return f.read()


def test_struct_layouts_match_header():
    src = header()
    assert re.search(r"typedef struct prk_xform \{\s*float M\[3\]\[4\];[^}]*\} prk_xform;", src)
    assert re.search(r"typedef struct prk_xform_run \{\s*uint32_t src_first_tri, tri_count, dst_first_tri, xform;"
                     r"[^}]*\} prk_xform_run;", src)
    assert C.sizeof(abi.PrkXform) == 48 and C.sizeof(abi.PrkXformRun) == 16
    assert [f[0] for f in abi.PrkXformRun._fields_] == ["src_first_tri", "tri_count", "dst_first_tri", "xform"]
    m = abi.PrkXform()
    m.M[1][3] = 7.0  # row-major: M[i][3] is the translation of component i
    assert np.frombuffer(m, np.float32).tolist().index(7.0) == 7


@pytest.mark.parametrize("name", sorted(abi.GEOMETRY_TRANSFORM_SIGS))
def test_signature_declared_exported_bound(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header(), re.M | re.S)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    types = [re.match(r"(.*?[ *])\w+$", p).group(1).strip() for p in params]
    assert [CTYPES[t] for t in types] == abi.GEOMETRY_TRANSFORM_SIGS[name], (name, types)
    assert name in prk.exported_symbols()
    f = getattr(prk.lib(), name)
    assert f.restype is C.c_int and list(f.argtypes) == abi.GEOMETRY_TRANSFORM_SIGS[name]
    out = subprocess.run(["nm", "-D", "--defined-only", prk.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT %s$" % name, out, re.M)


def test_python_surface_and_null_context():
    for m in ("geometry_alloc", "geometry_transform", "geometry_download", "geometry_info"):
        assert hasattr(prk.Renderer, m)
    L = prk.lib()
    h = C.c_int32(5)
    run, xf = abi.PrkXformRun(0, 1, 0, 0), abi.PrkXform()
    v = np.zeros((3, 3), np.float32)
    assert L.prk_geometry_alloc(None, C.byref(h)) == abi.PRK_ERR_ARG and h.value == 5
    assert L.prk_geometry_transform(None, 0, 1, C.byref(run), 1, C.byref(xf), 1) == abi.PRK_ERR_ARG
    assert L.prk_geometry_transform(None, 0, 1, None, 0, None, 0) == abi.PRK_ERR_ARG
    assert L.prk_geometry_download(None, 0, 0, 3, v.ctypes.data, None, None, None) == abi.PRK_ERR_ARG
    assert L.prk_geometry_info(None, 0, None, None) == abi.PRK_ERR_ARG


def test_xform_ref_against_float64():
    """The f32 expression is four rounded operations deep on the longest path
    (a product, two sums, the translation's sum); each rounds by at most half
    an ulp, a relative u = 2^-24 of its own result.  A term passes through at
    most four of them, so |f32 - f64| <= ((1 + u)^4 - 1) * (|M0 x| + |M1 y| +
    |M2 z| + |M3|), plus the float64 evaluation's own rounding (2^-50 of the
    same sum, generously); three operations for a normal."""
    u = 2.0 ** -24
    rng = np.random.default_rng(7)
    v = X.random_values(rng, (10000, 3))
    for _ in range(4):
        M = X.random_values(rng, (3, 4))
        got = X.positions(M, v).astype(np.float64)
        want = X.positions_f64(M, v)
        M64, v64 = M.astype(np.float64), v.astype(np.float64)
        mag = np.abs(v64) @ np.abs(M64[:, :3]).T + np.abs(M64[:, 3])
        assert (np.abs(got - want) <= ((1 + u) ** 4 - 1 + 2.0 ** -50) * mag).all()
        assert (got != want).any()  # (the f32 path does round)
        n = X.normals(M, v).astype(np.float64)
        assert (np.abs(n - v64 @ M64[:, :3].T) <= ((1 + u) ** 3 - 1 + 2.0 ** -50) * (mag - np.abs(M64[:, 3]))).all()
    assert np.isfinite(X.positions(M, v)).all()


def test_xform_ref_run_rules():
    rng = np.random.default_rng(8)
    src = X.random_arrays(rng, 10, colors=False)
    xf = X.random_values(rng, (2, 3, 4))
    out = X.apply_runs(src, (None,) * 4, [[0, 0, 50, 0], [2, 3, 4, 1]], xf)
    assert out[1] is None and out[0].shape == (21, 3) and not out[0][:12].any()
    assert np.array_equal(out[0][12:], X.positions(xf[1], src[0][6:15]))
    assert np.array_equal(out[3][12:].view(np.uint32), src[3][6:15].view(np.uint32))
    # identity + translation is v + t where no -0.0 is involved
    v = np.abs(src[0]) + np.float32(1.0)
    t = np.array([0.25, -3.0, 0.0], np.float32)
    assert np.array_equal(X.positions(X.translation(t), v).view(np.uint32), (v + t).view(np.uint32))
    # ... and -0.0 comes out of the identity as +0.0
    z = np.array([[-0.0, -0.0, -0.0]], np.float32)
    assert not np.signbit(X.positions(X.translation((0.0, 0.0, 0.0)), z)).any()


def test_host_stub_builds(tmp_path):
    """tools/hoststub: examples/dropin_bench still links against the stub,
    which now stands in for the transform calls too."""
    exe = tmp_path / "dropin_bench_stub"
    inc = os.path.join(ROOT, "include")
    stub = os.path.join(ROOT, "tools", "hoststub", "prk_host_stub.cpp")
    r = subprocess.run(["g++", "-O1", "-mavx2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", inc, "-o", str(exe),
                        os.path.join(ROOT, "examples", "dropin_bench.cpp"), stub], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(stub) as f:
        text = f.read()
    for name in abi.GEOMETRY_TRANSFORM_SIGS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
