"""prk_geometry_transform's arithmetic restated in numpy float32, op by op as
include/prk.h writes it, and its run / array rules on host arrays.

    positions  out[i] = ((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + M[i][3]
    normals    out[i] =  (M[i][0]*x + M[i][1]*y) + M[i][2]*z
    colours, uvs       copied bit for bit

Every numpy operation below takes float32 operands and returns float32, so
each product and each sum is rounded on its own (numpy never fuses).
"""
import numpy as np

COMP = (3, 4, 3, 2)  # floats a vertex: vertices, colors, normals, uvs


def _rows(M, v):
    M = np.asarray(M, np.float32)
    v = np.asarray(v, np.float32)
    assert M.shape == (3, 4) and v.ndim == 2 and v.shape[1] == 3
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    out = np.empty_like(v)
    for i in range(3):
        a = M[i, 0] * x
        b = M[i, 1] * y
        s = a + b
        c = M[i, 2] * z
        out[:, i] = s + c
    assert out.dtype == np.float32
    return out, M


def positions(M, v):
    out, M = _rows(M, v)
    for i in range(3):
        out[:, i] = out[:, i] + M[i, 3]
    return out


def normals(M, v):
    return _rows(M, v)[0]


def positions_f64(M, v):
    """The same expression in float64 (the value the f32 one approximates)."""
    M = np.asarray(M, np.float32).astype(np.float64)
    v = np.asarray(v, np.float32).astype(np.float64)
    return v @ M[:, :3].T + M[:, 3]


def apply(M, arrays):
    """One matrix on (vertices, colors, normals, uvs); None stays None."""
    V, Cc, N, UV = arrays
    return (positions(M, V), None if Cc is None else Cc.copy(), None if N is None else normals(M, N),
            None if UV is None else UV.copy())


def apply_runs(src, dst, runs, xforms):
    """What prk_geometry_transform leaves in dst: src / dst are 4-tuples of
    arrays or None (dst may be all None: a fresh prk_geometry_alloc), runs
    [n, 4] of (src_first_tri, tri_count, dst_first_tri, xform).  Destination
    ranges must not overlap (the library leaves the overlap unspecified)."""
    runs = np.asarray(runs, np.int64).reshape(-1, 4)
    old = max([a.shape[0] for a in dst if a is not None], default=0)
    live = runs[runs[:, 1] > 0]
    nv = max(old, int(3 * (live[:, 2] + live[:, 1]).max())) if live.size else old
    out = []
    for k in range(4):
        if dst[k] is None and (src[k] is None or not live.size):
            out.append(None)
            continue
        a = np.zeros((nv, COMP[k]), np.float32)
        if dst[k] is not None:
            a[:dst[k].shape[0]] = dst[k]
        out.append(a)
    for s0, n, d0, x in live.tolist():
        part = apply(xforms[x], tuple(None if a is None else a[3 * s0:3 * (s0 + n)] for a in src))
        for k in range(4):
            if part[k] is not None:
                out[k][3 * d0:3 * (d0 + n)] = part[k]
    return tuple(out)


def random_values(rng, shape):
    """float32 of magnitude in [2^-20, 2^20] and random sign, with exact +-0
    and +-1 entries mixed in: no product of two of them is denormal or
    overflows."""
    mag = np.exp2(rng.uniform(-20.0, 20.0, shape)).astype(np.float32)
    mag = np.clip(mag, np.float32(2.0 ** -20), np.float32(2.0 ** 20))
    v = np.where(rng.random(shape) < 0.5, -mag, mag).astype(np.float32)
    pick = rng.random(shape)
    for lo, val in ((0.00, 0.0), (0.03, -0.0), (0.06, 1.0), (0.09, -1.0)):
        v = np.where((pick >= lo) & (pick < lo + 0.03), np.float32(val), v)
    return np.ascontiguousarray(v, np.float32)


def random_arrays(rng, tris, colors=True, normals_=True, uvs=True):
    n = 3 * tris
    return (random_values(rng, (n, 3)), random_values(rng, (n, 4)) if colors else None,
            random_values(rng, (n, 3)) if normals_ else None, random_values(rng, (n, 2)) if uvs else None)


def translation(t):
    M = np.zeros((3, 4), np.float32)
    M[0, 0] = M[1, 1] = M[2, 2] = 1.0
    M[:, 3] = t
    return M


def rotation_yx(deg_y, deg_x, t=(0.0, 0.0, 0.0)):
    """Rotate about y, then about x, then translate: float32 entries of the
    float64 product."""
    ay, ax = np.deg2rad(deg_y), np.deg2rad(deg_x)
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    M = np.zeros((3, 4), np.float32)
    M[:, :3] = (Rx @ Ry).astype(np.float32)
    M[:, 3] = t
    return M
