"""prk_visibility_bounds (include/prk.h), written from the definition in numpy
float32, op for op: the min-z map of a target band in tiles of 8 x 8 pixels,
and for every bounding box an upper bound on the pixels anything inside it
could win over that depth.  The matrix arithmetic goes through
tests/xform_ref.py (prk_geometry_transform's, nothing fused); the projection
is pyref.project's expression on arrays (tests/test_bounds_abi.py holds the two
together corner by corner).
"""
import collections

import numpy as np

import xform_ref as X

f32 = np.float32
TILE = 8

Boxes = collections.namedtuple("Boxes", "znear whole rect")  # rect: int64 [n, 4] of x0, x1, y0, y1 (clamped)


def tile_shape(W, row0, row1):
    """(tiles_y, tiles_x, first_tile_row) of the band's map."""
    return (row1 + 7) // 8 - row0 // 8, (W + 7) // 8, row0 // 8


def ztiles(z, row0):
    """zmin float32 [tiles_y, tiles_x] of the band z (float32 [row1 - row0, W],
    frame rows row0 ...): per tile the smallest non-NaN word, +inf without one."""
    z = np.asarray(z, f32)
    rows, W = z.shape
    ty, tx, t0 = tile_shape(W, row0, row0 + rows)
    pad = np.full((8 * ty, 8 * tx), np.nan, f32)
    pad[row0 - 8 * t0:row0 - 8 * t0 + rows, :W] = z
    m = np.fmin.reduce(np.fmin.reduce(pad.reshape(ty, 8, tx, 8), axis=3), axis=1)  # (fmin drops a NaN)
    return np.where(np.isnan(m), f32(np.inf), m).astype(f32)


def corners(lo, hi):
    """float32 [n, 8, 3]: corner c takes hi on axis a where bit a of c is set."""
    lo, hi = np.asarray(lo, f32).reshape(-1, 3), np.asarray(hi, f32).reshape(-1, 3)
    pick = (np.arange(8)[:, None] >> np.arange(3)[None, :]) & 1
    return np.where(pick[None] == 1, hi[:, None, :], lo[:, None, :]).astype(f32)


def camera_space(lo, hi, xform, xforms, P):
    """float32 [n, 8, 3]: the corners through their matrices, then + P."""
    c = corners(lo, hi)
    xforms = np.asarray(xforms, f32).reshape(-1, 3, 4)
    P = np.zeros(3, f32) if P is None else np.asarray(P, f32)
    out = np.empty_like(c)
    for i, k in enumerate(np.asarray(xform, np.int64).reshape(-1).tolist()):
        out[i] = X.positions(xforms[k], c[i]) + P
    assert out.dtype == f32
    return out


def project(cam, c):
    """pyref.project's expression on arrays: (px, py, front) of the points c
    [..., 3] under cam = (D, F, M2P, cx, cy)."""
    D, F, M2P, cx, cy = [f32(v) for v in cam]
    with np.errstate(all="ignore"):
        d = D - c[..., 2]
        front = d > f32(0.2)
        k = (f32(1) / d) * F
        px = cx + M2P * (k * c[..., 0])
        py = cy + M2P * (k * c[..., 1])
    assert px.dtype == f32 and py.dtype == f32
    return px, py, front


def _axis(lo, hi, c0, c1):
    with np.errstate(all="ignore"):
        a = np.minimum(np.maximum(np.floor(lo) - f32(1), f32(c0)), f32(c1))
        b = np.minimum(np.maximum(np.floor(hi) + f32(2), f32(c0)), f32(c1))
    assert a.dtype == f32 and b.dtype == f32
    return a.astype(np.int64), b.astype(np.int64)  # (converted only after the clamp)


def boxes(lo, hi, xform, xforms, P, cam, W, row0, row1):
    """znear, the whole-band flag and the clamped rectangle of every item."""
    cs = camera_space(lo, hi, xform, xforms, P)
    px, py, front = project(cam, cs)
    whole = (~front).any(1) | np.isnan(px).any(1) | np.isnan(py).any(1)
    zc = cs[..., 2]
    with np.errstate(all="ignore"):
        znear = np.where(np.isnan(zc).any(1), f32(np.nan), np.fmax.reduce(zc, axis=1)).astype(f32)
        ok = ~whole
        sx, sy = np.where(ok[:, None], px, f32(0)), np.where(ok[:, None], py, f32(0))
        x0, x1 = _axis(sx.min(1), sx.max(1), 0, W)
        y0, y1 = _axis(sy.min(1), sy.max(1), row0, row1)
    rect = np.stack([np.where(whole, 0, x0), np.where(whole, W, x1), np.where(whole, row0, y0),
                     np.where(whole, row1, y1)], 1)
    return Boxes(znear, whole, rect)


def pixels_of(bx, zmin, first_tile_row):
    """pixels(i): the sum of area(rect ^ tile) over the tiles with !(znear < zmin)."""
    out = np.zeros(bx.rect.shape[0], np.uint32)
    for i, (x0, x1, y0, y1) in enumerate(bx.rect.tolist()):
        if x0 >= x1 or y0 >= y1:
            continue
        tx = np.arange(x0 // 8, (x1 + 7) // 8)
        ty = np.arange(y0 // 8, (y1 + 7) // 8)
        w = np.minimum(x1, 8 * tx + 8) - np.maximum(x0, 8 * tx)
        h = np.minimum(y1, 8 * ty + 8) - np.maximum(y0, 8 * ty)
        zm = zmin[ty[0] - first_tile_row:ty[-1] + 1 - first_tile_row, tx[0]:tx[-1] + 1]
        with np.errstate(invalid="ignore"):
            passes = ~(bx.znear[i] < zm)  # (equality passes, and so does a NaN znear)
        out[i] = int((np.outer(h, w) * passes).sum())
    return out


def pixels(lo, hi, xform, xforms, P, cam, z, row0):
    """The whole definition on a band z (float32 [rows, W] from frame row row0)."""
    z = np.asarray(z, f32)
    bx = boxes(lo, hi, xform, xforms, P, cam, z.shape[1], row0, row0 + z.shape[0])
    return pixels_of(bx, ztiles(z, row0), row0 // 8)


def aabb(vertices, per, margin):
    """(lo, hi) float32 [n, 3]: the box of every `per` consecutive vertices, widened by `margin` on each side."""
    v = np.asarray(vertices, f32).reshape(-1, per, 3)
    return (v.min(1) - f32(margin)).astype(f32), (v.max(1) + f32(margin)).astype(f32)
