"""The target layers' definition (include/prk.h) in numpy:
saving a rectangle of (colour, z) words, and merging one under a rule.  Every
array is uint32 words [rows, columns]; the rules' comparison runs on float32
views of the z words (IEEE: a NaN on either side loses, -0.0 equals +0.0,
denormals compare by value), and the words move as bits.
"""
import numpy as np

COPY, GREATER, GREATER_EQUAL = 0, 1, 2


def words(a):
    """An array of 4-byte elements as its uint32 words."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32)


def wins(zs, zd, rule):
    """bool per pixel: does the source pixel replace the destination's?"""
    zs, zd = words(zs), words(zd)
    if rule == COPY:
        return np.ones(zs.shape, bool)
    assert rule in (GREATER, GREATER_EQUAL), rule
    with np.errstate(invalid="ignore"):
        s, d = zs.view(np.float32), zd.view(np.float32)
        return s > d if rule == GREATER else s >= d


def _inside(rect, lx, ly, band_shape, row0, layer_shape):
    x0, y0, w, h = rect
    assert w > 0 and h > 0, rect
    assert 0 <= x0 and x0 + w <= band_shape[1] and row0 <= y0 and y0 + h <= row0 + band_shape[0], (rect, row0)
    assert 0 <= lx and lx + w <= layer_shape[1] and 0 <= ly and ly + h <= layer_shape[0], (lx, ly, rect)
    return slice(y0 - row0, y0 - row0 + h), slice(x0, x0 + w), slice(ly, ly + h), slice(lx, lx + w)


def save(band_c, band_z, row0, rect, layer_c, layer_z, dst=(0, 0)):
    """The layer (colour, z) after prk_layer_from_target: the band's pixels
    over rect = (x0, y0, width, height), in frame coordinates (the band holds
    frame rows row0 and up), at the layer's pixel dst = (x, y)."""
    band_c, band_z = words(band_c), words(band_z)
    out_c, out_z = words(layer_c).copy(), words(layer_z).copy()
    by, bx, ly, lx = _inside(rect, dst[0], dst[1], band_c.shape, row0, out_c.shape)
    out_c[ly, lx] = band_c[by, bx]
    out_z[ly, lx] = band_z[by, bx]
    return out_c, out_z


def merge(band_c, band_z, row0, layer_c, layer_z, src_rect, dst, rule):
    """The band (colour, z) after prk_target_from_layer: the layer's pixels
    over src_rect = (src_x, src_y, width, height) into the band at frame pixel
    dst = (x0, y0), where wins() says so."""
    layer_c, layer_z = words(layer_c), words(layer_z)
    out_c, out_z = words(band_c).copy(), words(band_z).copy()
    sx, sy, w, h = src_rect
    by, bx, ly, lx = _inside((dst[0], dst[1], w, h), sx, sy, out_c.shape, row0, layer_c.shape)
    win = wins(layer_z[ly, lx], out_z[by, bx], rule)
    out_c[by, bx] = np.where(win, layer_c[ly, lx], out_c[by, bx])
    out_z[by, bx] = np.where(win, layer_z[ly, lx], out_z[by, bx])
    return out_c, out_z


def merge_frames(first, second, rule):
    """Two whole frames (colour, z) of one size merged: second into first."""
    h, w = words(first[0]).shape
    return merge(first[0], first[1], 0, second[0], second[1], (0, 0, w, h), (0, 0), rule)
