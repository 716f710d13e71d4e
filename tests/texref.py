"""prk_texture_from_target's definition (include/prk.h) in numpy integer
arithmetic: per destination texel and per 8-bit channel of the 0xAARRGGBB word,

    out = (sum of the factor * factor source channel values + factor * factor / 2)
          >> (2 * log2(factor))

factor 1 copies the word.  A plain module: no fixtures, no pytest.
"""
import numpy as np

SHIFT = {1: 0, 2: 2, 4: 4}


def resolve(pixels, factor):
    """uint32 [h, w] (h, w multiples of factor) -> uint32 [h / factor, w / factor]."""
    pixels = np.ascontiguousarray(pixels, np.uint32)
    h, w = pixels.shape
    assert factor in SHIFT and h % factor == 0 and w % factor == 0
    if factor == 1:
        return pixels.copy()
    ch = pixels.view(np.uint8).reshape(h // factor, factor, w // factor, factor, 4).astype(np.uint32)
    out = (ch.sum(axis=(1, 3)) + factor * factor // 2) >> SHIFT[factor]
    assert out.max() <= 255
    return np.ascontiguousarray(out.astype(np.uint8)).view(np.uint32).reshape(h // factor, w // factor)


def from_target(band, row0, rect, factor, texels, dst=(0, 0)):
    """A copy of `texels` (uint32 [rows, columns], any rows and columns past
    the texture's own included) after prk_texture_from_target: band is the
    target's colour, uint32 [row1 - row0, W]; rect = (x0, y0, width, height)
    in frame pixels; dst = (x, y) in texels."""
    x0, y0, w, h = rect
    y = y0 - row0
    assert 0 <= x0 and x0 + w <= band.shape[1] and 0 <= y and y + h <= band.shape[0]
    out = np.array(texels, np.uint32)
    dw, dh = w // factor, h // factor
    assert 0 <= dst[0] and dst[0] + dw <= out.shape[1] and 0 <= dst[1] and dst[1] + dh <= out.shape[0]
    out[dst[1]:dst[1] + dh, dst[0]:dst[0] + dw] = resolve(band[y:y + h, x0:x0 + w], factor)
    return out
