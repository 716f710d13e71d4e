"""prk_geometry_select (include/prk.h), written from the definition in numpy:
the pixel count of every item, the first of its levels that the count passes,
the packed starts, and what the call leaves in the destination geometry.
Transforms go through tests/xform_ref.py (prk_geometry_transform's arithmetic
op by op), frame counts through tests/visref.py.  The table shapes the GPU
tests feed prk_selftest_select live here too.
"""
import collections

import numpy as np

import visref
import xform_ref as X

Sel = collections.namedtuple("Sel", "pixels chosen n out_first total")

VERTEX_LIMIT = 0xFFFFFFF0  # prk_geometry_write's
GUARD_WORD = 0xA5A5A5A5    # prk_selftest_select's destination before the emit pass


class Refused(Exception):
    """The call's status for these arguments: 'ARG' or 'LIMIT'."""

    def __init__(self, status, why):
        Exception.__init__(self, "%s: %s" % (status, why))
        self.status = status


def tables(items, levels):
    it = np.asarray(items, np.int64).reshape(-1, 5)
    lv = np.zeros((0, 3), np.int64) if levels is None else np.asarray(levels, np.int64).reshape(-1, 3)
    return it, lv


def pixels_of(items, pix_prefix=None, item_pixels=None):
    """pixels(i): item_pixels[i], or the sum of the frame's counts over the item's ids."""
    it = np.asarray(items, np.int64).reshape(-1, 5)
    if item_pixels is not None:
        px = np.asarray(item_pixels, np.int64).reshape(-1)
        assert px.shape[0] == it.shape[0]
        return px
    pp = np.asarray(pix_prefix, np.int64).reshape(-1)
    return pp[it[:, 0] + it[:, 1]] - pp[it[:, 0]]


def choose(items, levels, pixels, dst_first_tri=0):
    """The definition, an item at a time: the first level that passes wins."""
    it, lv = tables(items, levels)
    chosen = np.full(it.shape[0], -1, np.int32)
    n = np.zeros(it.shape[0], np.int64)
    for i, (_, _, l0, ln, _) in enumerate(it.tolist()):
        for l in range(ln):
            if pixels[i] >= lv[l0 + l, 0]:
                chosen[i] = l
                n[i] = lv[l0 + l, 2]
                break
    first = dst_first_tri + np.concatenate([[0], np.cumsum(n)])
    return Sel(np.asarray(pixels, np.int64), chosen, n, first.astype(np.uint32), int(n.sum()))


def check(items, levels, xform_count, src_tris, dst_first_tri, frame_ids=None, have_levels=True, have_xforms=True):
    """The call's argument errors (Refused), decided from the tables and worst
    cases alone; returns the worst-case total.  frame_ids: the frame's id
    count when the counts are the frame's, None with item_pixels."""
    it, lv = tables(items, levels)
    worst = 0
    for f_id, n_id, l0, ln, xf in it.tolist():
        if l0 + ln > lv.shape[0]:
            raise Refused("ARG", "levels past the table")
        if frame_ids is not None and f_id + n_id > frame_ids:
            raise Refused("ARG", "ids past the frame's")
        if ln == 0:
            continue
        if not have_levels or not have_xforms:
            raise Refused("ARG", "a NULL table an item needs")
        if xf >= xform_count:
            raise Refused("ARG", "xform past the table")
        live = lv[l0:l0 + ln]
        live = live[live[:, 2] > 0]
        if live.size and int((live[:, 1] + live[:, 2]).max()) > src_tris:
            raise Refused("ARG", "a level past the end of src")
        worst += int(live[:, 2].max()) if live.size else 0
    if worst > 2**31:
        raise Refused("LIMIT", "worst-case total above 2^31")
    if 3 * (dst_first_tri + worst) > VERTEX_LIMIT:
        raise Refused("ARG", "worst-case end past the vertex limit")
    return worst


def runs_of(items, levels, sel):
    """The chosen triangles as prk_geometry_transform runs (src_first_tri,
    tri_count, dst_first_tri, xform): the host route the call replaces."""
    it, lv = tables(items, levels)
    keep = np.flatnonzero(sel.n > 0)
    lev = it[keep, 2] + sel.chosen[keep]
    return np.stack([lv[lev, 1], sel.n[keep], sel.out_first[keep].astype(np.int64), it[keep, 4]], 1).astype(np.uint32)


def emit(items, levels, xforms, src, dst, sel):
    """What the call leaves in dst (4-tuples of arrays or None, as
    xform_ref.apply_runs): a call that chooses nothing leaves dst as it was."""
    if sel.total == 0:
        return tuple(None if a is None else a.copy() for a in dst)
    return X.apply_runs(src, dst, runs_of(items, levels, sel), np.asarray(xforms, np.float32).reshape(-1, 3, 4))


def emit_selftest(items, levels, xforms, src, dst_tris, sel):
    """prk_selftest_select's destination as uint32 words: dst_tris triangles of
    every array src has, the guard word wherever no triangle was written."""
    out = []
    for a, comp in zip(src, X.COMP):
        out.append(None if a is None else np.full((3 * dst_tris, comp), GUARD_WORD, np.uint32).view(np.float32))
    got = emit(items, levels, xforms, src, tuple(out), sel)
    return tuple(None if a is None else a.view(np.uint32) for a in got)


def frame_counts(winners, id_count):
    """(counts, pix_prefix) of a winner map: tests/visref.py's reduction."""
    v = visref.reduce(winners, id_count)
    return v.counts, v.pix_prefix


# ---- tables for the self-test -------------------------------------------------------------------
def one_level_items(tri_counts, drawn, xforms=1, min_pixels=1):
    """An item a source mesh, meshes back to back in src: item i has
    tri_counts[i] triangles and one level of `min_pixels`; its count is
    min_pixels where drawn[i], min_pixels - 1 where not.  Returns (items,
    levels, item_pixels, src_tris)."""
    tc = np.asarray(tri_counts, np.int64)
    n = tc.shape[0]
    s0 = np.concatenate([[0], np.cumsum(tc)])
    items = np.stack([np.zeros(n), np.zeros(n), np.arange(n), np.ones(n), np.arange(n) % xforms], 1).astype(np.uint32)
    levels = np.stack([np.full(n, min_pixels), s0[:-1], tc], 1).astype(np.uint32)
    px = np.where(np.asarray(drawn, bool), min_pixels, min_pixels - 1).astype(np.uint32)
    return items, levels, px, int(s0[-1])
