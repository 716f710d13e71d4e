"""GPU tests: prk_layer_alloc / prk_layer_wrap_device / prk_layer_from_target /
prk_target_from_layer / prk_layer_download / prk_layer_info /
prk_layer_destroy -- a drawn (colour, z) frame saved on the device, put back,
and merged into another by depth (include/prk.h).

Expected words come from tests/layerref.py, the header's definition in numpy,
and from the oracle; colour and z are both compared as uint32, every word.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import layerref
import oracle as O
import prk
from prk import abi
from test_target_layers_abi import CONTROL, PAIRS, SPLIT, split_scene

pytestmark = pytest.mark.gpu

W, H = 72, 40    # the target; W % 8 == 0; rows of 288 bytes: 32-byte aligned, not 64
LW, LH = 48, 24  # the layer
RULES = (abi.PRK_MERGE_COPY, abi.PRK_MERGE_GREATER, abi.PRK_MERGE_GREATER_EQUAL)
CLEAR_C = np.uint32(0xFF000000)
CLEAR_Z = np.array([-np.finfo(np.float32).max], np.float32).view(np.uint32)[0]


def f32_words(*values):
    return np.array(values, np.float32).view(np.uint32)


# every class of z word: NaN with sign 0, with sign 1, a NaN payload, +-0, +-the smallest denormal, +-FLT_MIN,
# +-1, nextafter(1), +-FLT_MAX, +-inf
Z_CLASSES = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                      0x00800000, 0x80800000, 0x3F800000, 0xBF800000, 0x3F800001, 0x7F7FFFFF, 0xFF7FFFFF,
                      0x7F800000, 0xFF800000], np.uint32)
# a small pool for the random planes: ties and losses are frequent
Z_POOL = f32_words(-1.0, -0.0, 0.0, 0.25, 0.5, 1.0)


def words(rng, shape):
    return rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32)


def pooled(rng, shape, pool=Z_POOL):
    return pool[rng.integers(0, len(pool), shape)]


def same_words(got, want, label):
    got, want = layerref.words(got), layerref.words(want)
    assert got.shape == want.shape, "%s: shape %r, expected %r" % (label, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d words differ, first at (x, y) = (%d, %d): %08x, expected %08x" % (
        label, bad.sum(), np.nonzero(bad)[1][0], np.nonzero(bad)[0][0], got[bad][0], want[bad][0])


def same_pixels(got, want, label):
    same_words(got[0], want[0], label + ": colour")
    same_words(got[1], want[1], label + ": z")


def upload(r, c, z):
    r.upload(c, layerref.words(z).view(np.float32))


def fill_layer(r, layer, c, z):
    """Give a library-owned layer the pixels (c, z) through the target: upload
    them, save them.  The target must be at least as large as the layer."""
    h, w = c.shape
    rows = r.row1 - r.row0
    tc, tz = np.zeros((rows, r.width), np.uint32), np.zeros((rows, r.width), np.uint32)
    tc[:h, :w], tz[:h, :w] = c, layerref.words(z)
    upload(r, tc, tz)
    r.layer_from_target(layer, (0, r.row0, w, h))
    same_pixels(r.layer_download(layer), (c, z), "the layer as filled")


@pytest.fixture(scope="module")
def planes(gpu):
    """A 72 x 40 target of random colour words whose z comes from a small
    pool, and a 48 x 24 layer built likewise."""
    rng = np.random.default_rng(31)
    tc, tz = words(rng, (H, W)), pooled(rng, (H, W))
    lc, lz = words(rng, (LH, LW)), pooled(rng, (LH, LW))
    r = prk.Renderer()
    r.target_alloc(W, H)
    layer = r.layer_alloc(LW, LH)
    fill_layer(r, layer, lc, lz)
    upload(r, tc, tz)
    yield r, (tc, tz), layer, (lc, lz)
    r.close()


# ---- 1. rectangles, per rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_merge_rectangles_word_for_word(planes, rule):
    r, target, layer, lay = planes
    n = won = lost = 0
    for w in (1, 2, 3, 4, 5, 15, 16, 17):
        for x0 in (0, 1, 3):
            for src_x in (0, 1, 2, 3):
                for src_y in (0, 7):
                    y0 = n % 5
                    upload(r, *target)
                    r.target_from_layer(layer, (src_x, src_y, w, 5), (x0, y0), rule)
                    want = layerref.merge(target[0], target[1], 0, lay[0], lay[1], (src_x, src_y, w, 5), (x0, y0), rule)
                    label = "rule %d rect %r to %r" % (rule, (src_x, src_y, w, 5), (x0, y0))
                    same_pixels(r.download(), want, label)
                    same_pixels(r.layer_download(layer), lay, label + ": the layer")
                    changed = int((want[1] != target[1]).sum() + (want[0] != target[0]).sum())
                    won += changed > 0
                    lost += changed < 2 * 5 * w
                    n += 1
    assert n == 192 and won > 150 and (rule == abi.PRK_MERGE_COPY or lost > 150)
    upload(r, *target)


def test_save_rectangles_word_for_word(planes):
    r, target, _, _ = planes
    layer = r.layer_alloc(LW, LH)
    want = (np.zeros((LH, LW), np.uint32), np.full((LH, LW), CLEAR_Z, np.uint32))
    same_pixels(r.layer_download(layer), want, "a fresh layer")
    n = 0
    for w in (1, 2, 3, 4, 5, 15, 16, 17):
        for x0 in (0, 1, 3):
            for dst_x in (0, 1, 2, 3):
                for dst_y in (0, 7):
                    rect = (x0, n % 5, w, 5)
                    r.layer_from_target(layer, rect, (dst_x, dst_y))
                    want = layerref.save(target[0], target[1], 0, rect, want[0], want[1], (dst_x, dst_y))
                    same_pixels(r.layer_download(layer), want, "rect %r to %r" % (rect, (dst_x, dst_y)))
                    n += 1
    assert n == 192
    same_pixels(r.download(), target, "the target after the saves")
    r.layer_destroy(layer)


# ---- 2. every z class against every other ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_every_z_class_against_every_other(gpu, rule):
    rng = np.random.default_rng(32)
    n = len(Z_CLASSES)
    assert n == 16
    tz = np.tile(Z_CLASSES[None, :], (n, 1))  # the target's z: a class a column
    lz = np.tile(Z_CLASSES[:, None], (1, n))  # the layer's: a class a row
    tc, lc = words(rng, (n, n)), words(rng, (n, n))
    r = prk.Renderer()
    try:
        r.target_alloc(n, n)
        layer = r.layer_alloc(n, n)
        fill_layer(r, layer, lc, lz)
        upload(r, tc, tz)
        r.target_from_layer(layer, rule=rule)
        want = layerref.merge_frames((tc, tz), (lc, lz), rule)
        same_pixels(r.download(), want, "rule %d" % rule)
        win = want[0] == lc
        if rule != abi.PRK_MERGE_COPY:  # a NaN on either side loses; the zeros tie; a denormal is above zero
            assert not win[:3].any() and not win[:, :3].any()
            assert win[3, 4] == win[4, 3] == (rule == abi.PRK_MERGE_GREATER_EQUAL)
            assert win[5, 3] and win[5, 4] and not win[6, 3] and win[3, 6] and win[11, 9] and not win[9, 11]
            assert win.sum() == (13 * 12 // 2 - 1 if rule == abi.PRK_MERGE_GREATER else 13 * 12 // 2 + 13 + 1)
    finally:
        r.close()


# ---- 3. more than one quad a lane, more than one workgroup a row ---------------------------------------------------------
@pytest.mark.parametrize("width", [260, 1028])
def test_long_rows_one_word_into_a_line(gpu, width):
    """Rows that start one word into a 16-byte line: 260 pixels are 66 quads
    (a lane's second quad), 1028 pixels 258 quads (a second workgroup)."""
    rng = np.random.default_rng(33)
    tw, th = 1032, 6
    tc, tz = words(rng, (th, tw)), pooled(rng, (th, tw))
    lc, lz = words(rng, (th, width + 3)), pooled(rng, (th, width + 3))
    r = prk.Renderer()
    try:
        r.target_alloc(tw, th)
        layer = r.layer_alloc(width + 3, th)
        fill_layer(r, layer, lc, lz)
        for rule in RULES:
            upload(r, tc, tz)
            r.target_from_layer(layer, (2, 0, width, th), (1, 0), rule)
            want = layerref.merge(tc, tz, 0, lc, lz, (2, 0, width, th), (1, 0), rule)
            same_pixels(r.download(), want, "%d pixels at x0 1, rule %d" % (width, rule))
        upload(r, tc, tz)
        r.layer_from_target(layer, (3, 1, width, th - 1), (1, 0))
        want = layerref.save(tc, tz, 0, (3, 1, width, th - 1), lc, lz, (1, 0))
        same_pixels(r.layer_download(layer), want, "%d pixels saved to dst_x 1" % width)
    finally:
        r.close()


# ---- 4. wrapped and caller-bound memory at 4-byte alignment ---------------------------------------------------------------
def test_wrapped_source_and_caller_bound_target_unaligned(gpu):
    import torch

    rng = np.random.default_rng(34)
    dev = torch.device("cuda:0")
    pitch = 4 * W + 4
    tc, tz = words(rng, (H, W)), pooled(rng, (H, W))
    lc, lz = words(rng, (H, W)), pooled(rng, (H, W))

    def color_buffer(c):
        """4 bytes in front, H rows of `pitch` bytes, 0xAB in every byte that is not a pixel's."""
        host = np.full(4 + H * pitch, 0xAB, np.uint8)
        rows = host[4:].reshape(H, pitch)
        rows[:, :4 * W] = c.view(np.uint8).reshape(H, 4 * W)
        return host, torch.from_numpy(host.copy()).to(dev)

    def z_buffer(z):
        """4 bytes in front and 12 behind, 0xAB."""
        host = np.full(4 + 4 * H * W + 12, 0xAB, np.uint8)
        host[4:4 + 4 * H * W] = layerref.words(z).view(np.uint8).reshape(-1)
        return host, torch.from_numpy(host.copy()).to(dev)

    (tch, tcd), (tzh, tzd) = color_buffer(tc), z_buffer(tz)
    (_, lcd), (_, lzd) = color_buffer(lc), z_buffer(lz)
    assert tcd.data_ptr() % 16 == 0 and tzd.data_ptr() % 16 == 0 and lcd.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    r = prk.Renderer()
    try:
        r.target_bind(tcd.data_ptr() + 4, pitch, tzd.data_ptr() + 4, W, H)
        layer = r.layer_wrap(lcd.data_ptr() + 4, pitch, lzd.data_ptr() + 4, W, H)
        assert r.layer_info(layer) == (W, H, pitch, True)
        same_pixels(r.layer_download(layer), (lc, lz), "the wrapped layer")
        own = r.layer_alloc(LW, LH)
        want = (tc, tz)
        saved = r.layer_download(own)
        for rule, rect, dst in ((abi.PRK_MERGE_GREATER, (0, 0, W, H), (0, 0)), (abi.PRK_MERGE_COPY, (1, 3, 17, 7), (3, 2)),
                                (abi.PRK_MERGE_GREATER_EQUAL, (3, 1, 34, 14), (1, 5)),
                                (abi.PRK_MERGE_GREATER, (2, 2, 64, 16), (5, 0)), (abi.PRK_MERGE_COPY, (55, 39, 17, 1), (7, 11)),
                                (abi.PRK_MERGE_GREATER_EQUAL, (0, 0, W, H), (0, 0))):
            r.target_from_layer(layer, rect, dst, rule)
            want = layerref.merge(want[0], want[1], 0, lc, lz, rect, dst, rule)
            same_pixels(r.download(), want, "rule %d rect %r to %r" % (rule, rect, dst))
            # ... and the unaligned target as a save's source
            r.layer_from_target(own, (dst[0], dst[1], min(rect[2], LW - 1), min(rect[3], LH)), (1, 0))
            saved = layerref.save(want[0], want[1], 0, (dst[0], dst[1], min(rect[2], LW - 1), min(rect[3], LH)),
                                  saved[0], saved[1], (1, 0))
            same_pixels(r.layer_download(own), saved, "saved from the bound target at %r" % (dst,))
        same_pixels(r.layer_download(layer), (lc, lz), "the wrapped layer after the calls")
        # a wrapped layer is read-only
        assert r._L.prk_layer_from_target(r._h, layer, 0, 0, 4, 4, 0, 0) == abi.PRK_ERR_ARG
        r.synchronize()
    finally:
        r.close()
    # every byte that is no pixel of the target: untouched
    got_c, got_z = tcd.cpu().numpy(), tzd.cpu().numpy()
    assert (got_c[:4] == 0xAB).all() and (got_c[4:].reshape(H, pitch)[:, 4 * W:] == 0xAB).all()
    assert (got_z[:4] == 0xAB).all() and (got_z[4 + 4 * H * W:] == 0xAB).all()
    same_words(got_c[4:].reshape(H, pitch)[:, :4 * W].copy().view(np.uint32), want[0], "the bound colour memory")


# ---- frames ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return split_scene()


@pytest.fixture(scope="module")
def oracle_frames(scene):
    """(semantics, phong, per) -> the oracle's whole frame, its first draws' frame and the rest's, (colour, z)
    each; computed once."""
    out = {}
    for sem, phong, _ in PAIRS + [CONTROL]:
        for per in (1, 7):
            if (sem, phong, per) in out:
                continue
            kw = dict(semantics=sem, phong=phong, tris_per_object=per, winners=False)
            out[sem, phong, per] = tuple(O.render(s, **kw)[:2] for s in (
                scene, scene.subset(0, SPLIT), scene.subset(SPLIT, scene.tri_count)))
    return out


class Ctx:
    """A renderer with the scene's target, camera, geometry and texture."""

    def __init__(self, s, rows=None):
        self.s = s
        self.r = r = prk.Renderer()
        r.target_alloc(s.width, s.height, *(rows or (0, s.height)))
        r.clear()
        r.set_camera(s.prk_transform(), s.prk_lights())
        self.g = r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        self.t = r.texture(s.texture)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.close()

    def draw(self, t0, t1, sem=abi.PRK_SEM_AVX, phong=True, per=1, P=None):
        self.r.draw(sem, self.g, t1 - t0, first_tri=t0, P=self.s.P if P is None else P, bitmap=self.t, phong=phong,
                    tris_per_object=per)


# ---- 5. a frame split over two layers, one context -------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 7])
@pytest.mark.parametrize("sem,phong,rule", PAIRS + [CONTROL])
def test_split_frame_one_context(gpu, scene, oracle_frames, sem, phong, rule, per):
    whole, first, second = oracle_frames[sem, phong, per]
    with Ctx(scene) as f:
        r = f.r
        a, b = r.layer_alloc(W, H), r.layer_alloc(W, H)
        f.draw(0, SPLIT, sem, phong, per)
        r.complete_all_work()
        r.layer_from_target(a)
        r.clear()
        f.draw(SPLIT, scene.tri_count, sem, phong, per)
        r.complete_all_work()
        r.layer_from_target(b)
        r.target_from_layer(a)                # restore the first
        r.target_from_layer(b, rule=rule)     # merge the second
        got = r.download()                    # (the first call that waits)
        same_pixels(r.layer_download(a), first, "the first draws' layer against the oracle")
        same_pixels(r.layer_download(b), second, "the other draws' layer against the oracle")
    same_pixels(got, layerref.merge_frames(first, second, rule), "the merged frame against the definition")
    if (sem, phong, rule) == CONTROL:  # the other tie rule: the later draw's colour where the halves tie
        assert (got[0] != whole[0]).sum() > 100 and (got[1] == whole[1]).all()
    else:
        same_pixels(got, whole, "the merged frame against the oracle's frame of all the draws")


# ---- 6. ... and over two contexts of one device ----------------------------------------------------------------------------
@pytest.mark.parametrize("sem,phong,rule", [PAIRS[0], PAIRS[3]])
def test_split_frame_two_contexts(gpu, scene, oracle_frames, sem, phong, rule):
    whole = oracle_frames[sem, phong, 1][0]
    with Ctx(scene) as fa, Ctx(scene) as fb:
        fb.draw(SPLIT, scene.tri_count, sem, phong)
        fb.r.complete_all_work()
        fa.draw(0, SPLIT, sem, phong)
        fa.r.complete_all_work()
        fb.r.synchronize()
        color, pitch, z = fb.r.target()[:3]
        layer = fa.r.layer_wrap(color, pitch, z, W, H)
        fa.r.target_from_layer(layer, rule=rule)
        got = fa.r.download()
        fa.r.layer_destroy(layer)  # (before B frees its target)
    same_pixels(got, whole, "A's draws merged with B's target")


# ---- 7. restore, then draw ---------------------------------------------------------------------------------------------------
def test_restore_then_draw(gpu, scene, oracle_frames):
    static = oracle_frames[abi.PRK_SEM_AVX, True, 1][1]
    t0, t1 = SPLIT, 300
    with Ctx(scene) as f:
        r = f.r
        f.draw(0, SPLIT)
        r.complete_all_work()
        layer = r.layer_alloc(W, H)
        r.layer_from_target(layer)
        frames = []
        for k in range(3):
            P = (0.2 * k - 0.1, 0.05 * k, 0.02 * k)
            r.target_from_layer(layer)
            f.draw(t0, t1, P=P)
            r.complete_all_work()
            frames.append((P, r.download()))
    for P, got in frames:
        moving = dataclasses.replace(scene.subset(t0, t1), P=P)
        want = O.render(moving, semantics=abi.PRK_SEM_AVX, phong=True, color=static[0], z=static[1], winners=False)[:2]
        assert (want[0] != static[0]).sum() > 200
        same_pixels(got, want, "the moving draws at P = %r over the restored frame" % (P,))
    assert (frames[0][1][0] != frames[2][1][0]).sum() > 100


# ---- 8. ordering without host waits ----------------------------------------------------------------------------------------
def test_ordering(gpu, scene, oracle_frames):
    whole, first, second = oracle_frames[abi.PRK_SEM_AVX, True, 1]
    clear = (np.full((H, W), CLEAR_C, np.uint32), np.full((H, W), CLEAR_Z, np.uint32))
    T = scene.tri_count
    with Ctx(scene) as f:
        r = f.r
        f.draw(0, SPLIT)
        r.complete_all_work()
        layer = r.layer_alloc(W, H)
        r.layer_from_target(layer)
        # a merge queued between recording a draw and its flush: the draw lands on top of it
        r.clear()
        f.draw(SPLIT, T)
        r.target_from_layer(layer)
        r.complete_all_work()
        same_pixels(r.download(), whole, "a restore between a draw and its flush")
        # a merge right after a flush with early z: the downloaded z is the merged one
        r.set_early_z(True)
        r.clear()
        f.draw(SPLIT, T)
        r.complete_all_work()
        r.target_from_layer(layer, rule=abi.PRK_MERGE_GREATER_EQUAL)  # (the layer holds the EARLIER draws: it wins ties)
        same_pixels(r.download(), whole, "a merge after an early-z flush")
        assert (layerref.words(second[1]) != layerref.words(whole[1])).sum() > 200
        r.set_early_z(False)
        # a pending clear_on_flush discards a restore, as it discards an upload
        r.clear_on_flush()
        r.target_from_layer(layer)
        f.draw(SPLIT, T)
        r.complete_all_work()
        same_pixels(r.download(), second, "a restore under a pending clear")
        r.clear_on_flush()
        r.target_from_layer(layer)
        r.complete_all_work()
        same_pixels(r.download(), clear, "a restore under a pending clear, nothing drawn")
        # a clear after a queued restore lands after it
        r.target_from_layer(layer)
        r.clear()
        same_pixels(r.download(), clear, "a clear after a restore")
        # ... and a save after a queued restore reads it
        other = r.layer_alloc(W, H)
        r.target_from_layer(layer)
        r.layer_from_target(other)
        same_pixels(r.layer_download(other), first, "a save after a restore")


# ---- 9. a band context -------------------------------------------------------------------------------------------------------
def test_band_context(gpu):
    rng = np.random.default_rng(35)
    row0 = 8
    bc, bz = words(rng, (H - row0, W)), pooled(rng, (H - row0, W))
    lc, lz = words(rng, (LH, LW)), pooled(rng, (LH, LW))
    r = prk.Renderer()
    try:
        r.target_alloc(W, H, row0, H)
        layer, other = r.layer_alloc(LW, LH), r.layer_alloc(LW, LH)
        fill_layer(r, layer, lc, lz)
        upload(r, bc, bz)
        want = (bc, bz)
        for rule, rect, dst in ((abi.PRK_MERGE_GREATER, (0, 0, LW, LH), (3, 8)), (abi.PRK_MERGE_COPY, (5, 2, 9, 3), (60, 37)),
                                (abi.PRK_MERGE_GREATER_EQUAL, (1, 0, 20, 24), (0, 16))):
            r.target_from_layer(layer, rect, dst, rule)
            want = layerref.merge(want[0], want[1], row0, lc, lz, rect, dst, rule)
            same_pixels(r.download(), want, "band: rule %d rect %r to %r" % (rule, rect, dst))
        saved = r.layer_download(other)
        for rect, dst in (((0, 8, LW, LH), (0, 0)), ((71, 39, 1, 1), (47, 23)), ((7, 9, 13, 5), (2, 3))):
            r.layer_from_target(other, rect, dst)
            saved = layerref.save(want[0], want[1], row0, rect, saved[0], saved[1], dst)
            same_pixels(r.layer_download(other), saved, "band: save %r to %r" % (rect, dst))
        L, h = r._L, r._h
        for y0, hh in ((7, 4), (7, 1), (0, 4), (38, 3), (40, 1)):  # across row0, above it, past the last row
            assert L.prk_target_from_layer(h, layer, 0, 0, 4, hh, 0, y0, abi.PRK_MERGE_COPY) == abi.PRK_ERR_ARG, (y0, hh)
            assert L.prk_layer_from_target(h, other, 0, y0, 4, hh, 0, 0) == abi.PRK_ERR_ARG, (y0, hh)
        same_pixels(r.download(), want, "band: the target after the refused calls")
        same_pixels(r.layer_download(other), saved, "band: the layer after the refused calls")
        # rect=None: the whole band, the whole layer at the band's first pixel
        band_layer = r.layer_alloc(W, H - row0)
        r.layer_from_target(band_layer)
        same_pixels(r.layer_download(band_layer), want, "band: the whole band saved")
        r.target_from_layer(layer)
        want = layerref.merge(want[0], want[1], row0, lc, lz, (0, 0, LW, LH), (0, row0), abi.PRK_MERGE_COPY)
        same_pixels(r.download(), want, "band: the whole layer restored")
    finally:
        r.close()


# ---- 10. refused calls -------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(planes):
    r, target, layer, lay = planes
    L, h = r._L, r._h
    merge, save = L.prk_target_from_layer, L.prk_layer_from_target
    big = 2**31 - 1
    dead = r.layer_alloc(4, 4)
    r.layer_destroy(dead)
    cases = [
        ("merge: null context", lambda: merge(None, layer, 0, 0, 4, 4, 0, 0, 0)),
        ("merge: layer < 0", lambda: merge(h, -1, 0, 0, 4, 4, 0, 0, 0)),
        ("merge: layer past the handles", lambda: merge(h, 999, 0, 0, 4, 4, 0, 0, 0)),
        ("merge: a destroyed layer", lambda: merge(h, dead, 0, 0, 4, 4, 0, 0, 0)),
        ("merge: rule 3", lambda: merge(h, layer, 0, 0, 4, 4, 0, 0, 3)),
        ("merge: rule -1", lambda: merge(h, layer, 0, 0, 4, 4, 0, 0, -1)),
        ("merge: width 0", lambda: merge(h, layer, 0, 0, 0, 4, 0, 0, 0)),
        ("merge: height 0", lambda: merge(h, layer, 0, 0, 4, 0, 0, 0, 1)),
        ("merge: width < 0", lambda: merge(h, layer, 0, 0, -4, 4, 0, 0, 0)),
        ("merge: height < 0", lambda: merge(h, layer, 0, 0, 4, -4, 0, 0, 2)),
        ("merge: src_x < 0", lambda: merge(h, layer, -1, 0, 4, 4, 0, 0, 0)),
        ("merge: src_y < 0", lambda: merge(h, layer, 0, -1, 4, 4, 0, 0, 0)),
        ("merge: source past the layer's width", lambda: merge(h, layer, LW - 3, 0, 4, 4, 0, 0, 0)),
        ("merge: source past the layer's height", lambda: merge(h, layer, 0, LH - 3, 4, 4, 0, 0, 0)),
        ("merge: src_x + width past int32", lambda: merge(h, layer, big, 0, 4, 4, 0, 0, 0)),
        ("merge: x0 < 0", lambda: merge(h, layer, 0, 0, 4, 4, -1, 0, 0)),
        ("merge: y0 < 0", lambda: merge(h, layer, 0, 0, 4, 4, 0, -1, 0)),
        ("merge: past the target's right edge", lambda: merge(h, layer, 0, 0, 4, 4, W - 3, 0, 0)),
        ("merge: past the target's last row", lambda: merge(h, layer, 0, 0, 4, 4, 0, H - 3, 0)),
        ("merge: x0 + width past int32", lambda: merge(h, layer, 0, 0, 4, 4, big, 0, 0)),
        ("merge: y0 + height past int32", lambda: merge(h, layer, 0, 0, 4, 4, 0, big, 0)),
        ("save: null context", lambda: save(None, layer, 0, 0, 4, 4, 0, 0)),
        ("save: layer < 0", lambda: save(h, -1, 0, 0, 4, 4, 0, 0)),
        ("save: layer past the handles", lambda: save(h, 999, 0, 0, 4, 4, 0, 0)),
        ("save: a destroyed layer", lambda: save(h, dead, 0, 0, 4, 4, 0, 0)),
        ("save: width 0", lambda: save(h, layer, 0, 0, 0, 4, 0, 0)),
        ("save: height < 0", lambda: save(h, layer, 0, 0, 4, -1, 0, 0)),
        ("save: x0 < 0", lambda: save(h, layer, -1, 0, 4, 4, 0, 0)),
        ("save: past the target's right edge", lambda: save(h, layer, W - 3, 0, 4, 4, 0, 0)),
        ("save: past the target's last row", lambda: save(h, layer, 0, H - 3, 4, 4, 0, 0)),
        ("save: y0 + height past int32", lambda: save(h, layer, 0, 4, 4, big - 3, 0, 0)),
        ("save: dst_x < 0", lambda: save(h, layer, 0, 0, 4, 4, -1, 0)),
        ("save: dst_y < 0", lambda: save(h, layer, 0, 0, 4, 4, 0, -1)),
        ("save: past the layer's width", lambda: save(h, layer, 0, 0, 4, 4, LW - 3, 0)),
        ("save: past the layer's height", lambda: save(h, layer, 0, 0, 4, 4, 0, LH - 3)),
        ("save: dst_x + width past int32", lambda: save(h, layer, 0, 0, 4, 4, big, 0)),
    ]
    for label, bad in cases:
        assert bad() == abi.PRK_ERR_ARG, label
        same_pixels(r.download(), target, "the target after the refused call: " + label)
        same_pixels(r.layer_download(layer), lay, "the layer after the refused call: " + label)
    # no target bound
    r2 = prk.Renderer()
    try:
        l2 = r2.layer_alloc(8, 8)
        fresh = r2.layer_download(l2)
        assert r2._L.prk_layer_from_target(r2._h, l2, 0, 0, 4, 4, 0, 0) == abi.PRK_ERR_NO_TARGET
        assert r2._L.prk_target_from_layer(r2._h, l2, 0, 0, 4, 4, 0, 0, 0) == abi.PRK_ERR_NO_TARGET
        assert r2._L.prk_target_from_layer(r2._h, l2, 0, 0, 4, 4, 0, 0, 7) == abi.PRK_ERR_ARG
        same_pixels(r2.layer_download(l2), fresh, "the layer of a context without a target")
    finally:
        r2.close()
    # the other calls' arguments
    n = C.c_int32(-1)
    out_c, out_z = np.zeros((LH, LW), np.uint32), np.zeros((LH, LW), np.float32)
    pc, pz = out_c.ctypes.data, out_z.ctypes.data
    for w_, h_ in ((0, 4), (4, 0), (-1, 4), (4, -1), (2**29, 1)):
        assert L.prk_layer_alloc(h, w_, h_, C.byref(n)) == abi.PRK_ERR_ARG and n.value == -1, (w_, h_)
    assert L.prk_layer_alloc(h, 4, 4, None) == abi.PRK_ERR_ARG
    color, pitch, z = r.target()[:3]
    for args in ((None, pitch, z, W, H), (color, pitch, None, W, H), (color, 4 * W - 4, z, W, H), (color, 4 * W + 2, z, W, H),
                 (color + 2, pitch, z, W, H), (color, pitch, z + 1, W, H), (color, pitch, z, 0, H), (color, pitch, z, W, -1)):
        assert L.prk_layer_wrap_device(h, *args, C.byref(n)) == abi.PRK_ERR_ARG and n.value == -1, args
    assert L.prk_layer_wrap_device(h, color, pitch, z, W, H, None) == abi.PRK_ERR_ARG
    assert L.prk_layer_download(h, layer, pc, 4 * LW - 4, pz) == abi.PRK_ERR_ARG
    assert L.prk_layer_download(h, layer, pc, 4 * LW + 2, pz) == abi.PRK_ERR_ARG
    assert L.prk_layer_download(h, 999, pc, 4 * LW, pz) == abi.PRK_ERR_ARG and not out_c.any() and not out_z.any()
    assert L.prk_layer_info(h, -1, C.byref(n), None, None, None) == abi.PRK_ERR_ARG and n.value == -1
    assert L.prk_layer_destroy(h, 999) == abi.PRK_ERR_ARG and L.prk_layer_destroy(h, -1) == abi.PRK_ERR_ARG


# ---- 11. info, download, destroy ----------------------------------------------------------------------------------------------
def test_info_download_and_destroy(planes):
    r, target, layer, lay = planes
    L, h = r._L, r._h
    assert r.layer_info(layer) == (LW, LH, 4 * LW, False)
    a = r.layer_alloc(33, 7)
    assert a != layer and r.layer_info(a) == (33, 7, 132, False)
    w = C.c_int32(0)
    assert L.prk_layer_info(h, a, None, None, None, None) == abi.PRK_OK
    assert L.prk_layer_info(h, a, C.byref(w), None, None, None) == abi.PRK_OK and w.value == 33
    # either host pointer may be NULL; a wider host pitch leaves the bytes between the rows alone
    r.layer_from_target(a, (2, 1, 33, 7))
    out_c, out_z = np.full((7, 40), 0xABABABAB, np.uint32), np.zeros((7, 33), np.uint32)
    assert L.prk_layer_download(h, a, out_c.ctypes.data, 160, None) == abi.PRK_OK
    assert L.prk_layer_download(h, a, None, 0, out_z.ctypes.data) == abi.PRK_OK
    assert L.prk_layer_download(h, a, None, 0, None) == abi.PRK_OK
    assert (out_c[:, 33:] == 0xABABABAB).all()
    same_pixels((out_c[:, :33], out_z), (target[0][1:8, 2:35], target[1][1:8, 2:35]), "download at a wider pitch")
    # destroy, then use
    r.layer_destroy(a)
    n = C.c_int32(-1)
    assert L.prk_layer_destroy(h, a) == abi.PRK_ERR_ARG
    assert L.prk_layer_info(h, a, C.byref(n), None, None, None) == abi.PRK_ERR_ARG and n.value == -1
    assert L.prk_layer_from_target(h, a, 0, 0, 4, 4, 0, 0) == abi.PRK_ERR_ARG
    assert L.prk_target_from_layer(h, a, 0, 0, 4, 4, 0, 0, abi.PRK_MERGE_COPY) == abi.PRK_ERR_ARG
    assert L.prk_layer_download(h, a, out_c.ctypes.data, 160, None) == abi.PRK_ERR_ARG
    b = r.layer_alloc(5, 5)
    assert b > a and r.layer_info(b) == (5, 5, 20, False)  # (the slot stays dead)
    same_pixels(r.download(), target, "the target")
    same_pixels(r.layer_download(layer), lay, "the layer")
