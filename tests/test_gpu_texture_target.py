"""GPU tests: prk_texture_alloc / prk_texture_from_target /
prk_texture_download / prk_texture_info -- a rectangle of the bound target's
colour box-filtered by 1, 2 or 4 into a rectangle of a texture, on the device
(include/prk.h).

Expected texels come from tests/texref.py, the header's expression in numpy
integers, and are compared word for word.  Frames are compared on bits
(same_frame / the parity tests' compare).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import prk
import texcases
import texref
from prk import abi, scenes
from test_gpu_edge_lists import same_frame
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

W, H = 72, 40  # W % 8 == 0; rows of 288 bytes: 32-byte aligned, not 64


def words(rng, shape):
    return rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32)


def same_texels(got, want, label):
    assert got.shape == want.shape, "%s: shape %r, expected %r" % (label, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d texels differ, first at (x, y) = (%d, %d): %08x, expected %08x" % (
        label, bad.sum(), np.nonzero(bad)[1][0], np.nonzero(bad)[0][0], got[bad][0], want[bad][0])


def padded(rng, w, h, pitch_texels):
    """A scenes.Texture of random words (the pad columns too) at a pitch wider than 4 * w."""
    t = np.zeros((h + 1, pitch_texels), np.uint32)
    t[:h] = words(rng, (h, pitch_texels))
    return scenes.Texture(t, w, h)


@pytest.fixture(scope="module")
def source(gpu):
    """A 72 x 40 target of random words, and a 24 x 12 texture of other random
    words at a pitch of 28 texels (112 bytes: rows start at every word of a
    16-byte line)."""
    rng = np.random.default_rng(21)
    frame = words(rng, (H, W))
    r = prk.Renderer()
    r.target_alloc(W, H)
    r.upload(frame, np.zeros((H, W), np.float32))
    tex = padded(rng, 24, 12, 28)
    t = r.texture(tex)
    yield r, frame, t, tex.texels[:12, :24].copy()
    r.close()


# ---- 1. rectangles, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1, 2, 4])
def test_rectangles_bit_for_bit(source, factor):
    r, frame, t, texels = source
    want = r.texture_download(t)  # (the other factors' calls have written it)
    if factor == 1:
        same_texels(want, texels, "the created texture")
    n = 0
    for dw in (1, 2, 3, 4, 5, 15, 16, 17):
        for x0 in (0, 1, 3):
            for dst_x in (0, 1, 2, 3):
                for dst_y in (0, 5):
                    y0 = n % 5  # (5 * factor rows from there: inside the 40)
                    rect = (x0, y0, factor * dw, factor * 5)
                    r.texture_from_target(t, rect, factor, (dst_x, dst_y))
                    want = texref.from_target(frame, 0, rect, factor, want, (dst_x, dst_y))
                    same_texels(r.texture_download(t), want, "factor %d rect %r dst %r" % (factor, rect,
                                                                                            (dst_x, dst_y)))
                    n += 1
    assert n == 192
    # the target is only read
    same_texels(r.download()[0], frame, "the target after the calls")


def test_every_channel_sum_at_its_maximum(gpu):
    rng = np.random.default_rng(22)
    r = prk.Renderer()
    try:
        r.target_alloc(W, H)
        r.upload(np.full((H, W), 0xFFFFFFFF, np.uint32), np.zeros((H, W), np.float32))
        tex = padded(rng, 24, 12, 28)
        t = r.texture(tex)
        r.texture_from_target(t, (3, 0, 68, 40), 4, (2, 1))
        want = tex.texels[:12, :24].copy()
        want[1:11, 2:19] = 0xFFFFFFFF
        same_texels(r.texture_download(t), want, "all ones by 4")
    finally:
        r.close()


def test_two_workgroups_a_row(gpu):
    """256 texels a row that start one word into a 16-byte line: 65 quads, the
    last one in a second workgroup."""
    rng = np.random.default_rng(23)
    frame = words(rng, (8, 256))
    r = prk.Renderer()
    try:
        r.target_alloc(256, 8)
        r.upload(frame, np.zeros((8, 256), np.float32))
        tex = padded(rng, 260, 8, 264)
        t = r.texture(tex)
        r.texture_from_target(t, None, 1, (1, 0))
        want = texref.from_target(frame, 0, (0, 0, 256, 8), 1, tex.texels[:8, :260], (1, 0))
        same_texels(r.texture_download(t), want, "256 texels at dst_x 1")
    finally:
        r.close()


# ---- 2. a caller-bound target at 4-byte alignment ------------------------------------------------------------------------
def test_caller_bound_unaligned_target(gpu):
    import torch

    rng = np.random.default_rng(24)
    frame = words(rng, (H, W))
    pitch = 4 * W + 4
    dev = torch.device("cuda:0")
    # 4 bytes in front, H rows of `pitch` bytes: the kernel reads inside the rows' 4 * W bytes only
    color = torch.zeros(4 + H * pitch, dtype=torch.uint8, device=dev)
    zbuf = torch.zeros((H, W), dtype=torch.float32, device=dev)
    assert color.data_ptr() % 16 == 0
    r = prk.Renderer()
    try:
        r.target_bind(color.data_ptr() + 4, pitch, zbuf.data_ptr(), W, H)
        r.upload(frame, np.zeros((H, W), np.float32))
        tex = padded(rng, 24, 12, 28)
        t = r.texture(tex)
        want = tex.texels[:12, :24].copy()
        for factor, rect, dst in ((1, (0, 0, 24, 12), (0, 0)), (1, (1, 3, 17, 7), (3, 2)), (2, (0, 0, 48, 24), (0, 0)),
                                  (2, (3, 1, 34, 14), (1, 5)), (4, (0, 0, 72, 40), (0, 0)), (4, (1, 2, 68, 36), (3, 3)),
                                  (4, (4, 4, 64, 16), (2, 0)), (1, (55, 39, 17, 1), (7, 11))):
            r.texture_from_target(t, rect, factor, dst)
            want = texref.from_target(frame, 0, rect, factor, want, dst)
            same_texels(r.texture_download(t), want, "factor %d rect %r dst %r" % (factor, rect, dst))
        same_texels(r.download()[0], frame, "the target after the calls")
    finally:
        r.close()
    assert not color.cpu().numpy()[:4].any()  # (the bytes in front of the target)


# ---- frames ----------------------------------------------------------------------------------------------------------------
def soup(n, size, seed, radius=10.0):
    """A soup whose uvs include u == 1 and v == 1 (the guard row is sampled)."""
    s = scenes.random_soup(n, size, size, radius=radius, seed=seed, centroid_margin=0)
    s.uvs = scenes.addressing_uvs(s.tri_count, ("edges01",), seed + 1)
    assert (s.uvs[:, 0] == 1).any() and (s.uvs[:, 1] == 1).any()
    return s


def as_texture(frame):
    """A frame's colour as a scenes.Texture (the guard row with it)."""
    h, w = frame.shape
    t = np.zeros((h + 1, w), np.uint32)
    t[:h] = frame
    return scenes.Texture(t, w, h)


class Ctx:
    """A renderer with a size x size target and the scenes' camera."""

    def __init__(self, s):
        self.r = r = prk.Renderer()
        r.target_alloc(s.width, s.height)
        r.clear()
        r.set_debug(True)
        r.set_camera(s.prk_transform(), s.prk_lights())
        self.g = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.close()

    def geom(self, s):
        if id(s) not in self.g:
            self.g[id(s)] = self.r.geometry(s.vertices, s.colors, s.normals, s.uvs)
        return self.g[id(s)]

    def draw(self, s, tex):
        self.r.draw_model_optimized(self.geom(s), s.tri_count, P=s.P, bitmap=tex, phong=True)

    def frame(self):
        c, z = self.r.download()
        return c, z, self.r.winners()


# ---- 3. render to texture equals the host way ------------------------------------------------------------------------------
def test_render_to_texture_equals_the_host_way(gpu):
    a, b = soup(40, 64, 31), soup(40, 64, 33)
    with Ctx(a) as f:
        r = f.r
        f.draw(a, r.texture(a.texture))
        r.complete_all_work()
        t = r.texture_alloc(64, 64)
        r.texture_from_target(t)
        r.clear()
        f.draw(b, t)
        r.complete_all_work()
        got = f.frame()
        # the host way: frame A again, downloaded and created as a texture
        r.clear()
        f.draw(a, r.texture(a.texture))
        r.complete_all_work()
        frame_a = f.frame()[0]
        same_texels(r.texture_download(t), frame_a, "the texture against frame A")
        r.clear()
        f.draw(b, r.texture(as_texture(frame_a)))
        r.complete_all_work()
        want = f.frame()
    assert (got[2] >= 0).sum() > 200 and len(np.unique(frame_a)) > 100
    same_frame(got, want, "frame B with the device's texture against frame B with the host's")
    o = O.render(texcases.with_texture(b, as_texture(frame_a)), semantics=abi.PRK_SEM_AVX, phong=True)
    compare(got + (None,), o, label="frame B against the oracle")


# ---- 4. supersample resolve ------------------------------------------------------------------------------------------------
def test_supersample_resolve(gpu):
    s = soup(60, 128, 35, radius=20.0)
    with Ctx(s) as f:
        r = f.r
        f.draw(s, r.texture(s.texture))
        r.complete_all_work()
        t2, t4 = r.texture_alloc(64, 64), r.texture_alloc(32, 32)
        r.texture_from_target(t2, factor=2)
        r.texture_from_target(t4, factor=4)
        got2, got4 = r.texture_download(t2), r.texture_download(t4)
        frame = f.frame()[0]
    assert len(np.unique(frame)) > 100
    same_texels(got2, texref.resolve(frame, 2), "128 x 128 by 2")
    same_texels(got4, texref.resolve(frame, 4), "128 x 128 by 4")


# ---- 5. order without host waits -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soups256():
    return [soup(3000, 256, seed, radius=12.0) for seed in (41, 43, 45)]


def test_three_frames_no_wait(gpu, soups256):
    sa, sb, sc = soups256
    with Ctx(sa) as f:
        r = f.r
        t0 = r.texture(sa.texture)
        t = r.texture_alloc(256, 256)
        for s in soups256:         # (every upload first: from here to the download no call waits for the device)
            f.geom(s)
        f.draw(sa, t0)
        r.complete_all_work()      # A
        r.texture_from_target(t)
        r.clear()
        f.draw(sb, t)
        r.complete_all_work()      # B samples A
        r.texture_from_target(t)   # (after B has sampled it)
        f.draw(sc, t)
        r.complete_all_work()      # C samples B, drawn over B
        got = f.frame()
        # the host way, a download and an upload between the frames
        r.clear()
        f.draw(sa, t0)
        r.complete_all_work()
        h = r.texture(as_texture(f.frame()[0]))
        r.clear()
        f.draw(sb, h)
        r.complete_all_work()
        frame_b = f.frame()[0]
        r.texture_update(h, as_texture(frame_b))
        f.draw(sc, h)
        r.complete_all_work()
        want = f.frame()
        same_texels(r.texture_download(t), frame_b, "the texture against frame B")
    assert (got[2] >= 0).sum() > 20000
    same_frame(got, want, "frame C of the device sequence against the host sequence")


def test_recorded_draw_samples_the_new_contents(gpu, soups256):
    sa, sb, _ = soups256
    with Ctx(sa) as f:
        r = f.r
        t = r.texture_alloc(256, 256)
        f.draw(sa, r.texture(sa.texture))
        r.complete_all_work()
        frame_a = f.frame()[0]
        f.draw(sb, t)              # recorded while the texture is all zeros
        r.texture_from_target(t)
        r.complete_all_work()
        got = f.frame()
        r.clear()                  # the host way: frame A again, then B over it with A as a host texture
        f.draw(sa, r.texture(sa.texture))
        r.complete_all_work()
        f.draw(sb, r.texture(as_texture(frame_a)))
        r.complete_all_work()
        want = f.frame()
    same_frame(got, want, "a draw recorded before texture_from_target")


def test_pending_clear_on_flush_is_not_seen(gpu):
    rng = np.random.default_rng(25)
    frame = words(rng, (H, W))
    r = prk.Renderer()
    try:
        r.target_alloc(W, H)
        r.upload(frame, np.zeros((H, W), np.float32))
        t = r.texture_alloc(W, H)
        r.clear_on_flush(0x11223344)
        r.texture_from_target(t)
        same_texels(r.texture_download(t), frame, "with a clear pending")
    finally:
        r.close()


# ---- 6. a band context -----------------------------------------------------------------------------------------------------
def test_band_context(gpu):
    rng = np.random.default_rng(26)
    band = words(rng, (32, 64))
    r = prk.Renderer()
    try:
        r.target_alloc(64, 64, 16, 48)
        r.upload(band, np.zeros((32, 64), np.float32))
        t = r.texture_alloc(20, 20)
        want = np.zeros((20, 20), np.uint32)
        for factor, rect, dst in ((2, (3, 18, 8, 8), (1, 2)), (1, (0, 16, 20, 1), (0, 0)), (4, (8, 16, 48, 32), (5, 9)),
                                  (1, (60, 47, 4, 1), (16, 19))):
            r.texture_from_target(t, rect, factor, dst)
            want = texref.from_target(band, 16, rect, factor, want, dst)
            same_texels(r.texture_download(t), want, "band rect %r by %d" % (rect, factor))
        L, h = r._L, r._h
        for rect in ((0, 15, 4, 4), (0, 15, 4, 1), (0, 45, 4, 4), (0, 48, 4, 1), (0, 0, 4, 4)):
            assert L.prk_texture_from_target(h, t, *rect, 1, 0, 0) == abi.PRK_ERR_ARG, rect
            same_texels(r.texture_download(t), want, "after the refused rect %r" % (rect,))
        r.texture_from_target(t, None, 4, (0, 0))  # the whole band: 64 x 32 by 4
        want = texref.from_target(band, 16, (0, 16, 64, 32), 4, want, (0, 0))
        same_texels(r.texture_download(t), want, "the whole band")
    finally:
        r.close()


# ---- 7. refused calls ------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(source):
    r, frame, t, _ = source
    before = r.texture_download(t)
    L, h = r._L, r._h
    call = L.prk_texture_from_target
    big = 2**31 - 1
    cases = [
        ("null context", lambda: call(None, t, 0, 0, 4, 4, 1, 0, 0)),
        ("texture < 0", lambda: call(h, -1, 0, 0, 4, 4, 1, 0, 0)),
        ("texture past the handles", lambda: call(h, 999, 0, 0, 4, 4, 1, 0, 0)),
        ("factor 0", lambda: call(h, t, 0, 0, 4, 4, 0, 0, 0)),
        ("factor 3", lambda: call(h, t, 0, 0, 6, 6, 3, 0, 0)),
        ("factor 8", lambda: call(h, t, 0, 0, 8, 8, 8, 0, 0)),
        ("factor -2", lambda: call(h, t, 0, 0, 4, 4, -2, 0, 0)),
        ("width 0", lambda: call(h, t, 0, 0, 0, 4, 1, 0, 0)),
        ("height 0", lambda: call(h, t, 0, 0, 4, 0, 1, 0, 0)),
        ("width < 0", lambda: call(h, t, 0, 0, -4, 4, 1, 0, 0)),
        ("height < 0", lambda: call(h, t, 0, 0, 4, -4, 2, 0, 0)),
        ("width no multiple of 2", lambda: call(h, t, 0, 0, 5, 4, 2, 0, 0)),
        ("height no multiple of 4", lambda: call(h, t, 0, 0, 8, 6, 4, 0, 0)),
        ("x0 < 0", lambda: call(h, t, -1, 0, 4, 4, 1, 0, 0)),
        ("y0 < 0", lambda: call(h, t, 0, -1, 4, 4, 1, 0, 0)),
        ("source past the right edge", lambda: call(h, t, W - 3, 0, 4, 4, 1, 0, 0)),
        ("source past the last row", lambda: call(h, t, 0, H - 3, 4, 4, 1, 0, 0)),
        ("x0 + width past int32", lambda: call(h, t, big, 0, 4, 4, 1, 0, 0)),
        ("y0 + height past int32", lambda: call(h, t, 0, 4, 4, big - 3, 4, 0, 0)),
        ("dst_x < 0", lambda: call(h, t, 0, 0, 4, 4, 1, -1, 0)),
        ("dst_y < 0", lambda: call(h, t, 0, 0, 4, 4, 1, 0, -1)),
        ("destination past the texture's width", lambda: call(h, t, 0, 0, 4, 4, 1, 21, 0)),
        ("destination past the texture's height", lambda: call(h, t, 0, 0, 8, 8, 2, 0, 9)),
        ("destination in the pad columns", lambda: call(h, t, 0, 0, 26, 4, 1, 0, 0)),
        ("destination on the guard row", lambda: call(h, t, 0, 0, 4, 1, 1, 0, 12)),
        ("dst_x + width past int32", lambda: call(h, t, 0, 0, 4, 4, 1, big, 0)),
    ]
    for label, bad in cases:
        assert bad() == abi.PRK_ERR_ARG, label
        same_texels(r.texture_download(t), before, "after the refused call: " + label)
    same_texels(r.download()[0], frame, "the target after the refused calls")
    # no target bound
    r2 = prk.Renderer()
    try:
        t2 = r2.texture_alloc(8, 8)
        assert r2._L.prk_texture_from_target(r2._h, t2, 0, 0, 4, 4, 1, 0, 0) == abi.PRK_ERR_NO_TARGET
        assert not r2.texture_download(t2).any()
        assert r2._L.prk_texture_from_target(r2._h, t2, 0, 0, 4, 4, 3, 0, 0) == abi.PRK_ERR_ARG
    finally:
        r2.close()
    # the other calls' arguments
    out = np.zeros((12, 24), np.uint32)
    n = C.c_int32(-1)
    assert L.prk_texture_download(h, t, None, 96) == abi.PRK_ERR_ARG
    assert L.prk_texture_download(h, t, out.ctypes.data, 92) == abi.PRK_ERR_ARG
    assert L.prk_texture_download(h, t, out.ctypes.data, 98) == abi.PRK_ERR_ARG
    assert L.prk_texture_download(h, 999, out.ctypes.data, 96) == abi.PRK_ERR_ARG and not out.any()
    assert L.prk_texture_info(h, -1, C.byref(n), None, None) == abi.PRK_ERR_ARG and n.value == -1
    for w_, h_ in ((0, 4), (4, 0), (-1, 4), (4, -1), (2**29, 1)):
        assert L.prk_texture_alloc(h, w_, h_, C.byref(n)) == abi.PRK_ERR_ARG and n.value == -1, (w_, h_)
    assert L.prk_texture_alloc(h, 4, 4, None) == abi.PRK_ERR_ARG


# ---- 8. info, and a fresh texture --------------------------------------------------------------------------------------
def test_info_and_fresh_texture(source):
    r, _, t, _ = source
    assert r.texture_info(t) == (24, 12, 112)
    a = r.texture_alloc(33, 7)
    assert a != t and r.texture_info(a) == (33, 7, 132)
    got = r.texture_download(a)
    assert got.shape == (7, 33) and not got.any()
    w = C.c_int32(0)
    assert r._L.prk_texture_info(r._h, a, None, None, None) == abi.PRK_OK
    assert r._L.prk_texture_info(r._h, a, C.byref(w), None, None) == abi.PRK_OK and w.value == 33
    # a wider host pitch: the rows land `pitch_bytes` apart, the bytes between them untouched
    out = np.full((7, 40), 0xABABABAB, np.uint32)
    r.texture_from_target(a, (0, 0, 33, 7), 1, (0, 0))
    assert r._L.prk_texture_download(r._h, a, out.ctypes.data, 160) == abi.PRK_OK
    assert (out[:, 33:] == 0xABABABAB).all()
    same_texels(out[:, :33], r.download()[0][:7, :33], "download at a wider pitch")
