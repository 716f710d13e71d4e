"""GPU tests: texture addressing of the HIP path against the oracle.

The scenes of tests/texcases.py (textures that are not square, padded, one
texel wide or high, with a pitch of 32768 and 65536 bytes or 33000 rows; uv on
the edge of [0, 1], outside it and far outside), which
tests/test_texture_addressing.py shows to tell a wrong address from a right
one, drawn per triangle (k_pix, k_shade) and as objects of five triangles (the
span path: k_pix<false, true>, k_span_shade) under every semantics that
samples a texture, nearest and bilinear; several textures of different shape in
one frame; and prk_texture_update / prk_texture_set_filter between frames.
Compared as tests/test_gpu_parity.py compares: z and winners bit for bit,
colours exact.  Reference-drawn frames of such textures are held to the GPU by
tests/test_gpu_ref_parity.py (the fixtures *_nonsquare and queue_edges01).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import prk
import texcases as T
from prk import abi
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

AVX, AVX_ST, SCALAR = abi.PRK_SEM_AVX, abi.PRK_SEM_AVX_ST, abi.PRK_SEM_SCALAR
WAYS = {"avx": (AVX, True), "avx_st": (AVX_ST, True), "scalar_phong": (SCALAR, True), "scalar_gouraud": (SCALAR, False)}
# 400 triangles of radius 14 on 256 x 192: several tiles, every row band, a frame in well under a second
N, W, H, RADIUS, SEED = 400, 256, 192, 14.0, 5

_ORACLE = {}


def gpu_case(name, filt=abi.PRK_FILTER_NEAREST):
    return T.case(name, N, W, H, RADIUS, SEED, filt=filt)


def oracle_frame(name, way, tpo, filt=abi.PRK_FILTER_NEAREST):
    key = (name, way, tpo, filt)
    if key not in _ORACLE:
        sem, phong = WAYS[way]
        f = O.render(gpu_case(name, filt), semantics=sem, phong=phong, tris_per_object=tpo)
        for a in f[:3]:
            a.setflags(write=False)
        _ORACLE[key] = f
    return _ORACLE[key]


def check(name, way, tpo, filt=abi.PRK_FILTER_NEAREST):
    sem, phong = WAYS[way]
    o = oracle_frame(name, way, tpo, filt)
    assert (o[2] >= 0).sum() > 0
    g = prk.render_scene(gpu_case(name, filt), semantics=sem, phong=phong, tris_per_object=tpo)
    compare(g, o, label="%s %s tpo=%d filter=%d" % (name, way, tpo, filt))


@pytest.mark.parametrize("tpo", [1, 5])
@pytest.mark.parametrize("way", ["avx", "avx_st", "scalar_phong"])
@pytest.mark.parametrize("name", T.NAMES)
def test_nearest(gpu, name, way, tpo):
    check(name, way, tpo)


@pytest.mark.parametrize("name", T.NAMES)
def test_nearest_scalar_gouraud(gpu, name):
    check(name, "scalar_gouraud", 1)


@pytest.mark.parametrize("tpo", [1, 5])
@pytest.mark.parametrize("name", T.BILINEAR)
def test_bilinear(gpu, name, tpo):
    check(name, "avx", tpo, abi.PRK_FILTER_BILINEAR)


def _shapes():
    """Four textures of four shapes (one bilinear), and uvs with whole
    triangles on u or v of exactly 0 and 1."""
    w, h, p, _ = T.CASES["padded"]
    padded = T.make_texture(w, h, p, 11)
    w, h, p, _ = T.CASES["nonsquare_t"]
    wide = T.make_texture(w, h, p, 12)
    wide_bilinear = T.make_texture(w, h, p, 13, filt=abi.PRK_FILTER_BILINEAR)
    w, h, p, _ = T.CASES["nonsquare"]
    tall = T.make_texture(w, h, p, 14)
    s = gpu_case("edges01")
    s.texture = None
    return s, padded, wide, wide_bilinear, tall


def test_mixed_semantics_frame_each_draw_its_own_texture(gpu):
    """AVX, scalar and single-thread draws in one flush, as
    test_mixed_semantics_one_frame has them (the AVX items then shade in
    k_shade / item_avx_pixel), each with a texture of another shape: padded nearest,
    24 x 40 under DrawModel, 40 x 24 bilinear, and the padded one again for
    objects of five triangles."""
    s, padded, wide, wide_bilinear, tall = _shapes()
    q = s.tri_count // 4
    s.draws = [(0, q, padded, AVX, 1), (q, q, tall, SCALAR, 1), (2 * q, q, wide_bilinear, AVX, 1),
               (3 * q, s.tri_count - 3 * q, padded, AVX_ST, 5)]
    compare(prk.render_scene(s), O.render(s), label="mixed semantics, four shapes")


@pytest.mark.parametrize("way,tpo", [("avx", 1), ("avx", 5), ("scalar_phong", 1), ("scalar_phong", 5)])
def test_two_nearest_textures_of_different_shape(gpu, way, tpo):
    """Two draws of one semantics, nearest both, 24 x 40 with a pitch of 32
    texels and 40 x 24: a kernel that shades one draw's pixels with the other
    draw's TexRec gets Width, Height or Pitch wrong."""
    sem, phong = WAYS[way]
    s, padded, wide, _, _ = _shapes()
    half = s.tri_count // 2
    s.draws = [(0, half, padded), (half, s.tri_count - half, wide)]
    o = O.render(s, semantics=sem, phong=phong, tris_per_object=tpo)
    compare(prk.render_scene(s, semantics=sem, phong=phong, tris_per_object=tpo), o, label="two shapes %s" % way)
    s.draws = [(0, half, wide), (half, s.tri_count - half, padded)]
    assert (O.render(s, semantics=sem, phong=phong, tris_per_object=tpo)[0] != o[0]).any()  # (they do differ)


class _Frames:
    """One context, one geometry, one texture handle: frames drawn one after
    the other, each downloaded with its winners."""

    def __init__(self, scene, texture, sem, phong):
        self.s, self.sem, self.phong = scene, sem, phong
        self.r = prk.Renderer(0)
        self.r.target_alloc(scene.width, scene.height)
        self.r.set_debug(True)
        self.r.set_camera(scene.prk_transform(), scene.prk_lights())
        self.g = self.r.geometry(scene.vertices, scene.colors, scene.normals, scene.uvs)
        self.tex = self.r.texture(texture)

    def frame(self):
        r = self.r
        r.clear()
        r.draw(self.sem, self.g, self.s.tri_count, P=self.s.P, bitmap=self.tex, phong=self.phong)
        r.complete_all_work()
        r.synchronize()
        col, z = r.download()
        return col, z, r.winners(), None

    def expect(self, texture, label):
        o = O.render(T.with_texture(self.s, texture), semantics=self.sem, phong=self.phong)
        assert (o[2] >= 0).sum() > 0
        compare(self.frame(), o, label=label)
        return o

    def close(self):
        self.r.close()


@pytest.mark.parametrize("way", ["avx", "scalar_phong"])
def test_texture_update_changes_shape_then_texels(gpu, way):
    """prk_texture_update onto a handle of another shape (24 x 40 with a pitch
    of 32 texels -> 40 x 24 tight: the reallocating branch), then onto the same
    shape with other texels (in place); each frame against the oracle."""
    sem, phong = WAYS[way]
    s, padded, wide, _, _ = _shapes()
    wide2 = T.make_texture(wide.width, wide.height, wide.texels.shape[1], 15)
    f = _Frames(s, padded, sem, phong)
    try:
        a = f.expect(padded, "before any update")
        f.r.texture_update(f.tex, wide)
        b = f.expect(wide, "after an update to another shape")
        f.r.texture_update(f.tex, wide2)
        c = f.expect(wide2, "after an update in place")
    finally:
        f.close()
    assert (a[0] != b[0]).any() and (b[0] != c[0]).any()


def test_set_filter_toggled_between_frames(gpu):
    """bilinear -> nearest -> bilinear on one handle, a frame each."""
    s, padded, _, _, _ = _shapes()
    nearest = padded
    bilinear = T.make_texture(24, 40, 32, 11, filt=abi.PRK_FILTER_BILINEAR)
    assert (bilinear.texels == nearest.texels).all()
    f = _Frames(s, bilinear, AVX, True)
    try:
        a = f.expect(bilinear, "bilinear at creation")
        f.r.set_filter(f.tex, abi.PRK_FILTER_NEAREST)
        b = f.expect(nearest, "nearest")
        f.r.set_filter(f.tex, abi.PRK_FILTER_BILINEAR)
        c = f.expect(bilinear, "bilinear again")
    finally:
        f.close()
    assert (a[0] != b[0]).any() and (a[0] == c[0]).all()


def test_bad_bitmaps_are_refused_and_change_nothing(gpu):
    """prk_texture_create / prk_texture_update return PRK_ERR_ARG for a Pitch
    below 4 * Width, a Pitch that is no multiple of 4, a Width or Height of
    zero, no bitmap, no Memory and (update) a handle that does not exist; no
    handle is made, the texture of the handle given stays, and the next frame
    is exact."""
    s, padded, _, _, _ = _shapes()
    texels = np.ascontiguousarray(padded.texels)
    mem = texels.ctypes.data
    bad = [abi.PrkBitmap(mem, 24, 40, 4 * 24 - 4), abi.PrkBitmap(mem, 24, 40, 4 * 32 + 2), abi.PrkBitmap(mem, 0, 40, 128),
           abi.PrkBitmap(mem, 24, 0, 128), abi.PrkBitmap(mem, -24, 40, 128), abi.PrkBitmap(None, 24, 40, 128)]
    good = abi.PrkBitmap(mem, 24, 40, 128)
    f = _Frames(s, padded, AVX, True)
    try:
        L, ctx = f.r._L, f.r._h
        f.expect(padded, "before the refused calls")
        for b in bad:
            h = C.c_int32(-7)
            assert L.prk_texture_create(ctx, C.byref(b), C.byref(h)) == abi.PRK_ERR_ARG and h.value == -7
            assert L.prk_texture_update(ctx, f.tex, C.byref(b)) == abi.PRK_ERR_ARG
        h = C.c_int32(-7)
        assert L.prk_texture_create(ctx, None, C.byref(h)) == abi.PRK_ERR_ARG and h.value == -7
        assert L.prk_texture_create(ctx, C.byref(good), None) == abi.PRK_ERR_ARG
        assert L.prk_texture_update(ctx, f.tex, None) == abi.PRK_ERR_ARG
        for handle in (-1, f.tex + 1, 1 << 20):
            assert L.prk_texture_update(ctx, handle, C.byref(good)) == abi.PRK_ERR_ARG
            assert L.prk_texture_set_filter(ctx, handle, abi.PRK_FILTER_NEAREST) == abi.PRK_ERR_ARG
        assert L.prk_texture_set_filter(ctx, f.tex, 2) == abi.PRK_ERR_ARG
        f.expect(padded, "after the refused calls")
        # no handle was made: the next one is the second
        assert f.r.texture(padded) == f.tex + 1
    finally:
        f.close()
