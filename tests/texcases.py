"""Scenes that put texture addressing to the test: non-square, padded, huge
textures and uv on and outside the edge of [0, 1].

Shared by tests/test_texture_addressing.py (CPU: the oracle, pyref and the AVX2
baseline against each other, and the proof that each scene tells a wrong
address from a right one) and tests/test_gpu_texture_addressing.py (the HIP
path against the oracle).  A plain module: no fixtures, no pytest.

A case is a scenes.random_soup whose texture and uvs are replaced
(scenes.retexture: the builders live in the package, where
tools/make_ref_golden.py finds them too).  The texture is uint32 [h + 1, pitch_texels] with pitch_texels >= w: a seeded
random w x h body, the zeroed guard row (all pitch_texels of it) and, in the
pad columns of the h body rows, PAD_FILL: a constant, so a texel fetched from
the pad shows up as that one colour.
"""
import numpy as np

from prk import abi, scenes

PAD_FILL = scenes.PAD_FILL
make_texture, make_uvs, retexture = scenes.padded_texture, scenes.addressing_uvs, scenes.retexture

# name -> (w, h, pitch in texels, uv recipe)
CASES = {
    "nonsquare": (24, 40, 24, ("uniform", 0.0, 1.0)),
    "nonsquare_t": (40, 24, 40, ("uniform", 0.0, 1.0)),
    "padded": (24, 40, 32, ("uniform", 0.0, 1.0)),
    "edges01": (24, 40, 32, ("edges01",)),
    "outside": (24, 40, 32, ("uniform", -0.75, 1.75)),
    "far_outside": (24, 40, 32, ("far",)),
    "one_wide": (1, 5, 3, ("uniform", -0.5, 1.5)),
    "one_high": (5, 1, 8, ("uniform", -0.5, 1.5)),
    "pitch_sign": (8192, 2, 8192, ("uniform", 0.0, 1.0)),    # 32768 bytes: the int16 sign bit of the pitch's low half
    "pitch_64k": (16384, 2, 16384, ("uniform", 0.0, 1.0)),   # 65536 bytes: low half 0, high half 1
    "tall": (3, 33000, 3, ("tall",)),                        # rows from 32768 on: the sign bit of the row's low half
}
NAMES = list(CASES)
# bilinear is defined by the oracle for uv a float -> int32 conversion can hold
BILINEAR = ["nonsquare", "nonsquare_t", "padded", "edges01", "outside", "one_wide", "one_high"]
TALL_V = scenes.TALL_V


def case(name, n=60, W=96, H=64, radius=14.0, seed=5, pad_fill=PAD_FILL, filt=abi.PRK_FILTER_NEAREST):
    """The named case: n triangles on a W x H frame (the defaults are what
    pyref can afford; the GPU tests ask for more)."""
    w, h, pitch, recipe = CASES[name]
    s = scenes.random_soup(n, W, H, radius=radius, seed=seed, tex_size=8,
                           lights=scenes.LIGHTS_TWO, ambient=scenes.AMBIENT_TWO)
    s = retexture(s, w, h, pitch, recipe, seed, pad_fill, filt)
    s.name = "tex_%s_%dx%d_n%d_s%d" % (name, W, H, n, seed)
    return s


def with_texture(scene, texture):
    """A shallow copy of the scene that draws with another texture."""
    s = scene.subset(0, scene.tri_count)
    s.texture, s.name = texture, scene.name
    return s


def folded(scene):
    """The same geometry with every uv folded into [0, 1) (its fractional part)."""
    s = scene.subset(0, scene.tri_count)
    uv = s.uvs.astype(np.float64)
    s.uvs = np.minimum(uv - np.floor(uv), np.nextafter(np.float32(1), np.float32(0))).astype(np.float32)
    return s


def transposed_description(tex):
    """The same body bytes of an unpadded w x h texture described as h x w
    (Pitch 4 * h), with a guard row of that width."""
    w, h = tex.width, tex.height
    assert tex.texels.shape == (h + 1, w)
    t = np.zeros((w + 1, h), np.uint32)
    t[:w] = tex.texels[:h].reshape(w, h)
    return scenes.Texture(t, h, w, tex.filter)
