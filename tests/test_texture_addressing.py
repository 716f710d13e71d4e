"""CPU tests: texture addressing on textures that are not square, not tightly
pitched, one texel wide or high, or large enough for the 16-bit pitch multiply
to matter, with uv on the edge of [0, 1] and outside it (tests/texcases.py).

Three things are shown here, before tests/test_gpu_texture_addressing.py holds
the HIP path to the oracle on the same scenes:

* the restatements agree bit for bit on every case: oracle/prk_oracle.c,
  tests/pyref.py and (AVX semantics, where the host has AVX2) the AVX2 baseline;
* each scene has teeth: the address mistake it is there for changes the frame.
  These are conditions on the oracle or pyref alone, met by the seeds chosen;
* where this machine has the reference (oracle/_ref/), the non-square textures
  and the one with a pitch of 65536 bytes (whose 16-bit row product is 0: row 1
  reads row 0, inside the texture) drawn live by the reference itself equal
  the oracle through all three entry points.  The reference's driver describes
  a texture with Pitch = 4 * Width, so pad columns are the oracle's alone.

Pixel counts seen with the seeds used (96x64, 60 triangles, seed 5) stand in the
docstrings of the teeth tests.
"""
import numpy as np
import pytest

import oracle as O
import pyref
import texcases as T
from prk import abi
from test_ref_parity import assert_same, make_ref_golden, needs_driver, ref_run

AVX, AVX_ST, SCALAR = abi.PRK_SEM_AVX, abi.PRK_SEM_AVX_ST, abi.PRK_SEM_SCALAR
# (semantics, phong): FillLineOptimized through the queue and the single-thread overload, DrawModel + texture
WAYS = {"avx": (AVX, True), "avx_st": (AVX_ST, True), "scalar_phong": (SCALAR, True), "scalar_gouraud": (SCALAR, False)}

_FRAMES = {}


def oracle_frame(name, way):
    """The oracle's (colour, z, winners) of a case, drawn once and not written to."""
    if (name, way) not in _FRAMES:
        sem, phong = WAYS[way]
        f = O.render(T.case(name), semantics=sem, phong=phong)[:3]
        for a in f:
            a.setflags(write=False)
        _FRAMES[name, way] = f
    return _FRAMES[name, way]


def differing(a, b):
    """Pixels at which two frames differ in colour, z or winner."""
    return int(((a[0] != b[0]) | (a[1].view(np.uint32) != b[1].view(np.uint32)) | (a[2] != b[2])).sum())


def covered(f):
    return int((f[2] >= 0).sum())


def same(a, b, what):
    nz = int((a[1].view(np.uint32) != b[1].view(np.uint32)).sum())
    nw, nc = int((a[2] != b[2]).sum()), int((a[0] != b[0]).sum())
    assert (nz, nw, nc) == (0, 0, 0), "%s: z %d, winners %d, colours %d pixels differ" % (what, nz, nw, nc)


# ---- the restatements agree -------------------------------------------------
@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("name", T.NAMES)
def test_restatements_agree(name, way):
    sem, phong = WAYS[way]
    s = T.case(name)
    o = oracle_frame(name, way)
    assert covered(o) > 0
    same(pyref.render(s, sem, phong), o, "pyref against the oracle")
    if sem == AVX and O.cpu_lib() is not None:
        for cpu, threads in (("banded", 3), ("rows", 1), ("queue", 1)):
            same(O.render(s, semantics=sem, phong=phong, threads=threads, cpu=cpu)[:3], o, "AVX2 baseline (%s)" % cpu)


@pytest.mark.parametrize("name", T.BILINEAR)
def test_restatements_agree_bilinear(name):
    """The bilinear extension (AVX semantics): pyref and the AVX2 baseline
    against the oracle, whose or_bilinear is its definition."""
    s = T.case(name, filt=abi.PRK_FILTER_BILINEAR)
    o = O.render(s)[:3]
    assert covered(o) > 0
    assert differing(o, oracle_frame(name, "avx")) > 0, "the filter changes nothing"
    same(pyref.render(s, AVX, True), o, "pyref against the oracle")
    if O.cpu_lib() is not None:
        for cpu, threads in (("banded", 3), ("rows", 1), ("queue", 1)):
            same(O.render(s, threads=threads, cpu=cpu)[:3], o, "AVX2 baseline (%s)" % cpu)


# ---- teeth ------------------------------------------------------------------
@pytest.mark.parametrize("way", list(WAYS))
def test_teeth_width_and_height_exchanged(way):
    """`nonsquare` against the same texels described as 40 x 24: 1719 (avx,
    avx_st), 2163 (scalar_phong) and 2166 (scalar_gouraud) pixels change."""
    sem, phong = WAYS[way]
    s = T.case("nonsquare")
    t = T.with_texture(s, T.transposed_description(s.texture))
    assert differing(O.render(t, semantics=sem, phong=phong), oracle_frame("nonsquare", way)) > 0


@pytest.mark.parametrize("name", ["padded", "outside", "edges01"])
@pytest.mark.parametrize("way", ["scalar_phong", "scalar_gouraud"])
def test_teeth_scalar_reads_the_pad_columns(name, way):
    """DrawModel masks no uv: with only the pad fill changed, 16 (padded),
    455 (outside) and 12 (edges01) pixels change colour."""
    sem, phong = WAYS[way]
    other = O.render(T.case(name, pad_fill=0xFF112233), semantics=sem, phong=phong)
    assert differing(other, oracle_frame(name, way)) > 0


@pytest.mark.parametrize("way", ["avx", "avx_st"])
def test_teeth_avx_masks_uv_outside(way):
    """FillLineOptimized keeps a lane only with u and v in [0, 1]: `outside`
    covers 687 pixels, the same triangles with uv folded into [0, 1) 1752."""
    sem, phong = WAYS[way]
    o = oracle_frame("outside", way)
    f = O.render(T.folded(T.case("outside")), semantics=sem, phong=phong)
    assert 0 < covered(o) < covered(f)


def _plain_mul(y, p):
    r = (y * p) & 0xFFFFFFFF
    return r - (1 << 32) if r & 0x80000000 else r


@pytest.mark.parametrize("way", ["avx", "avx_st"])
@pytest.mark.parametrize("name", ["pitch_sign", "pitch_64k", "tall"])
def test_teeth_sixteen_bit_pitch_multiply(name, way, monkeypatch):
    """The row offset is the reference's 16-bit mullo / mulhi product, not
    y * Pitch: with a plain 32-bit multiply in pyref 768 (pitch_sign), 770
    (pitch_64k) and 401 (tall) pixels change."""
    sem, phong = WAYS[way]
    assert pyref.mul16(1, 64) == _plain_mul(1, 64) == 64
    monkeypatch.setattr(pyref, "mul16", _plain_mul)
    assert differing(pyref.render(T.case(name), sem, phong), oracle_frame(name, way)) > 0


def _texel_unclamped(tex, off):
    flat = tex.texels.reshape(-1).view(np.uint8)
    off %= flat.size - 3  # (any offset reads inside the buffer)
    return int(flat[off:off + 4].copy().view(np.uint32)[0])


@pytest.mark.parametrize("way", ["scalar_phong", "scalar_gouraud"])
@pytest.mark.parametrize("name", ["outside", "far_outside"])
def test_teeth_offset_clamp(name, way, monkeypatch):
    """Byte offsets outside [0, Pitch * (Height + 1) - 4] read offset 0: with
    the clamp taken out of pyref (offsets wrapped into the buffer) 718 / 722
    (outside, Phong / Gouraud) and 1048 (far_outside) pixels change."""
    sem, phong = WAYS[way]
    monkeypatch.setattr(pyref, "texel", _texel_unclamped)
    assert differing(pyref.render(T.case(name), sem, phong), oracle_frame(name, way)) > 0


@pytest.mark.parametrize("way", ["avx", "avx_st"])
@pytest.mark.parametrize("part", ["guard_row", "pad_column"])
def test_teeth_u_and_v_of_exactly_one(part, way):
    """The AVX mask is 0 <= u <= 1 and 0 <= v <= 1 (oracle/prk_oracle.c's Mask;
    projekt.cpp:1874-1877 compares with the predicates >= and <=, and the
    fixture queue_edges01 is such a frame from the reference): u == 1 is kept
    and fetches texel x == Width, the first pad column (the next row's first
    texel where Pitch == 4 * Width);
    v == 1 is kept and fetches the guard row.  `edges01` has such pixels: with
    only the guard row changed 432 pixels change, with only the first pad
    column 83."""
    sem, phong = WAYS[way]
    s = T.case("edges01")
    w, h = s.texture.width, s.texture.height
    texels = s.texture.texels.copy()
    if part == "guard_row":
        texels[h, :] = 0xFF336699
    else:
        texels[:h, w] = 0xFF336699
    t = T.with_texture(s, type(s.texture)(texels, w, h, s.texture.filter))
    assert differing(O.render(t, semantics=sem, phong=phong), oracle_frame("edges01", way)) > 0


@pytest.mark.parametrize("way", ["avx", "avx_st"])
def test_teeth_avx_inside_never_reads_the_pad(way):
    """With uv in [0, 1) the AVX paths fetch body texels only: `padded` draws
    the same frame whatever the pad holds, so its GPU test pins Pitch against
    4 * Width and nothing else."""
    sem, phong = WAYS[way]
    other = O.render(T.case("padded", pad_fill=0xFF112233), semantics=sem, phong=phong)
    assert differing(other, oracle_frame("padded", way)) == 0
    s = T.case("padded")
    tight = T.with_texture(s, T.make_texture(24, 40, 24, 5 + 1))
    assert (tight.texture.texels[:, :24] == s.texture.texels[:, :24]).all()
    assert differing(O.render(tight, semantics=sem, phong=phong), oracle_frame("padded", way)) == 0


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("name", T.NAMES)
def test_every_case_covers_pixels(name, way):
    assert covered(oracle_frame(name, way)) > 0


def test_tall_reaches_the_rows_past_32767():
    s = T.case("tall")
    assert s.texture.texels.shape == (33001, 3) and (s.uvs[:, 1] >= T.TALL_V).sum() >= 30
    assert int(np.float32(33000) * np.float32(T.TALL_V)) >= 32768


def test_case_textures_are_as_described():
    for name, (w, h, pitch, _) in T.CASES.items():
        tex = T.case(name).texture
        assert tex.texels.shape == (h + 1, pitch) and (tex.width, tex.height, tex.pitch) == (w, h, 4 * pitch)
        assert not tex.texels[h].any() and (tex.texels[:h, w:] == T.PAD_FILL).all()
        assert tex.texels.nbytes <= 400 * 1024
    assert T.CASES["pitch_sign"][2] * 4 == 0x8000 and T.CASES["pitch_64k"][2] * 4 == 0x10000


# ---- with the reference at hand ---------------------------------------------
# DrawModel masks nothing, so its uvs are kept inside the texture, and of the seeds from 5 on the first (14)
# with no pixel that depends on memory around the texture is taken (ref_run reports them)
LIVE = [("DrawModelOptimized(RenderQueue)", 5, None), ("DrawModelOptimized(single thread)", 5, None),
        ("DrawModel", 14, (0.35, 0.65))]


@needs_driver
@pytest.mark.parametrize("entry,seed,inner", LIVE)
@pytest.mark.parametrize("name", ["nonsquare", "nonsquare_t", "pitch_64k"])
def test_live_reference_equals_oracle(name, entry, seed, inner):
    s = T.case(name, seed=seed)
    if inner is not None:
        s = make_ref_golden.inner_uvs(s, *inner)
    col, z, win, info = ref_run.render(s, entry, True, patches=("P3",))
    assert info["undefined_pixels"] == 0
    assert (win >= 0).sum() > 0
    sem = ref_run.ENTRY_POINTS[entry][1]
    assert_same(O.render(s, semantics=sem, phong=True), dict(color=col, z=z, winners=win), "oracle")
