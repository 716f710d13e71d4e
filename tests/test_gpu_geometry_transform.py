"""GPU tests: prk_geometry_alloc / prk_geometry_transform /
prk_geometry_download -- runs of a resident geometry's triangles written
through 3x4 matrices into another resident geometry (include/prk.h).

Expected values come from tests/xform_ref.py, the header's expression in
numpy float32 op by op, and are compared through a uint32 view: every word of
every array.  Frames are compared on bits too (same_frame / the parity tests'
compare).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import prk
import xform_ref as X
from prk import abi, scenes
from test_gpu_edge_lists import AVX, SC_PHONG, same_frame
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

NAMES = ("vertices", "colors", "normals", "uvs")


def same_arrays(got, want, label):
    for k in range(4):
        assert (got[k] is None) == (want[k] is None), "%s: %s present %r, expected %r" % (
            label, NAMES[k], got[k] is not None, want[k] is not None)
        if want[k] is None:
            continue
        assert got[k].shape == want[k].shape, "%s: %s shape %r, expected %r" % (label, NAMES[k], got[k].shape,
                                                                                 want[k].shape)
        bad = got[k].view(np.uint32) != want[k].view(np.uint32)
        assert not bad.any(), "%s: %s differs in %d words, first at vertex %d" % (
            label, NAMES[k], bad.sum(), np.nonzero(bad.any(1))[0][0])


class Ctx:
    """A renderer with a scene's target, camera and texture."""

    def __init__(self, s, textured=True):
        self.s = s
        self.r = r = prk.Renderer()
        r.target_alloc(s.width, s.height)
        r.clear()
        r.set_debug(True)
        r.set_camera(s.prk_transform(), s.prk_lights())
        self.tex = r.texture(s.texture) if textured else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.close()

    def draw(self, g, n, mode=AVX, per=1, first=0, P=None):
        self.r.draw(mode[0], g, n, first_tri=first, P=P, bitmap=self.tex, phong=mode[1], tris_per_object=per)

    def done(self):
        self.r.complete_all_work()
        c, z = self.r.download()
        return c, z, self.r.winners()


def small_soup(n=40, W=64, H=64, seed=5, radius=10):
    return scenes.random_soup(n, W, H, radius=radius, seed=seed, centroid_margin=0)


def arrays_of(s):
    return s.vertices, s.colors, s.normals, s.uvs


# ---- 1. runs, bit for bit ------------------------------------------------------------------------------------------------
# (src_first_tri, tri_count, dst_first_tri, xform): lengths 1, 2, 5, 63, 64, 65 and 0, out of destination order; triangles
# 68..74 of dst are written by no run; source triangles 50..54 go out three times through three matrices
RUNS = np.array([[137, 63, 90, 3],   # (ends on src's last triangle)
                 [0, 0, 500, 0],     # no triangles: skipped, dst does not grow to 500
                 [0, 1, 65, 1],
                 [50, 5, 85, 2],
                 [10, 65, 0, 0],
                 [30, 64, 153, 1],
                 [50, 5, 75, 0],
                 [100, 2, 66, 2],
                 [50, 5, 80, 1]], np.uint32)


@pytest.fixture(scope="module")
def r(gpu):
    rr = prk.Renderer()
    yield rr
    rr.close()


def test_runs_bit_for_bit(r):
    rng = np.random.default_rng(1)
    src = X.random_arrays(rng, 200)
    xf = X.random_values(rng, (5, 3, 4))
    g = r.geometry(*src)
    d = r.geometry_alloc()
    assert r.geometry_info(d) == (0, (False, False, False, False))
    r.geometry_transform(g, d, RUNS, xf)
    want = X.apply_runs(src, (None,) * 4, RUNS, xf)
    assert want[0].shape[0] == 3 * 217 and r.geometry_info(d) == (3 * 217, (True,) * 4)
    got = r.geometry_download(d)
    same_arrays(got, want, "first call")
    for k in range(4):
        assert not got[k][3 * 68:3 * 75].view(np.uint32).any(), "the gap of %s is not zero" % NAMES[k]
    # a second call over triangles 60..79: the rest stays as it was
    again = np.array([[20, 20, 60, 4]], np.uint32)
    r.geometry_transform(g, d, again, xf)
    want2 = X.apply_runs(src, want, again, xf)
    got2 = r.geometry_download(d)
    same_arrays(got2, want2, "second call")
    keep = np.r_[0:3 * 60, 3 * 80:3 * 217]
    same_arrays(tuple(a[keep] for a in got2), tuple(a[keep] for a in got), "outside the second call")
    # a part of the geometry, positions alone
    part = r.geometry_download(d, first_tri=64, tri_count=30, arrays=(True, False, False, False))
    same_arrays(part, (want2[0][3 * 64:3 * 94], None, None, None), "partial download")


def test_long_run_and_many_runs(r):
    """A run longer than several workgroups' triangles beside runs of 1: the
    same words (the search finds a run's first, inner and last triangle)."""
    rng = np.random.default_rng(2)
    src = X.random_arrays(rng, 700)
    xf = X.random_values(rng, (37, 3, 4))
    ones = np.stack([np.arange(300), np.ones(300), 1000 - np.arange(300), np.arange(300) % 37], 1)
    runs = np.concatenate([[[0, 700, 0, 36]], ones]).astype(np.uint32)
    g, d = r.geometry(*src), r.geometry_alloc()
    r.geometry_transform(g, d, runs, xf)
    same_arrays(r.geometry_download(d), X.apply_runs(src, (None,) * 4, runs, xf), "700 + 300 x 1")


# ---- 2. identity -----------------------------------------------------------------------------------------------------
def test_identity(r):
    rng = np.random.default_rng(3)
    src = X.random_arrays(rng, 70)
    g, d = r.geometry(*src), r.geometry_alloc()
    r.geometry_transform(g, d, [[0, 70, 0, 0]], X.translation((0.0, 0.0, 0.0))[None])
    got = r.geometry_download(d)
    assert (src[0] == 0).any() and np.signbit(src[0][src[0] == 0]).any()  # (-0.0 is among the inputs)
    assert np.array_equal(got[0], src[0]) and np.array_equal(got[2], src[2])  # ==: -0.0 may come out as +0.0
    assert np.array_equal(got[1].view(np.uint32), src[1].view(np.uint32))
    assert np.array_equal(got[3].view(np.uint32), src[3].view(np.uint32))


# ---- 3. absent arrays ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lacks", ["colors", "uvs"])
def test_absent_arrays(r, lacks):
    rng = np.random.default_rng(4)
    src = X.random_arrays(rng, 30, colors=lacks != "colors", uvs=lacks != "uvs")
    xf = X.random_values(rng, (2, 3, 4))
    runs = np.array([[0, 30, 4, 1]], np.uint32)
    g, d = r.geometry(*src), r.geometry_alloc()
    r.geometry_transform(g, d, runs, xf)
    got = r.geometry_download(d)
    assert got[NAMES.index(lacks)] is None
    same_arrays(got, X.apply_runs(src, (None,) * 4, runs, xf), "fresh dst, src without " + lacks)
    # a dst that has the array keeps it: untouched where it was, zeros where dst grew
    had = X.random_arrays(rng, 20)
    d2 = r.geometry(*had)
    r.geometry_transform(g, d2, runs, xf)
    got2 = r.geometry_download(d2)
    want2 = X.apply_runs(src, had, runs, xf)
    k = NAMES.index(lacks)
    assert np.array_equal(want2[k][:60].view(np.uint32), had[k].view(np.uint32)) and not want2[k][60:].any()
    same_arrays(got2, want2, "dst with %s, src without" % lacks)


# ---- 4. growth under a recorded draw -------------------------------------------------------------------------------------
def test_growth_repoints_recorded_draws(gpu):
    s = small_soup(50)
    first = tuple(a[:30] for a in arrays_of(s))
    src = tuple(a[30:] for a in arrays_of(s))
    M = X.rotation_yx(10.0, -5.0, (0.05, -0.1, 0.1))
    runs = np.array([[0, 40, 50, 0]], np.uint32)
    with Ctx(s) as f:
        d = f.r.geometry(*first)
        g = f.r.geometry(*src)
        f.draw(d, 10)  # recorded, not flushed: the transform below moves dst's buffers
        f.r.geometry_transform(g, d, runs, M[None])
        got = f.r.geometry_download(d)
        want = X.apply_runs(src, first, runs, M[None])
        same_arrays(got, want, "grown dst")
        same_arrays(tuple(a[:30] for a in got), first, "the first 10 triangles")
        f.draw(d, 40, first=50)
        a = f.done()
        f.r.clear()
        h = f.r.geometry(*want)
        f.draw(h, 10)
        f.draw(h, 40, first=50)
        b = f.done()
    assert (a[2] >= 0).any() and (a[2] >= 10).any()
    same_frame(a, b, "grown dst against prk_geometry_create of the same data")


# ---- 5. order without host waits -----------------------------------------------------------------------------------------
def test_two_transforms_two_frames_no_wait(gpu):
    s = small_soup(40)
    src = arrays_of(s)
    A = X.rotation_yx(8.0, 4.0, (0.1, 0.0, 0.0))
    B = X.rotation_yx(-12.0, 6.0, (-0.15, 0.1, 0.2))
    run = np.array([[0, 40, 0, 0]], np.uint32)
    with Ctx(s) as f:
        g, d = f.r.geometry(*src), f.r.geometry_alloc()
        frames = []
        for M in (A, B):  # (no synchronize anywhere: the target is downloaded after each flush)
            f.r.geometry_transform(g, d, run, M[None])
            f.draw(d, 40)
            frames.append(f.done())
            f.r.clear()
        for M, got, name in ((A, frames[0], "A"), (B, frames[1], "B")):
            h = f.r.geometry(*X.apply(M, src))
            f.draw(h, 40)
            want = f.done()
            f.r.clear()
            assert (want[2] >= 0).any()
            same_frame(got, want, "frame of device transform " + name)
    assert (frames[0][1].view(np.uint32) != frames[1][1].view(np.uint32)).any()  # (A and B really differ)


# ---- 6. frame parity against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [AVX, SC_PHONG], ids=["avx_textured", "scalar_phong"])
def test_rotated_sphere_against_the_oracle(gpu, mode):
    V, Cc, N, UV = prk.construct_sphere()
    assert V.shape[0] == 3 * 2208
    base = scenes.random_soup(1, 128, 128, seed=0)
    M = X.rotation_yx(30.0, 30.0, (0.0, 0.0, 2.0))  # (the parity tests' sphere sits at P = (0, 0, 2))
    src = (V.copy(), Cc.copy(), N.copy(), UV.copy())
    hv, hc, hn, huv = X.apply(M, src)
    s = scenes.Scene(128, 128, hv, hc, hn, huv, base.transform, scenes.LIGHTS_ONE, scenes.AMBIENT_ONE,
                     base.texture if mode[2] else None, name="rotated sphere")
    with Ctx(s, textured=mode[2]) as f:
        g, d = f.r.geometry(*src), f.r.geometry_alloc()
        f.r.geometry_transform(g, d, [[0, 2208, 0, 0]], M[None])
        f.draw(d, 2208, mode, per=2208)
        c, z, w = f.done()
    assert (w >= 0).sum() > 500
    o = O.render(s, semantics=mode[0], phong=mode[1], tris_per_object=2208)
    compare((c, z, w, None), o, label="rotated sphere")


# ---- 7. records ----------------------------------------------------------------------------------------------------------
def test_records_of_the_transformed_geometry(gpu):
    s = small_soup(64, 128, 96, seed=9, radius=16)
    src = arrays_of(s)
    M = X.rotation_yx(6.0, -9.0, (0.2, 0.1, -0.1))
    with Ctx(s) as f:
        g, d = f.r.geometry(*src), f.r.geometry_alloc()
        f.r.geometry_transform(g, d, [[0, 64, 0, 0]], M[None])
        rec = f.r.records_from_geometry(d, 64, setup=3, tris_per_object=8)
        h = f.r.geometry(*X.apply(M, src))
        ref = f.r.records_from_geometry(h, 64, setup=3, tris_per_object=8)
        assert rec.list_count == ref.list_count == 8 and ref.total > 0
        assert np.array_equal(rec.counts(), ref.counts())
        assert np.array_equal(rec.download(), ref.download())


# ---- 8. instancing -------------------------------------------------------------------------------------------------------
def test_instancing(gpu):
    s = small_soup(16, 64, 64, seed=11, radius=6)
    src = arrays_of(s)
    rng = np.random.default_rng(12)
    T = np.ascontiguousarray(rng.uniform(-0.4, 0.4, (12, 3)) * (1, 1, 0.5), np.float32)
    xf = np.stack([X.translation(t) for t in T])
    # identity + translation is the draw's own v + P, bit for bit, for these inputs (no -0.0 among them)
    assert not np.signbit(src[0][src[0] == 0]).any() and not np.signbit(T[T == 0]).any()
    for t, M in zip(T, xf):
        assert np.array_equal(X.positions(M, src[0]).view(np.uint32), (src[0] + t).view(np.uint32))
        assert np.array_equal(X.normals(M, src[2]), src[2])
    runs = np.stack([np.zeros(12), np.full(12, 16), 16 * np.arange(12), np.arange(12)], 1).astype(np.uint32)
    with Ctx(s) as f:
        g, d = f.r.geometry(*src), f.r.geometry_alloc()
        f.r.geometry_transform(g, d, runs, xf)
        f.draw(d, 12 * 16, per=16)
        a = f.done()
        f.r.clear()
        for t in T:
            f.draw(g, 16, per=16, P=tuple(float(x) for x in t))
        b = f.done()
    assert len(np.unique(a[2][a[2] >= 0] // 16)) >= 6  # (several of the instances are on screen)
    same_frame(a, b, "12 instances in one draw against 12 draws with P")


# ---- 9. refused calls ----------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(gpu):
    rng = np.random.default_rng(13)
    src = X.random_arrays(rng, 20)
    xf = X.random_values(rng, (2, 3, 4))
    s = small_soup(1)
    with Ctx(s) as f:
        r = f.r
        g, d = r.geometry(*src), r.geometry_alloc()
        r.geometry_transform(g, d, [[0, 20, 0, 0]], xf)
        before = r.geometry_download(d)
        _, _, zp, W, H, _, _ = r.target()
        wrapped = r.geometry_device(zp, None, None, None, 30)  # (any device memory: the call must not touch it)
        L, h = r._L, r._h
        runs = np.array([[0, 20, 0, 1]], np.uint32)
        rp = C.cast(runs.ctypes.data, C.POINTER(abi.PrkXformRun))
        xp = C.cast(xf.ctypes.data, C.POINTER(abi.PrkXform))
        limit_tri = 0xFFFFFFF0 // 3
        cases = [
            ("null context", lambda: L.prk_geometry_transform(None, g, d, rp, 1, xp, 2)),
            ("src < 0", lambda: L.prk_geometry_transform(h, -1, d, rp, 1, xp, 2)),
            ("src past the handles", lambda: L.prk_geometry_transform(h, 999, d, rp, 1, xp, 2)),
            ("dst < 0", lambda: L.prk_geometry_transform(h, g, -1, rp, 1, xp, 2)),
            ("dst past the handles", lambda: L.prk_geometry_transform(h, g, 999, rp, 1, xp, 2)),
            ("src == dst", lambda: L.prk_geometry_transform(h, d, d, rp, 1, xp, 2)),
            ("wrapped dst", lambda: L.prk_geometry_transform(h, g, wrapped, rp, 1, xp, 2)),
            ("null runs", lambda: L.prk_geometry_transform(h, g, d, None, 1, xp, 2)),
            ("null xforms", lambda: L.prk_geometry_transform(h, g, d, rp, 1, None, 2)),
        ]
        for label, bad in (("xform == xform_count", [[0, 20, 0, 2]]), ("source range past src", [[1, 20, 0, 0]]),
                           ("source start past src", [[21, 1, 0, 0]]),
                           ("destination past the vertex limit", [[0, 1, limit_tri, 0]]),
                           ("a bad run after a good one", [[0, 5, 0, 0], [0, 5, 5, 7]])):
            b = np.array(bad, np.uint32)
            cases.append((label, lambda b=b: L.prk_geometry_transform(
                h, g, d, C.cast(b.ctypes.data, C.POINTER(abi.PrkXformRun)), b.shape[0], xp, 2)))
        for label, call in cases:
            assert call() == abi.PRK_ERR_ARG, label
            assert r.geometry_info(d) == (60, (True,) * 4), label
            same_arrays(r.geometry_download(d), before, "after the refused call: " + label)
        # the last triangle below the limit is accepted as far as the arguments go (no test allocates it);
        # downloads: ranges and absent arrays
        v = np.empty((60, 3), np.float32)
        assert L.prk_geometry_download(h, d, 0, 63, v.ctypes.data, None, None, None) == abi.PRK_ERR_ARG
        assert L.prk_geometry_download(h, d, 3, 60, v.ctypes.data, None, None, None) == abi.PRK_ERR_ARG
        assert L.prk_geometry_download(h, d, 1, 3, v.ctypes.data, None, None, None) == abi.PRK_ERR_ARG
        assert L.prk_geometry_download(h, d, 0, 4, v.ctypes.data, None, None, None) == abi.PRK_ERR_ARG
        assert L.prk_geometry_download(h, 999, 0, 3, v.ctypes.data, None, None, None) == abi.PRK_ERR_ARG
        assert L.prk_geometry_download(None, d, 0, 3, v.ctypes.data, None, None, None) == abi.PRK_ERR_ARG
        nocol = r.geometry(src[0], None, src[2], src[3])
        c4 = np.empty((60, 4), np.float32)
        assert L.prk_geometry_download(h, nocol, 0, 60, None, c4.ctypes.data, None, None) == abi.PRK_ERR_ARG
        assert L.prk_geometry_download(h, nocol, 0, 60, v.ctypes.data, None, None, None) == abi.PRK_OK
        assert np.array_equal(v.view(np.uint32), src[0].view(np.uint32))
        assert L.prk_geometry_alloc(h, None) == abi.PRK_ERR_ARG and L.prk_geometry_alloc(None, None) == abi.PRK_ERR_ARG


# ---- a source of caller device pointers at float alignment ---------------------------------------------------------------
def test_wrapped_source_at_float_alignment(gpu):
    """A prk_geometry_wrap_device source whose arrays start 4 bytes past a
    16-byte boundary (the target's z-buffer, uploaded with known words)."""
    rng = np.random.default_rng(14)
    s = small_soup(1)
    src = X.random_arrays(rng, 9)
    z = np.zeros(64 * 64, np.float32)
    at = (1, 101, 301, 501)  # float offsets of vertices, colors, normals, uvs: all odd
    for a, o in zip(src, at):
        z[o:o + a.size] = a.reshape(-1)
    xf = X.random_values(rng, (1, 3, 4))
    with Ctx(s) as f:
        f.r.upload(np.zeros((64, 64), np.uint32), z.reshape(64, 64))
        zp = f.r.target()[2]
        assert zp % 16 == 0
        g = f.r.geometry_device(*[zp + 4 * o for o in at], 27)
        d = f.r.geometry_alloc()
        f.r.synchronize()
        f.r.geometry_transform(g, d, [[0, 9, 2, 0]], xf)
        same_arrays(f.r.geometry_download(d), X.apply_runs(src, (None,) * 4, [[0, 9, 2, 0]], xf), "wrapped source")
