"""The hostile triangles the tile binning's bound is held to
(tests/test_binref.py on the host, tests/test_gpu_bins.py on the device): one
scene of a 64 x 16064 frame (census.TALL_W, TALL_H), built class by class in
screen space and unprojected as prk.scenes does.  hostile() returns the scene
and, per class, the indices of its triangles."""
import numpy as np

import census
from prk import scenes

W, H = census.TALL_W, census.TALL_H
BANDS = [(0, 128), (128, 300), (300, 301), (37, 91)]
TILES = [(8, 8), (32, 8), (256, 8), (512, 8), (128, 64)]
P_OFF = (0.375, -0.21875, 0.0625)  # the non-zero object position


def screen_scene(s, z, seed, P=(0.0, 0.0, 0.0), W=W, H=H):
    """Triangles given in screen space (s [n, 3, 2], z [n, 3]) of a W x H
    frame under prk.scenes' camera, wound front-facing; no texture."""
    rng = np.random.default_rng(seed)
    cam = scenes.default_camera(W, H)
    s = np.array(s, np.float64)
    n = s.shape[0]
    e1, e2 = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]
    flip = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0
    s[flip, 1], s[flip, 2] = s[flip, 2].copy(), s[flip, 1].copy()
    z = np.array(z, np.float64)
    z[flip, 1], z[flip, 2] = z[flip, 2].copy(), z[flip, 1].copy()
    x, y = scenes.unproject(s[..., 0], s[..., 1], z, cam)
    verts = (np.stack([x, y, z], -1).reshape(-1, 3) - np.array(P)).astype(np.float32)
    nrm = rng.normal(size=(3 * n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cols = rng.uniform(0.0, 1.0, (3 * n, 4)).astype(np.float32)
    cols[:, 3] = 1.0
    return scenes.Scene(W, H, verts, cols, nrm.astype(np.float32), rng.uniform(0.0, 1.0, (3 * n, 2)).astype(np.float32),
                        cam, scenes.LIGHTS_ONE, scenes.AMBIENT_ONE, None, P, "hostile")


def _classes(rng):
    """{class: (screen triangles [n, 3, 2], z [n, 3] or None)}."""
    out = {}
    # 2000 - 16000 rows tall, inside the frame's columns
    t = []
    for h in (2000, 4500, 9000, 16000):
        y0 = rng.uniform(5, H - h - 5)
        t.append([[rng.uniform(2, 20), y0], [rng.uniform(40, 62), y0 + rng.uniform(0.3, 0.7) * h], [rng.uniform(5, 60), y0 + h]])
        t.append([[rng.uniform(40, 62), y0 + 3], [rng.uniform(2, 20), y0 + h - 7.5], [rng.uniform(-30, 90), y0 + 0.5 * h]])
    out["tall"] = (t, None)
    # one or two vertices far left / right of the frame, the others inside
    for mag in (1e4, 1e5, 1e6, 1e7):
        t = []
        for sign in (-1, 1):
            for far in (1, 2):
                for h in (3.0, 240.0, 3100.0, 15000.0):
                    y0 = rng.uniform(10, H - h - 10)
                    v = [[rng.uniform(1, 63), y0 + rng.uniform(0, 1)], [rng.uniform(1, 63), y0 + h * rng.uniform(0.4, 0.6)],
                         [rng.uniform(1, 63), y0 + h]]
                    for k in rng.permutation(3)[:far]:
                        v[k][0] = sign * mag * rng.uniform(0.8, 1.2) + (W if sign > 0 else 0)
                    t.append(v)
        out["far_%g" % mag] = (t, None)
    # edges within a row of horizontal with |dx| of 1e5
    t = []
    for sign in (-1, 1):
        for dy in (0.02, 0.4, 0.97):
            for h in (1.5, 60.0):
                y0 = rng.uniform(100, H - 200)
                t.append([[rng.uniform(2, 62), y0], [sign * 1e5 + rng.uniform(2, 62), y0 + dy], [rng.uniform(2, 62), y0 + h]])
    out["flat"] = (t, None)
    # D - z just above 0.2: the largest magnification ProjectVertex gives
    t, z = [], []
    for d in (0.2000001, 0.2001, 0.21, 0.25):
        for h in (12.0, 900.0):
            y0 = rng.uniform(10, H - h - 10)
            t.append([[rng.uniform(-40, 20), y0], [rng.uniform(40, 110), y0 + 0.5 * h], [rng.uniform(0, 64), y0 + h]])
            z.append([4.0 - d, 4.0 - d * rng.uniform(1.0, 1.5), 4.0 - d * rng.uniform(1.0, 3.0)])
    out["magnified"] = (t, z)
    # the largest x within a pixel of W, W - 0.5 and 0; bottoms on the last row of a tile and of a band
    t = []
    bottoms = [8.0, 64.0, 91.0, 128.0, 300.0, 301.0, 96.0, float(H)]
    for i, xm in enumerate([W - 1.0, W - 0.75, W - 0.5, W - 0.5 + 2 ** -18, W - 0.5 - 2 ** -18, W - 0.25, float(W),
                            W + 0.25, W + 1.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0]):
        for rep in range(2):
            yb = bottoms[(2 * i + rep) % len(bottoms)] - (0.0 if rep else 0.25)
            t.append([[xm - rng.uniform(6, 30), yb - rng.uniform(9, 20)], [xm, yb - rng.uniform(0, 5)],
                      [xm - rng.uniform(0, 4), yb]])
    out["xmax"] = (t, None)
    # triangles that straddle a band edge by under a row
    t = []
    for e in sorted({r for b in BANDS for r in b}):
        for top, bot in ((-0.3, 0.3), (-0.6, 0.05), (-0.05, 0.8), (-7.5, 0.4), (-0.4, 9.2)):
            x0 = rng.uniform(-10, 50)
            t.append([[x0, e + top], [x0 + rng.uniform(8, 40), e + 0.5 * (top + bot)], [x0 + rng.uniform(0, 8), e + bot]])
    out["band_edge"] = (t, None)
    return {k: (np.array(s), None if z is None else np.array(z)) for k, (s, z) in out.items()}


def hostile(P=(0.0, 0.0, 0.0), seed=7):
    """(scene, {class: triangle indices}).  The classes above, then
    scenes.slivers and a small soup with scenes.with_ties' duplicates."""
    rng = np.random.default_rng(seed)
    parts, cls, n0 = [], {}, 0
    for name, (s, z) in _classes(rng).items():
        z = rng.uniform(-0.8, 0.8, (s.shape[0], 1)) + rng.uniform(-0.1, 0.1, (s.shape[0], 3)) if z is None else z
        parts.append(screen_scene(s, z, seed + len(parts), P))
        cls[name] = np.arange(n0, n0 + s.shape[0])
        n0 += s.shape[0]
    for name, sc in (("slivers", scenes.slivers(40, W, H, seed=seed, textured=False)),
                     ("ties", scenes.with_ties(scenes.random_soup(40, W, 600, radius=30, seed=seed, textured=False),
                                               frac=0.5, seed=seed))):
        sc.vertices = (sc.vertices.astype(np.float64) - np.array(P)).astype(np.float32)
        parts.append(sc)
        cls[name] = np.arange(n0, n0 + sc.tri_count)
        n0 += sc.tri_count
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])  # noqa: E731
    tex = scenes.random_texture(np.random.default_rng(seed), 64, 64)
    return scenes.Scene(W, H, cat("vertices"), cat("colors"), cat("normals"), cat("uvs"), scenes.default_camera(W, H),
                        scenes.LIGHTS_ONE, scenes.AMBIENT_ONE, tex, P, "hostile_P" if any(P) else "hostile"), cls
