"""Run the reference driver (oracle/_ref/ref_driver) on a prk.scenes.Scene —
TEST INFRASTRUCTURE ONLY; see build_ref.py for how the driver is made."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "cpu-renderer_amd"))
import build_ref  # noqa: E402
from prk import abi  # noqa: E402

MAGIC = 0x31464552
# the reference's ways of drawing an edge list, and the semantics of ours that
# restates each (include/projekt.h)
ENTRY_POINTS = {
    "DrawModelOptimized(RenderQueue)": (0, abi.PRK_SEM_AVX),
    "DrawModelOptimized(single thread)": (1, abi.PRK_SEM_AVX_ST),
    "DrawModel": (2, abi.PRK_SEM_SCALAR),
    "DrawModelOptimizedLines": (3, abi.PRK_SEM_AVX),
}


class ReferenceFailed(RuntimeError):
    """The verbatim reference did not survive the scene (crash, failed Assert
    or no end)."""


def driver(sanitize=False, patches=()):
    """Path of the built driver, or None."""
    p = build_ref.driver_path(sanitize, tuple(patches))
    return p if os.path.exists(p) else None


def write_scene(path, scene, entry, phong, tris_per_object=1, dump_edges=False):
    mode = ENTRY_POINTS[entry][0]
    tex = scene.texture
    head = np.zeros(16, np.int32)
    head[:11] = [0, scene.width, scene.height, scene.tri_count, tris_per_object, mode, int(bool(phong)),
                 tex.width if tex is not None else 0, tex.height if tex is not None else 0, len(scene.lights),
                 int(bool(dump_edges))]
    head.view(np.uint32)[0] = MAGIC
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()  # noqa: E731
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(f32(scene.P))
        f.write(f32(scene.transform))
        f.write(f32(scene.ambient))
        f.write(f32([list(p) + list(i) for p, i in scene.lights]))
        for a in (scene.vertices, scene.colors, scene.normals, scene.uvs):
            f.write(f32(a))
        if tex is not None:
            t = np.ascontiguousarray(tex.texels, np.uint32)
            assert t.shape == (tex.height + 1, tex.width) and not t[tex.height].any(), "texture needs its zeroed guard row"
            f.write(t.tobytes())


def render(scene, entry, phong, tris_per_object=1, dump_edges=False, sanitize=False, timeout=120, patches=()):
    """(colour u32[H,W], z f32[H,W], winners i32[H,W], info) as the reference
    drew the scene through `entry`.  info: objects_without_edges,
    undefined_pixels (pixels that change with the bytes around the texture)
    and, with dump_edges, edges u32[n,27] + next i32[n] of the first object
    after FillEdgeTable."""
    exe = driver(sanitize, patches)
    if exe is None:
        raise RuntimeError("reference driver not built (oracle/ref/build_ref.py)")
    H, W = scene.height, scene.width
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.bin")
        out = os.path.join(tmp, "out")
        write_scene(path, scene, entry, phong, tris_per_object, dump_edges)
        try:
            r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            raise ReferenceFailed("no end after %d s" % timeout)
        if r.returncode != 0:
            raise ReferenceFailed("exit status %d: %s" % (r.returncode, r.stderr.strip()[-2000:]))
        m = re.search(r"objects_without_edges=(\d+) undefined_pixels=(\d+)", r.stdout)
        info = dict(objects_without_edges=int(m.group(1)), undefined_pixels=int(m.group(2)))
        col = np.fromfile(out + ".color", np.uint32).reshape(H, W)
        z = np.fromfile(out + ".z", np.float32).reshape(H, W)
        win = np.fromfile(out + ".winners", np.int32).reshape(H, W)
        if dump_edges:
            e = np.fromfile(out + ".edges", np.uint32).reshape(-1, 28)
            info["edges"] = e[:, :27].copy()
            info["next"] = e[:, 27].view(np.int32).copy()
    return col, z, win, info


def construct_sphere():
    """ConstructSphere's output: vertices [n,3], colours [n,4], normals [n,3], uvs [n,2]."""
    exe = driver()
    if exe is None:
        raise RuntimeError("reference driver not built (oracle/ref/build_ref.py)")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out")
        subprocess.run([exe, "--sphere", out], check=True, capture_output=True, timeout=60)
        raw = np.fromfile(out + ".sphere", np.uint32)
    n = int(raw[0])
    f = raw[1:].view(np.float32)
    return (f[:3 * n].reshape(n, 3).copy(), f[3 * n:7 * n].reshape(n, 4).copy(),
            f[7 * n:10 * n].reshape(n, 3).copy(), f[10 * n:12 * n].reshape(n, 2).copy())
