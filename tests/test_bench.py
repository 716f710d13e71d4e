"""bench.py's command line: a plain run, --full and --dump-outputs.

CPU: the dump writer (float32 arrays, the seeded sample of a large frame) and
the argument rules.  GPU: one small plain run of bench.py itself, its result
line and its dumped frame against the oracle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(h, w, seed):
    import torch
    rng = np.random.default_rng(seed)
    c = rng.integers(-2**31, 2**31, (h, w), dtype=np.int64).astype(np.int32)
    z = rng.uniform(-2, 2, (h, w)).astype(np.float32)
    return c, z, torch.from_numpy(c), torch.from_numpy(z)


def test_dump_small_frame_is_whole(tmp_path):
    c, z, tc, tz = _frame(37, 53, 1)
    bench.dump_outputs(str(tmp_path / "d"), tc, tz)
    dc = np.load(tmp_path / "d" / "color.npy")
    dz = np.load(tmp_path / "d" / "z.npy")
    assert dc.dtype == np.float32 and dz.dtype == np.float32
    assert dc.shape == (37, 53, 4) and dz.shape == (37, 53)
    assert (dc.astype(np.uint8) == c.view(np.uint8).reshape(37, 53, 4)).all()
    assert (dz.view(np.uint32) == z.view(np.uint32)).all()


def test_dump_large_frame_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 1000)
    c, z, tc, tz = _frame(64, 48, 2)
    bench.dump_outputs(str(tmp_path / "a"), tc, tz)
    bench.dump_outputs(str(tmp_path / "b"), tc, tz)
    ac, az = np.load(tmp_path / "a" / "color.npy"), np.load(tmp_path / "a" / "z.npy")
    assert ac.shape == (1000, 4) and az.shape == (1000,)
    assert ac.dtype == np.float32 and az.dtype == np.float32
    assert (ac == np.load(tmp_path / "b" / "color.npy")).all()
    assert (az.view(np.uint32) == np.load(tmp_path / "b" / "z.npy").view(np.uint32)).all()
    # the same pixels of both planes, all taken from the frame
    idx = np.random.default_rng(0).integers(0, 64 * 48, size=1000)
    assert (az.view(np.uint32) == z.reshape(-1)[idx].view(np.uint32)).all()
    assert (ac.astype(np.uint8) == c.reshape(-1)[idx].view(np.uint8).reshape(-1, 4)).all()


def test_dump_stays_within_64_mb():
    assert bench.DUMP_MAX_PIXELS * (4 * 4 + 4) + 2 * 128 <= 64 * 10**6


def test_check_needs_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--check", "1"])
    with pytest.raises(SystemExit) as e:
        bench.parse()
    assert e.value.code == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--check", "1", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.check == 1 and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert not bench.parse().full


@pytest.mark.gpu
def test_plain_run_line_and_dump(gpu, tmp_path):
    """A plain run does the timed frames only; its dump is the oracle's frame."""
    import oracle as O
    from prk import scenes
    W, H, T, steps = 160, 96, 1500, 3
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", "1", "--width", str(W), "--height", str(H), "--tris", str(T), "--seed", "5",
                          "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    d = json.loads(run.stdout.strip().splitlines()[-1])
    assert d["steps"] == steps and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(W * H / (d["ms_per_step"] * 1e-3) / 1e6)
    assert d["cpu_baseline"] is None and d["ms_kernels_serial"] is None and d["ms_download"] is None
    assert "check" not in d and "valu" not in d["roofline"]
    s = scenes.random_soup(T, W, H, radius=16.0, seed=5, textured=True)
    oc, oz, _, _ = O.render(s, winners=False)
    dc, dz = np.load(tmp_path / "out" / "color.npy"), np.load(tmp_path / "out" / "z.npy")
    assert dc.dtype == np.float32 and dz.dtype == np.float32
    assert (dz.view(np.uint32) == oz.view(np.uint32)).all()
    assert (dc.astype(np.uint8) == np.ascontiguousarray(oc).view(np.uint8).reshape(H, W, 4)).all()
