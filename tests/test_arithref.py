"""CPU tests of tests/arithref.py, the host references tests/test_gpu_arith.py
holds the kernels' arithmetic primitives to: its two routes to a quotient and
a root agree, its input sets hold the in-range counts the GPU test's
fast-path conditions rely on, its conversion and select rules equal what an
x86 compiler's casts and SSE intrinsics do, and prk_selftest_ops refuses bad
arguments and fails loudly without a GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import arithref as A
import prk
from prk import abi


def test_two_routes_agree():
    for name, (x, d) in A.div_sets().items():
        assert A.same_words(A.div_ref(x, d), A.div_ref64(x, d)).size == 0, name
    x = A.sqrt_set()
    assert A.same_words(A.sqrt_ref(x), A.sqrt_ref64(x)).size == 0


def test_sets_hold_the_in_range_counts():
    sets = A.div_sets()
    n_in = sum(int(A.div_in_range([x], d).sum()) for x, d in sets.values())
    assert n_in >= 1 << 16  # whole fast-path waves of arrangement (a)
    assert A.div_in_range([sets["fast_range"][0]], sets["fast_range"][1]).all()
    for name, (x, d) in sets.items():  # three numerators: rotations of x
        assert A.div_in_range([x, np.roll(x, 1), np.roll(x, 2)], d).sum() >= (1 << 16 if name == "fast_range" else 0)
    x, y, z = A.norm_set()
    ok = A.norm_in_range(x, y, z)
    assert ok.sum() >= 1 << 14 and (~ok).sum() >= 1 << 14
    d = A.sq_len(x, y, z)
    for bound in (2.0 ** -64, 2.0 ** 62):  # squared lengths on both sides of each bound
        assert (d < np.float32(bound)).sum() > 1000 and (d > np.float32(bound)).sum() > 1000
    # quotients that are denormal or overflow, and denormal operands, are there
    x, d = sets["extreme_quotient"]
    q = A.floats(A.div_ref(x, d))
    assert (np.isinf(q)).sum() > 1000 and ((q != 0) & (np.abs(q) < np.float32(2.0 ** -126))).sum() > 1000
    x, d = sets["all_exponents"]
    assert (((x >> 23) & 0xFF) == 0).sum() > 100 and (((d >> 23) & 0xFF) == 0).sum() > 100


X86_CHECK = r"""
#include <emmintrin.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
int main(void) {
    uint32_t w, v;
    while (scanf("%x %x", &w, &v) == 2) {
        float f, g;
        volatile float vf;
        memcpy(&f, &w, 4);
        memcpy(&g, &v, 4);
        vf = f;
        int32_t t = _mm_cvttss_si32(_mm_set_ss(vf));
        int32_t rs = _mm_cvttss_si32(_mm_set_ss(roundf(vf)));
        uint32_t ru = (uint32_t)_mm_cvttss_si64(_mm_set_ss(roundf(vf)));
        int32_t ne = _mm_cvtsi128_si32(_mm_cvtps_epi32(_mm_set1_ps(vf)));
        float mn = _mm_cvtss_f32(_mm_min_ps(_mm_set1_ps(f), _mm_set1_ps(g)));
        float mx = _mm_cvtss_f32(_mm_max_ps(_mm_set1_ps(f), _mm_set1_ps(g)));
        uint32_t a, b;
        memcpy(&a, &mn, 4);
        memcpy(&b, &mx, 4);
        printf("%08x %08x %08x %08x %08x %08x\n", (uint32_t)t, (uint32_t)rs, ru, (uint32_t)ne, a, b);
    }
    return 0;
}
"""


def test_conversions_equal_x86(tmp_path):
    """The conversion, MINPS and MAXPS references against the instructions
    themselves (cvttss2si, its 64-bit form for the unsigned cast, cvtps2dq,
    minps, maxps) on the conversion set and on every pair of specials."""
    src, exe = tmp_path / "x86_check.c", tmp_path / "x86_check"
    src.write_text(X86_CHECK)
    r = subprocess.run(["gcc", "-O2", "-msse2", "-o", str(exe), str(src), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cv = A.conversion_set()
    S = A.specials()
    a, b = A._cross(S, S)
    a, b = np.concatenate([cv, a]), np.concatenate([cv[::-1], b])
    text = "".join("%08x %08x\n" % (x, y) for x, y in zip(a.tolist(), b.tolist()))
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0
    got = np.array([[int(t, 16) for t in line.split()] for line in run.stdout.splitlines()], np.uint64).astype(np.uint32)
    assert got.shape == (a.size, 6)
    for k, ref in enumerate((A.cvtt_s32_ref(a), A.round_s32_ref(a), A.round_u32_ref(a), A.cvt_rne_s32_ref(a),
                             A.minps_ref(a, b), A.maxps_ref(a, b))):
        bad = A.same_words(got[:, k], ref)
        assert bad.size == 0, (k, hex(a[bad[0]]), hex(b[bad[0]]), hex(got[bad[0], k]), hex(ref[bad[0]]))
    # the rules the issue names
    assert A.maxps_ref(A.words([0.0]), A.words([-0.0]))[0] == 0x80000000
    assert A.round_s32_ref(A.words([0.5, -0.5, 2.5, 0.49999997])).tolist() == [1, 0xFFFFFFFF, 3, 0]
    assert A.cvt_rne_s32_ref(A.words([0.5, 1.5, 2.5, -0.5])).tolist() == [0, 2, 2, 0]


def test_mul16_and_u8_unit_references():
    y, p = A.mul16_set()
    r = A.mul16_trick_ref(y, p)
    small = (y < 0x8000) & (p < 0x8000) & (y.astype(np.uint64) * p < (1 << 31))
    assert small.sum() > 20 and (r[small] == (y[small] * p[small])).all()  # a plain product where it fits
    assert A.mul16_trick_ref([0x8000], [2])[0] == 0xFFFF0000  # the signed high half
    k = np.arange(256)
    assert A.floats(A.u8_unit_ref(k))[255] == 1.0 and A.u8_unit_ref(k)[0] == 0


def test_selftest_ops_argument_errors():
    L = prk.lib()
    w = np.zeros(64, np.uint32)
    p = C.c_void_p(w.ctypes.data)
    args = lambda *a: L.prk_selftest_ops(*a)  # noqa: E731
    assert args(0, -1, 64, p, p, p, p, p, None, None, None) == abi.PRK_ERR_ARG
    assert args(0, abi.PRK_OP_COUNT, 64, p, p, p, p, p, None, None, None) == abi.PRK_ERR_ARG
    assert args(-1, abi.PRK_OP_DIV, 64, p, p, None, None, p, None, None, None) == abi.PRK_ERR_ARG
    assert args(0, abi.PRK_OP_DIV, 64, p, None, None, None, p, None, None, None) == abi.PRK_ERR_ARG  # b missing
    assert args(0, abi.PRK_OP_DIV_ALL3, 64, p, p, p, None, p, None, None, None) == abi.PRK_ERR_ARG  # d missing
    assert args(0, abi.PRK_OP_DIV, 64, p, p, None, None, None, None, None, None) == abi.PRK_ERR_ARG  # no out0
    assert args(0, abi.PRK_OP_DIV, (1 << 24) + 1, p, p, None, None, p, None, None, None) == abi.PRK_ERR_ARG
    assert L.prk_selftest_div_paths(0, 64, 1, None, None) == abi.PRK_ERR_ARG


@pytest.mark.skipif(os.environ.get("PRK_EXPECT_GPU") == "1", reason="GPU box")
def test_selftest_ops_fails_loudly_without_gpu():
    if prk.device_count() > 0:
        pytest.skip("a GPU is visible")
    w = np.zeros(64, np.uint32)
    with pytest.raises(prk.PrkError) as e:
        prk.selftest_ops(abi.PRK_OP_DIV, w, w)
    assert e.value.code == abi.PRK_ERR_DEVICE
    with pytest.raises(prk.PrkError) as e:
        prk.selftest_div_paths(n=64)
    assert e.value.code == abi.PRK_ERR_DEVICE
