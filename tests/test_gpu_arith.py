"""The kernels' arithmetic primitives (csrc/prk_device.h) on the GPU against
host references written from the definitions (tests/arithref.py): every word
equal bit for bit, a NaN where the reference has one.  prk_selftest_ops runs
element i on thread i, so 64 consecutive elements share a wave; div_all and
normalize_div choose their shared-reciprocal path per wave, and the tests
require that path exactly in the waves whose every element lies inside the
documented bounds -- in an order that packs such waves, in an order that
spoils every wave, and in the caller's order -- with the same words each time.

What these tests see and do not see, tried on mutated builds: a fast-range
bound moved by a binade, rintf for roundf, and maxps with swapped operands
each fail a test here.  div_fast without its last correction step does not:
on every input of these sets -- 10^4 quotients within 2^-24 ulp of a rounding
boundary among them -- the value before that step was already the host's
quotient.  That is an observation on these inputs, not a proof that the step
is redundant in range.

Not covered here: the Phong power and the colour pack, which are still inline
in k_shade (moving them into named functions changed k_shade's code).
"""
import numpy as np
import pytest

import arithref as A
import prk
from prk import abi

pytestmark = pytest.mark.gpu

ONE = int(A.words(np.float32(1.0))[0])


def check(got, want, label, *inputs):
    bad = A.same_words(got, want)
    assert bad.size == 0, "%s: %d of %d words differ; first at %d: inputs %s gpu %08x ref %08x" % (
        label, bad.size, len(want), bad[0], [hex(int(x[bad[0]])) for x in inputs], got[bad[0]], want[bad[0]])


def wave_all(in_range):
    """Per element: every element of its wave is in range."""
    n = in_range.size
    padded = np.concatenate([in_range, np.ones((-n) % A.WAVE, bool)]).reshape(-1, A.WAVE)
    return np.repeat(padded.all(1), A.WAVE)[:n]


def run_arranged(op, ins, in_range, refs, filler, label, min_fast):
    """One op over the three wave arrangements of the issue."""
    n = in_range.size
    # (c) the caller's own order
    outs_c = prk.selftest_ops(op, *ins)
    for k, r in enumerate(refs):
        check(outs_c[k], r, "%s own order out%d" % (label, k), *ins)
    assert (outs_c[3] == wave_all(in_range)).all(), label + ": own order, fast flag differs from the documented bounds"
    # (a) in-range elements in whole waves of their own
    idx, n_in = A.arrange_uniform(in_range)
    assert n_in >= min_fast
    outs_a = prk.selftest_ops(op, *[x[idx] for x in ins])
    assert (outs_a[3][:n_in] == 1).all(), label + ": an in-range wave left the fast path"
    assert (outs_a[3] == wave_all(in_range[idx])).all(), label + ": uniform order, fast flag differs from the bounds"
    for k, r in enumerate(refs):
        check(outs_a[k], r[idx], "%s uniform out%d" % (label, k), *[x[idx] for x in ins])
    # (b) an out-of-range element at the head of every wave
    total, pos, _ = A.arrange_mixed(n)
    mixed = [np.full(total, f, np.uint32) for f in filler]
    for m, x in zip(mixed, ins):
        m[pos] = x
    outs_b = prk.selftest_ops(op, *mixed)
    assert (outs_b[3] == 0).all(), label + ": a spoiled wave took the fast path"
    for k, r in enumerate(refs):
        check(outs_b[k][pos], r, "%s mixed out%d" % (label, k), *ins)
        m = ~A.is_nan(r)  # the three orders give the same words
        assert (outs_b[k][pos][m] == outs_c[k][m]).all() and (outs_a[k][m[idx]] == outs_c[k][idx][m[idx]]).all()


def bound_pairs():
    """Quotient operands at the very bounds of the fast range: in range."""
    p = A.pow2
    xs = [p(32) - 1, p(-80), ONE, p(32)]
    ds = [p(-32), p(32), p(-32) | 0x80000000, p(32) | 0x80000000]
    x, d = A._cross(np.array(xs, np.uint32), np.array(ds, np.uint32))
    return x, d


@pytest.fixture(scope="module")
def div_inputs():
    sets = A.div_sets()
    bx, bd = bound_pairs()
    ox, od = A.just_outside_div()  # at the head: whole waves in every order that keeps the others' order
    assert not A.div_in_range([ox], od).any()
    x = np.concatenate([ox] + [v[0] for v in sets.values()] + [bx])
    d = np.concatenate([od] + [v[1] for v in sets.values()] + [bd])
    return x, d, A.div_ref(x, d)


def test_plain_division(gpu, div_inputs):
    x, d, ref = div_inputs
    check(prk.selftest_ops(abi.PRK_OP_DIV, x, d)[0], ref, "x / d", x, d)
    out = prk.selftest_ops(abi.PRK_OP_DIV_FOCAL, x, d)
    check(out[0], ref, "div_focal", x, d)


def test_div_all1(gpu, div_inputs):
    x, d, ref = div_inputs
    ok = A.div_in_range([x], d)
    bx, bd = bound_pairs()
    assert ok[-bx.size:].all()  # 2^-32, 2^32, a numerator of exactly 2^32 and of 2^-80: in range
    run_arranged(abi.PRK_OP_DIV_ALL1, [x, d], ok, [ref], [0, ONE], "div_all<1>", 1 << 16)


@pytest.mark.parametrize("K", [3, 4, 5, 7, 8])
def test_div_all_k(gpu, div_inputs, K):
    """K numerators a, b, c, a, ... over one divisor: the numerators are the
    sets' x and two rotations of the whole concatenated array; the sum bound
    is on all K of them.  Four constructed elements put the float sum of the
    K numerators on exactly 2^32, the bound itself (in range), over divisors
    at both of theirs."""
    x, d, _ = div_inputs
    p = A.pow2
    ea, eb, ec = {3: (31, 30, 30), 4: (30, 30, 30), 5: (30, 29, 30), 7: (30, 28, 28), 8: (30, 28, 27)}[K]
    four = lambda w: np.full(4, w, np.uint32)  # noqa: E731
    a = np.concatenate([x, four(p(ea))])
    b = np.concatenate([np.roll(x, 1), four(p(eb))])
    c = np.concatenate([np.roll(x, 2), four(p(ec))])
    d = np.concatenate([d, np.array([p(-32), p(32), ONE, p(32) | 0x80000000], np.uint32)])
    with np.errstate(all="ignore"):
        total = np.zeros(4, np.float32)
        for k in range(K):
            total = total + np.abs(A.floats([a, b, c][k % 3][-4:]))
    assert (total == np.float32(2.0 ** 32)).all()
    nums = [a, b, c]
    full = [nums[k % 3] for k in range(K)]
    ok = A.div_in_range(full, d)
    assert ok[-4:].all()
    refs = [A.div_ref(v, d) for v in nums]
    op = {3: abi.PRK_OP_DIV_ALL3, 4: abi.PRK_OP_DIV_ALL4, 5: abi.PRK_OP_DIV_ALL5, 7: abi.PRK_OP_DIV_ALL7,
          8: abi.PRK_OP_DIV_ALL8}[K]
    run_arranged(op, [a, b, c, d], ok, refs, [0, 0, 0, ONE], "div_all<%d>" % K, 1 << 16)


def test_sqrt(gpu):
    x = A.sqrt_set()
    ref = A.sqrt_ref(x)
    check(prk.selftest_ops(abi.PRK_OP_SQRT, x)[0], ref, "sqrtf", x)
    f = A.floats(x)
    mid = (f >= np.float32(2.0 ** -96)) & np.isfinite(f)  # sqrt_mid's stated domain
    assert mid.sum() > 1 << 15
    check(prk.selftest_ops(abi.PRK_OP_SQRT_MID, x[mid])[0], ref[mid], "sqrt_mid", x[mid])


def norm_bounds():
    """Squared lengths of exactly 2^-64 and 2^62, components >= 2^-80: in range."""
    p = A.pow2
    return (np.array([p(-32), p(31), p(-33)], np.uint32), np.array([p(-80), p(-80), p(-33)], np.uint32),
            np.array([p(-80), p(-80), p(-33)], np.uint32))


def test_normalize_div(gpu):
    x, y, z = (np.concatenate(t) for t in zip(A.just_outside_norm(), A.norm_set(), norm_bounds()))
    ok = A.norm_in_range(x, y, z)
    assert not ok[:3 * A.WAVE].any()
    assert ok[-3:-1].all() and A.sq_len(x, y, z)[-3] == np.float32(2.0 ** -64) and \
        A.sq_len(x, y, z)[-2] == np.float32(2.0 ** 62)
    run_arranged(abi.PRK_OP_NORMALIZE_DIV, [x, y, z], ok, A.normalize_div_ref(x, y, z), [0, 0, 0], "normalize_div",
                 1 << 14)


def test_normalize_rcp(gpu):
    x, y, z = A.norm_set()
    out = prk.selftest_ops(abi.PRK_OP_NORMALIZE_RCP, x, y, z)
    for k, r in enumerate(A.normalize_rcp_ref(x, y, z)):
        check(out[k], r, "normalize_rcp out%d" % k, x, y, z)


@pytest.mark.parametrize("name", ["cvtt_s32", "round_s32", "round_u32", "cvt_rne_s32", "clamp01"])
def test_conversions(gpu, name):
    x = A.conversion_set()
    op = getattr(abi, "PRK_OP_" + name.upper())
    check(prk.selftest_ops(op, x)[0], getattr(A, name + "_ref")(x), name, x)


@pytest.mark.parametrize("name", ["minps", "maxps"])
def test_min_max(gpu, name):
    S = np.unique(np.concatenate([A.specials(), A.conversion_set()]))
    a, b = A._cross(S, S)
    check(prk.selftest_ops(getattr(abi, "PRK_OP_" + name.upper()), a, b)[0], getattr(A, name + "_ref")(a, b), name, a, b)


def test_mul16_trick_and_u8_unit(gpu):
    y, p = A.mul16_set()
    check(prk.selftest_ops(abi.PRK_OP_MUL16_TRICK, y, p)[0], A.mul16_trick_ref(y, p), "mul16_trick", y, p)
    k = np.arange(256, dtype=np.uint32)
    check(prk.selftest_ops(abi.PRK_OP_U8_UNIT, k)[0], A.u8_unit_ref(k), "u8_unit", k)


def test_zkey_properties(gpu):
    """zkey orders as '<' does, merges exactly the values that compare equal
    (+-0), and zkey_z gives back the bits of z except -0 -> +0 (no NaN: a
    fragment with a NaN z never takes a key)."""
    x = np.unique(np.concatenate([A.specials(), A.random_words(np.random.default_rng(5), 1 << 14)]))
    x = x[~A.is_nan(x)]
    f = A.floats(x)
    order = np.argsort(f, kind="stable")
    x, f = x[order], f[order]
    key, back, _, _ = prk.selftest_ops(abi.PRK_OP_ZKEY, x)
    assert (key[1:] >= key[:-1]).all()
    assert ((key[1:] == key[:-1]) == (f[1:] == f[:-1])).all()
    assert (back == np.where(x == 0x80000000, 0, x)).all()


def test_pair_tags(gpu):
    j = np.concatenate([np.arange(0, 70, dtype=np.uint32), np.array([0x7FFFFFFD, 0x7FFFFFFE, 12345678], np.uint32)])
    j, ge = A._cross(j, np.array([0, 1], np.uint32))
    tag, jb, is_pair, _ = prk.selftest_ops(abi.PRK_OP_PAIR_TAG, j, ge)
    # queue pairs 0x7FFFFFFE - j (below the prior z's 0x7FFFFFFF), single-thread pairs 0x80000000 + j
    assert (tag == np.where(ge == 1, np.uint32(0x80000000) + j, np.uint32(0x7FFFFFFE) - j)).all()
    assert (jb == j).all() and (is_pair == 1).all()
    low = np.array([0x7FFFFFFF, 0xFFFFFFFF, 0x7FFFFFFE, 0x80000000, 0], np.uint32)
    jj, pp, _, _ = prk.selftest_ops(abi.PRK_OP_TAG_PAIR, low)
    assert pp.tolist() == [0, 0, 1, 1, 1] and jj.tolist() == [0, 0, 0, 0, 0x7FFFFFFE]


def test_span_ends(gpu):
    lx, rx, wst = A.span_set()
    mn, mx, xd, _ = prk.selftest_ops(abi.PRK_OP_SPAN_ENDS, lx, rx, wst)
    xo, drawn, _, _ = prk.selftest_ops(abi.PRK_OP_SPAN_OFFSET, lx, rx, wst)
    for W in (8, 1920, 4096):
        for st in (0, 1):
            m = wst == (W | (st << 31))
            ref = A.span_ends_ref(lx[m], rx[m], W, bool(st))
            for k, got in enumerate((mn, mx, xd, xo, drawn)):
                check(got[m], ref[k], "span_ends W=%d st=%d out%d" % (W, st, k), lx[m], rx[m])


@pytest.mark.parametrize("seed", [1, 2])
def test_shared_divisor_paths(gpu, seed):
    """prk_selftest_div_paths on a small draw: no mismatch, and the odd waves
    -- half of them -- take both shared-reciprocal paths."""
    n = 1 << 16
    nq, nn, fq, fn = prk.selftest_div_paths(n=n, seed=seed)
    assert (nq, nn) == (0, 0)
    assert fq == fn == n // 128
