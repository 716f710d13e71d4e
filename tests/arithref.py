"""Host references and input sets for the kernels' arithmetic primitives
(csrc/prk_device.h through prk_selftest_ops), written from the definitions:
IEEE-754 binary32 arithmetic as numpy does it on the host, x86's conversion
and MINPS / MAXPS rules, and the reference's span-end and pitch-multiply
statements (projekt.cpp:1545-1592, 2508, 1916-1920).  Nothing here is taken
from prk_device.h or oracle/prk_oracle.c, with one exception that is a
convention of this project and not a value of the reference: a span with a
NaN end draws nothing (span_ends_ref).

Everything travels as uint32 words.  `same_words` is the comparison every
test uses: bit for bit, except that a NaN reference word admits any NaN.
"""
import math

import numpy as np

U32 = np.uint32
INT_MIN = 0x80000000
FLT_MAX = 0x7F7FFFFF
QNAN = 0x7FC00000
WAVE = 64


def words(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(U32)


def floats(w):
    return np.ascontiguousarray(np.asarray(w, U32)).view(np.float32)


def is_nan(w):
    w = np.asarray(w, U32)
    return (w & U32(0x7FFFFFFF)) > U32(0x7F800000)


def same_words(got, want):
    """Mismatching positions: equal bits, or both NaN where the reference is."""
    got, want = np.asarray(got, U32), np.asarray(want, U32)
    return np.nonzero(~((got == want) | (is_nan(want) & is_nan(got))))[0]


def pow2(e):
    return int(words(np.float32(math.ldexp(1.0, e)))[0])


def specials():
    """S of the issue: +- each of 0, the denormal extremes, FLT_MIN,
    1.5*2^-126, the powers of two that bound a path (each also one ulp below
    and above), 3, FLT_MAX, inf; and a quiet NaN."""
    pos = [0, 1, 0x007FFFFF, 0x00800000, 0x00C00000, int(words(np.float32(3.0))[0]), FLT_MAX, 0x7F800000]
    for e in (-126, -96, -80, -64, -32, 0, 31, 32, 62, 63, 64, 96):
        p = pow2(e)
        pos += [p - 1, p, p + 1]
    pos = sorted(set(pos))
    return np.array(pos + [p | 0x80000000 for p in pos] + [QNAN], U32)


def random_words(rng, n, emin=0, emax=255):
    """Random sign and mantissa, biased exponent uniform in [emin, emax)
    (0: zero and denormals; 255 is never drawn: finite values only)."""
    e = rng.integers(emin, emax, n, dtype=np.uint32)
    return (rng.integers(0, 2, n, dtype=np.uint32) << U32(31)) | (e << U32(23)) | rng.integers(0, 1 << 23, n,
                                                                                               dtype=np.uint32)


# ---- references ------------------------------------------------------------
def div_ref(x, d):
    with np.errstate(all="ignore"):
        return words(floats(x) / floats(d))


def div_ref64(x, d):
    # 53 >= 2*24 + 2: rounding the double quotient to float is the IEEE float quotient
    with np.errstate(all="ignore"):
        return words((floats(x).astype(np.float64) / floats(d).astype(np.float64)).astype(np.float32))


def sqrt_ref(x):
    with np.errstate(all="ignore"):
        return words(np.sqrt(floats(x)))


def sqrt_ref64(x):
    with np.errstate(all="ignore"):
        return words(np.sqrt(floats(x).astype(np.float64)).astype(np.float32))


def normalize_div_ref(x, y, z):
    with np.errstate(all="ignore"):
        fx, fy, fz = floats(x), floats(y), floats(z)
        ln = np.sqrt((fx * fx + fy * fy) + fz * fz)
        return words(fx / ln), words(fy / ln), words(fz / ln)


def normalize_rcp_ref(x, y, z):
    with np.errstate(all="ignore"):
        fx, fy, fz = floats(x), floats(y), floats(z)
        s = np.float32(1.0) / np.sqrt((fx * fx + fy * fy) + fz * fz)
        return words(s * fx), words(s * fy), words(s * fz)


def sq_len(x, y, z):
    with np.errstate(all="ignore"):
        fx, fy, fz = floats(x), floats(y), floats(z)
        return (fx * fx + fy * fy) + fz * fz


def _each(fn, *ws):
    return np.array([fn(*[float(v) for v in t]) & 0xFFFFFFFF
                     for t in zip(*[floats(w).astype(np.float64) for w in ws])], np.uint64).astype(U32)


def _roundf(x):
    """roundf: half away from zero; |x| + 0.5 is exact in float64 for a float x."""
    if math.isnan(x) or math.isinf(x):
        return x
    return math.copysign(math.floor(abs(x) + 0.5), x)


def _cvtt(x):  # cvttss2si: INT_MIN for NaN and outside [-2^31, 2^31)
    if math.isnan(x) or not (-2.0 ** 31 <= x < 2.0 ** 31):
        return INT_MIN
    return int(x)


def cvtt_s32_ref(w):
    return _each(_cvtt, w)


def round_s32_ref(w):
    return _each(lambda x: _cvtt(_roundf(x)), w)


def round_u32_ref(w):
    def f(x):  # x86-64 (u32)float: the 64-bit truncation's low word; its "indefinite" 2^63 has a zero low word
        r = _roundf(x)
        if math.isnan(r) or not (-2.0 ** 63 <= r < 2.0 ** 63):
            return 0
        return int(r)
    return _each(f, w)


def cvt_rne_s32_ref(w):
    def f(x):  # cvtps2dq, default MXCSR: nearest even, INT_MIN when the result does not fit
        if math.isnan(x) or math.isinf(x):
            return INT_MIN
        r = round(x)  # Python rounds half to even, exactly
        return r if -2 ** 31 <= r < 2 ** 31 else INT_MIN
    return _each(f, w)


def _sel(a, b, take_a):
    a, b = np.asarray(a, U32), np.asarray(b, U32)
    with np.errstate(all="ignore"):
        return np.where(take_a(floats(a), floats(b)), a, b)


def minps_ref(a, b):  # MINPS: the second operand unless a < b (so on NaN in either, and on equal values)
    return _sel(a, b, lambda x, y: x < y)


def maxps_ref(a, b):
    return _sel(a, b, lambda x, y: x > y)


def clamp01_ref(a):  # Clamp01: below 0 -> 0, above 1 -> 1, everything else (NaN, -0) unchanged
    a = np.asarray(a, U32)
    with np.errstate(all="ignore"):
        f = floats(a)
        return np.where(f < 0, U32(0), np.where(f > 1, words(np.float32(1.0))[0], a)).astype(U32)


def mul16_trick_ref(y, p):
    """_mm_or_si128(_mm_mullo_epi16(y, p), _mm_slli_epi32(_mm_mulhi_epi16(y, p), 16))
    of one 32-bit lane: 16-bit lanes (lo, hi) of y and p; mullo keeps the low
    16 bits of each lane product, mulhi the high 16 bits of the SIGNED lane
    product, and the shift moves mulhi's low lane up and drops its high lane."""
    def s16(v):
        return v - 0x10000 if v & 0x8000 else v
    out = []
    for yy, pp in zip(np.asarray(y, U32).tolist(), np.asarray(p, U32).tolist()):
        ylo, yhi, plo, phi = yy & 0xFFFF, yy >> 16, pp & 0xFFFF, pp >> 16
        mullo = ((ylo * plo) & 0xFFFF) | (((yhi * phi) & 0xFFFF) << 16)
        mulhi_lo = ((s16(ylo) * s16(plo)) >> 16) & 0xFFFF
        out.append(mullo | ((mulhi_lo << 16) & 0xFFFFFFFF))
    return np.array(out, np.uint64).astype(U32)


def u8_unit_ref(k):
    return words((np.asarray(k, np.float64) / 255.0).astype(np.float32))


def span_ends_ref(lx, rx, W, st):
    """projekt.cpp:1545-1592 (st: the single-thread overload's XOffset =
    -XOffset, 2508).  Returns MinX, MaxX, XDiff, XOffset words and the drawn
    flag.  A NaN end is NOT derived from the reference (which would go on with
    an INT_MIN column): the project pins such a span to "draws nothing", and
    this function states that convention -- flag 0, every word 0 -- so that the
    device's pin is at least held to what it documents."""
    out = []
    for L, R in zip(floats(lx).astype(np.float64).tolist(), floats(rx).astype(np.float64).tolist()):
        if math.isnan(L) or math.isnan(R):
            out.append((0, 0, 0, 0, 0))
            continue
        xoff = 0.0
        left, right = L, R
        if left < 0:
            xoff = -xoff if st else -left
            left = 0.0
        elif left >= W:
            left = float(np.float32(W) - np.float32(1))
        if right < 0:
            right = 0.0
        elif right >= W:
            right = float(np.float32(W) - np.float32(1))
        cl, cr = _cvtt(_roundf(L)), _cvtt(_roundf(R))
        xdiff = (cr - cl) & 0xFFFFFFFF
        # (s32)(r32)RoundR32ToS32 of a clamped end: an integer in [0, W - 1], exact as a float
        mn, mx = _cvtt(_roundf(left)), _cvtt(_roundf(right))
        out.append((mn & 0xFFFFFFFF, mx & 0xFFFFFFFF, xdiff, int(words(np.float32(xoff))[0]), 1))
    a = np.array(out, np.uint64).astype(U32)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4]


# ---- input sets --------------------------------------------------------------
def _cross(*sets):
    g = np.meshgrid(*sets, indexing="ij")
    return [x.ravel().astype(U32) for x in g]


def div_sets(seed=1):
    """name -> (x, d) of the issue's division sets."""
    rng = np.random.default_rng(seed)
    S = specials()
    sets = {"special": tuple(_cross(S, S))}
    n = 1 << 17
    sets["all_exponents"] = (random_words(rng, n), random_words(rng, n))
    # the fast range: |d| in [2^-32, 2^32], |x| in [2^-80, 2^32)
    sets["fast_range"] = (random_words(rng, n, 127 - 80, 127 + 32), random_words(rng, n, 127 - 32, 127 + 32))
    m = 1 << 15
    d = random_words(rng, m, 1, 254)
    ed = ((d >> U32(23)) & U32(0xFF)).astype(np.int64)
    gap = np.where(rng.integers(0, 2, m) == 1, rng.integers(120, 151, m), -rng.integers(120, 151, m))
    ex = ed + gap  # an exponent gap in [-150, -120] or [120, 150]; kept where x is representable (denormal x included)
    keep = (ex >= 0) & (ex <= 254)
    x = (random_words(rng, m, 1, 2) & U32(0x807FFFFF)) | (np.clip(ex, 0, 254).astype(U32) << U32(23))
    sets["extreme_quotient"] = (x[keep], d[keep])
    # hard roundings: x = float(q * d) and its neighbours, so x / d lies next to q or a midpoint
    q, d = random_words(rng, m // 3, 64, 190), random_words(rng, m // 3, 64, 190)
    x0 = words((floats(q).astype(np.float64) * floats(d).astype(np.float64)).astype(np.float32))
    sets["hard_rounding"] = (np.concatenate([x0 - U32(1), x0, x0 + U32(1)]), np.concatenate([d, d, d]))
    sets["hard_midpoint"] = midpoint_pairs(rng, m)
    return sets


def midpoint_pairs(rng, n):
    """Quotients as close to a rounding boundary as two floats allow: for an
    odd 24-bit D and r = +-1, the odd 25-bit M with M * D = -r (mod 2^25)
    gives X = (M * D + r) / 2^25, and X / D = (M + r / D) / 2^25 lies within
    2^-24 ulp of the midpoint M / 2^25 of two floats.  A quotient routine that
    is off by 2^-24 ulp before its last rounding gets a share of these wrong."""
    D = rng.integers(1 << 23, 1 << 24, n, dtype=np.uint64) | np.uint64(1)
    r = np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int64)
    inv = D.copy()  # Newton: D * inv = 1 (mod 2^25)
    for _ in range(5):
        inv = (inv * (np.uint64(2) - D * inv)) & np.uint64((1 << 25) - 1)
    M = ((-r).astype(np.uint64) * inv) & np.uint64((1 << 25) - 1)
    X = ((M * D).astype(np.int64) + r) >> 25
    keep = (M >= (1 << 24)) & (X >= (1 << 23)) & (X < (1 << 24))
    assert ((((M * D).astype(np.int64) + r) & ((1 << 25) - 1)) == 0).all()
    sign = rng.integers(0, 2, n, dtype=np.uint32) << U32(31)
    return (words(X[keep].astype(np.float32)) | sign[keep]), words(D[keep].astype(np.float32))


def just_outside_div(seed=6):
    """Four whole waves, each wholly one binade outside one bound of the
    shared-reciprocal range: |d| in [2^-33, 2^-32), |d| in (2^32, 2^33),
    |x| in (2^32, 2^33), |x| in [2^-81, 2^-80)."""
    rng = np.random.default_rng(seed)
    mid = lambda: random_words(rng, WAVE, 127 - 10, 127 + 10)  # noqa: E731
    x = [mid(), mid(), random_words(rng, WAVE, 127 + 32, 127 + 33) | U32(1), random_words(rng, WAVE, 127 - 81, 127 - 80)]
    d = [random_words(rng, WAVE, 127 - 33, 127 - 32), random_words(rng, WAVE, 127 + 32, 127 + 33) | U32(1), mid(), mid()]
    return np.concatenate(x), np.concatenate(d)


def just_outside_norm(seed=7):
    """Three whole waves one binade outside normalize_div's bounds: squared
    length in [2^-66, 2^-64), in (2^62, 2^64), smallest component in [2^-81, 2^-80)."""
    rng = np.random.default_rng(seed)
    c = lambda e: np.full(WAVE, pow2(e), U32)  # noqa: E731
    x = [random_words(rng, WAVE, 127 - 33, 127 - 32), random_words(rng, WAVE, 127 + 31, 127 + 32) | U32(1), c(0)]
    y = [c(-60), c(0), c(0)]
    z = [c(-60), c(0), random_words(rng, WAVE, 127 - 81, 127 - 80)]
    return np.concatenate(x), np.concatenate(y), np.concatenate(z)


def div_in_range(nums, d):
    """The documented bounds of the shared-reciprocal quotient, per element:
    |d| in [2^-32, 2^32], the numerators' absolute sum <= 2^32 (float
    additions in order), the smallest |numerator| >= 2^-80."""
    with np.errstate(all="ignore"):
        ab = [np.abs(floats(x)) for x in nums]
        s, mn = ab[0].copy(), ab[0].copy()
        for v in ab[1:]:
            s = s + v
            mn = np.fmin(mn, v)
        ad = np.abs(floats(d))
        return (ad >= np.float32(2.0 ** -32)) & (ad <= np.float32(2.0 ** 32)) & (s <= np.float32(2.0 ** 32)) & \
               (mn >= np.float32(2.0 ** -80))


def norm_in_range(x, y, z):
    with np.errstate(all="ignore"):
        d = sq_len(x, y, z)
        mn = np.fmin(np.fmin(np.abs(floats(x)), np.abs(floats(y))), np.abs(floats(z)))
        return (d >= np.float32(2.0 ** -64)) & (d <= np.float32(2.0 ** 62)) & (mn >= np.float32(2.0 ** -80))


def sqrt_set(seed=2):
    return np.concatenate([specials(), random_words(np.random.default_rng(seed), 1 << 17)])


def norm_set(seed=3):
    """S^3 thinned to ~2^15 triples, 2^15 random triples around each of the
    two squared-length bounds (2^-64, 2^62), 2^14 well inside, and the zero vector."""
    rng = np.random.default_rng(seed)
    S = specials()
    x, y, z = _cross(S, S, S)
    pick = rng.permutation(x.size)[: 1 << 15]
    parts = [(x[pick], y[pick], z[pick])]
    for lo, hi, n in ((127 - 36, 127 - 28, 1 << 15), (127 + 27, 127 + 35, 1 << 15), (127 - 20, 127 + 20, 1 << 14)):
        parts.append(tuple(random_words(rng, n, lo, hi) for _ in range(3)))
    parts.append(tuple(np.zeros(1, U32) for _ in range(3)))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def conversion_set():
    S = specials()
    v = []
    for k in range(-4, 5):
        h = int(words(np.float32(k + 0.5))[0])
        v += [h - 1, h, h + 1]
    v += [int(w) for w in words(np.array([0.49999997, 8388607.5, 2.0 ** 23 - 1, 2.0 ** 23 + 1, 2.0 ** 31 - 128,
                                          -2.0 ** 31, -2.0 ** 31 - 256, 2.0 ** 63 - 2.0 ** 39], np.float32))]
    v = np.array(v, U32)
    return np.unique(np.concatenate([S, v, v ^ U32(0x80000000)]))


def mul16_set(seed=4):
    e = np.array([0, 1, 255, 256, 0x7FFF, 0x8000, 0xFFFF, 0x10000, 0x18000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], U32)
    y, p = _cross(e, e)
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 1 << 32, (2, 1 << 12), dtype=np.uint64).astype(U32)
    return np.concatenate([y, r[0]]), np.concatenate([p, r[1]])


def span_set():
    """(LX, RX, W | st << 31) for W in {8, 1920, 4096} and both st."""
    parts = []
    for W in (8, 1920, 4096):
        ends = np.unique(np.concatenate([conversion_set(), words(np.array(
            [-0.5, -0.0, W - 1, W - 0.5, W, np.nan], np.float32))]))
        few = words(np.array([-0.5, -0.0, 0.5, 2.5, W - 1, W - 0.5, W, np.nan, -3.0e9, 3.0e9, 2.0 ** 31], np.float32))
        p, q = _cross(ends, few), _cross(few, ends)  # every end on each side, against a few on the other
        lx, rx = np.concatenate([p[0], q[0]]), np.concatenate([p[1], q[1]])
        for st in (0, 1):
            parts.append((lx, rx, np.full(lx.size, W | (st << 31), U32)))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


# ---- wave arrangements ---------------------------------------------------------
def arrange_uniform(in_range):
    """Order (a): in-range elements first, padded to whole waves by repeating
    the last of them, then the rest.  Returns (index array, count of leading
    elements that sit in wholly in-range waves)."""
    idx_in, idx_out = np.nonzero(in_range)[0], np.nonzero(~in_range)[0]
    if idx_in.size:
        pad = (-idx_in.size) % WAVE
        idx_in = np.concatenate([idx_in, np.repeat(idx_in[-1:], pad)])
    return np.concatenate([idx_in, idx_out]), idx_in.size


def arrange_mixed(n):
    """Order (b): positions of the caller's order with one slot kept free at
    the head of every wave (the caller puts an out-of-range element there).
    Returns (total length, positions of the n elements, positions of the heads)."""
    per = WAVE - 1
    waves = (n + per - 1) // per
    pos = np.arange(n) + np.arange(n) // per + 1
    return waves * WAVE, pos, np.arange(waves) * WAVE


def unclamped_colour_scene(seed=77):
    """The frame-level case of the colour pack's round_u32 on unclamped values
    (DrawModel non-Phong, projekt.cpp:515 "no clamp"): random_soup(300, 128,
    96), untextured, vertex colours uniform in [-2, 3], and a dozen vertices
    with a NaN, +-inf, 2^31 / 255 * 1.5 or 2^63 / 255 * 1.5 channel."""
    from prk import scenes
    s = scenes.random_soup(300, 128, 96, radius=16, seed=seed, textured=False, lights=scenes.LIGHTS_TWO,
                           ambient=scenes.AMBIENT_TWO)
    rng = np.random.default_rng(seed)
    cols = rng.uniform(-2.0, 3.0, s.colors.shape).astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, 2.0 ** 31 / 255 * 1.5, 2.0 ** 63 / 255 * 1.5, -(2.0 ** 31) / 255 * 1.5],
                   np.float32)
    for k, v in enumerate(rng.permutation(cols.shape[0])[:12]):
        cols[v, k % 4] = odd[k % odd.size]
    s.colors = cols
    return s
