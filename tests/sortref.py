"""The span path's radix sort and exclusive scans (csrc/prk_sort.hip through
prk_selftest_sort / prk_selftest_scan), written from the definitions in numpy,
and the input families tests/test_gpu_sort_scan.py runs them on.

sort_ref    a stable argsort of keys & mask.  The mask covers the low
            8 * ceil(end_bit / 8) bits: prk_obj_sort runs whole 8-bit passes,
            so the bits from end_bit up to the next multiple of 8 take part in
            the order (csrc/prk_launch.h states the contract).
scan_ref    the exclusive sum modulo 2^width, without arithmetic of that
            width: every value is cut into 32-bit limbs, each limb column is
            summed exactly in 64 bits (n < 2^32 limbs below 2^32), and the
            carries are added by hand.  tests/test_sortref.py holds it to a
            loop over Python ints.

Every generator is a pure function of its arguments (a seed derived from
them), so the CPU and the GPU tests draw the same inputs.
"""
import zlib

import numpy as np

U64 = np.uint64
ALL_ONES = U64(0xFFFFFFFFFFFFFFFF)

# prk_sort.hip's constants, which the sizes below come from
WAVE_SEG_SHORT, WAVE_SEG_LONG = 256, 1024   # a wave's items of a short / long tile
TILE_SHORT, TILE_LONG = 1024, 4096
SMALL_MAX = 262144                          # up to here: short tiles
SCAN_TILE = 4096

END_BITS = (0, 1, 8, 9, 16, 17, 24, 26, 33, 40, 41, 48, 49, 56, 57, 64)  # 0 .. 8 passes
SORT_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 262143, 262144, 262145, 266240, 266241,
              1100003)  # (the last: 269 long tiles, more than 256)
SORT_SIZE_SHORT, SORT_SIZE_LONG = 5003, 266241
# 258 tiles is the first size whose last tile adds up its predecessors' sums
# in two trips of k_scan_down's stride loop (256 threads, 257 sums)
SCAN_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 1048576, 1048577, 1052673,
              1300021)


def passes(end_bit):
    return (int(end_bit) + 7) // 8


def low_mask(bits):
    return U64((1 << int(bits)) - 1)


def order_mask(end_bit):
    """The key bits prk_obj_sort orders by."""
    return low_mask(8 * passes(end_bit))


def sort_ref(keys, vals, end_bit):
    k = np.asarray(keys, U64)
    v = np.asarray(vals, np.uint32)
    idx = np.argsort(k & order_mask(end_bit), kind="stable")
    return k[idx], v[idx]


def scan_ref(x, width):
    assert width in (32, 64)
    x = np.asarray(x, U64)
    n = x.shape[0]
    assert n < (1 << 32)
    m32 = U64(0xFFFFFFFF)

    def excl(limb):  # exact: fewer than 2^32 terms below 2^32
        out = np.zeros(n, U64)
        if n > 1:
            np.cumsum(limb[:-1], out=out[1:])
        return out

    lo = excl(x & m32)
    if width == 32:
        return (lo & m32).astype(np.uint32)
    hi = excl(x >> U64(32)) + (lo >> U64(32))  # below 2^33: exact
    return ((hi & m32) << U64(32)) | (lo & m32)


def rng_of(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def random_u64(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=U64)


def sort_vals(n, *what):
    """Random u32 values with duplicates (never arange: a sort that wrote the
    index where it should carry the value would pass on that)."""
    rng = rng_of("vals", n, *what)
    pool = rng.integers(0, 1 << 32, size=max(1, (n + 1) // 2), dtype=np.uint32)
    return pool[rng.integers(0, pool.shape[0], size=n)]


def tied(rng, n, bits):
    """n values below 2^bits drawn from about n / 4 of them: many ties."""
    pool = random_u64(rng, max(1, n // 4)) & low_mask(bits)
    return pool[rng.integers(0, pool.shape[0], size=n)]


# ---- key families: name -> f(n, end_bit) -> uint64 [n] -------------------------
def keys_equal(n, end_bit):
    """All keys equal: the output is the input order (stability across lanes,
    rounds, waves and tiles; the look-back prefix carries the whole count)."""
    return np.full(n, random_u64(rng_of("equal", end_bit), 1)[0], U64)


def keys_alt2(n, end_bit):
    """Two key values alternating, the larger first: a lane's 32 peers are
    every other lane."""
    ab = random_u64(rng_of("alt2", end_bit), 2)
    m = order_mask(end_bit)
    if (ab[0] & m) == (ab[1] & m):
        ab[1] ^= U64(1)
    a, b = (ab[0], ab[1]) if (ab[0] & m) > (ab[1] & m) else (ab[1], ab[0])
    return np.where(np.arange(n) % 2 == 0, a, b).astype(U64)


def keys_runs64(n, end_bit):
    """Runs of exactly 64 equal keys aligned to a wave round: a lane's peer
    mask is all 64 lanes.  15 values, neighbours always different."""
    rng = rng_of("runs64", end_bit)
    vals15 = random_u64(rng, 15)
    m = order_mask(end_bit)
    if m:  # make them differ in the ordered bits
        vals15 = (vals15 & ~U64(15)) | np.arange(15, dtype=U64)
    run = np.arange(n) // 64
    return vals15[(7 * run) % 15]


def keys_digit(n, end_bit, q):
    """Keys that differ in digit position q only (q < passes): a wrong shift
    or a wrong histogram row for pass q sees one constant digit."""
    rng = rng_of("digit", n, end_bit, q)
    base = random_u64(rng, 1)[0] & ~(U64(0xFF) << U64(8 * q))
    return base | (rng.integers(0, 256, size=n, dtype=U64) << U64(8 * q))


def keys_uniform(n, end_bit):
    """Uniform draws masked to end_bit, every bit of every digit random."""
    return random_u64(rng_of("uniform", n, end_bit), n) & low_mask(end_bit)


def keys_sorted(n, end_bit):
    return np.sort(keys_uniform(n, end_bit))


def keys_reverse(n, end_bit):
    return keys_sorted(n, end_bit)[::-1].copy()


def keys_high_bits(n, end_bit):
    """Random bits at and above 8 * passes over tied low bits: they must not
    affect the order (ties stay in input order) and must arrive intact."""
    rng = rng_of("high", n, end_bit)
    ob = 8 * passes(end_bit)
    return tied(rng, n, ob) | (random_u64(rng, n) & ~low_mask(ob))


def keys_mid_bits(n, end_bit):
    """Random bits in [end_bit, 8 * passes) over tied low end_bit bits, zero
    above: by the contract they take part in the order.  A sort that masked
    its last digit to end_bit would leave the ties in input order instead."""
    rng = rng_of("mid", n, end_bit)
    ob = 8 * passes(end_bit)
    return tied(rng, n, end_bit) | (random_u64(rng, n) & low_mask(ob) & ~low_mask(end_bit))


SORT_FAMILIES = {
    "equal": keys_equal, "alt2": keys_alt2, "runs64": keys_runs64, "uniform": keys_uniform, "sorted": keys_sorted,
    "reverse": keys_reverse, "high_bits": keys_high_bits, "mid_bits": keys_mid_bits,
}


# ---- MergeSort-shaped keys -------------------------------------------------------
def bitlen(v):
    return int(v).bit_length()


def merge_path(i, n, pbits):
    """prk_spans.hip merge_path: entry i of an n-entry MergeSort's recursion
    path (Half1 = 0, Half0 = 1, the position in a two-entry run last),
    left-aligned in pbits.  i, n: int64 arrays."""
    i = np.asarray(i, np.int64)
    first = np.zeros_like(i)
    count = np.asarray(n, np.int64).copy()
    path = np.zeros_like(i)
    bits = np.zeros_like(i)
    while True:
        go = count > 2
        if not go.any():
            break
        h0 = count // 2
        left = go & (i < first + h0)
        right = go & ~left
        path = np.where(go, (path << 1) | left, path)
        first = np.where(right, first + h0, first)
        count = np.where(left, h0, np.where(right, count - h0, count))
        bits += go
    two = count == 2
    path = np.where(two, (path << 1) | (i - first), path)
    bits += two
    return (path << (pbits - bits)).astype(U64)


MERGE_H = 1080


def keys_merge(slots, layout, pads):
    """The keys k_objtri_emit / k_rec_emit hand to the sort: (object <<
    (ybits + pbits)) | (ymin << pbits) | path in object order, YMin nearly
    sorted inside an object, and all-ones pad keys in one to two thirds of the
    slots.  layout "H": ybits = bitlen(H), YMin clamped to H (the object
    passes); "31": ybits = 31, any YMin (the edge records).  pads "tail": the
    real keys packed first, as the emit kernels leave them (escan places
    them); "interleaved": every triangle's three slots hold one or two real
    keys, then pads.  Returns (keys, end_bit, real: bool [slots])."""
    rng = rng_of("merge", slots, layout, pads)
    tris = (slots + 2) // 3
    c = rng.integers(1, 3, size=tris)  # visible edges of each triangle: 1 or 2
    real = (np.arange(3 * tris) % 3 < np.repeat(c, 3))[:slots]
    total = int(real.sum())
    # objects of 1 .. 200 edges (some over 64, the radix path's reason) until total
    sizes = []
    left = total
    while left > 0:
        s = min(left, int(rng.integers(1, 201)))
        sizes.append(s)
        left -= s
    sizes = np.asarray(sizes, np.int64)
    nobj = max(1, sizes.shape[0])
    maxn = int(sizes.max()) if total else 1
    pbits = bitlen(maxn) + 1
    ybits = max(1, bitlen(MERGE_H)) if layout == "H" else 31
    obits = max(1, bitlen(nobj - 1))
    end_bit = obits + ybits + pbits
    assert end_bit <= 64
    obj = np.repeat(np.arange(sizes.shape[0], dtype=np.int64), sizes)
    start = np.repeat(np.cumsum(sizes) - sizes, sizes)
    idx = np.arange(total, dtype=np.int64) - start
    nn = np.repeat(sizes, sizes)
    ycap = MERGE_H if layout == "H" else (1 << 31) - 1
    # nearly sorted: a ramp over the object with a few rows of jitter and ties
    y = (idx * MERGE_H) // np.maximum(nn, 1) + rng.integers(-3, 4, size=total)
    if layout == "31":
        far = rng.random(total) < 0.01
        y = np.where(far, rng.integers(0, 1 << 31, size=total), y)
    y = np.clip(y, 0, ycap)
    k = (obj.astype(U64) << U64(ybits + pbits)) | (y.astype(U64) << U64(pbits)) | merge_path(idx, nn, pbits)
    keys = np.full(slots, ALL_ONES, U64)
    if pads == "tail":
        keys[:total] = k
        real = np.arange(slots) < total
    else:
        keys[real] = k
    return keys, end_bit, real


# ---- scan value families: name -> f(n, width) -> unsigned [n] ---------------------
def scan_dtype(width):
    return np.uint32 if width == 32 else U64


def scan_zero(n, width):
    return np.zeros(n, scan_dtype(width))


def scan_one(n, width):
    return np.ones(n, scan_dtype(width))


def scan_max32(n, width):
    return np.full(n, 0xFFFFFFFF, scan_dtype(width))


def scan_random(n, width):
    """Full-range random: the sums wrap modulo 2^width."""
    return rng_of("scan_random", n, width).integers(0, 1 << width, size=n, dtype=scan_dtype(width))


def scan_edge32(n, width):
    """Width 64: values of exactly 0xFFFFFFFF and 0x100000000."""
    pick = rng_of("scan_edge32", n).integers(0, 2, size=n)
    return np.where(pick == 0, U64(0xFFFFFFFF), U64(0x100000000)).astype(U64)


def scan_below40(n, width):
    """Width 64: random below 2^40, so a few hundred values cross 2^32: inside
    one wave, between waves, between tiles."""
    return rng_of("scan_below40", n).integers(0, 1 << 40, size=n, dtype=U64)


SCAN_FAMILIES = {
    32: {"zero": scan_zero, "one": scan_one, "max32": scan_max32, "random": scan_random},
    64: {"zero": scan_zero, "one": scan_one, "edge32": scan_edge32, "below40": scan_below40, "random": scan_random},
}
SCAN_SINGLE_VALUE = {32: 0xDEADBEEF, 64: 0x123456789ABCDEF1}


def scan_single_positions(n):
    """A thread's items (15/16), 63/64, a wave's items (1023/1024), a tile
    (4095/4096), and the last value."""
    return sorted({p for p in (15, 16, 63, 64, 1023, 1024, 4095, 4096, n - 1) if 0 <= p < n})


def scan_single(n, width, p):
    x = np.zeros(n, scan_dtype(width))
    x[p] = SCAN_SINGLE_VALUE[width]
    return x
