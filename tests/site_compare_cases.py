"""The two-sample comparison of the per-site histograms (dyn_aligner_site_compare) and the exact add of host columns
(dyn_aligner_site_summary_add), restated in Python ints, and the inputs of the device harness
(tests/device_math/site_compare.hip). The comparison itself uses plain loops over the counters: no NumPy arithmetic."""
import bisect
from fractions import Fraction

import numpy as np

NO_AT = 0xFFFFFFFF
DWELL_BINS = 16
M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1
COLUMNS = ("n_a", "n_b", "level_num", "level_at", "level_side", "dwell_num", "dwell_at", "dwell_side")
DTYPES = dict(n_a=np.uint32, n_b=np.uint32, level_num=np.uint64, level_at=np.uint32, level_side=np.int32, dwell_num=np.uint64,
              dwell_at=np.uint32, dwell_side=np.int32)


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def compare(a, b, tie="smallest"):
    """(nA, nB, num, at, side) of two lists of counters. tie="largest" is a wrong version the cases must tell apart."""
    assert len(a) == len(b)
    pa, pb, ra, rb = [], [], 0, 0
    for e in range(len(a)):
        ra = (ra + int(a[e])) & M32
        rb = (rb + int(b[e])) & M32
        pa.append(ra)
        pb.append(rb)
    n_a, n_b = ra, rb
    if n_a == 0 or n_b == 0:
        return n_a, n_b, 0, NO_AT, 0
    num, at, side = -1, 0, 0
    for e in range(len(a)):
        x, y = pa[e] * n_b, pb[e] * n_a
        assert x <= M64 and y <= M64
        d = x - y if x > y else y - x
        if d > num or (tie == "largest" and d == num):
            num, at = d, e
            side = 1 if x > y else (-1 if x < y else 0)
    return n_a, n_b, num, at, side


def compare_pair(level_a, dwell_a, level_b, dwell_b, tie="smallest"):
    n_a, n_b, num, at, side = compare(level_a, level_b, tie)
    _, _, dnum, dat, dside = compare(dwell_a, dwell_b, tie)
    return dict(n_a=n_a, n_b=n_b, level_num=num, level_at=at, level_side=side, dwell_num=dnum, dwell_at=dat, dwell_side=dside)


def compare_arrays(level, dwell, site_lo, other_lo, count, tie="smallest"):
    """the eight columns over the pairs (site_lo + i, other_lo + i) of level [n][Bc] and dwell [n][16] (lists of lists of ints)"""
    rows = [compare_pair(level[site_lo + i], dwell[site_lo + i], level[other_lo + i], dwell[other_lo + i], tie) for i in range(count)]
    return {k: np.array([r[k] for r in rows], dtype=DTYPES[k]) for k in COLUMNS}


def ks_exact(xs, ys):
    """the two-sample Kolmogorov-Smirnov distance over raw samples as an exact fraction (numerator over len(xs) * len(ys))"""
    xs, ys = sorted(xs), sorted(ys)
    best = 0
    for v in xs + ys:
        fa, fb = bisect.bisect_right(xs, v), bisect.bisect_right(ys, v)
        best = max(best, abs(fa * len(ys) - fb * len(xs)))
    return best, len(xs) * len(ys)


def bin_share(a, b):
    """max_e max(a[e] / nA, b[e] / nB) as an exact fraction"""
    n_a, n_b = sum(a), sum(b)
    return max(max(Fraction(int(v), n_a) for v in a), max(Fraction(int(v), n_b) for v in b))


def level_bin(m, bins, lo, hi):
    """the definition's two operations (tests/site_histogram_cases.py restates them the same way)"""
    inv_w = np.float64(bins) / (np.float64(hi) - np.float64(lo))
    u = float((np.float64(m) - np.float64(lo)) * inv_w)
    return 0 if u < 0 else (bins + 1 if u >= bins else 1 + int(u))


def binned(values, bins, lo, hi):
    h = [0] * (bins + 2)
    for v in values:
        h[level_bin(v, bins, lo, hi)] += 1
    return h


# ---- the add -----------------------------------------------------------------------------------------------------------------------
def add_cell(cell, inc):
    """seven limbs [n_rows, n_samples, dwell_sq, m1_lo, m1_hi, m2_lo, m2_hi] plus seven: mod 2^64 and, for the two pairs, mod 2^128"""
    out = [(int(cell[f]) + int(inc[f])) & M64 for f in range(3)]
    for f in (3, 5):
        v = (((int(cell[f + 1]) << 64) | int(cell[f])) + ((int(inc[f + 1]) << 64) | int(inc[f]))) & M128
        out += [v & M64, v >> 64]
    return out


def add_counters(row, inc):
    return [(int(r) + int(i)) & M32 for r, i in zip(row, inc)]


def add_restated(acc, hist, n_sites, width, lo, cols, totals, counters, rows=None):
    """acc: uint64 [7 * n_sites + 5] and hist: uint32 [n_sites * width] as the harness holds them; cols [count][7], totals (5 or
    None), counters [count][width] or None. rows: the window rows to visit (default all; the others must add zeros). Returns the
    arrays after the add."""
    acc, hist = acc.copy(), hist.copy()
    count = len(cols)
    for c in (range(count) if rows is None else rows):
        s = lo + c
        acc[7 * s:7 * s + 7] = np.array(add_cell(acc[7 * s:7 * s + 7].tolist(), [int(v) for v in cols[c]]), dtype=np.uint64)
        if counters is not None:
            hist[width * s:width * (s + 1)] = np.array(add_counters(hist[width * s:width * (s + 1)].tolist(), counters[c]), dtype=np.uint32)
    if totals is not None:
        for f in range(5):
            acc[7 * n_sites + f] = np.uint64((int(acc[7 * n_sites + f]) + int(totals[f])) & M64)
    return acc, hist


def limbs(v):
    v = int(v) & M128
    return v & M64, v >> 64


# ---- the harness inputs: comparison ------------------------------------------------------------------------------------------------
N_SITES, PAIRS = 80, 37
WIDTHS = (4, 8, 34, 66, 256)
# (site_lo, other_lo, count): the built pairs with the other window BELOW; a window overlapping itself by half; one pair starting at
# the table's last site; a window against itself
WINDOWS = ((40, 0, PAIRS), (3, 21, PAIRS), (N_SITES - 1, 5, 1), (7, 7, PAIRS))
BUILT = ("round0", "last", "tie", "equal", "empty_a", "empty_b", "empty_both", "top")


def pattern(kind, w, rng):
    """two counter rows of width w. d[w - 1] is 0 whatever the counters hold (both prefix sums are the totals there): the last
    counter at which a maximum can sit is w - 2."""
    a, b = [0] * w, [0] * w
    if kind == "round0":                      # a unique maximum at counter 0, smaller differences behind it
        a[0], a[w - 1] = 9, 1
        b[1], b[w - 1] = 3, 7
    elif kind == "last":                      # d rises up to w - 2: the last live counter of the last round that can hold it
        a[w - 1] = 7
        for e in range(w - 1):
            b[e] = 1
    elif kind == "tie":                       # |PA - PB| = 1 at counter 0 (side +1) and at w - 3 (side -1), 0 elsewhere
        a[0] += 1
        a[w - 2] += 1
        b[1] += 1
        b[w - 3] += 1
    elif kind == "equal":
        a = [int(v) for v in rng.integers(0, 50, w)]
        a[0] += 1
        b = list(a)
    elif kind == "empty_a":
        b = [int(v) for v in rng.integers(0, 9, w)]
        b[2] += 1
    elif kind == "empty_b":
        a = [int(v) for v in rng.integers(0, 9, w)]
        a[1] += 1
    elif kind == "top":                       # nA = nB = 2^32 - 1 at opposite ends: the product touches the top of the uint64 range
        a[0] = M32
        b[w - 1] = M32
    elif kind != "empty_both":
        raise ValueError(kind)
    return a, b


def compare_tables():
    """{Bc: uint32 [N_SITES][Bc + 16]}: pair i of WINDOWS[0] (A = 40 + i, B = i) holds BUILT[i] in its level counters and in its
    dwell counters; everything else seeded random counts, sparse ones (ties, empty sites) and large ones mixed"""
    out = {}
    for w in WIDTHS:
        rng = np.random.default_rng(7700 + w)
        t = np.zeros((N_SITES, w + DWELL_BINS), dtype=np.uint32)
        for s in range(N_SITES):
            style = s % 4
            for off, width in ((0, w), (w, DWELL_BINS)):
                if style == 0:
                    row = rng.integers(0, 3, width) * (rng.random(width) < 0.3)
                elif style == 1:
                    row = rng.integers(0, 1 << 20, width)
                elif style == 2:
                    row = rng.integers(0, 40, width)
                else:
                    row = rng.integers(0, 1 << 24, width) * (rng.random(width) < 0.5)  # (256 * 2^24 = 2^32: the sum is capped below)
                    if int(row.sum()) > M32:
                        row = row // 2
                t[s, off:off + width] = row
        for i, kind in enumerate(BUILT):
            for off, width in ((0, w), (w, DWELL_BINS)):
                a, b = pattern(kind, width, rng)
                t[40 + i, off:off + width] = a
                t[i, off:off + width] = b
        out[w] = t
    return out


def split(table, w):
    return table[:, :w].tolist(), table[:, w:].tolist()


# ---- the harness inputs: add -------------------------------------------------------------------------------------------------------
ADD_SITES, ADD_BINS = 50, 6
ADD_WIDTH = ADD_BINS + 2 + DWELL_BINS


def add_case(count, seed, n_sites=ADD_SITES, lo=None):
    """a seeded table, counters and `count` columns at window [lo, lo + count). Window row 0 forces a carry from the low into the
    high limb of M1, a negative M2 increment (two's complement), dwell_sq wrapping 2^64 and a counter wrapping 2^32."""
    rng = np.random.default_rng(seed)
    lo = (n_sites - count) // 2 if lo is None else lo
    acc = rng.integers(0, 1 << 40, 7 * n_sites + 5).astype(np.uint64)
    hist = rng.integers(0, 1 << 16, n_sites * ADD_WIDTH).astype(np.uint32)
    cols = rng.integers(0, 1 << 44, (count, 7)).astype(np.uint64)
    cols[:, 4] = 0
    cols[:, 6] = 0
    neg = rng.random(count) < 0.3                                    # negative M1 increments: sign-extended high limbs
    cols[neg, 4] = M64
    counters = rng.integers(0, 1 << 12, (count, ADD_WIDTH)).astype(np.uint32)
    counters[rng.random((count, ADD_WIDTH)) < 0.4] = 0
    s = lo
    acc[7 * s + 2], cols[0, 2] = M64 - 2, 10                         # dwell_sq wraps
    acc[7 * s + 3], acc[7 * s + 4], cols[0, 3], cols[0, 4] = M64 - 4, 6, 10, 0   # M1: the low limb carries
    acc[7 * s + 5], acc[7 * s + 6] = 1000, 0
    cols[0, 5], cols[0, 6] = limbs(-12345)                           # M2: 1000 - 12345 < 0
    hist[ADD_WIDTH * s + 3], counters[0, 3] = 0xFFFFFFF0, 0x20       # a counter wraps
    totals = rng.integers(0, 1 << 50, 5).astype(np.uint64)
    totals[4] = M64                                                  # ... and so does a total
    return dict(n_sites=n_sites, lo=lo, acc=acc, hist=hist, cols=cols, counters=counters, totals=totals)
