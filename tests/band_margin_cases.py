"""Shared by tests/test_band_margin_host.py and tests/test_gpu_band_margin.py: the band-margin definition (INTEGRATION.md section
3, dyn_aligner_set_band_margin) restated in Python ints over ALL path rows, the segment-end shortcut the kernel uses, three
deliberately wrong readings of the definition, and build_batch(): the smallest shapes at which the kernel can still go wrong.
No GPU, no library."""
from types import SimpleNamespace

import numpy as np

NONE = 0xFFFFFFFF


def mid(t: int, ratio: float) -> int:
    """the reference's band centre: one fp64 product, truncated"""
    return int(float(t) * ratio)


def borders(segrow, T, N):
    """[(n, a, b)]: output row j is lattice column n = j + 1 and covers the lattice rows [a, b)"""
    n_seg = N - 1
    return [(j + 1, int(segrow[j]), int(segrow[j + 1]) if j + 1 < n_seg else int(T)) for j in range(n_seg)]


def brute(segrow, T, N, bw, ratio):
    """(low, high, edge_rows): the definition, row by row"""
    low = high = NONE
    edge = 0
    for n, a, b in borders(segrow, T, N):
        for t in range(a, b):
            m = mid(t, ratio)
            zero = False
            if m - bw >= 2:                      # the lower edge is real: a column of 1 .. N-1 below the band is excluded
                s = n - (m - bw)
                low = min(low, s)
                zero |= s == 0
            if m + bw + 1 < N:                   # the upper edge is real
                s = (m + bw) - n
                high = min(high, s)
                zero |= s == 0
            edge += zero
    return low, high, edge


def first_row_reaching(m, ratio, lo, hi):
    """the first row t of [lo, hi] with mid(t) >= m (mid(hi) >= m): bisection on the monotone staircase"""
    while lo < hi:
        h = (lo + hi) // 2
        if mid(h, ratio) >= m:
            hi = h
        else:
            lo = h + 1
    return lo


def rows_at(m, a, b, ratio):
    """rows t of [a, b) with mid(t) == m"""
    if m < 0 or mid(b - 1, ratio) < m or mid(a, ratio) > m:
        return 0
    lo = first_row_reaching(m, ratio, a, b - 1)
    hi = first_row_reaching(m + 1, ratio, lo, b - 1) if mid(b - 1, ratio) > m else b
    return hi - lo


def shortcut(segrow, T, N, bw, ratio, wrong=None):
    """What the kernel computes: a segment's lower minimum on its LAST row, its upper minimum on its FIRST row, its rows of slack
    0 as one run of the staircase each. ``wrong``: one of the three misreadings the host test must tell from the definition --
    "clamped" (an edge counts as real where the lattice's own border clamps it), "ge1" (mid - bw >= 1 for the lower edge),
    "upper_last" (the upper minimum taken on the segment's last row)."""
    low = high = NONE
    edge = 0
    lo_floor = 1 if wrong == "ge1" else 2
    for n, a, b in borders(segrow, T, N):
        if not a < b:
            continue
        m_last, m_first = mid(b - 1, ratio), mid(a, ratio)
        if wrong == "clamped" or m_last - bw >= lo_floor:
            low = min(low, n - (m_last - bw))
        m_up = m_last if wrong == "upper_last" else m_first
        if wrong == "clamped" or m_up + bw + 1 < N:
            high = min(high, (m_up + bw) - n)
        lo_can = wrong == "clamped" or n >= lo_floor
        hi_can = wrong == "clamped" or n + 1 < N
        if lo_can:
            edge += rows_at(n + bw, a, b, ratio)
        if hi_can and not (bw == 0 and lo_can):
            edge += rows_at(n - bw, a, b, ratio)
    return low & NONE, high & NONE, edge


def column_range(t, N, bw, ratio):
    """the columns of 1 .. N-1 inside the band at row t"""
    m = mid(t, ratio)
    return max(1, m - bw), min(N - 1, m + bw)


def make_path(T, N, bw, ratio, how, rng=None, stall=None, start=1):
    """segrow of a monotone path from column 1 at row ``start`` to column N - 1 at row T - 1 that stays inside the band: how =
    "low" hugs the band's lower edge, "high" its upper edge, "random" walks in between. ``stall`` = (column, rows): the path
    waits in that column for at least that many rows where the band lets it. (The aligner's paths start at row 1; a later start
    is a shape only the kernel's harness can be given.)"""
    segrow = np.zeros(N - 1, dtype=np.uint32)
    n = 1
    segrow[0] = start
    waited = 0
    for t in range(start + 1, T):
        lo, hi = column_range(t, N, bw, ratio)
        must = max(lo, N - 1 - (T - 1 - t), n)   # the path still has to reach column N - 1 at row T - 1
        may = min(hi, n + 1)
        assert must <= may, (T, N, bw, t, n, lo, hi)
        if stall is not None and n == stall[0] and waited < stall[1] and must == n:
            waited += 1
            continue
        if how == "low":
            nxt = must
        elif how == "high":
            nxt = may
        else:
            nxt = int(rng.integers(must, may + 1))
        if nxt == n + 1:
            segrow[n] = t
        n = nxt
    assert n == N - 1, (T, N, bw, n)
    return segrow


def near_integer_products(T, ratio):
    """rows t of 1 .. T-1 whose product t * ratio lies within one ulp of an integer without being one"""
    t = np.arange(1, T, dtype=np.float64)
    p = t * ratio
    r = np.rint(p)
    return np.flatnonzero((p != r) & (np.abs(p - r) <= np.spacing(r)) & (r > 0)) + 1


def build_batch(seed=20261019):
    """Tens of reads. Per descriptor: seg_off, T, N, bw, ratio, read; status per read; segrow concatenated. reads[i] holds the
    same per read with a label, in read order (descriptors are in another order, as a launch's processing order is)."""
    rng = np.random.default_rng(seed)
    reads = []

    def add(label, T, N, band_half, how="random", status=0, stall=None, start=1, bw=None):
        bw = min(band_half, N // 2) if bw is None else bw
        ratio = float(N) / float(T)
        if bw == 0:   # the band is the centre column alone: the path is the staircase itself, from the row where it reaches 1
            segrow = np.array([first_row_reaching(j + 1, ratio, 1, T - 1) for j in range(N - 1)], dtype=np.uint32)
        else:
            segrow = make_path(T, N, bw, ratio, how, rng, stall, start)
        reads.append(SimpleNamespace(label=label, T=T, N=N, bw=bw, ratio=ratio, status=status, segrow=segrow))

    add("N = 2: one output row, the band covers every column", 40, 2, 25)
    add("T = N = 3: the band covers every column", 3, 3, 25)
    add("bw = N / 2 clamped, N = 10", 90, 10, 25)                       # read 2: the first of the range [2, 9)
    add("bw = N / 2 clamped, N = 11", 95, 11, 25)
    add("a half band of N - 1 (no clamp: harness only) covers every column", 300, 40, 0, bw=39)
    add("only the upper edge is ever real (N = 4, bw = 2)", 40, 4, 25, "high")
    add("a failed read between ok reads", 200, 60, 10, status=7)
    add("only the lower edge is ever real (a path that starts at row 200: harness only)", 400, 36, 25, "low", start=200)
    add("on the lower edge for a run of rows", 3000, 300, 25, "low")   # read 8: the last of the range [2, 9)
    add("on the upper edge for a run of rows", 3000, 300, 25, "high")
    add("bw = 1: a row on either edge", 200, 50, 1)
    add("bw = 1, hugging low", 150, 50, 1, "low")
    add("bw = 1, hugging high", 150, 50, 1, "high")
    add("bw = 0 (no band the aligner builds: harness only): both slacks 0 on one row, counted once", 120, 30, 0, bw=0)
    for N in (256, 257, 258, 1001):                                     # N - 1 = 255, 256, 257 and ~1 000 output rows
        add("N - 1 = %d output rows" % (N - 1), 4 * N + 3, N, 25, ("low", "high", "random", "random")[N % 4])
    add("a stall of 20 001 rows across many staircase steps", 24000, 400, 210, stall=(150, 20001))
    add("a stall that lasts until the lower edge reaches it", 24000, 400, 180, "high", stall=(150, 20001))
    # T about 100 001 with ratios whose products land within one ulp of an integer (drawn until some do)
    drawn = 0
    for k, (T, N) in enumerate([(100000, 1000), (100001, 9091)]):   # T a multiple of N: every (T / N)-th product is an integer
        add("T = %d, N = %d: T a multiple of N" % (T, N), T, N, 25, ("low", "high")[k])
    while drawn < 4:
        T, N = 100001 - int(rng.integers(0, 50)), int(rng.integers(300, 2500))
        if near_integer_products(T, float(N) / float(T)).size:
            add("T = %d, N = %d: products within an ulp of an integer" % (T, N), T, N, 25, ("low", "high", "random")[drawn % 3])
            drawn += 1
    for k in range(6):
        T = int(rng.integers(60, 900))
        N = int(rng.integers(2, max(3, T // 2)))
        add("random %d" % k, T, N, int(rng.integers(1, 40)), ("low", "high", "random")[k % 3])
    b = SimpleNamespace(reads=reads)
    order = rng.permutation(len(reads))
    seg_off = np.concatenate([[0], np.cumsum([r.N - 1 for r in reads])]).astype(np.uint64)
    b.segrow = np.concatenate([r.segrow for r in reads]).astype(np.uint32)
    b.status = np.array([r.status for r in reads], dtype=np.int32)
    b.read = order.astype(np.uint32)
    b.seg_off = np.array([seg_off[i] for i in order], dtype=np.uint64)
    b.T = np.array([reads[i].T for i in order], dtype=np.uint32)
    b.N = np.array([reads[i].N for i in order], dtype=np.uint32)
    b.bw = np.array([reads[i].bw for i in order], dtype=np.uint32)
    b.ratio = np.array([reads[i].ratio for i in order], dtype=np.float64)
    return b


def reference(b, lo=0, hi=None, fn=brute, untouched=0xdeadbeef, **kw):
    """(low, high, edge_rows) uint32 arrays over the reads: the definition for the ok reads of [lo, hi), NONE, NONE, 0 for the
    failed ones of that range, ``untouched`` outside it (what the harness fills its arrays with beforehand)"""
    n = len(b.reads)
    hi = n if hi is None else hi
    out = np.full((3, n), untouched, dtype=np.uint32)
    for i, r in enumerate(b.reads):
        if not lo <= i < hi:
            continue
        out[:, i] = (NONE, NONE, 0) if r.status != 0 else fn(r.segrow, r.T, r.N, r.bw, r.ratio, **kw)
    return out


def margins_of_result(res, i, T, band, wrong=None):
    """the definition over what a batch returned for read i: its borders (signal_positions + 1 = the lattice row of each output
    row's first cell), T = signal length + 1, N = output rows + 1, bw = min(band / 2, N / 2), ratio = N / T"""
    a = int(res.seg_offsets[i])
    ns = int(res.n_segments[i])
    N = ns + 1
    segrow = res.signal_positions[a:a + ns].astype(np.int64) + 1
    return brute(segrow, T, N, min(band // 2, N // 2), float(N) / float(T))


# The reads of the GPU retry test (tests/test_gpu_band_margin.py), picked on the CPU oracle alone and held to it by
# tests/test_band_margin_host.py: family, min_margin, read -> the first band of the chain 50, 100, 200, ... at which
# min(low, high) >= min_margin (flagged at band 50), and reads whose margin passes at band 50 already (never retried).
RETRY_FAMILY = "rna002_squeezed_band50"
RETRY_MIN_MARGIN = 1
RETRY_FLAGGED = {0: 200, 8: 100, 9: 200, 13: 100}
RETRY_CLEAN = (3, 5, 7)
RETRY_CHAIN = (50, 100, 200, 400)
