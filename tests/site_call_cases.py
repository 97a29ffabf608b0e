"""The per-read site calls (dyn_aligner_set_site_calls) restated in Python floats: one IEEE fp64 operation
per operation of the definition. exp is the library's strict exp built for the host with g++ from dp_math_strict.hpp
(site_mixture_cases.exp_lib), not math.exp. Also the batch, the model and the upload windows of the device harness
(tests/device_math/site_calls.hip).

``call(..., wrong=...)`` and ``event_mean(..., wrong=...)`` restate WRONG versions a kernel could compute instead;
tests/test_site_call_host.py asserts that the built rows tell each of them from the definition."""
import math
import struct

import numpy as np

import site_mixture_cases as smc
from kmer_summary_cases import chunked

NONE = 0xFFFFFFFF
NAN_BITS = 0x7FF8000000000000
NAN = struct.unpack("<d", struct.pack("<Q", NAN_BITS))[0]
COLUMNS = ("pi1", "mu0", "mu1", "var0", "var1")
WRONG = ("pi0_half", "swapped", "z_var1", "value_without_two", "chunk_order", "chunk_wrap")
SUM_WRONG = ("chunk_order", "chunk_wrap")      # wrong sums of a row above SHORT_MAX samples: they move m
SHORT_MAX = 256


def bits(values):
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def is_set(row):
    return row[3] > 0.0 and math.isfinite(row[1]) and math.isfinite(row[3])


def is_two(row):
    return is_set(row) and 0.0 < row[0] < 1.0 and row[4] > 0.0 and math.isfinite(row[2]) and math.isfinite(row[4])


def event_mean(x, wrong=None):
    """m of one row: the chunked sum (chunks of 64 left to right, the chunk sums left to right) over L, one IEEE division.
    wrong = "chunk_order": the chunk sums added from the last to the first; "chunk_wrap": lane l of 256 adds the chunks l, l + 256, ..
    and the lanes' partials are added in order (the same additions up to 256 chunks, others beyond)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if wrong == "chunk_order":
            sums = [np.add.accumulate(x[c:c + 64])[-1] for c in range(0, len(x), 64)]
            s1 = np.add.accumulate(np.array(sums[::-1]))[-1]
        elif wrong == "chunk_wrap":
            sums = [np.add.accumulate(x[c:c + 64])[-1] for c in range(0, len(x), 64)]
            s1 = np.add.accumulate(np.array([np.add.accumulate(np.array(sums[l::256]))[-1] for l in range(min(256, len(sums)))]))[-1]
        else:
            s1 = chunked(x)
        return float(np.float64(s1) / np.float64(len(x)))


def call(row, m, wrong=None):
    """(site_probability, site_z) of a row with event mean m against the model row (pi1, mu0, mu1, var0, var1), or (NAN, NAN); the
    caller has looked at the id, the map and the row's length"""
    pi1, mu0, mu1, var0, var1 = (float(v) for v in row)
    if not math.isfinite(m) or not m * m < 2.0 ** 64:
        return NAN, NAN
    if not is_set(row):
        return NAN, NAN
    z = (m - mu0) / math.sqrt(var1 if wrong == "z_var1" and var1 > 0 else var0)
    if not is_two(row):
        if wrong != "value_without_two" or not var1 > 0.0 or not math.isfinite(mu1 + var1):
            return NAN, z
    pi0 = 0.5 if wrong == "pi0_half" else 1.0 - pi1
    if wrong == "swapped":
        pi0, pi1, mu0, mu1, var0, var1 = pi1, pi0, mu1, mu0, var1, var0
    try:
        a0, a1 = pi0 / math.sqrt(var0), pi1 / math.sqrt(var1)
        d0, d1 = m - mu0, m - mu1
        q0, q1 = -0.5 * ((d0 * d0) / var0), -0.5 * ((d1 * d1) / var1)
        up = q1 > q0
        e = smc.exp_strict(q0 - q1 if up else q1 - q0)
        p0, p1 = a0 * (e if up else 1.0), a1 * (1.0 if up else e)
        s = p0 + p1
        g = p1 / s
    except ZeroDivisionError:
        g = NAN
    return (NAN if g != g else g), (NAN if z != z else z)


def reference(reads, model, num_sites, read_lo, read_hi, present=None, poison=None, wrong=None):
    """the two columns over every output row of ``reads`` ((status, [(id, samples)]) in read order, the rows laid out read after
    read): rows of reads that are not ok or outside [read_lo, read_hi) keep ``poison``. model: {id: row}; present: the ids a
    sparse map holds (None: a dense table)."""
    prob, z = [], []
    for i, (status, segs) in enumerate(reads):
        for s, x in segs:
            if status != 0 or not read_lo <= i < read_hi:
                prob.append(poison)
                z.append(poison)
                continue
            s = int(s)
            row = model.get(s) if s != NONE and s < num_sites and (present is None or s in present) else None
            if row is None or len(x) < 1:
                prob.append(NAN)
                z.append(NAN)
                continue
            long_row = len(x) > SHORT_MAX
            g, zz = call(row, event_mean(x, wrong if (wrong in SUM_WRONG and long_row) else None), None if wrong in SUM_WRONG else wrong)
            prob.append(g)
            z.append(zz)
    return np.array(prob, dtype=np.float64), np.array(z, dtype=np.float64)


# ---- the device harness's batch ------------------------------------------------------------------------------------------------------
NUM_SITES = 40
CAPACITY = 8                                   # of the sparse run: the probe window is the whole map, and window 1 fills it
TWO, UNSET, FAR, EQUAL, SHORT_ONLY, LATE = 0, 1, 6, 7, 8, 9
ONE_COMPONENT = (2, 3, 4, 5)
MODEL = {
    TWO: (0.3, -0.5, 0.8, 0.09, 0.16),
    UNSET: (0.0, 0.0, 0.0, 0.0, 0.0),
    2: (0.0, 0.1, 0.9, 0.25, 0.25),            # pi1 = 0: one component
    3: (1.0, 0.1, 0.9, 0.25, 0.25),            # pi1 = 1
    4: (0.4, 0.1, 0.9, 0.25, 0.0),             # var1 = 0
    5: (0.4, 0.1, float("inf"), 0.25, 0.25),   # mu1 not finite
    FAR: (0.5, 0.0, 100.0, 1.0, 1.0),          # the exp argument is 100 m - 5 000 below m = 50
    EQUAL: (0.25, -1.0, 1.0, 1.0, 1.0),        # m = 0: q_0 == q_1
    SHORT_ONLY: (0.6, 0.2, 0.7, 0.04, 0.09),
    LATE: (0.45, -0.2, 0.6, 0.05, 0.07),       # uploaded by the second window: a full sparse map has no bucket left for it
    12: (0.5, 0.0, 1.0, float("nan"), 1.0),    # var0 NaN: not set
    13: (0.5, float("-inf"), 1.0, 1.0, 1.0),   # mu0 not finite: not set
    14: (0.5, 0.0, 1.0, -1.0, 1.0),            # var0 < 0: not set
}
WINDOWS = ((0, 9), (9, 6))                     # (lo, count): sites 0 .. 8 hold CAPACITY set rows; then 9 .. 14 one more set row
SET_FIRST = (0, 2, 3, 4, 5, 6, 7, 8)


def model_rows(lo, count):
    return np.array([MODEL.get(s, (0.0,) * 5) for s in range(lo, lo + count)], dtype=np.float64)


def _reads():
    """(status, [(site id, samples)]) per read, in read-index order"""
    rng = np.random.default_rng(20290)
    near = lambda n: rng.normal(0.1, 0.5, n)  # noqa: E731
    one = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    reads = []
    # the short / long split and the wrap of the chunk loop, on the two-component site
    # (samples of mixed magnitude: the order of the additions shows in the sum's last bits)
    wide = lambda n: rng.normal(0.1, 0.5, n) * np.exp(rng.normal(0.0, 2.0, n))  # noqa: E731
    rows = [wide(L) for L in (1, 255, 256, 257, 16385 + 64)]
    # the last row's chunks 256 and 257 (the wrap's) are large and cancel: added early, as a lane-strided sum would, they round
    # every later addition differently
    rows[4][16384:16448] *= 4096.0
    rows[4][16448] = 0.25 - rows[4][16384:16448].sum()
    reads.append((0, [(TWO, x) for x in rows]))
    # a read of only short rows in the same launch: the long kernel leaves it alone
    reads.append((0, [(SHORT_ONLY, near(int(L))) for L in rng.integers(1, 40, 12)]))
    # a failed read and (read 3) a read outside [read_lo, read_hi): their rows keep the poison
    reads.append((7, [(TWO, near(5)), (TWO, near(300))]))
    reads.append((0, [(TWO, near(5)), (TWO, near(300))]))
    # the ids: none, the first id outside the table, the largest id; the unset rows; the one-component rows -- in both kernels
    ids = [NONE, NUM_SITES, NONE - 1, UNSET, 12, 13, 14, NUM_SITES - 1] + list(ONE_COMPONENT)
    reads.append((0, [(s, near(int(L))) for s, L in zip(ids, rng.integers(1, 30, len(ids)))] +
                  [(s, near(int(L))) for s, L in zip(ids, rng.integers(257, 330, len(ids)))]))
    # the exp argument: above -512 (44.9: -510), the special path (43: -700; 42.6: -740, a denormal; 40.24: -976, its underflow), the
    # exact +0 below -1 024 (39: -1 100; -2: -5 200), and the same on the other side of the crossing (102: component 1 takes all)
    reads.append((0, [(FAR, one(v)) for v in FAR_MEANS]))
    # q_0 == q_1 (m = 0 exactly, and -0.0), its neighbours on either side
    reads.append((0, [(EQUAL, one(v)) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-9, -1e-9)]))
    # m * m = 2^64 exactly (no call), the double just below 2^32 (a call), -2^32, a NaN sample, an infinity, in both kernels
    big = np.nextafter(2.0 ** 32, 0.0)
    reads.append((0, [(TWO, one(2.0 ** 32)), (TWO, np.array([big] * 2)), (TWO, np.array([-2.0 ** 32] * 3)), (TWO, np.array([1.0, np.nan, 2.0])),
                      (TWO, one(np.inf)), (TWO, np.concatenate([near(300), [np.nan]])), (TWO, np.full(260, 2.0 ** 32)), (TWO, np.full(258, big))]))
    # the site the second window uploads, in both kernels
    reads.append((0, [(LATE, near(9)), (LATE, near(400)), (TWO, near(9))]))
    # 300 short rows over the set sites: more than one block of one read
    sites = [TWO, SHORT_ONLY, EQUAL, LATE, 2, UNSET]
    reads.append((0, [(sites[j % len(sites)], near(int(L))) for j, L in enumerate(rng.integers(1, 20, 300))]))
    return reads


FAR_MEANS = (44.9, 43.0, 42.6, 40.24, 39.0, -2.0, 102.0, 50.0, 49.9, 55.12)
READ_LO, READ_HI = 0, 3                        # reads 0 .. 2 of the first run; the second run takes 4 .. the end
OUTSIDE = 3


class Batch:
    pass


def build_batch():
    """what launch.cpp hands the kernels, as tests/site_summary_cases.build_batch lays it out"""
    reads = _reads()
    b = Batch()
    b.reads = reads
    n = len(reads)
    sig, segrow, sites = [], [], []
    sig_off, par_off, seg_off = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    T, N = (np.zeros(n, dtype=np.uint32) for _ in range(2))
    o_sig = o_seg = 0
    for i, (_, segs) in enumerate(reads):
        lens = [len(x) for _, x in segs]
        sig_off[i], par_off[i], seg_off[i] = o_sig, o_seg, o_seg
        T[i], N[i] = sum(lens) + 1, len(segs) + 1
        segrow += list(1 + np.concatenate([[0], np.cumsum(lens)[:-1]]))
        sites += [s for s, _ in segs]
        sig += [x for _, x in segs]
        o_sig += sum(lens)
        o_seg += len(segs)
    b.sig = np.ascontiguousarray(np.concatenate(sig), dtype=np.float64)
    b.segrow = np.array(segrow, dtype=np.uint32)
    b.sites = np.array(sites, dtype=np.uint32)
    b.status = np.array([s for s, _ in reads], dtype=np.int32)
    order = np.argsort(-T.astype(np.int64), kind="stable")               # processing order: longest first
    b.read = order.astype(np.uint32)
    b.sig_off, b.par_off, b.seg_off, b.T, b.N = sig_off[order], par_off[order], seg_off[order], T[order], N[order]
    b.row_read = np.repeat(np.arange(n), [len(segs) for _, segs in reads])
    for a in (b.sig, b.segrow, b.sites, b.status, b.read, b.sig_off, b.par_off, b.seg_off, b.T, b.N):
        a.setflags(write=False)
    return b
