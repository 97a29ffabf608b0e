"""The per-site level summary (dyn_aligner_set_site_summary), restated with Python ints, and the inputs of its device harness.

The DEFINITION over a list of output rows (site id, samples):
    S1       chunked fp64 sum of x (chunks of 64, each left to right, the chunk sums left to right)
    m        S1 / L, one IEEE division: level_mean of dyn_event_out
    m1, m2   m * 2**40 and (m * m, one IEEE product) * 2**40 rounded to an integer, ties to even -- through fractions.Fraction
    no site  id == DYN_SITE_NONE: counted in rows_without_site
    skipped  id >= num_sites, a non-finite m or m * m >= 2**64: counted in rows_skipped
    per site: n_rows, n_samples = sum L, dwell_sq = sum L * L, M1 = sum m1, M2 = sum m2 (Python ints: unbounded, so limb
    arithmetic cannot hide here)
`limbs()` turns the sums into the seven uint64 arrays of the C interface (dwell_sq mod 2**64, M1 / M2 128-bit two's complement).
Row j of a read takes the id of base j + k // 2 (`row_ids`).

A BATCH is what launch.cpp hands the kernels (tests/device_math/site_summary.hip): descriptors in processing order, the signal
pool, the borders (segrow), the site id of every output row. build_batch() holds every case the issue names. Deliberately WRONG
accumulations (carry dropped, high limb not sign-extended, m1 / m2 truncated, m = S1 * (1 / L), row j keyed by ids[j]) are
computed on the host from the same inputs: tests/test_site_summary_host.py shows that each differs from the right one.
"""
import numpy as np

from kmer_summary_cases import chunked, rint_scaled

NUM_SITES = 40
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
TOTALS = ("reads_ok", "rows_added", "samples_added", "rows_without_site", "rows_skipped")
COLS = ("n_rows", "n_samples", "dwell_sq", "M1", "M2")


def row_terms(x, truncate=False, reciprocal=False):
    """(L, m1, m2) of one row, or None when the definition skips it"""
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    with np.errstate(over="ignore", invalid="ignore"):
        s1 = np.float64(chunked(x))
        m = s1 * (np.float64(1.0) / np.float64(L)) if reciprocal else s1 / np.float64(L)
        mm = m * m
    if not np.isfinite(m) or not mm < 2.0 ** 64:
        return None
    return L, rint_scaled(m, truncate), rint_scaled(mm, truncate)


def empty(num_sites):
    acc = {c: [0] * num_sites for c in COLS}
    acc["totals"] = dict.fromkeys(TOTALS, 0)
    return acc


def add_read(acc, ids, segments, **how):
    """one ok read: segments[j] (arrays of samples) is output row j, ids[j] its site"""
    num_sites = len(acc["n_rows"])
    acc["totals"]["reads_ok"] += 1
    for s, x in zip(ids, segments):
        s = int(s)
        if s == NONE:
            acc["totals"]["rows_without_site"] += 1
            continue
        t = row_terms(x, **how) if s < num_sites else None
        if t is None:
            acc["totals"]["rows_skipped"] += 1
            continue
        L, m1, m2 = t
        acc["n_rows"][s] += 1
        acc["n_samples"][s] += L
        acc["dwell_sq"][s] += L * L
        acc["M1"][s] += m1
        acc["M2"][s] += m2
        acc["totals"]["rows_added"] += 1
        acc["totals"]["samples_added"] += L
    return acc


def row_ids(base_ids, n_rows, k, shift=None):
    """the ids of a read's output rows from its per-base ids: row j <- base j + k // 2 (shift: a wrong one)"""
    h = k // 2 if shift is None else shift
    return [int(v) for v in np.asarray(base_ids)[h:h + n_rows]]


def add_aligned_read(acc, base_ids, k, signal, signal_positions, shift=None, **how):
    """one ok read from what a batch returned: its per-base ids, the signal it aligned and its rows' first samples"""
    x = np.asarray(signal, dtype=np.float64)
    b = [int(s) for s in signal_positions] + [len(x)]
    n = len(signal_positions)
    return add_read(acc, row_ids(base_ids, n, k, shift), [x[b[j]:b[j + 1]] for j in range(n)], **how)


def limbs(acc):
    """the seven uint64 arrays of dyn_aligner_site_summary_fetch and the five totals"""
    out = [np.array([v & M64 for v in acc[c]], dtype=np.uint64) for c in ("n_rows", "n_samples", "dwell_sq")]
    for name in ("M1", "M2"):
        tw = [v & M128 for v in acc[name]]
        out.append(np.array([v & M64 for v in tw], dtype=np.uint64))
        out.append(np.array([v >> 64 for v in tw], dtype=np.uint64))
    return out, np.array([acc["totals"][k] for k in TOTALS], dtype=np.uint64)


def summed(a, b):
    out = {c: [x + y for x, y in zip(a[c], b[c])] for c in COLS}
    out["totals"] = {k: a["totals"][k] + b["totals"][k] for k in TOTALS}
    return out


# ---- the device harness's batch --------------------------------------------------------------------------------------------
class Batch:
    pass


def _reads():
    """(status, [(site id, samples)]) per read, in read-index order"""
    rng = np.random.default_rng(20261)
    norm = lambda n: rng.normal(0.2, 1.1, n)  # noqa: E731
    reads = []
    # the chunk (64) and kernel (256) borders, one site each; lengths whose 1 / L is inexact (63, 65, 257)
    reads.append((0, [(s, norm(L)) for s, L in zip(range(0, 6), (1, 63, 64, 65, 256, 257))]))
    # the chunk loop's wrap at 256 chunks (16 384 samples) and beyond; short neighbours between the long ones
    reads.append((0, [(6, norm(16384)), (7, norm(3)), (8, norm(16385 + 7)), (7, norm(255))]))
    # no site, the last site, the first id outside the table -- in both kernels (1 .. 7 samples, 257 .. 300 samples)
    reads.append((0, [(NONE, norm(5)), (NUM_SITES - 1, norm(7)), (NUM_SITES, norm(4)), (NONE, norm(257)), (NUM_SITES - 1, norm(300)),
                      (NUM_SITES, norm(258)), (NONE - 1, norm(2)), (NONE, norm(1))]))
    # a failed read between ok reads: nothing of it may be added
    reads.append((7, [(s, np.full(5, 1000.0)) for s in (0, 6, 11, 12, 20)]))
    # 300 rows on ONE site from two blocks of one read, level about +2^22: m1 about 2^62 each, the low limb wraps some 70 times
    # and M1 ends near 2^70; M2 (about 2^84 per row) lives in the high limb and takes the low limb's carries
    reads.append((0, [(11, 2.0 ** 22 + rng.normal(0.0, 300.0, int(L))) for L in rng.integers(1, 6, 300)]))
    # the same with negative means on another site, and 300 more rows of both signs on site 11 from a second read
    reads.append((0, [(12, -2.0 ** 22 + rng.normal(0.0, 300.0, int(L))) for L in rng.integers(1, 6, 300)]))
    reads.append((0, [(11, (2.0 ** 22 if j % 3 else -2.0 ** 22) + rng.normal(0.0, 300.0, 3)) for j in range(300)]))
    # m * m = 2^64 exactly (skipped), the double just below 2^32 (kept: m2 = 2^104 - 2^52), -2^32 (skipped), a NaN sample and an
    # infinity (skipped), and a finite neighbour on the same site
    reads.append((0, [(14, np.array([2.0 ** 32])), (14, np.array([np.nextafter(2.0 ** 32, 0.0)] * 2)), (15, np.array([1.0, np.nan, 2.0])),
                      (15, np.array([np.inf])), (15, np.array([0.5])), (14, np.array([-2.0 ** 32] * 3)),
                      (15, np.concatenate([norm(300), [np.nan]]))]))
    # ties of rint: m1 = 0.5, 1.5, 2.5 and their negatives -> 0, 2, 2, -0, -2, -2 (truncation gives 0, 1, 2, 0, -1, -2); and
    # fractions that round away from the truncated value (0.75 -> 1, -0.75 -> -1)
    h = 2.0 ** -41
    reads.append((0, [(17 + (v < 0), np.array([v * h])) for v in (1.0, 3.0, 5.0, -1.0, -3.0, -5.0)] +
                  [(19, np.array([1.5 * h])), (20, np.array([-1.5 * h]))]))
    # -0.0 and denormals: all round to zero, the counts still move
    reads.append((0, [(16, np.array([-0.0])), (16, np.array([-0.0, 5e-324, -5e-324, 1e-310])), (16, np.array([2.0 ** -1074] * 70))]))
    # overlapping reads: the sites 21 .. 30 covered by three reads at different offsets, NONE runs inside
    for start in (21, 23, 26):
        ids = [s if s <= 30 else NONE for s in range(start, start + 8)]
        ids[3] = NONE
        reads.append((0, [(s, norm(int(L))) for s, L in zip(ids, rng.integers(2, 40, 8))]))
    return reads


def build_batch():
    reads = _reads()
    b = Batch()
    b.reads = reads
    b.num_sites = NUM_SITES
    n = len(reads)
    sig, segrow, sites = [], [], []
    sig_off, par_off, seg_off = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    T, N = (np.zeros(n, dtype=np.uint32) for _ in range(2))
    o_sig = o_seg = 0
    for i, (_, segs) in enumerate(reads):
        lens = [len(x) for _, x in segs]
        sig_off[i], par_off[i], seg_off[i] = o_sig, o_seg, o_seg
        T[i], N[i] = sum(lens) + 1, len(segs) + 1
        segrow += list(1 + np.concatenate([[0], np.cumsum(lens)[:-1]]))   # lattice row of each row's first sample
        sites += [s for s, _ in segs]
        sig += [x for _, x in segs]
        o_sig += sum(lens)
        o_seg += len(segs)
    b.sig = np.ascontiguousarray(np.concatenate(sig), dtype=np.float64)
    b.segrow = np.array(segrow, dtype=np.uint32)
    b.sites = np.array(sites, dtype=np.uint32)
    b.status = np.array([s for s, _ in reads], dtype=np.int32)
    # processing order: longest first (launch.cpp sorts by cost), so descriptor k is not read k
    order = np.argsort(-T.astype(np.int64), kind="stable")
    b.read = order.astype(np.uint32)
    b.sig_off, b.par_off, b.seg_off, b.T, b.N = sig_off[order], par_off[order], seg_off[order], T[order], N[order]
    for a in (b.sig, b.segrow, b.sites, b.status, b.read, b.sig_off, b.par_off, b.seg_off, b.T, b.N):
        a.setflags(write=False)
    return b


def reference(b, lo=0, hi=None, num_sites=None, **how):
    """the definition over the ok reads [lo, hi) of the batch, for a table of num_sites"""
    acc = empty(b.num_sites if num_sites is None else num_sites)
    for i, (status, segs) in enumerate(b.reads):
        if status == 0 and lo <= i < (len(b.reads) if hi is None else hi):
            add_read(acc, [s for s, _ in segs], [x for _, x in segs], **how)
    return acc


def wrong_limbs(b, how):
    """The seven arrays as a WRONG accumulation would leave them, rows added in read order:
    'carry_dropped' the high limb never receives the carry of the low one; 'no_sign_extension' a negative value's high limb is
    zero instead of all ones; 'truncated' m1 / m2 cut towards zero instead of rint; 'reciprocal' m = S1 * (1 / L)."""
    if how == "truncated":
        return limbs(reference(b, truncate=True))[0]
    if how == "reciprocal":
        return limbs(reference(b, reciprocal=True))[0]
    right = reference(b)
    cols = [np.array([v & M64 for v in right[c]], dtype=np.uint64) for c in ("n_rows", "n_samples", "dwell_sq")]
    lo = {"M1": [0] * b.num_sites, "M2": [0] * b.num_sites}
    hi = {"M1": [0] * b.num_sites, "M2": [0] * b.num_sites}
    for status, segs in b.reads:
        if status != 0:
            continue
        for s, x in segs:
            t = row_terms(x) if s < b.num_sites else None
            if t is None:
                continue
            for name, v in (("M1", t[1]), ("M2", t[2])):
                tw = v & M128
                l, h = tw & M64, tw >> 64
                if how == "no_sign_extension" and v < 0:
                    h = 0
                c = lo[name][s] + l
                carry = c >> 64
                lo[name][s] = c & M64
                hi[name][s] = (hi[name][s] + h + (0 if how == "carry_dropped" else carry)) & M64
    for name in ("M1", "M2"):
        cols.append(np.array(lo[name], dtype=np.uint64))
        cols.append(np.array(hi[name], dtype=np.uint64))
    return cols
