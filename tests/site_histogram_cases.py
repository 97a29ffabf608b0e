"""The per-site histograms and quantiles (dyn_aligner_set_site_histogram, dyn_aligner_site_quantiles), restated with NumPy
doubles and Python ints over the row model of tests/site_summary_cases.py, and the inputs of their device harness.

The DEFINITION. A row is counted iff the per-site table adds it (site_summary_cases.row_terms is not
None, id < num_sites, an ok read). With inv_w = float64(bins) / (float64(hi) - float64(lo)) and m = S1 / L as the table forms it:
    level    u = (m - lo) * inv_w, one IEEE subtraction and one IEEE product; u < 0: counter 0; u >= bins: counter bins + 1;
             otherwise counter 1 + int(u)
    dwell    min(L.bit_length() - 1, 15)
    per site H = bins + 2 + 16 counters: [under, level bins 1 .. bins, over, dwell bins 0 .. 15]
Quantiles of one site's B = bins + 2 level counters: n = their sum, k = min(max(ceil(q * n), 1), n) with q * n one IEEE product,
bin = the smallest index whose inclusive prefix sum (Python ints) is >= k, below = the prefix sum in front of it, in_bin = its
count; n = 0: bin = 0xFFFFFFFF, rank = below = in_bin = 0.

Deliberately WRONG versions (`how=`) are computed from the same inputs; tests/test_site_histogram_host.py shows that each
differs from the right one on the harness inputs: 'float32' binning, 'rint' for truncation, 'clamped' under / over, and for the
quantiles 'prefix_gt' (prefix > k), 'floor' (k = floor(q n)); a row stride of bins instead of H is shown on the flat counter
array (`flat`, `wrong_stride_level`). 'gt' (u > bins for >=) is kept to show that it CANNOT differ: the only u it treats otherwise
is u == bins, and 1 + int(bins) is the over counter's index.
"""
import math

import numpy as np

import site_summary_cases as ssc
from kmer_summary_cases import chunked

DWELL_BINS = 16
NO_BIN = 0xFFFFFFFF
EXACT = (32, -4.0, 4.0)      # inv_w = 4 exactly
ROUNDED = (30, -3.3, 4.1)    # inv_w is rounded
PROBS = (0.0, 1e-12, 0.25, 0.5, 0.75, 1.0)
PROBS8 = (0.0, 1e-12, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0)


def inv_width(bins, lo, hi):
    return np.float64(bins) / (np.float64(hi) - np.float64(lo))


def level_bin(m, bins, lo, hi, how=None):
    """the level counter (0 .. bins + 1) of an event mean m"""
    m = np.float64(m)
    if how == "float32":
        u = float((np.float32(m) - np.float32(lo)) * np.float32(inv_width(bins, lo, hi)))
    else:
        u = float((m - np.float64(lo)) * inv_width(bins, lo, hi))
    if how == "clamped":
        return min(max(1 + int(math.floor(u)), 1), bins) if math.isfinite(u) else (1 if u < 0 else bins)
    if u < 0:
        return 0
    if (u > bins) if how == "gt" else (u >= bins):
        return bins + 1
    return 1 + (int(np.rint(u)) if how == "rint" else int(u))   # ('gt' lets u == bins through: 1 + bins IS the over counter)


def dwell_bin(L):
    return min(int(L).bit_length() - 1, DWELL_BINS - 1)


def row_mean(x):
    """m of one row as the table forms it, or None when the table skips the row"""
    x = np.asarray(x, dtype=np.float64)
    if ssc.row_terms(x) is None:
        return None
    return np.float64(chunked(x)) / np.float64(len(x))


def empty(num_sites, bins):
    return {"level": [[0] * (bins + 2) for _ in range(num_sites)], "dwell": [[0] * DWELL_BINS for _ in range(num_sites)]}


def add_read(h, ids, segments, bins, lo, hi, how=None):
    """one ok read: segments[j] is output row j, ids[j] its site"""
    num_sites = len(h["level"])
    for s, x in zip(ids, segments):
        s = int(s)
        if s == ssc.NONE or s >= num_sites:
            continue
        m = row_mean(x)
        if m is None:
            continue
        lb = level_bin(m, bins, lo, hi, how)
        if lb <= bins + 1:            # ('rint' can step past the over counter: such a row is simply another table)
            h["level"][s][lb] += 1
        h["dwell"][s][dwell_bin(len(x))] += 1
    return h


def add_aligned_read(h, base_ids, k, signal, signal_positions, bins, lo, hi):
    x = np.asarray(signal, dtype=np.float64)
    b = [int(s) for s in signal_positions] + [len(x)]
    n = len(signal_positions)
    return add_read(h, ssc.row_ids(base_ids, n, k), [x[b[j]:b[j + 1]] for j in range(n)], bins, lo, hi)


def reference(b, bins, lo, hi, read_lo=0, read_hi=None, how=None):
    """the definition over the ok reads [read_lo, read_hi) of a batch"""
    h = empty(b.num_sites, bins)
    for i, (status, segs) in enumerate(b.reads):
        if status == 0 and read_lo <= i < (len(b.reads) if read_hi is None else read_hi):
            add_read(h, [s for s, _ in segs], [x for _, x in segs], bins, lo, hi, how)
    return h


def flat(h):
    """the counters as the device holds them: uint32 [num_sites * H]"""
    return np.array([row_l + row_d for row_l, row_d in zip(h["level"], h["dwell"])], dtype=np.uint32).reshape(-1)


def wrong_stride_level(flat_counters, num_sites, bins):
    """the level counters a reader would see that steps from site to site by `bins` words instead of H"""
    return np.array([flat_counters[s * bins:s * bins + bins + 2] for s in range(num_sites)], dtype=np.uint32)


def quantiles(counts, probs, how=None):
    """(n, [(rank, bin, below, in_bin) per probability]) of one site's level counters"""
    counts = [int(c) for c in counts]
    n = sum(counts)
    out = []
    for q in probs:
        if n == 0:
            out.append((0, NO_BIN, 0, 0))
            continue
        qn = float(np.float64(q) * np.float64(n))
        k = min(max(int(math.floor(qn)) if how == "floor" else int(math.ceil(qn)), 1), n)
        prefix = 0
        for i, c in enumerate(counts):
            if (prefix + c > k) if how == "prefix_gt" else (prefix + c >= k):
                out.append((k, i, prefix, c))
                break
            prefix += c
        else:
            out.append((k, NO_BIN, 0, 0))   # ('prefix_gt' at q = 1: no counter's prefix exceeds n)
    return n, out


def quantile_arrays(level_rows, probs, how=None):
    """n [sites] and rank, bin, below, in_bin [sites, probs] as uint32, the layout of dyn_aligner_site_quantiles"""
    n = np.zeros(len(level_rows), dtype=np.uint32)
    cols = [np.zeros((len(level_rows), len(probs)), dtype=np.uint32) for _ in range(4)]
    for s, row in enumerate(level_rows):
        n[s], per = quantiles(row, probs, how)
        for q, vals in enumerate(per):
            for f in range(4):
                cols[f][s, q] = vals[f]
    return n, cols


# ---- the device harness's inputs -----------------------------------------------------------------------------------------------
def exact_edge_samples():
    """(32, -4, 4): -4 and the double below it, 4 and the double below it, every interior edge and its lower neighbour"""
    bins, lo, hi = EXACT
    v = [lo, np.nextafter(lo, -np.inf), hi, np.nextafter(hi, 0.0)]
    for i in range(1, bins):
        e = lo + i * (hi - lo) / bins   # multiples of 0.25: exact
        v += [e, np.nextafter(e, -np.inf)]
    return [float(x) for x in v]


def edge_neighbours(spec=ROUNDED, ulps=8):
    """the 527 doubles within 8 ulp of the 31 nominal edges lo + i * w of (30, -3.3, 4.1)"""
    bins, lo, hi = spec
    w = (np.float64(hi) - np.float64(lo)) / np.float64(bins)
    out = []
    for i in range(bins + 1):
        e = np.float64(lo) + np.float64(i) * w
        down = [e]
        for _ in range(ulps):
            down.append(np.nextafter(down[-1], -np.inf))
        up = [e]
        for _ in range(ulps):
            up.append(np.nextafter(up[-1], np.inf))
        out += down[:0:-1] + [e] + up[1:]
    return [float(x) for x in out]


DWELL_ROWS = (1, 2, 3, 4, 32767, 32768, 40000)


def extra_reads():
    """three reads more than site_summary_cases' batch: single-sample rows on the edges of EXACT (site 31) and around the edges of
    ROUNDED (site 32), where m is the sample; and rows of 1 .. 40 000 samples for the dwell bins (sites 33 .. 38), both kernels"""
    rng = np.random.default_rng(20262)
    one = lambda vals, site: [(site, np.array([v])) for v in vals]  # noqa: E731
    return [(0, one(exact_edge_samples(), 31)), (0, one(edge_neighbours(), 32)),
            (0, [(33 + j % 6, rng.normal(0.1, 1.2, L)) for j, L in enumerate(DWELL_ROWS)])]


def pack(reads, num_sites=ssc.NUM_SITES):
    """what launch.cpp hands the kernels, laid out as site_summary_cases.build_batch lays it out"""
    b = ssc.Batch()
    b.reads = reads
    b.num_sites = num_sites
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
    order = np.argsort(-T.astype(np.int64), kind="stable")   # processing order: longest first
    b.read = order.astype(np.uint32)
    b.sig_off, b.par_off, b.seg_off, b.T, b.N = sig_off[order], par_off[order], seg_off[order], T[order], N[order]
    return b


def build_batch():
    """site_summary_cases.build_batch()'s reads (rows of 1 .. 16 392 samples, both kernels, a failed read, skipped and site-less
    rows) and extra_reads() behind them"""
    return pack(ssc._reads() + extra_reads())


def quantile_tables():
    """{B: uint32 [100, B + 16]}: level histograms of 100 sites for B = 4, 34, 66 and 256 counters (dwell words poisoned: the
    kernel must not read them into a sum). Sites 0 .. 9 hold the named cases, the others random counts of mixed density."""
    out = {}
    for B in (4, 34, 66, 256):
        rng = np.random.default_rng(900 + B)
        t = np.zeros((100, B + DWELL_BINS), dtype=np.uint32)
        t[:, B:] = 0xABCD0000
        lv = t[:, :B]
        # site 0, 3: empty. 1: all mass under. 2: all mass over. 4: a single count, in the last interior bin
        lv[1, 0] = 7
        lv[2, B - 1] = 9
        lv[4, B - 2] = 1
        # 5: the prefix sum meets k exactly at a bin's end (4 rows: 1 | 1 | 2; k = 1 and 2 of q = 0.25, 0.5 end counters 0 and 1)
        lv[5, 0], lv[5, 1], lv[5, B - 1] = 1, 1, 2
        # 6: 2^31 beside small ones -- the prefix sum needs bit 31; 7: 2^31 + 2^30 + small: below 2^32 in all
        lv[6, 0], lv[6, 1], lv[6, B - 1] = 3, 1 << 31, 5
        lv[7, 0], lv[7, B // 2], lv[7, B - 1] = 1 << 30, 1 << 31, 11
        # 8: one count in every counter; 9: the first and the last counter only
        lv[8, :] = 1
        lv[9, 0], lv[9, B - 1] = 2, 2
        for s in range(10, 100):
            dense = rng.random(B) < (0.1 if s % 3 else 0.9)
            lv[s, :] = np.where(dense, rng.integers(1, 50 if s % 2 else 5000, B), 0)
        out[B] = t
    return out
