"""The per-k-mer level summary (dyn_aligner_set_kmer_summary), restated with Python ints, and the inputs of its device harness.

The DEFINITION over a list of segments (k-mer code, samples):
    S1, S2   chunked fp64 sums of x and x * x (chunks of 64, each left to right, the chunk sums left to right)
    q1, q2   S * 2**40 rounded to an integer, ties to even -- here through fractions.Fraction, no float rounding involved
    skipped  S2 >= 2**64 or a non-finite sum
    per k-mer: n_segments, n_samples, Q1 = sum q1, Q2 = sum q2 (Python ints: unbounded, so limb arithmetic cannot hide here)
`limbs()` turns the sums into the six uint64 arrays of the C interface (128-bit two's complement).

A BATCH is what launch.cpp hands the kernels (tests/device_math/kmer_summary.hip): descriptors in processing order, the
signal pool, the borders (segrow), the k-mer code of every lattice column. build_batch() holds every case the issue names.
Three deliberately WRONG accumulations (carry dropped, q truncated, high limb not sign-extended) are computed on the host from
the same batch: tests/test_kmer_summary_host.py shows that each differs from the right one, i.e. that these inputs can fail.
"""
from fractions import Fraction

import numpy as np

NUM_KMERS = 64
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
SCALE = 1 << 40
TOTALS = ("reads_ok", "segments", "samples", "skipped_segments")


def chunked(v):
    sums = np.array([np.add.accumulate(v[c:c + 64])[-1] for c in range(0, len(v), 64)])
    return np.add.accumulate(sums)[-1]


def rint_scaled(s, truncate=False):
    """S * 2**40 as an exact integer: ties to even (the definition), or cut towards zero (a wrong one)"""
    f = Fraction(float(s)) * SCALE
    if truncate:
        return int(f)          # int(Fraction) truncates towards zero
    return round(f)            # round(Fraction) rounds half to even


def segment_q(x, truncate=False):
    """(L, q1, q2) of one segment, or None when the definition skips it"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s1, s2 = chunked(x), chunked(x * x)
    if not (np.isfinite(s1) and np.isfinite(s2)) or s2 >= 2.0 ** 64:
        return None
    return len(x), rint_scaled(s1, truncate), rint_scaled(s2, truncate)


def empty(num_kmers):
    return {"n_segments": [0] * num_kmers, "n_samples": [0] * num_kmers, "Q1": [0] * num_kmers, "Q2": [0] * num_kmers,
            "totals": dict.fromkeys(TOTALS, 0)}


def add_read(acc, codes, segments, truncate=False):
    """one ok read: segments[j] (arrays of samples) belongs to k-mer codes[j]"""
    acc["totals"]["reads_ok"] += 1
    for c, x in zip(codes, segments):
        q = segment_q(x, truncate)
        if q is None:
            acc["totals"]["skipped_segments"] += 1
            continue
        L, q1, q2 = q
        acc["n_segments"][c] += 1
        acc["n_samples"][c] += L
        acc["Q1"][c] += q1
        acc["Q2"][c] += q2
        acc["totals"]["segments"] += 1
        acc["totals"]["samples"] += L
    return acc


def add_aligned_read(acc, codes, signal, signal_positions, truncate=False):
    """one ok read from what a batch returned: its k-mer codes, the signal it aligned and its segments' first samples"""
    x = np.asarray(signal, dtype=np.float64)
    b = [int(s) for s in signal_positions] + [len(x)]
    assert len(codes) == len(signal_positions)
    return add_read(acc, [int(c) for c in codes], [x[b[j]:b[j + 1]] for j in range(len(codes))], truncate)


def limbs(acc):
    """the six uint64 arrays of dyn_aligner_kmer_summary_fetch and the four totals"""
    n = len(acc["n_segments"])
    out = [np.array([v & M64 for v in acc["n_segments"]], dtype=np.uint64), np.array([v & M64 for v in acc["n_samples"]], dtype=np.uint64)]
    for name in ("Q1", "Q2"):
        tw = [v & M128 for v in acc[name]]
        out.append(np.array([v & M64 for v in tw], dtype=np.uint64))
        out.append(np.array([v >> 64 for v in tw], dtype=np.uint64))
    assert all(len(a) == n for a in out)
    return out, np.array([acc["totals"][k] for k in TOTALS], dtype=np.uint64)


def summed(a, b):
    out = empty(len(a["n_segments"]))
    for k in ("n_segments", "n_samples", "Q1", "Q2"):
        out[k] = [x + y for x, y in zip(a[k], b[k])]
    out["totals"] = {k: a["totals"][k] + b["totals"][k] for k in TOTALS}
    return out


# ---- the device harness's batch --------------------------------------------------------------------------------------------
class Batch:
    pass


def _reads():
    """(status, [(code, samples)]) per read, in read-index order"""
    rng = np.random.default_rng(20260)
    norm = lambda n: rng.normal(0.2, 1.1, n)  # noqa: E731
    reads = []
    # the chunk (64) and kernel (256) borders, one k-mer each
    reads.append((0, [(c, norm(L)) for c, L in zip(range(0, 6), (1, 63, 64, 65, 256, 257))]))
    # the chunk loop's wrap at 256 chunks (16 384 samples) and beyond; short neighbours between the long ones
    reads.append((0, [(6, norm(16384)), (7, norm(3)), (8, norm(16385)), (7, norm(255))]))
    reads.append((0, [(9, norm(20001)), (10, norm(2))]))
    # a failed read between ok reads: nothing of it may be added (its values would move every sum it touches)
    reads.append((7, [(c, np.full(5, 1000.0)) for c in (0, 6, 11, 12, 20)]))
    # one k-mer hit by 5 000 segments from many blocks (10 reads x 500 rows: two blocks of 256 rows each), dwell 1 .. 4
    for _ in range(10):
        reads.append((0, [(11, norm(int(L))) for L in rng.integers(1, 5, 500)]))
    # |q1| = 2^70 both ways on ONE k-mer: whatever the order, the running total crosses limb boundaries upwards, downwards
    # and through zero; it ends negative (Q1 = -2^71). x = 2^30 alone gives q2 = 2^100.
    big = 2.0 ** 30
    reads.append((0, [(12, np.array([v])) for v in (big, -big, -big, big, -big, -0.5)] + [(13, np.array([big])), (13, np.array([3.25]))]))
    reads.append((0, [(12, np.array([-big, 0.25])), (12, np.array([big])), (12, np.array([-big])), (21, np.array([-big])), (21, np.array([-1.0])),
                      (12, np.array([-big - 0.5])), (12, np.array([big + 0.75]))] +   # low limbs that carry into the high one
                  [(22, np.array([4095.0]))] * 3))                                   # q2 just below 2^64 each: Q2's low limb wraps twice
    # S2 = 2^64 exactly (skipped) and the double just below 2^32 (kept: q2 = 2^104 - 2^52), a NaN and an infinity (skipped)
    reads.append((0, [(14, np.array([2.0 ** 32])), (14, np.array([np.nextafter(2.0 ** 32, 0.0)])), (15, np.array([1.0, np.nan])),
                      (15, np.array([np.inf])), (15, np.array([0.5])), (14, np.array([-2.0 ** 32]))]))
    # -0.0 and denormals: all round to zero, the counts still move
    reads.append((0, [(16, np.array([-0.0])), (16, np.array([-0.0, 5e-324, -5e-324, 1e-310])), (16, np.array([2.0 ** -1074] * 70))]))
    # ties of rint: q1 = 0.5, 1.5, 2.5, -0.5, -1.5, -2.5 -> 0, 2, 2, -0, -2, -2 (truncation gives 0, 1, 2, 0, -1, -2)
    h = 2.0 ** -41
    reads.append((0, [(17 + (v < 0), np.array([v * h])) for v in (1.0, 3.0, 5.0, -1.0, -3.0, -5.0)]))
    # a fraction that rounds away from the truncated value (q1 = 0.75 -> 1, -0.75 -> -1)
    reads.append((0, [(19, np.array([1.5 * h])), (20, np.array([-1.5 * h]))]))
    return reads


def build_batch():
    reads = _reads()
    b = Batch()
    b.reads = reads
    b.num_kmers = NUM_KMERS
    n = len(reads)
    sig, segrow, kmers = [], [], []
    sig_off, par_off, seg_off = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    T, N = (np.zeros(n, dtype=np.uint32) for _ in range(2))
    o_sig = o_seg = 0
    for i, (_, segs) in enumerate(reads):
        lens = [len(x) for _, x in segs]
        sig_off[i], par_off[i], seg_off[i] = o_sig, o_seg, o_seg
        T[i], N[i] = sum(lens) + 1, len(segs) + 1
        segrow += list(1 + np.concatenate([[0], np.cumsum(lens)[:-1]]))   # lattice row of each segment's first sample
        kmers += [c for c, _ in segs]
        sig += [x for _, x in segs]
        o_sig += sum(lens)
        o_seg += len(segs)
    b.sig = np.ascontiguousarray(np.concatenate(sig), dtype=np.float64)
    b.segrow = np.array(segrow, dtype=np.uint32)
    b.kmers = np.array(kmers, dtype=np.int32)
    b.status = np.array([s for s, _ in reads], dtype=np.int32)
    # processing order: longest first (launch.cpp sorts by cost), so descriptor k is not read k
    order = np.argsort(-T.astype(np.int64), kind="stable")
    b.read = order.astype(np.uint32)
    b.sig_off, b.par_off, b.seg_off, b.T, b.N = sig_off[order], par_off[order], seg_off[order], T[order], N[order]
    for a in (b.sig, b.segrow, b.kmers, b.status, b.read, b.sig_off, b.par_off, b.seg_off, b.T, b.N):
        a.setflags(write=False)
    return b


def reference(b, lo=0, hi=None, truncate=False):
    """the definition over the ok reads [lo, hi) of the batch"""
    acc = empty(b.num_kmers)
    for i, (status, segs) in enumerate(b.reads):
        if status == 0 and lo <= i < (len(b.reads) if hi is None else hi):
            add_read(acc, [c for c, _ in segs], [x for _, x in segs], truncate)
    return acc


def wrong_limbs(b, how):
    """The six arrays as a WRONG accumulation would leave them, segments added in read order:
    'carry_dropped' the high limb never receives the carry of the low one; 'truncated' q cut towards zero instead of rint;
    'no_sign_extension' a negative q's high limb is its magnitude's (zero-extended low limb) instead of all ones."""
    if how == "truncated":
        return limbs(reference(b, truncate=True))[0]
    right = reference(b)
    cols = [np.array(right["n_segments"], dtype=np.uint64), np.array(right["n_samples"], dtype=np.uint64)]
    lo = {"Q1": [0] * b.num_kmers, "Q2": [0] * b.num_kmers}
    hi = {"Q1": [0] * b.num_kmers, "Q2": [0] * b.num_kmers}
    for status, segs in b.reads:
        if status != 0:
            continue
        for c, x in segs:
            q = segment_q(x)
            if q is None:
                continue
            for name, v in (("Q1", q[1]), ("Q2", q[2])):
                tw = v & M128
                l, h = tw & M64, tw >> 64
                if how == "no_sign_extension" and v < 0:
                    h = 0
                s = lo[name][c] + l
                carry = s >> 64
                lo[name][c] = s & M64
                hi[name][c] = (hi[name][c] + h + (0 if how == "carry_dropped" else carry)) & M64
    for name in ("Q1", "Q2"):
        cols.append(np.array(lo[name], dtype=np.uint64))
        cols.append(np.array(hi[name], dtype=np.uint64))
    return cols
