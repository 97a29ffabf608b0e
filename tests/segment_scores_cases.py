"""The per-border segment scores (dyn_aligner_set_segment_scores), restated with NumPy, and the inputs of their device harness.

The DEFINITION (include/dynamont_mi.h) for one ok read: x[0 .. S) the aligned signal, sp[j] the first
sample of output row j, e[j] = sp[j + 1] (e[n - 1] = S), W the window:
    med(v)          s[L/2] (odd L) or (s[L/2 - 1] + s[L/2]) / 2.0 (even L) of the sorted values
    mad(v)          med(|v - med(v)|)
    median_delta[j] |med(B) - med(A)|, A = x[max(0, sp[j] - W) : sp[j]], B = x[sp[j] : min(sp[j] + W, S)]; mad_delta likewise
                    sp[j] == 0: NaN
    homogeneity[j]  L = e[j] - sp[j] >= 10: mad(x[sp[j] + trim : e[j] - trim]), trim = max(L // 10, 1); otherwise NaN
`scores()` is that, and this feature's oracle. Its `wrong=` variants are deliberately WRONG readings of the definition:
tests/test_segment_scores_host.py shows that each of them differs from the right answer on the inputs below, i.e. that these
inputs can fail.

A BATCH is what launch.cpp hands the kernels (tests/device_math/segment_scores.hip): descriptors in processing order (path_off
ascending in that order, `read` a permutation), the signal pool, the borders (segrow = sp + 1) and the per-row column (pathn).
build_batch() holds every case the issue names.
"""
import numpy as np

NAN_BITS = np.uint64(0x7ff8000000000000)
WINDOWS = (1, 2, 3, 63, 64, 65, 255, 256)
SHORT_MAX = 256           # trimmed samples: the split between rank counting and the radix select
RANDOM_READS = {"dna_r9": (7101, 16), "rna004": (7102, 16)}   # (seed, reads) of the random reads of 60 .. 400 bases of the GPU tests
WRONG = ("lower_median", "left_inclusive", "trim_plus_one", "mad_about_mean", "windows_not_cut")


def med(v, lower=False):
    s = np.sort(np.asarray(v, dtype=np.float64))
    L = len(s)
    if L % 2:
        return s[L // 2]
    if lower:
        return s[L // 2 - 1]
    return (s[L // 2 - 1] + s[L // 2]) / np.float64(2.0)


def mad(v, lower=False, about_mean=False):
    v = np.asarray(v, dtype=np.float64)
    m = v.mean() if about_mean else med(v, lower)
    return med(np.abs(v - m), lower)


def scores(x, sp, W, wrong=None, pool=None, off=0):
    """(median_delta, mad_delta, homogeneity), float64 [n]. pool / off: where x lies in a larger array (only the wrong
    variant that does not cut its windows looks there)."""
    x = np.asarray(x, dtype=np.float64)
    S, n = len(x), len(sp)
    sp = [int(p) for p in sp]
    e = sp[1:] + [S]
    lower, mean = wrong == "lower_median", wrong == "mad_about_mean"
    out = np.full((3, n), np.nan)
    for j in range(n):
        p = sp[j]
        if p > 0:
            if wrong == "windows_not_cut":
                A = pool[max(0, off + p - W):off + p]
                B = pool[off + p:off + p + W]
            else:
                A = x[max(0, p - W):p + (1 if wrong == "left_inclusive" else 0)]
                B = x[p:min(p + W, S)]
            out[0, j] = np.abs(med(B, lower) - med(A, lower))
            out[1, j] = np.abs(mad(B, lower, mean) - mad(A, lower, mean))
        L = e[j] - p
        if L >= 10:
            trim = max(L // 10, 1) + (1 if wrong == "trim_plus_one" else 0)
            out[2, j] = mad(x[p + trim:e[j] - trim], lower, mean)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the harness batch ---------------------------------------------------------------------------------------------------------
class Batch:
    pass


def _values(rng, kind, n):
    if kind == "normal":
        return rng.normal(0.2, 1.1, n)
    if kind == "levels":          # quantised to a handful of levels: ranks are decided by the tie rule
        return rng.choice(np.array([-1.25, -0.5, 0.0, 0.75, 2.0]), n)
    if kind == "signed_zero":     # negative values, both zeros, denormals
        return rng.choice(np.array([-1.5, -0.0, 0.0, 5e-324, -5e-324, 1e-310, -2.2250738585072014e-308, 1.0, -3.0e-3]), n)
    if kind == "steps":           # constant stretches (MAD 0) between jumps
        return np.repeat(rng.normal(0, 1, n // 37 + 1), 37)[:n]
    raise ValueError(kind)


def case_reads():
    """[(name, x, sp, status)] in read order"""
    rng = np.random.default_rng(20261018)
    reads = []

    def add(name, kind, lens, status=0):
        lens = [int(v) for v in lens]
        sp = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        reads.append((name, np.ascontiguousarray(_values(rng, kind, int(sum(lens)))), sp, status))

    edge = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 19, 20, 29, 30, 318, 319, 320, 321, 12, 1, 30, 9, 10]
    for kind in ("normal", "levels", "signed_zero", "steps"):
        add("edge_" + kind, kind, edge)
        add("edge_rev_" + kind, kind, edge[::-1])
    add("stall_normal", "normal", [12, 20000, 15, 20001, 11])
    add("failed_between", "normal", [10, 20, 30], status=4)
    add("stall_levels", "levels", [3, 20001, 700, 20000])
    add("single_segment", "normal", [40])
    add("single_sample_rows", "levels", [1] * 25)
    add("two_sample_rows", "normal", [2] * 20)                # windows of two samples at W = 3: the first and the last border
    add("shorter_than_w", "normal", [5, 12, 8, 25])          # 50 samples: W >= 63 is cut at both ends of every border
    add("stall_steps", "steps", [11, 3000, 2])
    add("constant", "steps", [10, 17])                         # 27 samples of one value
    for k in range(300 - len(reads)):                          # 300 descriptors for the bisection, some of them failed
        n = int(rng.integers(1, 7))
        add(f"small_{k}", ("normal", "levels")[k % 2], np.maximum(1, rng.poisson(11, n)), status=3 if k % 41 == 7 else 0)
    return reads


def build_batch():
    reads = case_reads()
    n = len(reads)
    rng = np.random.default_rng(7)
    order = rng.permutation(n)                                 # processing order: rd.read is a permutation
    b = Batch()
    b.reads = reads
    S = np.array([len(r[1]) for r in reads], dtype=np.int64)
    nseg = np.array([len(r[2]) for r in reads], dtype=np.int64)
    sig_off = np.concatenate([[0], np.cumsum(S)[:-1]])         # the pool in read order, back to back: an uncut window reads a neighbour
    seg_off = np.concatenate([[0], np.cumsum(nseg)[:-1]])      # output rows in read order
    b.sig = np.ascontiguousarray(np.concatenate([r[1] for r in reads]))
    b.segrow = np.ascontiguousarray(np.concatenate([r[2] + 1 for r in reads]).astype(np.uint32))
    b.status = np.array([r[3] for r in reads], dtype=np.int32)
    b.read = order.astype(np.uint32)
    b.T = (S[order] + 1).astype(np.uint32)
    b.N = (nseg[order] + 1).astype(np.uint32)
    b.sig_off = sig_off[order].astype(np.uint64)
    b.seg_off = seg_off[order].astype(np.uint64)
    b.path_off = np.concatenate([[0], np.cumsum(S[order] + 1)[:-1]]).astype(np.uint64)   # ascending in processing order
    b.rows_total = int((S + 1).sum())
    pathn = np.zeros(b.rows_total, dtype=np.uint32)
    for k, i in enumerate(order):
        sp = reads[i][2]
        col = np.repeat(np.arange(1, len(sp) + 1), np.diff(np.append(sp, S[i]))).astype(np.uint32)
        col[sp] |= np.uint32(0x80000000)                       # the top bit is a flag of the traceback's: the kernels mask it
        pathn[int(b.path_off[k]) + 1:int(b.path_off[k]) + 1 + S[i]] = col
    b.pathn = pathn
    b.n_seg = int(nseg.sum())
    b.read_sig_off, b.read_seg_off = sig_off, seg_off
    return b


# ---- more reads than one launch of k_score_window takes ----------------------------------------------------------------------
SLICE = 65535            # segment_score_kernels.hpp, SC_MAX_GRID_Y
TAIL = 6                 # descriptors 65 535 .. 65 540: the second launch
SLICED_WINDOWS = (8, 64)


def build_sliced_batch():
    """65 541 reads, built without a loop over the reads: T = 3 .. 6 and N = 2 .. 3, but for nine reads of three rows of
    11 .. 30 samples (finite values in all three columns) -- three in the first slice, and descriptors 65 535 .. 65 540. The
    fields ss_run reads, as build_batch() lays them out, and b.sliced for reference_sliced()."""
    rng = np.random.default_rng(4712)
    n = SLICE + TAIL
    S = rng.integers(2, 6, n)
    two = rng.random(n) < 0.6
    cut = 1 + (rng.random(n) * (S - 1)).astype(np.int64)       # 1 .. S - 1: the first sample of row 1
    lens3 = np.zeros((n, 3), dtype=np.int64)
    lens3[:, 0] = np.where(two, cut, S)
    lens3[:, 1] = np.where(two, S - cut, 0)
    tail = np.sort(rng.choice(np.arange(1000, n - 1000), TAIL, replace=False))
    long_reads = np.concatenate([[5, 30000, n - 7], tail])
    lens3[long_reads] = rng.integers(11, 31, (len(long_reads), 3))
    S = lens3.sum(axis=1)
    nseg = (lens3 > 0).sum(axis=1)
    status = np.zeros(n, dtype=np.int32)
    status[rng.choice(np.setdiff1d(np.arange(n), long_reads), 300, replace=False)] = 3
    rest = np.setdiff1d(np.arange(n), tail)
    order = np.concatenate([rest[rng.permutation(len(rest))], tail])
    b = Batch()
    sig_off, seg_off = np.cumsum(S) - S, np.cumsum(nseg) - nseg
    b.sig = np.ascontiguousarray(rng.choice(np.array([-1.25, -0.5, 0.0, 0.75, 2.0]), int(S.sum())) + 0.01 * rng.standard_normal(int(S.sum())))
    seg_len = lens3[lens3 > 0]
    seg_read = np.repeat(np.arange(n), nseg)
    sp = (np.cumsum(seg_len) - seg_len) - sig_off[seg_read]   # the first sample of every row inside its read
    b.segrow = (sp + 1).astype(np.uint32)
    b.status = status
    b.read = order.astype(np.uint32)
    b.T, b.N = (S[order] + 1).astype(np.uint32), (nseg[order] + 1).astype(np.uint32)
    b.sig_off, b.seg_off = sig_off[order].astype(np.uint64), seg_off[order].astype(np.uint64)
    b.path_off = (np.cumsum(S[order] + 1) - (S[order] + 1)).astype(np.uint64)
    b.rows_total = int((S + 1).sum())
    b.n_seg = int(nseg.sum())
    b.read_sig_off, b.read_seg_off = sig_off, seg_off
    path_of_read = np.zeros(n, dtype=np.int64)
    path_of_read[order] = b.path_off.astype(np.int64)
    smp_seg = np.repeat(np.arange(b.n_seg), seg_len)          # per sample: its row, its read, its place in the read
    smp_read = seg_read[smp_seg]
    smp_t = np.arange(len(b.sig)) - sig_off[smp_read]
    col = (smp_seg - seg_off[smp_read] + 1).astype(np.uint32) | np.where(smp_t == sp[smp_seg], np.uint32(0x80000000), np.uint32(0))
    b.pathn = np.zeros(b.rows_total, dtype=np.uint32)
    b.pathn[path_of_read[smp_read] + 1 + smp_t] = col
    b.sliced = dict(S=S, nseg=nseg, cut=lens3[:, 0], tail=tail, long_reads=long_reads)
    return b


def _med_padded(m, L):
    """med() of every row of m, whose first L[i] entries count"""
    m = np.where(np.arange(m.shape[1])[None, :] < L[:, None], m, np.inf)
    m = np.sort(m, axis=1)
    k = np.arange(len(L))
    return np.where(L % 2 == 1, m[k, L // 2], (m[k, np.maximum(L // 2 - 1, 0)] + m[k, L // 2]) / np.float64(2.0))


def _mad_padded(m, L):
    return _med_padded(np.abs(m - _med_padded(m, L)[:, None]), L)


def reference_sliced(b, W, skip_descs=()):
    """reference() for build_sliced_batch() and a window of 5 samples or more: a read of at most five samples has NaN in
    row 0 and no homogeneity, and the windows of row 1 are cut by the read's ends: A = x[:p], B = x[p:] -- every such read at
    once; the nine longer reads by scores(). skip_descs: descriptors k_score_window was not handed (median_delta and
    mad_delta of their rows keep the zeros; homogeneity comes from the kernels that take the whole batch)."""
    assert W >= 5
    s = b.sliced
    n = len(s["S"])
    out = np.zeros((3, b.n_seg))
    windowed = np.ones(n, dtype=bool)
    windowed[b.read[np.asarray(skip_descs, dtype=np.int64)]] = False
    small = (b.status == 0) & (s["S"] <= 5)
    row0 = b.read_seg_off[small]
    out[2, row0] = np.nan
    out[:2, b.read_seg_off[small & windowed]] = np.nan
    two = np.flatnonzero(small & (s["nseg"] == 2))
    out[2, b.read_seg_off[two] + 1] = np.nan
    two = two[windowed[two]]
    x = np.full((len(two), 5), np.inf)
    for c in range(5):
        has = s["S"][two] > c
        x[has, c] = b.sig[b.read_sig_off[two[has]] + c]
    p, S = s["cut"][two], s["S"][two]
    k = np.arange(len(two))[:, None]
    right = x[k, np.minimum(p[:, None] + np.arange(4)[None, :], 4)]           # x[p:], shifted to the front
    out[0, b.read_seg_off[two] + 1] = np.abs(_med_padded(right, S - p) - _med_padded(x[:, :4], p))
    out[1, b.read_seg_off[two] + 1] = np.abs(_mad_padded(right, S - p) - _mad_padded(x[:, :4], p))
    for i in s["long_reads"]:
        a, m = int(b.read_seg_off[i]), int(s["nseg"][i])
        x_i = b.sig[int(b.read_sig_off[i]):int(b.read_sig_off[i]) + int(s["S"][i])]
        sc = scores(x_i, b.segrow[a:a + m].astype(np.int64) - 1, W)
        out[2, a:a + m] = sc[2]
        if windowed[i]:
            out[:2, a:a + m] = sc[:2]
    return out


def reference(b, W, wrong=None):
    """the three columns [n_seg] of the batch: rows of failed reads are 0"""
    out = np.zeros((3, b.n_seg))
    for i, (_, x, sp, status) in enumerate(b.reads):
        if status != 0:
            continue
        a = int(b.read_seg_off[i])
        out[:, a:a + len(sp)] = scores(x, sp, W, wrong, pool=b.sig, off=int(b.read_sig_off[i]))
    return out
