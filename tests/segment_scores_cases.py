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


def reference(b, W, wrong=None):
    """the three columns [n_seg] of the batch: rows of failed reads are 0"""
    out = np.zeros((3, b.n_seg))
    for i, (_, x, sp, status) in enumerate(b.reads):
        if status != 0:
            continue
        a = int(b.read_seg_off[i])
        out[:, a:a + len(sp)] = scores(x, sp, W, wrong, pool=b.sig, off=int(b.read_sig_off[i]))
    return out
