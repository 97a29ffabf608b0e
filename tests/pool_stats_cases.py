"""The inputs of tests/test_gpu_pool_stats.py and their reference, NumPy only (no GPU, no product code).

A CASE is what dyn_batch_device_pooled hands launch_pool_stats (csrc/pool_stats.hip): read descriptors in PROCESSING order
(par_off = the read's first lattice column in the flat per-column arrays, N - 1 columns, `read` = its index in INPUT order),
the per-read status, the k-mer code of every column, and the per-column sums (w, s1, s2) of the training launch. par_off
ascends with the read index: the flat column order IS the input order.

reference() restates the host's pooled sum (finalise_train, dynamont_mi.cpp) in plain float64, one IEEE addition at a time:
    per ok read in input (par_off) order, per code:  w = 0.0; w += c over the read's columns of that code, ascending
    then                                             pooled[code] += w          (pooled starts from 0.0)
and leaves the codes no ok read has at the initial contents of pooled[]: the kernels write only the codes that occur (the
product zeroes the array first; the tests fill it with other values to see that). Its `assoc=` variants are three
deliberately WRONG associations; tests/test_gpu_pool_stats.py shows on the CPU that each differs in bits from the right one
on the inputs below, i.e. that a kernel summing in any of these orders cannot pass.
"""
import numpy as np

FAILED = 3                # any status != 0 (dyn_read_status)
POISON = 0xA5             # byte the harness fills the work and temp buffers and the guard behind pooled[] with
POISON_U64 = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD = 256               # tests/device_math/pool_stats.hip, PS_GUARD
SLICE = 65535             # the most reads one launch of k_pool_keys takes (gridDim.y)
WRONG = ("flat", "desc_order", "cols_desc")
FAMILY_KMERS = (1, 3, 4, 1024, 262144)   # the sentinel (= num_kmers) at a power of two and one above it
SIZES = (1, 255, 256, 257, 1001)         # total_cols: the u32 regions of the work buffer are rounded to 8 bytes
# seeds of the families with fewer than 8 codes, searched on the CPU so that every wrong association differs in every statistic
# (test_inputs_tell_a_wrong_association_apart): with one to four sums to look at, not every draw shows every order
FAMILY_SEED = {1: 84, 3: 42, 4: 49}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the reference -------------------------------------------------------------------------------------------------------
def seq_group_sum(keys, vals):
    """(unique keys, sums [3, n_unique]): per key, 0.0 + v0 + v1 + ... over its entries in the order given, each + one
    float64 addition. Vectorised over the keys: step p adds the p-th entry of every key that has one."""
    keys = np.asarray(keys, dtype=np.int64)
    o = np.argsort(keys, kind="stable")
    k, v = keys[o], vals[:, o]
    uniq, start, count = np.unique(k, return_index=True, return_counts=True)
    gid = np.repeat(np.arange(len(uniq)), count)
    rank = np.arange(len(k)) - start[gid]
    o2 = np.argsort(rank, kind="stable")                      # entries of rank 0 first, then rank 1, ...
    gid, v = gid[o2], v[:, o2]
    ends = np.cumsum(np.bincount(rank, minlength=1))
    acc = np.zeros((3, len(uniq)))
    a = 0
    for b in ends:
        acc[:, gid[a:b]] = acc[:, gid[a:b]] + v[:, a:b]       # one key at most once per step
        a = b
    return uniq, acc


def _columns(case, descs):
    """(flat column index, descriptor) of every column of the ok reads among the descriptors `descs`"""
    k = np.unique(np.asarray(descs, dtype=np.int64))
    k = k[case.status[case.read[k]] == 0]
    ncol = case.N[k].astype(np.int64) - 1
    first = np.repeat(np.cumsum(ncol) - ncol, ncol)
    flat = np.repeat(case.par_off[k].astype(np.int64), ncol) + np.arange(int(ncol.sum())) - first
    return flat, np.repeat(k, ncol)


def reference(case, assoc="right", descs=None):
    """pooled[3 * num_kmers] as launch_pool_stats must leave it. assoc: "right" or one of WRONG --
    "flat": one sum per code over all columns in flat order, read borders ignored; "desc_order": the reads' partial sums added
    in descriptor (processing) order; "cols_desc": the columns of a read added in descending order.
    descs: the descriptors that take part (default: all) -- what a launch that handed a slice the wrong descriptors leaves."""
    K = case.num_kmers
    flat, dk = _columns(case, np.arange(len(case.read)) if descs is None else descs)
    out = case.pooled_init.copy()
    if not len(flat):
        return out
    code = case.kmers[flat].astype(np.int64)
    vals = np.stack([case.col_w[flat], case.col_s1[flat], case.col_s2[flat]])
    if assoc == "flat":
        o = np.argsort(flat, kind="stable")
        codes, sums = seq_group_sum(code[o], vals[:, o])
    else:
        o = np.argsort(-flat if assoc == "cols_desc" else flat, kind="stable")
        pair, part = seq_group_sum(dk[o] * K + code[o], vals[:, o])                  # one partial sum per (read, code)
        pdk, pcode = pair // K, pair % K
        o = np.argsort(pdk if assoc == "desc_order" else case.par_off[pdk].astype(np.int64), kind="stable")
        codes, sums = seq_group_sum(pcode[o], part[:, o])
    for s in range(3):
        out[s * K + codes] = sums[s]
    return out


def differing_codes(case, a, b):
    """per statistic, how many codes differ in bits between two pooled arrays"""
    d = (bits(a) != bits(b)).reshape(3, case.num_kmers)
    return d.sum(axis=1)


def sorted_runs(case):
    """{code: (first sorted index, length)} of the runs k_pool_segments walks: the ok columns sorted by code"""
    flat, _ = _columns(case, np.arange(len(case.read)))
    codes, count = np.unique(case.kmers[flat], return_counts=True)
    start = np.cumsum(count) - count
    return {int(c): (int(s), int(n)) for c, s, n in zip(codes, start, count)}


# ---- building a case -----------------------------------------------------------------------------------------------------
class Case:
    pass


def assemble(name, num_kmers, ncols, status, has_desc, order, codes, rng, gap=0):
    """ncols / status / has_desc: per read in INPUT order; order: the reads in processing order (those without a descriptor
    are dropped); codes: the code of every column in flat order, the columns of reads without a descriptor and `gap` unowned
    columns behind every such read included."""
    c = Case()
    c.name, c.num_kmers = name, int(num_kmers)
    ncols, status, has_desc = np.asarray(ncols, dtype=np.int64), np.asarray(status, dtype=np.int32), np.asarray(has_desc, dtype=bool)
    width = ncols + np.where(has_desc, 0, gap)
    par_off = np.cumsum(width) - width
    c.total_cols = int(width.sum())
    assert len(codes) == c.total_cols
    c.kmers = np.ascontiguousarray(codes, dtype=np.int32)
    order = np.asarray([i for i in order if has_desc[i]], dtype=np.int64)
    c.read = order.astype(np.uint32)
    c.N = (ncols[order] + 1).astype(np.uint32)
    c.par_off = par_off[order].astype(np.uint64)
    c.status = status
    c.read_par_off, c.read_ncols, c.has_desc = par_off, ncols, has_desc
    # the column sums: every code has its own magnitude 2^-60 .. 2^20, so that the entries of one code are comparable and the
    # order of their additions shows in the last bits; s1 signed with -0.0 among it
    expo = np.random.default_rng(num_kmers).integers(-60, 21, size=c.num_kmers)
    n = c.total_cols
    w = np.ldexp(rng.uniform(1.0, 2.0, n), expo[c.kmers])
    x = rng.normal(0.0, 1.0, n)
    s1, s2 = w * x, w * x * x
    s1[rng.random(n) < 0.03] = -0.0
    col_read = np.repeat(np.arange(len(ncols)), width)
    owned = has_desc[col_read]
    bad = owned & (status[col_read] != 0)                     # a read that failed on the device: its sums are whatever was there
    for a in (w, s1, s2):
        a[bad] = 1e300
        a[~owned] = np.nan                                    # columns no descriptor owns: kept out by k_pool_fill alone
    c.col_w, c.col_s1, c.col_s2 = w, s1, s2
    c.owned = owned
    c.pooled_init = 1000.0 + 0.5 * np.arange(3 * c.num_kmers, dtype=np.float64)    # not the zeros the product starts from
    for a in (c.kmers, c.read, c.N, c.par_off, c.status, c.col_w, c.col_s1, c.col_s2, c.pooled_init):
        a.setflags(write=False)
    return c


def _code_pool(K, rng):
    """the codes a family uses: all of them for a small table, else 128 with 0 and K - 1 among them (a dozen terms per
    code: an order that differs inside one read still shows in the total)"""
    if K <= 128:
        return np.arange(K)
    return np.concatenate([[0, 1, K - 2, K - 1], rng.choice(np.arange(2, K - 2), 124, replace=False)])


def by_n_descending(ncols, rng):
    """launch.cpp's processing order: long reads first (ties in a shuffled order, as its page planning leaves them)"""
    p = rng.permutation(len(ncols))
    return p[np.argsort(-np.asarray(ncols)[p], kind="stable")]


def build_family(K):
    """330 reads (30 where the table has at most four codes: with hundreds of terms per code an order that differs inside one
    read is rounded away in the total) of 1 .. 12 columns over a pool of codes (0 and K - 1 in use), every read drawing from
    two codes so that a code repeats inside a read; failed reads first, in the middle and last (in input and in processing
    order); reads without a descriptor, each followed by unowned columns; one read with the same code at columns 1, 5 and 9;
    descriptors by N descending."""
    rng = np.random.default_rng([FAMILY_SEED.get(K, 41), K])
    pool = _code_pool(K, rng)
    n = 330 if K > 4 else 30
    ncols = rng.integers(1, 13, n)
    status = np.zeros(n, dtype=np.int32)
    failed = [0, 1, n // 2, n // 2 + 1, 2 * n // 3, n - 1]
    status[failed] = FAILED
    has_desc = np.ones(n, dtype=bool)
    nodesc = [5, n // 2 + 3, n - 3]
    has_desc[nodesc] = False
    status[nodesc] = 1
    gap = 3
    rep = 7                                                   # the read with one code at the non-adjacent columns 1, 5, 9
    ncols[rep] = 11
    codes = []
    for i in range(n):
        two = rng.choice(pool, min(2, len(pool)), replace=False)
        cc = rng.choice(two, ncols[i])
        if i == rep:
            cc = np.full(11, pool[-1] if len(pool) == 1 else two[0])
            if len(pool) > 1:
                cc[[0, 2, 3, 4, 6, 7, 8, 10]] = two[1]
        codes.append(cc)
        if not has_desc[i]:
            codes.append(rng.choice(pool, gap))               # a valid code under NaN sums
    order = [i for i in by_n_descending(ncols, rng) if i not in failed]
    t = len(order) // 3
    order = [failed[0]] + order[:t] + [failed[1], failed[2]] + order[t:2 * t] + [failed[3], failed[4]] + order[2 * t:] + [failed[5]]
    c = assemble("family/%d" % K, K, ncols, status, has_desc, order, np.concatenate(codes), rng, gap)
    c.pool, c.repeat_read, c.failed, c.nodesc = pool, rep, failed, nodesc
    return c


def build_long_run():
    """one code in every column of 300 reads of 20 columns -- a run of 6 000 sorted entries over 24 blocks, one partial sum per
    read -- between reads of other codes; two of the 300 failed"""
    K = 1024
    rng = np.random.default_rng(43)
    hot = 511
    ncols = np.concatenate([rng.integers(1, 9, 20), np.full(300, 20), rng.integers(1, 9, 20)])
    n = len(ncols)
    status = np.zeros(n, dtype=np.int32)
    status[[100, 250]] = FAILED
    codes = np.concatenate([np.full(m, hot) if m == 20 else rng.choice(np.array([0, 3, 510, 512, 1023]), m) for m in ncols])
    c = assemble("long_run", K, ncols, status, np.ones(n, dtype=bool), by_n_descending(ncols, rng), codes, rng)
    c.hot = hot
    return c


RUN_COUNTS = {0: 255, 1: 1, 2: 511, 3: 10, 5: 2}   # sorted starts 0, 255, 256, 767 (= 2 * 256 + 255), 777


def build_runs():
    """runs that start at sorted index = 0 and = 255 (mod 256): code 0 fills [0, 255), code 1 is the one entry at 255, code 2
    runs from 256 over two block borders to 766, code 3 starts at 767. Every read ok: the sorted index is the count below."""
    K = 8
    rng = np.random.default_rng(44)
    codes = rng.permutation(np.concatenate([np.full(m, c) for c, m in RUN_COUNTS.items()]))
    ncols = []
    while sum(ncols) < len(codes):
        ncols.append(min(int(rng.integers(1, 15)), len(codes) - sum(ncols)))
    n = len(ncols)
    return assemble("runs", K, ncols, np.zeros(n, dtype=np.int32), np.ones(n, dtype=bool), by_n_descending(ncols, rng), codes, rng)


def build_sized(total):
    """total_cols columns exactly, all owned: reads of 1 .. 9 columns, four codes, one read failed where there are three"""
    K = 4
    rng = np.random.default_rng([45, total])
    ncols = []
    while sum(ncols) < total:
        ncols.append(min(int(rng.integers(1, 10)), total - sum(ncols)))
    n = len(ncols)
    status = np.zeros(n, dtype=np.int32)
    if n >= 3:
        status[1] = FAILED
    return assemble("size/%d" % total, K, ncols, status, np.ones(n, dtype=bool), by_n_descending(ncols, rng),
                    rng.integers(0, K, total), rng)


def build_neg_zero():
    """every s1 of code 1 is -0.0, over three reads: 0.0 + -0.0 is +0.0 (a sum that starts from its first entry says -0.0)"""
    K = 4
    rng = np.random.default_rng(46)
    ncols = [3, 2, 4, 1]
    codes = np.array([1, 0, 1, 1, 2, 3, 1, 1, 0, 2])
    c = assemble("neg_zero", K, ncols, np.zeros(4, dtype=np.int32), np.ones(4, dtype=bool), [2, 0, 1, 3], codes, rng)
    s1 = c.col_s1.copy()
    s1[codes == 1] = -0.0
    s1.setflags(write=False)
    c.col_s1 = s1
    return c


TAIL = 6                         # descriptors 65 535 .. 65 540: the second launch of k_pool_keys
TAIL_CODES = np.arange(1000, 1000 + TAIL)


def build_sliced():
    """65 541 descriptors of N in {2, 3}. The first 65 535 in processing order use the codes 0 .. 499; the last six are reads from
    the middle of the input order with two columns each: a code shared with the first slice and a code nobody else has."""
    K = 1024
    rng = np.random.default_rng(47)
    n = SLICE + TAIL
    ncols = rng.integers(1, 3, n)
    tail = np.sort(rng.choice(np.arange(1000, n - 1000), TAIL, replace=False))
    ncols[tail] = 2
    status = np.zeros(n, dtype=np.int32)
    status[rng.choice(np.setdiff1d(np.arange(n), tail), 300, replace=False)] = FAILED
    start = np.cumsum(ncols) - ncols
    codes = rng.integers(0, 500, int(ncols.sum()))
    codes[start[tail] + 1] = TAIL_CODES                       # first column: shared with the first slice; second: its own
    rest = np.setdiff1d(np.arange(n), tail)
    order = np.concatenate([rest[np.argsort(-ncols[rest], kind="stable")], tail])
    c = assemble("sliced", K, ncols, status, np.ones(n, dtype=bool), order, codes, rng)
    c.tail_reads = tail
    return c


def small_cases():
    """every case but the 65 541-descriptor one, by name"""
    cases = [build_family(K) for K in FAMILY_KMERS] + [build_long_run(), build_runs(), build_neg_zero()]
    cases += [build_sized(t) for t in SIZES]
    return {c.name: c for c in cases}
