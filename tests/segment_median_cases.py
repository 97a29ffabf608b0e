"""The inputs of tests/test_gpu_segment_median.py and their reference, NumPy only (no GPU, no product code).

A BATCH is what launch.cpp hands launch_segments: read descriptors in processing order (path_off ascending in that order,
seg_off by read INDEX as host_prepare assigns it, rd.read a permutation), the per-read state, and the three path arrays
the traceback leaves on the device: pp[] (the posterior of the path cell of each row; row 0 of a read is not on the path
and holds NaN here), pathn[] (the path cell's column, bit 31 = state M) and segrow[] (the row of each segment's M cell).

A CASE is one segment with a name: "len/<L>/<first|inner|last>", "fam/<family>/<variant>/<L>", "shape/<what>". Every case
knows the read and the segment it became, so a failure names length, family and position.

order_stats(): per segment s = sort(pp[a:b]); probability = s[L//2] (odd L) or (s[L//2-1] + s[L//2]) / 2.0 (even L);
with `wrong`, one of the four selections a subtly wrong kernel would make (test_inputs_tell_a_wrong_selection_apart).
"""
import numpy as np

MEDIAN_SHORT_MAX = 256   # segment_kernels.hpp: longer segments take k_median_long
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 258, 511, 512, 513, 1023, 1024, 1025, 20_000, 20_001]
POSITIONS = ["first", "inner", "last"]
FAMILY_LENGTHS = [31, 32, 255, 256, 257, 258, 700, 701]   # odd and even, both sides of the 256 / 257 split
WRONG = ["rank_up", "rank_down", "even_is_hi", "lo_is_largest_below"]
FAILED = 3               # any status != 0 (dyn_read_status)
KMER_SIZE = 5
POISON = 0xA5            # byte the harness fills med_hi, med_lo and the rows with
POISON_U64 = np.uint64(0xA5A5A5A5A5A5A5A5)
POISON_U32 = np.uint32(0xA5A5A5A5)
GUARD = 64               # output slots beyond the last segment


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


# ---- the reference -------------------------------------------------------------------------------------------------------
def order_stats(v, wrong=None):
    """(hi, lo, probability) of one segment; lo is None for odd L. `wrong`: one of WRONG."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    L = len(s)
    mid = L // 2
    if wrong == "rank_up":
        mid = min(mid + 1, L - 1)
    elif wrong == "rank_down":
        mid = max(mid - 1, 0)
    hi = s[mid]
    if L & 1:
        return hi, None, hi
    lo = s[max(mid - 1, 0)]
    if wrong == "even_is_hi":
        lo = hi
    elif wrong == "lo_is_largest_below":
        below = s[s < hi]
        lo = below[-1] if len(below) else hi
    return hi, lo, (lo + hi) / 2.0


# ---- value families ------------------------------------------------------------------------------------------------------
def _median_tie(pool_sorted, L):
    """L values of a sorted pool of L - 1 distinct ones: ranks mid-1 and mid hold the same value ("another copy of hi")"""
    assert len(pool_sorted) == L - 1 and L >= 2
    return np.insert(pool_sorted, L // 2 - 1, pool_sorted[L // 2 - 1])


def _distinct(draw, n, rng):
    """n distinct values of draw(rng, m), sorted"""
    v = np.unique(draw(rng, 4 * n + 16))
    assert len(v) >= n, (len(v), n)
    return np.sort(rng.choice(v, n, replace=False))


def _plain_and_tie(draw):
    """variants of a family that can supply L distinct values: "plain" (distinct: ranks mid-1, mid, mid+1 all differ) and
    "tie" (ranks mid-1 and mid equal, every other value distinct), both in random row order"""
    def variants(L, rng):
        out = {"plain": rng.permutation(_distinct(draw, L, rng))}
        if L >= 4:
            out["tie"] = rng.permutation(_median_tie(_distinct(draw, L - 1, rng), L))
        return out
    return variants


def _uniform(rng, n):
    return 1.0 - rng.random(n)   # (0, 1]


def _all_equal(L, rng):
    return {"one": np.full(L, 1.0), "zero": np.full(L, 0.0), "other": np.full(L, 0.3141592653589793)}


def _two_values(L, rng):
    """lo < hi with mid-1, mid and mid+1 copies of lo: the even rule's two branches and the value below the middle"""
    mid = L // 2
    out = {}
    for name, c in (("mid-1", mid - 1), ("mid", mid), ("mid+1", mid + 1)):
        if 0 <= c <= L:
            out[name] = rng.permutation(np.concatenate([np.full(c, 0.25), np.full(L - c, 0.75)]))
    return out


def _tie_runs(L, rng):
    """a run of one value over the sorted ranks [a, b], distinct values below and above it: the run straddles the middle,
    ends on it, starts on rank mid-1, or starts on rank mid"""
    mid, q = L // 2, max(1, L // 4)
    out = {}
    for name, a, b in (("straddle", mid - q, mid + q), ("ends_at_mid", mid - q, mid), ("from_mid-1", mid - 1, mid + q),
                       ("from_mid", mid, mid + q)):
        a, b = max(a, 0), min(b, L - 1)
        below = np.sort(rng.uniform(0.05, 0.45, a))
        above = np.sort(rng.uniform(0.55, 0.95, L - 1 - b))
        out[name] = rng.permutation(np.concatenate([below, np.full(b - a + 1, 0.5), above]))
    return out


def _exp_fp32(L, rng):
    """pp as the product forms it: exp((double)lp) of an fp32 log-probability. lp = 0 and fp32 denormals give exactly 1.0,
    |lp| ~ 1e-16 gives 1 -+ k ulp (heavy ties), lp > 0 gives values a little above 1.0 (the oracle produces them too)"""
    def draw(weights):
        kind = rng.choice(6, L, p=np.array(weights) / np.sum(weights))
        lp = np.zeros(L)
        den = rng.integers(1, 1 << 23, L).astype(np.uint32).view(np.float32).astype(np.float64)   # fp32 denormals
        lp = np.where(kind == 1, den * rng.choice([-1.0, 1.0], L), lp)
        lp = np.where(kind == 2, -10.0 ** rng.uniform(-17, -15, L), lp)
        lp = np.where(kind == 3, rng.choice([-1.0, 1.0], L) * 10.0 ** rng.uniform(-9, -3, L), lp)
        lp = np.where(kind == 4, -10.0 ** rng.uniform(-9, -3, L), lp)
        lp = np.where(kind == 5, -0.7 * rng.random(L), lp)
        return np.exp(lp.astype(np.float32).astype(np.float64))
    return {"near_one": draw([3, 2, 3, 2, 0, 0]),        # ties at 1.0 and 1 - k ulp, some above 1.0
            "around_one": draw([0, 0, 0, 1, 1, 0]),      # 1 +- 1e-9 .. 1e-3, hardly a tie
            "mixed": draw([2, 1, 2, 2, 2, 3]),           # the middle falls wherever
            "tie": rng.permutation(_median_tie(np.sort(draw([0, 0, 0, 1, 1, 0]))[:L - 1], L)) if L >= 4 else draw([1, 0, 0, 0, 0, 0])}


def _low_byte(rng, n):
    return from_bits(bits(0.5) | np.arange(256, dtype=np.uint64))   # all there are (_distinct picks among them)


def _low_byte_variants(L, rng):
    """equal in the top seven bytes: only the last pass of the radix select tells them apart. 256 distinct values exist, so
    segments longer than that carry ties away from the middle ("plain") or on it ("tie")"""
    if L <= 256:
        return _plain_and_tie(_low_byte)(L, rng)
    if L > 258:
        return {}
    every = from_bits(bits(0.5) | np.arange(256, dtype=np.uint64))
    return {"plain": rng.permutation(np.concatenate([every, every[3:3 + L - 256]])),
            # the tied value's last byte is odd (127): its mean with the value below it is no third value's bits
            "tie": rng.permutation(np.concatenate([every, every[128 - (L - 256):128]]))}


def _exponent_only(rng, n):
    return 2.0 ** -rng.integers(0, 997, n).astype(np.float64)   # 1 .. 1.5e-300: the mantissa is zero throughout


def _ff_bytes(L, rng):
    """0xff in byte 0, 3, 6 or bytes 0-5 of EVERY value, the median's too: the scan over the histogram must end in bin 255"""
    out = {}
    for name, positions in (("byte0", [0]), ("byte3", [3]), ("byte6", [6]), ("bytes0-5", [0, 1, 2, 3, 4, 5])):
        force = np.uint64(sum(0xff << (8 * p) for p in positions))
        top = np.uint64(0x3e) << np.uint64(56) if 6 in positions else np.uint64(0)

        def draw(r, n, force=force, top=top):
            u = bits(2.0 ** -r.uniform(0, 100, n)) | force      # 100 binades: bytes 0-5 forced still leaves 1 600 values
            if top:
                u = (u & np.uint64(0x00ffffffffffffff)) | top   # exponent 0x3ef: ~2^-16, not [1.9, 2)
            return from_bits(u)
        for v, a in _plain_and_tie(draw)(L, rng).items():
            out[name + "_" + v] = a
    return out


def _zero_denormal(rng, n):
    return from_bits(rng.integers(0, 4 * n + 16, n).astype(np.uint64))   # +0.0, 5e-324, 1e-323, ...


def _zero_denormal_variants(L, rng):
    out = _plain_and_tie(_zero_denormal)(L, rng)
    out["lowest"] = rng.permutation(from_bits(np.arange(L, dtype=np.uint64)))       # +0.0 and 5e-324 themselves
    out["half_zero"] = rng.permutation(from_bits((np.arange(L) >= L // 2).astype(np.uint64)))  # (0 + 5e-324) / 2 on even L
    return out


def _ordered(L, rng):
    """ascending and descending rows (the short kernel breaks ties by row): distinct values, and values with ties
    throughout (L / 3 distinct levels) and on the middle"""
    plain = _distinct(_uniform, L, rng)
    out = {"asc": plain, "desc": plain[::-1].copy()}
    levels = np.sort(rng.choice(_distinct(_uniform, max(1, L // 3), rng), L))
    out["asc_ties"], out["desc_ties"] = levels, levels[::-1].copy()
    if L >= 4:
        tie = _median_tie(_distinct(_uniform, L - 1, rng), L)
        out["asc_tie"], out["desc_tie"] = tie, tie[::-1].copy()
    return out


FAMILIES = {
    "uniform": _plain_and_tie(_uniform),          # distinct uniform values in (0, 1] (+ one tie on the middle)
    "all_equal": _all_equal,
    "two_values": _two_values,
    "tie_runs": _tie_runs,
    "exp_fp32": _exp_fp32,
    "low_byte": _low_byte_variants,
    "exponent_only": _plain_and_tie(_exponent_only),
    "ff_bytes": _ff_bytes,
    "zero_denormal": _zero_denormal_variants,
    "ordered": _ordered,
}
EXEMPT = {"all_equal"}   # every order statistic is the same value: no selection can be told from another


def family_segments():
    """{(family, variant, L): values in row order}, seeded"""
    out = {}
    for f, (name, variants) in enumerate(FAMILIES.items()):
        for L in FAMILY_LENGTHS:
            for v, a in variants(L, np.random.default_rng([17, f, L])).items():
                a = np.ascontiguousarray(a, dtype=np.float64)
                assert len(a) == L and not np.isnan(a).any() and not np.signbit(a).any(), (name, v, L)
                out[(name, v, L)] = a
    return out


# ---- the batch -----------------------------------------------------------------------------------------------------------
class Batch:
    """reads: list of dict(segments=[array, ...], status=int, desc=bool) in INPUT order (index = rd.read)"""

    def __init__(self, reads, order, cases, seg_by="read"):
        self.reads, self.order, self.cases = reads, np.asarray(order), cases
        n = len(reads)
        self.status = np.array([r["status"] for r in reads], dtype=np.int32)
        nseg = np.array([len(r["segments"]) for r in reads], dtype=np.uint64)
        T = np.array([1 + sum(len(s) for s in r["segments"]) for r in reads], dtype=np.uint64)
        proc = [i for i in order if reads[i]["desc"]]          # a read refused by validation has no descriptor
        self.read = np.array(proc, dtype=np.uint32)
        self.T = T[proc].astype(np.uint32)
        self.N = (nseg[proc] + 1).astype(np.uint32)
        self.path_off = np.concatenate([[0], np.cumsum(T[proc])[:-1]]).astype(np.uint64)
        self.rows_total = int(T[proc].sum())
        self.read_seg_off = np.zeros(n, dtype=np.uint64)       # by read index
        if seg_by == "read":                                   # host_prepare: every read has its rows, in input order
            self.read_seg_off[:] = np.concatenate([[0], np.cumsum(nseg)[:-1]])
        else:                                                  # ascending in processing order (reads without descriptor last)
            rest = [i for i in range(n) if not reads[i]["desc"]]
            seq = proc + rest
            self.read_seg_off[seq] = np.concatenate([[0], np.cumsum(nseg[seq])[:-1]])
        self.seg_off = self.read_seg_off[proc]
        self.n_seg = int(nseg.sum())
        self.pp = np.full(self.rows_total, np.nan)
        self.pathn = np.zeros(self.rows_total, dtype=np.uint32)
        self.segrow = np.full(self.n_seg, 0xffffffff, dtype=np.uint32)   # rows of a read without descriptor: never read
        for k, i in enumerate(proc):
            segs = reads[i]["segments"]
            lens = np.array([len(s) for s in segs])
            starts = 1 + np.concatenate([[0], np.cumsum(lens)[:-1]])
            po, so = int(self.path_off[k]), int(self.seg_off[k])
            self.pp[po + 1:po + int(T[i])] = np.concatenate(segs)
            col = np.repeat(np.arange(1, len(segs) + 1, dtype=np.uint32), lens)
            col[starts - 1] |= np.uint32(0x80000000)           # the segment's first row is its M cell
            self.pathn[po + 1:po + int(T[i])] = col
            self.segrow[so:so + len(segs)] = starts
        self.proc_index = {i: k for k, i in enumerate(proc)}

    def where(self, case):
        """(read index, segment index, output slot) of a named case"""
        i, j = self.cases[case]
        return i, j, int(self.read_seg_off[i]) + j

    def reference(self, wrong=None):
        """med_hi, med_lo, rows (signal_pos, sequence_pos, probability) as the kernels must leave them: poison wherever
        they must not write (failed reads, reads without descriptor, med_lo of short odd segments, the guard)"""
        n = self.n_seg + GUARD
        hi, lo, prob = from_bits(np.full(n, POISON_U64)), from_bits(np.full(n, POISON_U64)), from_bits(np.full(n, POISON_U64))
        sig, seq = np.full(n, POISON_U32), np.full(n, POISON_U32)
        for i, r in enumerate(self.reads):
            if not r["desc"] or r["status"] != 0:
                continue
            so, start = int(self.read_seg_off[i]), 1
            for j, v in enumerate(r["segments"]):
                h, l, p = order_stats(v, wrong)
                hi[so + j], prob[so + j] = h, p
                if l is not None:
                    lo[so + j] = l
                elif len(v) > MEDIAN_SHORT_MAX:
                    lo[so + j] = h                             # k_median_long writes both: lo = hi for odd L
                sig[so + j], seq[so + j] = start - 1, j + KMER_SIZE // 2
                start += len(v)
        return dict(med_hi=hi, med_lo=lo, probability=prob, signal_pos=sig, sequence_pos=seq)


def build_batch(seg_by="read"):
    rng = np.random.default_rng(2024)
    reads, cases = [], {}

    def fill(L):
        return 1.0 - rng.random(L)

    def add(segments, status=0, desc=True, names=None):
        reads.append(dict(segments=[np.ascontiguousarray(s, dtype=np.float64) for s in segments], status=status, desc=desc))
        for name, j in (names or {}).items():
            assert name not in cases, name
            cases[name] = (len(reads) - 1, j)
        return len(reads) - 1

    # every length as the first, an inner and the last segment of a read (the last one ends at T)
    for L in LENGTHS:
        add([fill(L), fill(7), fill(12)], names={"len/%d/first" % L: 0})
        add([fill(9), fill(L), fill(6)], names={"len/%d/inner" % L: 1})
        add([fill(5), fill(8), fill(L)], names={"len/%d/last" % L: 2})
    # the value families, each segment between two short ones
    for (f, v, L), a in family_segments().items():
        add([fill(3), a, fill(4)], names={"fam/%s/%s/%d" % (f, v, L): 1})
    # read shapes
    add([fill(1)], names={"shape/T=2": 0})                                   # the smallest read: T = 2, N = 2
    for L in (2, 256, 257, 300):
        add([fill(L)], names={"shape/one_segment/%d" % L: 0})                # N = 2
    for where, at in (("first", 0), ("index300", 300), ("last", 599)):       # > 512 segments, one long: the strided scan
        segs = [fill(int(rng.integers(1, 9))) for _ in range(600)]
        segs[at] = fill(301 + at % 2)
        add(segs, names={"shape/600_segments/long_%s" % where: at, "shape/600_segments/long_%s/short_neighbour" % where: 1 if at == 0 else at - 1})
    add([fill(40), fill(256), fill(3)], names={"shape/no_long_segment": 1})
    add([fill(300), fill(10), fill(257), fill(1000)], names={"shape/several_long/0": 0, "shape/several_long/2": 2, "shape/several_long/3": 3})
    # failed reads: their rows keep the poison although their path arrays are as good as anyone's
    failed = [add([fill(5), fill(300), fill(256), fill(2)], status=FAILED) for _ in range(5)]
    nodesc = [add([fill(4), fill(3)], status=1, desc=False) for _ in range(3)]
    # many small reads: the bisection over path_off runs over ~300 descriptors
    while len(reads) < 301:
        add([fill(int(rng.integers(1, 30))) for _ in range(int(rng.integers(1, 6)))])
    # processing order: a permutation of the reads that is not the identity, failed reads first, last and in between
    order = [int(i) for i in rng.permutation(len(reads)) if i not in failed]
    order = [failed[0]] + order[:100] + [failed[1], failed[2]] + order[100:200] + [failed[3]] + order[200:] + [failed[4]]
    b = Batch(reads, order, cases, seg_by)
    if b.rows_total % 256 == 0:                                              # the last block of k_median is a partial one
        reads.append(dict(segments=[fill(3)], status=0, desc=True))
        b = Batch(reads, order + [len(reads) - 1], cases, seg_by)
    return b


# ---- more reads than one launch of the per-read kernels takes ------------------------------------------------------------
SLICE = 65535            # segment_kernels.hpp, MAX_GRID_Y: k_median_long and k_final put the read in gridDim.y
TAIL = 6                 # descriptors 65 535 .. 65 540: the second launch of both


def build_sliced_batch():
    """65 541 reads of T = 3 .. 6 and N = 2 .. 3, built without a loop over the reads; one read of the first slice and one of
    the last six descriptors have a third segment, 300 and 301 rows long (k_median_long has work in both launches). The
    fields sm_run reads, as Batch has them (seg_off by read index), and the per-segment arrays reference_sliced() needs."""
    rng = np.random.default_rng(4711)
    n = SLICE + TAIL
    rows = rng.integers(2, 6, n)                               # T - 1
    two = rng.random(n) < 0.6
    cut = 1 + (rng.random(n) * (rows - 1)).astype(np.int64)    # 1 .. rows - 1
    lens3 = np.zeros((n, 3), dtype=np.int64)
    lens3[:, 0] = np.where(two, cut, rows)
    lens3[:, 1] = np.where(two, rows - cut, 0)
    tail = np.sort(rng.choice(np.arange(1000, n - 1000), TAIL, replace=False))   # read indices from the middle of the input
    long_reads = np.array([777, tail[2]])
    lens3[long_reads] = [[3, 4, 300], [2, 301, 5]]
    status = np.zeros(n, dtype=np.int32)
    status[rng.choice(np.setdiff1d(np.arange(n), np.concatenate([tail, long_reads])), 300, replace=False)] = FAILED
    rest = np.setdiff1d(np.arange(n), tail)
    proc = np.concatenate([rest[rng.permutation(len(rest))], tail])
    b = Batch.__new__(Batch)
    nseg = (lens3 > 0).sum(axis=1)
    rows = lens3.sum(axis=1)
    T = rows + 1
    b.status = status
    b.read = proc.astype(np.uint32)
    b.T, b.N = T[proc].astype(np.uint32), (nseg[proc] + 1).astype(np.uint32)
    b.path_off = (np.cumsum(T[proc]) - T[proc]).astype(np.uint64)
    b.rows_total = int(T.sum())
    b.read_seg_off = (np.cumsum(nseg) - nseg).astype(np.uint64)
    b.seg_off = b.read_seg_off[proc]
    b.n_seg = int(nseg.sum())
    path_of_read = np.zeros(n, dtype=np.int64)
    path_of_read[proc] = b.path_off.astype(np.int64)
    # per segment, in input order
    seg_len = lens3[lens3 > 0]
    seg_read = np.repeat(np.arange(n), nseg)
    seg_j = np.arange(b.n_seg) - b.read_seg_off.astype(np.int64)[seg_read]
    rows_before = np.cumsum(rows) - rows
    seg_first = np.cumsum(seg_len) - seg_len                   # among the rows of all reads (row 0 of a read not counted)
    seg_start = seg_first - rows_before[seg_read] + 1          # its first row inside the read
    b.segrow = seg_start.astype(np.uint32)
    # per row
    total = int(seg_len.sum())
    row_seg = np.repeat(np.arange(b.n_seg), seg_len)
    row_t = np.arange(total) - rows_before[seg_read[row_seg]] + 1
    at = path_of_read[seg_read[row_seg]] + row_t
    vals = 1.0 - rng.random(total)
    b.pp = np.full(b.rows_total, np.nan)
    b.pp[at] = vals
    b.pathn = np.zeros(b.rows_total, dtype=np.uint32)
    b.pathn[at] = (seg_j[row_seg] + 1).astype(np.uint32) | np.where(row_t == seg_start[row_seg], np.uint32(0x80000000), np.uint32(0))
    b.sliced = dict(seg_len=seg_len, seg_read=seg_read, seg_j=seg_j, seg_first=seg_first, seg_start=seg_start, vals=vals, tail=tail,
                    long_reads=long_reads)
    for a in (b.pp, b.pathn, b.segrow, b.path_off, b.seg_off, b.T, b.N, b.read, b.status):
        a.setflags(write=False)
    return b


def reference_sliced(b, skip_descs=()):
    """Batch.reference() for build_sliced_batch(): the segments of up to five rows by one sort of a padded matrix, the longer
    ones by order_stats(). skip_descs: descriptors whose reads no per-read kernel was handed (their rows keep the poison)."""
    s = b.sliced
    L, first, vals = s["seg_len"], s["seg_first"], s["vals"]
    n = b.n_seg + GUARD
    hi, lo, prob = from_bits(np.full(n, POISON_U64)), from_bits(np.full(n, POISON_U64)), from_bits(np.full(n, POISON_U64))
    sig, seq = np.full(n, POISON_U32), np.full(n, POISON_U32)
    ok = b.status[s["seg_read"]] == 0
    ok[np.isin(s["seg_read"], b.read[np.asarray(skip_descs, dtype=np.int64)])] = False
    small = np.flatnonzero(ok & (L <= 5))
    m = np.full((len(small), 5), np.inf)
    for c in range(5):
        has = L[small] > c
        m[has, c] = vals[first[small[has]] + c]
    m.sort(axis=1)
    k = np.arange(len(small))
    mid = L[small] // 2
    even = L[small] % 2 == 0
    hi[small] = m[k, mid]
    lo[small[even]] = m[k[even], mid[even] - 1]
    prob[small] = np.where(even, (m[k, np.maximum(mid - 1, 0)] + m[k, mid]) / 2.0, m[k, mid])
    for i in np.flatnonzero(ok & (L > 5)):
        h, l, p = order_stats(vals[first[i]:first[i] + L[i]])
        hi[i], prob[i] = h, p
        lo[i] = l if l is not None else (h if L[i] > MEDIAN_SHORT_MAX else from_bits(np.array([POISON_U64]))[0])
    at = np.flatnonzero(ok)
    sig[at] = (s["seg_start"][at] - 1).astype(np.uint32)
    seq[at] = (s["seg_j"][at] + KMER_SIZE // 2).astype(np.uint32)
    return dict(med_hi=hi, med_lo=lo, probability=prob, signal_pos=sig, sequence_pos=seq)
