"""Shared by tests/test_guided_band_host.py and tests/test_gpu_guided_band.py (no GPU, no library): the guided lattice of
dyn_batch_set_guide restated in plain NumPy float64 -- forward, backward, posterior,
posterior-Viterbi with the reference's tie rule ``vE == vM_prev + LPE``, traceback --, the guided band margin restated in Python
ints, ``covers()`` and the read families of the two test files.

Lattice: rows t = 0 .. T-1 (T = samples + 1), columns n = 0 .. N-1 (N = k-mers + 1). centre(0) = 0, centre(t) = guide[t - 1];
the cells of row t are n in [max(centre - hw, lo), min(centre + hw + 1, N)), lo = 0 for the backward sweep and 1 for the
forward one (the reference's computeBounds with mid -> centre). Everything outside is -inf. The model keeps whole rows in
absolute columns, so shifts between rows need no bookkeeping: that is what the kernel's band-column addressing has to equal.
"""
from types import SimpleNamespace

import numpy as np

from dynamont_amd import guide as G
from dynamont_amd import synth

NONE = 0xFFFFFFFF
PORE = "dna_r9"            # k = 5 on conftest's "syn5" table, no polyA pad: no structural ties
K = 5
NEG = -np.inf

Z_RTOL = 8 * 3.53e-16
"""Bound on |Z_device - Z_model| / |Z_model| for the narrow-window test: eight times the largest |Z_model - Z_oracle| /
|Z_oracle| over every family of build_reads() with a diagonal guide at half_width = min(band / 2, N / 2) (the model's window is
then the oracle's band; the device carries the reference's own bits there, so the model's NumPy exp / log / log1p are the
only source of deviation). Measured over every read of families a, a2, b, stall, stall_mv and e: 3.52e-16 (family e, all 600 reads; a2 1.86e-16; 0 on the
others: the model's bits are then the oracle's), rounded up to 3.53e-16, by
    python -m pytest tests/test_guided_band_host.py -k restatement -s
which prints the maximum per family; the factor 8 covers reads and windows other than the ones measured."""


# ---------------------------------------------------------------------------------------------- the lattice in NumPy float64
def log_normal_pdf(x, mean, sd):
    z = (x - mean) / sd
    return -0.5 * z * z - np.log(sd) - 0.5 * np.log(2.0 * np.pi)


def log_plus(x, y):
    """the reference's logPlus, element-wise: an infinite operand returns the other one unchanged"""
    hi, lo = np.maximum(x, y), np.minimum(x, y)
    with np.errstate(invalid="ignore", over="ignore"):
        s = hi + np.log1p(np.exp(lo - hi))
    s = np.where(np.isinf(x), y, np.where(np.isinf(y), x, s))
    return s


def centres(guide, T):
    c = np.zeros(T, dtype=np.int64)
    c[1:] = np.asarray(guide, dtype=np.int64)[:T - 1]
    return c


def model_align(signal, mean, sd, log_m1, log_e2, guide, hw):
    """mean / sd: the emission parameters of lattice columns 1 .. N-1 (entry n - 1). Returns ok (the reference's Z check), Z
    (= Zb), Zf, and for an ok read segrow (lattice row of each output row's M cell), signal_positions (= segrow - 1), pathn
    (column of the path cell of every row, 0 before segrow[0]) and the per-segment probabilities."""
    x = np.asarray(signal, dtype=np.float64)
    T, N = len(x) + 1, len(mean) + 1
    hw = int(hw)
    B = 2 * hw + 3
    c = centres(guide, T)
    lo_b = np.maximum(c - hw, 0)
    lo_f = np.maximum(c - hw, 1)
    hi = np.minimum(c + hw + 1, N)
    # score[t, n - 1] = log N(x[t]; column n): sample t is consumed by the step into row t + 1
    score = log_normal_pdf(x[:, None], np.asarray(mean)[None, :], np.asarray(sd)[None, :])
    with np.errstate(invalid="ignore"):
        bE = np.full((T, N), NEG)
        bM = np.full((T, N), NEG)
        if lo_b[T - 1] <= N - 1 < hi[T - 1]:
            bE[T - 1, N - 1] = 0.0
        for t in range(T - 2, -1, -1):
            a, b = int(lo_b[t]), int(hi[t])
            if a >= b:
                continue
            n = np.arange(a, b)
            ext = np.full(b - a, NEG)
            up = n + 1 < N                                          # a move into column n + 1 (entry n)
            ext[up] = (bM[t + 1, n[up] + 1] + score[t, n[up]]) + log_m1
            st = n > 0
            e_next = bE[t + 1, n[st]]
            sc = score[t, n[st] - 1]
            bM[t, n[st]] = e_next + sc
            ext[st] = log_plus(ext[st], (e_next + sc) + log_e2)
            bE[t, a:b] = ext
        Zb = bE[0, 0]
        fE = np.full((T, N), NEG)
        fM = np.full((T, N), NEG)
        fE[0, 0] = 0.0
        for t in range(1, T):
            a, b = int(lo_f[t]), int(hi[t])
            if a >= b:
                continue
            n = np.arange(a, b)
            sc = score[t - 1, n - 1]
            fM[t, a:b] = (fE[t - 1, n - 1] + sc) + log_m1
            fE[t, a:b] = log_plus((fM[t - 1, n] + sc) + 0.0, (fE[t - 1, n] + sc) + log_e2)
        Zf = fE[T - 1, N - 1]
        size = float(T * B)
        ok = bool(np.isfinite(Zf) and np.isfinite(Zb) and not abs(Zf - Zb) / size > 1e-8)
        out = SimpleNamespace(ok=ok, Z=float(Zb), Zf=float(Zf), T=T, N=N)
        if not ok:
            return out
        LPM = (fM + bM) - Zb
        LPE = (fE + bE) - Zb
        LPM[np.isnan(LPM)] = NEG
        LPE[np.isnan(LPE)] = NEG
        vE = np.full((T, N), NEG)
        vM = np.full((T, N), NEG)
        bit = np.zeros((T, N), dtype=bool)
        vE[0, 0] = 0.0
        for t in range(1, T):
            a, b = int(lo_f[t]), int(hi[t])
            if a >= b:
                continue
            n = np.arange(a, b)
            vM[t, a:b] = vE[t - 1, n - 1] + LPM[t, a:b]
            um, ue = vM[t - 1, n], vE[t - 1, n]
            v = np.where(um < ue, ue, um) + LPE[t, a:b]
            vE[t, a:b] = v
            bit[t, a:b] = v == um + LPE[t, a:b]
    segrow = np.zeros(N - 1, dtype=np.int64)
    pathn = np.zeros(T, dtype=np.int64)
    pp = np.zeros(T)
    t, n, is_m = T - 1, N - 1, False
    while t > 0 and n > 0:
        pathn[t] = n
        if is_m:
            pp[t] = np.exp(LPM[t, n])
            segrow[n - 1] = t
            t, n, is_m = t - 1, n - 1, False
        else:
            pp[t] = np.exp(LPE[t, n])
            is_m = bool(bit[t, n])
            t -= 1
    assert t == 0 and n == 0, "the traceback of an ok read ends in (0, 0)"
    ends = np.append(segrow[1:], T)
    prob = np.empty(N - 1)
    for j in range(N - 1):
        v = np.sort(pp[segrow[j]:ends[j]])
        m = len(v) // 2
        prob[j] = v[m] if len(v) % 2 else (v[m - 1] + v[m]) / 2.0
    out.segrow, out.signal_positions, out.pathn, out.probabilities = segrow, segrow - 1, pathn, prob
    return out


# ------------------------------------------------------------------------------------------- the guided margin in Python ints
def guided_margin(segrow, T, N, guide, hw):
    """(low, high, edge_rows): INTEGRATION.md section 3's definition with mid(t) -> centre(t) = guide[t - 1], bw -> hw, over the
    path rows [segrow[0], T); the path's column at row t is the number of borders at or before t"""
    low = high = NONE
    edge = 0
    hw = int(hw)
    seg = [int(v) for v in segrow]
    n = 0
    for t in range(seg[0], int(T)):
        while n < len(seg) and seg[n] <= t:
            n += 1
        mid = int(guide[t - 1])
        zero = False
        if mid - hw >= 2:
            s = n - (mid - hw)
            low = min(low, s)
            zero |= s == 0
        if mid + hw + 1 < N:
            s = (mid + hw) - n
            high = min(high, s)
            zero |= s == 0
        edge += zero
    return low, high, edge


def covers(T, N):
    """Does the fixed band at bw = N // 2 hold every cell that lies on some complete path? A column takes at least two rows (M
    then E), so at row t those cells are N - 1 - (T - 1 - t) // 2 <= n <= (t + 1) // 2 (within 1 .. N - 1)."""
    bw = N // 2
    ratio = float(N) / float(T)
    for t in range(1, T):
        lo = max(1, N - 1 - (T - 1 - t) // 2)
        hi = min(N - 1, (t + 1) // 2)
        if lo > hi:
            continue
        mid = int(float(t) * ratio)
        if lo < mid - bw or hi > mid + bw:
            return False
    return True


# ----------------------------------------------------------------------------------------------------------------- the reads
def make_read(rng, mean_code, sd_code, n_kmers, dwell, stall=None):
    """a synth.read_from_digits read with its true starts kept: starts[j] = first sample of k-mer j. ``stall`` = fraction of
    the read one segment of the middle half takes"""
    digits = rng.integers(0, 4, size=n_kmers + K - 1)
    codes = synth._seq_codes(digits, K)
    dw = np.maximum(2, rng.poisson(dwell, size=n_kmers))
    if stall is not None:
        j = int(rng.integers(n_kmers // 4, 3 * n_kmers // 4))
        dw[j] = int(round(stall / (1.0 - stall) * (dw.sum() - dw[j])))
    c = rng.uniform(0.8, 2.0)
    idx = np.repeat(codes, dw)
    sig = mean_code[idx] + c * sd_code[idx] * rng.standard_normal(len(idx))
    starts = np.concatenate([[0], np.cumsum(dw)[:-1]]).astype(np.int64)
    return SimpleNamespace(signal=np.ascontiguousarray(sig, dtype=np.float64), sequence="".join(synth.BASES[d] for d in digits),
                           starts=starts, n_kmers=n_kmers)


# stall family: the candidates (seed STALL_SEED, in order) that tests/test_guided_band_host.py::test_the_purpose_on_the_cpu holds
# to all three conditions -- covers(), oracle(band 50) != oracle(band 4093), model(true starts, half width 16) == oracle(band
# 4093). A candidate that misses one is left out here, not tolerated there.
STALL_SEED = 20261019
STALL_CANDIDATES = 40
STALL_KEEP = (0, 3, 7, 9, 13, 14, 17, 21, 27, 29, 30, 31, 33, 34, 38, 39)
STALL_HALF_WIDTH = 16
STALL_BAND = 50


def stall_candidates(mean_code, sd_code):
    rng = np.random.default_rng(STALL_SEED)
    return [make_read(rng, mean_code, sd_code, int(rng.integers(60, 151)), 1.0, stall=float(rng.uniform(0.3, 0.5)))
            for _ in range(STALL_CANDIDATES)]


def moves_over_starts(starts, n_samples, stride=5):
    """(mv, ts): a synthetic move table (mv[0] = stride) laid over the true starts: base j + K // 2 -- the centre base of k-mer
    j -- moves in the block that holds k-mer j's first sample (the next free block when that one is taken: one move per block),
    the K // 2 bases before the first centre base in the two blocks before it (hence ts = -(K // 2) * stride: the table starts
    that far before the aligner's first sample) and the bases behind the last centre base in the blocks that follow"""
    shift = K // 2
    blocks = list(range(shift))
    last = shift - 1
    for s in starts:
        b = max(int(s) // stride + shift, last + 1)
        blocks.append(b)
        last = b
    for _ in range(K - 1 - shift):
        last += 1
        blocks.append(last)
    flags = np.zeros(max((int(n_samples) + stride - 1) // stride + shift, last + 1), dtype=np.int8)
    flags[blocks] = 1
    return np.concatenate([[stride], flags]).astype(np.int8), -shift * stride


def build_reads(mean_file, sd_file):
    """name -> list of reads (signal, sequence, starts, n_kmers). a: band 50, 60-400 k-mers; a2: band 270, 300-400 k-mers;
    b: 30-150 k-mers at dwell 3 with covers() true; stall: STALL_KEEP of the candidates; w: one read of 4 100 k-mers; stall_mv: six stalled reads at dwell 9 (for
    guide_from_moves: a stride-5 table needs five samples per base); e: 600 reads of 20-60 k-mers"""
    mean_code, sd_code = synth.code_order_table(mean_file, sd_file, K, False)
    fam = {}
    rng = np.random.default_rng(7001)
    fam["a"] = [make_read(rng, mean_code, sd_code, int(rng.integers(60, 401)), 9.0) for _ in range(24)]
    rng = np.random.default_rng(7002)
    fam["a2"] = [make_read(rng, mean_code, sd_code, int(rng.integers(300, 401)), 6.0) for _ in range(4)]
    rng = np.random.default_rng(7003)
    fam["b"] = []
    while len(fam["b"]) < 16:
        r = make_read(rng, mean_code, sd_code, int(rng.integers(30, 151)), 3.0)
        if covers(len(r.signal) + 1, r.n_kmers + 1):
            fam["b"].append(r)
    cand = stall_candidates(mean_code, sd_code)
    fam["stall"] = [cand[i] for i in STALL_KEEP]
    rng = np.random.default_rng(7004)   # the stall at ~9 samples per k-mer: what a stride-5 move table can be laid over
    fam["stall_mv"] = [make_read(rng, mean_code, sd_code, int(rng.integers(60, 151)), 9.0, stall=float(rng.uniform(0.3, 0.5))) for _ in range(6)]
    rng = np.random.default_rng(7005)
    rng = np.random.default_rng(7006)   # one read wider than 2 x 2046 columns: the widest window the entry point accepts
    fam["w"] = [make_read(rng, mean_code, sd_code, 4100, 1.0)]
    fam["e"] = [make_read(rng, mean_code, sd_code, int(rng.integers(20, 61)), float(rng.uniform(2.0, 12.0))) for _ in range(600)]
    return fam


def random_staircase(rng, n_samples, n_columns):
    """a monotone guide with steps of 0 .. 7 columns and long plateaus, from 0 up to n_columns - 1"""
    g = np.zeros(n_samples, dtype=np.int64)
    c = 0
    s = 0
    while s < n_samples:
        run = int(rng.integers(1, 40))
        g[s:s + run] = c
        s += run
        c = min(n_columns - 1, c + int(rng.integers(0, 8)))
    return g.astype(np.int32)


def true_guide(r):
    return G.guide_from_starts(r.starts, len(r.signal), r.n_kmers + 1)


def diagonal(r):
    return G.diagonal_guide(len(r.signal), r.n_kmers + 1)
