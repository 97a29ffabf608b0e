"""Posterior path sampling (Aligner.set_posterior_samples; include/dynamont_mi.h) restated in NumPy
over the CPU oracle's lattices, and the read sets the tests share.

Lattice rows t = 0 .. T-1, columns n = 0 .. N-1. LPM(t, n) = fM + bM - Z and LPE(t, n) = fE + bE - Z, both -inf outside the
band window of row t (Oracle.bounds; column 0 is never filled), LPM -inf in row 0, LPE(0, 0) = 0: the arrays of
border_confidence_cases.lpm_columns and their E twin, in the same band-column addressing.
    u(seed, i, k, t) = (mix(mix(mix(seed + i) + k) + t) >> 11) * 2^-53, mix the SplitMix64 step, all mod 2^64
Sample k of read i starts in E(0, 0). While (t, n) != (T-1, N-1): a = LPM(t+1, n+1) (-inf when n+1 >= N or t+1 > T-1),
b = LPE(t+1, n). Both -inf: dead. One finite: that way. Both finite: p = exp(a - LPE(t, n)), move iff u < p. A move records
start[k][n] = t and continues in E(t+2, n+1); a stay continues in E(t+1, n). A dead sample is 0xFFFFFFFF throughout.

The device reads log-posteriors that were rounded to fp32 (two of its three layouts) or rebuilt from an fp32 value (the third).
Every draw therefore carries the margin 2 * (p * 2^-23 * (|a| + |LPE(t, n)|) + 1e-9): twice the bound that two fp32-rounded
log-posteriors put on p. A path with a draw inside its margin is UNDECIDED and left out of exact comparisons; `check_cap` holds
how many may be (one per read, 2 % per test -- the yardstick alone has none on the sets below).

`mutate` builds the deliberately wrong versions tests/test_posterior_samples_host.py holds the yardstick against."""
import numpy as np

import border_confidence_cases as bcc

DEAD = 0xFFFFFFFF
MUTATIONS = ("u_ge_p", "column_n", "stream_not_keyed_by_k", "start_off_by_one")
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix(x):
    """the SplitMix64 step on a uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform(seed, i, k, t):
    """u(seed, i, k, t) for arrays k, t (uint64-compatible)"""
    with np.errstate(over="ignore"):
        s = np.full(np.shape(k), (int(seed) + int(i)) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        h = mix(mix(mix(s) + np.asarray(k, dtype=np.uint64)) + np.asarray(t, dtype=np.uint64))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def lattices(orc, signal, seq, band=400, res=None):
    """(LPM [T, N], LPE [T, N], res): the two log-posterior arrays of the definition"""
    lpm, res = bcc.lpm_columns(orc, signal, seq, band, res)
    T, N = lpm.shape
    bw = min(band // 2, N // 2)
    fb = orc.debug_fb(signal, seq, 2 * bw + 1)
    start, n_start, n_end = orc.bounds(T, N, bw)
    lpe = np.full((T, N), -np.inf)
    for t in range(1, T):
        lo, hi = max(int(n_start[t]), 1), int(n_end[t])
        c = np.arange(lo, hi) - int(start[t])
        lpe[t, lo:hi] = fb["fE"][t, c] + fb["bE"][t, c] - res["Z"]
    lpe[0, 0] = 0.0
    return lpm, lpe, res


def walk(lpm, lpe, seed, i, K, mutate=None, fp32=False, rel_margin=None):
    """K samples of read i: (starts uint32 [K, N-1], dead bool [K], undecided bool [K]). All samples step together, each at its
    own cell. fp32: every log-posterior rounded to float first (what two of the three device layouts store). rel_margin: the
    lattice holds the very values the device reads (the device harness), so a draw's margin is rel_margin * p -- what two
    implementations of exp may differ by -- instead of the fp32 one."""
    T, N = lpm.shape
    if fp32:
        lpm, lpe = lpm.astype(np.float32).astype(np.float64), lpe.astype(np.float32).astype(np.float64)
    M = np.full((T + 2, N + 1), -np.inf)          # rows T, T+1 and column N: the cells that do not exist
    E = np.full((T + 2, N + 1), -np.inf)
    M[:T, :N], E[:T, :N] = lpm, lpe
    k = np.arange(K, dtype=np.uint64)
    t, n = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    starts = np.zeros((K, N - 1), dtype=np.uint32)
    dead, undecided = np.zeros(K, dtype=bool), np.zeros(K, dtype=bool)
    for _ in range(T + 1):
        live = ~dead & ~((t == T - 1) & (n == N - 1))
        if not live.any():
            break
        idx = np.nonzero(live)[0]
        tt, nn = t[idx], n[idx]
        off_end = tt >= T - 1
        tc = np.minimum(tt, T - 1)
        a = M[tc + 1, nn if mutate == "column_n" else nn + 1]
        b = E[tc + 1, nn]
        a[off_end], b[off_end] = -np.inf, -np.inf
        here = E[tc, nn]
        fa, fb_ = a != -np.inf, b != -np.inf
        dies = ~fa & ~fb_
        both = fa & fb_
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.exp(np.where(both, a - here, 0.0))
            margin = 2.0 * (p * 2.0 ** -23 * (np.abs(np.where(both, a, 0.0)) + np.abs(np.where(both, here, 0.0))) + 1e-9)
            if rel_margin is not None:
                margin = rel_margin * p
        u = uniform(seed, i, np.zeros_like(k[idx]) if mutate == "stream_not_keyed_by_k" else k[idx], tt.astype(np.uint64))
        move = np.where(both, (u >= p) if mutate == "u_ge_p" else (u < p), fa)
        with np.errstate(invalid="ignore"):
            undecided[idx] |= both & np.isfinite(p) & (np.abs(u - p) <= margin)      # (p = inf, LPE(t, n) = -inf: u < p whatever u)
        dead[idx[dies]] = True
        mv = idx[move & ~dies]
        if mutate == "column_n":                   # (the wrong column may run off the lattice's corner: such a path is dead)
            over = n[mv] >= N - 1
            dead[mv[over]] = True
            mv = mv[~over]
        starts[mv, n[mv]] = (t[mv] + (1 if mutate == "start_off_by_one" else 0)).astype(np.uint32)
        t[mv] += 2
        n[mv] += 1
        st = idx[~move & ~dies]
        t[st] += 1
    starts[dead] = DEAD
    return starts, dead, undecided


def check_cap(undecided_per_read, what):
    """at most one undecided path per read and 2 % per test"""
    total = sum(len(u) for u in undecided_per_read)
    n_und = sum(int(u.sum()) for u in undecided_per_read)
    for i, u in enumerate(undecided_per_read):
        assert int(u.sum()) <= 1, (what, "read", i, "undecided paths", int(u.sum()))
    assert n_und <= 0.02 * total, (what, n_und, total)
    return n_und


# ---- the read sets: those of tests/border_confidence_cases.py (fixed seeds) -----------------------------------------------------------
def read_sets(model):
    """name -> (pore, band, reads)"""
    long_read = bcc.imperfect_reads(model, "dna_r9", bcc.BAND50_LONG_SEED, 1, 600)
    return {
        "rna002": ("rna002", 400, bcc.plain_reads(model, "rna002", bcc.RNA002_SEED, 3, 120)),
        "dna_r9": ("dna_r9", 400, bcc.plain_reads(model, "dna_r9", bcc.DNA_R9_SEED, 3, 200)),
        "band50": ("dna_r9", 50, bcc.imperfect_reads(model, "dna_r9", bcc.BAND50_SEED, 3, 200)),
        "band50_long": ("dna_r9", 50, long_read),
        "band400_long": ("dna_r9", 400, long_read),
        "wide": ("rna002", 600, bcc.plain_reads(model, "rna002", bcc.WIDE_SEED, 1, 600)),
    }
