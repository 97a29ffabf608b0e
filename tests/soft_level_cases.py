"""The posterior-weighted per-base sums (Aligner.set_soft_levels; include/dynamont_mi.h) restated in
NumPy over the CPU oracle's lattices, the bounds the device is held to, and the read sets the tests share.

An ok read has signal x, T = len(x) + 1 lattice rows and N columns; sample x[t-1] belongs to row t; output row j is lattice
column n = j + 1. LPM / LPE are posterior_sample_cases.lattices' arrays: -inf outside the band window of row t and in row 0.
    pM = exp(LPM(t, n)), pE = exp(LPE(t, n)) (0 where the log is -inf),  g(t) = pM + pE
    soft_weight = sum over t = 1 .. T-1 of g(t),  soft_sum = sum g(t) * x[t-1],  soft_sumsq = sum (g(t) * x[t-1]) * x[t-1]
every sum fp64, ascending t, g formed first, one IEEE operation per step (np.cumsum adds in sequence, np.sum does not).

The device reads a FLOAT log-posterior l (or rebuilds one of that accuracy): its p differs from exp of the exact value by at
most 2^-24 p |ln p| relatively rounded, so per column
    tol_w  = 2^-23 * sum (pM |ln pM| + pE |ln pE|) + 1e-9
    tol_s1 = the same with |x| inside the sum,   tol_s2 = the same with x^2 inside the sum
There is no discrete decision here: no cell and no column is left out of any comparison.

`mutate` builds the deliberately wrong versions tests/test_soft_levels_host.py holds the yardstick against."""
import numpy as np

import border_interval_cases as bic
import posterior_sample_cases as psc

MUTATIONS = ("pm_alone", "pe_alone", "next_sample", "column_minus_one", "no_band_mask", "square_first")
NAMES = ("plain", "plain_band50", "long", "long_band50", "imperfect", "imperfect_band50")
read_sets = bic.read_sets


def unmasked(a, window):
    """an out-of-band cell of rows 1 .. T-1 takes the value of the nearest in-band cell of its row (what an unmasked read of a
    band slot may return; border_confidence_cases.lpm_columns(mask=False)) -- a mutation. window = (lo [T], hi [T]): the
    columns [lo, hi) of every row's band window"""
    out = a.copy()
    lo, hi = window
    for t in range(1, a.shape[0]):
        out[t, :lo[t]] = a[t, lo[t]]
        out[t, hi[t]:] = a[t, hi[t] - 1]
    return out


def _p_and_plnp(l):
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.exp(l)                                                # exp(-inf) = 0
        plnp = np.where(p > 0, p * np.abs(np.where(p > 0, l, 0.0)), 0.0)
    return p, plnp


def sums(lpm, lpe, x, mutate=None, fp32=False, window=None):
    """(soft_weight, soft_sum, soft_sumsq, tol_w, tol_s1, tol_s2), one entry per output row j = 0 .. N-2, over the two
    log-posterior arrays [T, N] and the signal x [T-1]. fp32: every log-posterior rounded to float first (what two of the three
    device layouts store)."""
    x = np.asarray(x, dtype=np.float64)
    if fp32:
        lpm, lpe = lpm.astype(np.float32).astype(np.float64), lpe.astype(np.float32).astype(np.float64)
    if mutate == "no_band_mask":
        lpm, lpe = unmasked(lpm, window), unmasked(lpe, window)
    m, e = lpm[1:, 1:], lpe[1:, 1:]                                  # rows 1 .. T-1, columns 1 .. N-1
    if mutate == "column_minus_one":                                 # column n - 1 (column 0 holds nothing)
        m, e = lpm[1:, :-1], lpe[1:, :-1]
    pm, am = _p_and_plnp(m)
    pe, ae = _p_and_plnp(e)
    g = pm + pe
    if mutate == "pm_alone":
        g = pm
    elif mutate == "pe_alone":
        g = pe
    xs = x[:, None]
    if mutate == "next_sample":                                      # x[t] for x[t - 1] (the last row takes the last sample)
        xs = np.concatenate((x[1:], x[-1:]))[:, None]
    gx = g * xs
    sq = g * (xs * xs) if mutate == "square_first" else gx * xs
    w, s1, s2 = (np.cumsum(a, axis=0)[-1] for a in (g, gx, sq))
    a = am + ae
    ax = np.abs(x)[:, None]
    tol = [2.0 ** -23 * np.sum(a * f, axis=0) + 1e-9 for f in (1.0, ax, ax * ax)]
    return w, s1, s2, tol[0], tol[1], tol[2]


def derived(w, s1, s2):
    """(soft_dwell, soft_mean, soft_stdv) as the definition derives them"""
    from dynamont_amd._dynamont import soft_level_columns
    return soft_level_columns(w, s1, s2)


class Yard:
    """the yardstick of one read at one band: the lattices are computed once"""

    def __init__(self, orc, signal, seq, band=400):
        self.orc, self.signal, self.seq, self.band = orc, np.asarray(signal, dtype=np.float64), seq, band
        self.lpm, self.lpe, self.res = psc.lattices(orc, signal, seq, band)
        self.T, self.N = self.lpm.shape
        self.kmers = orc.kmers(seq)[:self.N - 1]                     # entry n - 1 <-> column n
        _, n_start, n_end = orc.bounds(self.T, self.N, min(band // 2, self.N // 2))
        self.window = (np.maximum(n_start.astype(np.int64), 1), n_end.astype(np.int64))
        self._cache = {}

    def at(self, mutate=None, fp32=False):
        key = (mutate, fp32)
        if key not in self._cache:
            self._cache[key] = sums(self.lpm, self.lpe, self.signal, mutate, fp32, self.window)
        return self._cache[key]

    def called_dwell(self):
        """samples between the called borders, per output row"""
        pos = self.res["signal_positions"].astype(np.int64)
        return np.diff(np.concatenate((pos, [self.T - 1])))

    def pooled(self, cols, num_kmers):
        """per-k-mer sums of per-column values, added in column order"""
        return [np.bincount(self.kmers, weights=c, minlength=num_kmers) for c in cols]


def check_device(y, w, s1, s2, what):
    """hold one read's three device columns to the yardstick, every column; returns the worst error as a share of its bound, per
    sum"""
    yw, ys1, ys2, tw, t1, t2 = y.at()
    assert len(w) == len(s1) == len(s2) == y.N - 1, (what, y.N - 1, len(w))
    worst = []
    for got, want, tol, name in ((w, yw, tw, "weight"), (s1, ys1, t1, "sum"), (s2, ys2, t2, "sumsq")):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        j = int(np.argmax(err / tol))
        assert (err <= tol).all(), (what, name, j, float(got[j]), float(want[j]), float(tol[j]))
        worst.append(float((err / tol).max()))
    print(f"{what}: {y.N - 1} columns, weight / sum / sumsq error <= {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f} of its bound")
    return worst


def make_yards(models, sets, name, cache=None):
    """[Yard] of a read set (cached per (name, read) in `cache`)"""
    from dynamont_amd import synth
    from oracle.pyoracle import Oracle
    key, pore, band, reads = sets[name]
    cache = cache if cache is not None else {}
    if ("orc", key, pore, band) not in cache:
        cache["orc", key, pore, band] = Oracle(models[key], synth.PORES[pore][0], band)
    orc = cache["orc", key, pore, band]
    out = []
    for i, r in enumerate(reads):
        if (name, i) not in cache:
            cache[name, i] = Yard(orc, r.signal, r.sequence, band)
        out.append(cache[name, i])
    return out


def grouping_lattice():
    """(LPM, LPE, x) of a small lattice on which g * (x * x) and (g * x) * x DO differ: on the read sets they differ in last bits
    only, far inside the bounds. One in-band row per column with g = 1/3 + 1/3 and x = 0.1 * n: the two groupings round apart
    for some n, and one add of one term shows it."""
    import math
    T, N = 12, 10
    lpm, lpe = np.full((T, N), -np.inf), np.full((T, N), -np.inf)
    third = math.log(1.0 / 3.0)
    for n in range(1, N):
        lpm[n, n] = lpe[n, n] = third
    x = 0.1 * np.arange(1, T)
    return lpm, lpe, x
